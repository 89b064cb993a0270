#!/usr/bin/env python3
"""Wall time of the simulated robot for a whole batch: ONE pddp_simulate_batch call (host plans / the plans the handle holds on the device) against
B serial pddp_simulate calls.  Shape: arm, float32, N = 64, M = 4, A = 16, 150 sub-steps; B in {1, 64, 1024, 4096}.

    python tools/sim_batch_time.py [--serial-lib PATH/libpddp.so] [--out profiles/sim_batch_time.md]

--serial-lib: the library whose pddp_simulate gives the serial figure -- a build of the commit BEFORE pddp_simulate_batch existed (pddp_simulate is the
yardstick; its code path is unchanged since, so without the option the tree's own library is timed and the table says so).
Every figure is the median over the repetitions of the time between entering and leaving the Python call(s), after one untimed warm-up call."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
import pyddp  # noqa: E402

KW = dict(N=64, M=4, A=16, wafr_urdf=1, mpc_mode=1, tol_cost=1e-5, total_time=0.5, max_iter=4, ee_cost=1, ignore_max_rho_exit=0)
SUBSTEPS = 150


def solver(B, lib=None):
    return pyddp.Solver(pyddp.default_config(4, _lib_path=lib, dtype=0, batch=B, **KW), _lib_path=lib)


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--serial-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_batch_time.md"))
    ap.add_argument("--batches", default="1,64,1024,4096")
    a = ap.parse_args()
    N = KW["N"]
    step_us = KW["total_time"] / (N - 1) * 1e6
    rows = []
    for B in (int(v) for v in a.batches.split(",")):
        rng = np.random.default_rng(B)
        s = solver(B)
        x0 = np.zeros((B, N, 14), np.float32); x0[:, :, 1] = 0.7; x0[:, :, 3] = -0.8; x0[:, :, 5] = 0.75
        u0 = np.full((B, N, 7), 0.01, np.float32)
        xg = np.zeros((B, 14), np.float32); xg[:, :3] = np.array([0.45, 0.15, 0.75]) + rng.uniform(-0.03, 0.03, (B, 3))
        out = s.solve(x0, u0, xg)
        xa = (out["x"][:, 0] + rng.normal(0, 0.004, (B, 14))).astype(np.float32)
        t0, el, g = np.zeros(B), rng.uniform(0.8, 1.2, B) * step_us, xg[:, :3].copy()
        reps = 20 if B <= 64 else 7
        host = median_ms(lambda: s.simulate_batch(t0, el, SUBSTEPS, g, xa, x=out["x"], u=out["u"], KT=out["KT"]), reps)
        dev = median_ms(lambda: s.simulate_batch(t0, el, SUBSTEPS, g, xa), reps)
        rh, rd = s.simulate_batch(t0, el, SUBSTEPS, g, xa, x=out["x"], u=out["u"], KT=out["KT"]), s.simulate_batch(t0, el, SUBSTEPS, g, xa)
        ss = solver(1, a.serial_lib) if a.serial_lib else s

        def serial():
            return [ss.simulate(out["x"][b], out["u"][b], out["KT"][b], t0[b], el[b], SUBSTEPS, g[b], xa[b]) for b in range(B)]
        ser = median_ms(serial, 5 if B <= 64 else 1)
        rs = serial()
        same = all(np.array_equal(rh[0], r[0]) and (rh[1] == r[1]).all() and (rh[2] == r[2]).all() for r in (rd, (np.stack([v[0] for v in rs]), np.array([v[1] for v in rs]), np.array([v[2] for v in rs]))))
        rows.append((B, host, dev, ser, same))
        print(f"B {B:5d}: batched, host plans {host:9.3f} ms   batched, device plans {dev:9.3f} ms   {B} serial calls {ser:10.3f} ms   identical results: {same}", flush=True)
        s.close()
        if ss is not s:
            ss.close()
    src = "a build of the parent commit (--serial-lib)" if a.serial_lib else "this tree's own library (pddp_simulate's code path is unchanged)"
    with open(a.out, "w") as f:
        f.write("# pddp_simulate_batch against serial pddp_simulate calls (tools/sim_batch_time.py)\n\n")
        f.write(f"Arm, float32, N = {N}, M = {KW['M']}, A = {KW['A']}, {SUBSTEPS} sub-steps, tool-point goals; wall time of the call(s) in ms, median over repetitions\n")
        f.write(f"(serial at B >= 1024: one pass).  Serial figures: {src}.\n\n")
        f.write("| B | one batched call, host plans | one batched call, device-resident plans | B serial `pddp_simulate` calls | serial / batched (host plans) | same bits |\n|---|---|---|---|---|---|\n")
        for B, host, dev, ser, same in rows:
            f.write(f"| {B} | {host:.3f} | {dev:.3f} | {ser:.3f} | {ser / host:.1f} | {'yes' if same else 'NO'} |\n")
    bad = [r for r in rows if r[0] == 64 and not r[1] < r[3]]
    if bad:
        print("ONE BATCHED CALL AT B = 64 IS NOT FASTER THAN THE 64 SERIAL CALLS: something is wrong with the host path", flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
