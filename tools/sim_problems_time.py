#!/usr/bin/env python3
"""Wall time of pddp_simulate_problems on one MI355X: the wave family (a wavefront per entry) against the thread family (a thread per entry), and the wave family
against pddp_simulate_batch of a build of the parent commit.

    python tools/sim_problems_time.py [--parent-lib PATH/libpddp.so] [--out profiles/sim_problems.md] [--json FILE]

Part 1, the two families: pendulum, cart-pole, quadrotor x float32, float64; N = 32, M = 2, A = 4, RK3; count in {1, 64, 256, 1024, 4096, 16384} entries idx = 0 .. count - 1
of a handle of 16384 slots after a load and two sweeps; 150 sub-steps over about one knot; device-resident plans.
Part 2, against the parent: pddp_simulate_batch of --parent-lib (without the option: of this tree's library, and the table says so) against
pddp_simulate_problems(idx = 0 .. batch - 1, family 1) on a handle WITHOUT a step table -- the arm at the shape of tools/sim_batch_time.py (float32, N = 64, M = 4, A = 16,
tool-point goals) and the quadrotor (float32, the shape of part 1).

Every figure is a time between entering and leaving the Python call (which ends in the call's stream synchronisation), after untimed warm-up calls of both rows of a
pair.  A row is ROUNDS rounds of CALLS calls; the two rows of a pair alternate round by round inside one process.  Figure = the median of the round medians;
spread = the largest minus the smallest round median.  The thread family counts as faster at a count when the wave figure minus the thread figure exceeds the larger of
the two spreads; a plant's threshold is the smallest measured count from which that holds at every larger measured count."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyddp  # noqa: E402
from oracle_binding import example_inputs  # noqa: E402  (the examples' inputs)

COUNTS = (1, 64, 256, 1024, 4096, 16384)
SUBSTEPS = 150
ROUNDS, CALLS = 5, 7
CF_KW = dict(N=32, M=2, A=4, integrator=3, total_time=1.0, max_iter=8)
ARM_KW = dict(N=64, M=4, A=16, wafr_urdf=1, mpc_mode=1, tol_cost=1e-5, total_time=0.5, max_iter=4, ee_cost=1, ignore_max_rho_exit=0)      # tools/sim_batch_time.py
DIMS = {1: (2, 1), 2: (4, 1), 3: (12, 4)}
NAMES = {1: "pendulum", 2: "cart-pole", 3: "quadrotor", 4: "arm"}


def pair_ms(fa, fb, rounds=ROUNDS, calls=CALLS):
    """two rows measured alternately: (figure, spread) of each"""
    for _ in range(2):
        fa(); fb()
    meds = ([], [])
    for _ in range(rounds):
        for f, m in ((fa, meds[0]), (fb, meds[1])):
            t = []
            for _ in range(calls):
                t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
            m.append(statistics.median(t))
    return [(statistics.median(m), max(m) - min(m)) for m in meds]


def closed_form_handle(plant, dtype, B, lib=None):
    T = np.float32 if dtype == 0 else np.float64
    N, (n, m) = CF_KW["N"], DIMS[plant]
    s = pyddp.Solver(pyddp.default_config(plant, _lib_path=lib, dtype=dtype, batch=B, **CF_KW), _lib_path=lib)
    rng = np.random.default_rng(plant)
    x0, u0, xg = example_inputs(plant, N, np.float64)
    x = np.tile(x0.reshape(1, N, n), (B, 1, 1)) + rng.normal(0, 0.002, (B, N, n))
    s.load(x.astype(T), np.tile(u0.reshape(1, N, m), (B, 1, 1)).astype(T), np.tile(xg, (B, 1)).astype(T), clear_vars=1)
    s.iterate(2); s.sync()
    xa = (s.store()["x"][:, 0] + rng.normal(0, 0.004, (B, n))).astype(T)
    step_us = CF_KW["total_time"] / (N - 1) * 1e6
    return s, xa, np.zeros(B), rng.uniform(0.8, 1.2, B) * step_us, None


def arm_handle(B, lib=None):
    N = ARM_KW["N"]
    s = pyddp.Solver(pyddp.default_config(4, _lib_path=lib, dtype=0, batch=B, **ARM_KW), _lib_path=lib)
    rng = np.random.default_rng(B)
    x0 = np.zeros((B, N, 14), np.float32); x0[:, :, 1] = 0.7; x0[:, :, 3] = -0.8; x0[:, :, 5] = 0.75
    u0 = np.full((B, N, 7), 0.01, np.float32)
    xg = np.zeros((B, 14), np.float32); xg[:, :3] = np.array([0.45, 0.15, 0.75]) + rng.uniform(-0.03, 0.03, (B, 3))
    out = s.solve(x0, u0, xg)
    xa = (out["x"][:, 0] + rng.normal(0, 0.004, (B, 14))).astype(np.float32)
    step_us = ARM_KW["total_time"] / (N - 1) * 1e6
    return s, xa, np.zeros(B), rng.uniform(0.8, 1.2, B) * step_us, xg[:, :3].copy()


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))


def families(out):
    rows = []
    for plant in (1, 2, 3):
        for dtype in (0, 1):
            s, xa, t0, el, _ = closed_form_handle(plant, dtype, max(COUNTS))
            for count in COUNTS:
                idx = np.arange(count, dtype=np.int32)
                args = (idx, t0[:count], el[:count], SUBSTEPS, None, xa[:count])
                (wave, wave_sp), (ts, ts_sp) = pair_ms(lambda: s.simulate_problems(*args, family=1), lambda: s.simulate_problems(*args, family=2))
                r1 = s.simulate_problems(*args, family=1)
                assert np.isfinite(r1[0]).all() and not r1[2].any(), "the timed robots must run to the end of their elapsed time"
                ok = same(r1, s.simulate_problems(*args, family=2))
                rows.append(dict(plant=plant, dtype=dtype, count=count, wave_ms=wave, wave_spread=wave_sp, thread_ms=ts, thread_spread=ts_sp, same_bits=ok,
                                 thread_faster=bool(wave - ts > max(wave_sp, ts_sp))))
                print(f"{NAMES[plant]:9s} f{32 if dtype == 0 else 64} count {count:6d}: wave {wave:8.3f} ms (spread {wave_sp:.3f})   thread {ts:8.3f} ms (spread {ts_sp:.3f})"
                      f"   same bits {ok}", flush=True)
            s.close()
    out["families"] = rows
    thresholds = {}
    for plant in (1, 2, 3):
        for dtype in (0, 1):
            mine = [r for r in rows if r["plant"] == plant and r["dtype"] == dtype]
            thr = None
            for r in reversed(mine):                           # the smallest count from which the thread family STAYS faster
                if not r["thread_faster"]:
                    break
                thr = r["count"]
            thresholds[f"{plant}/{dtype}"] = thr
    out["thresholds"] = thresholds
    return rows, thresholds


def against_parent(out, parent_lib):
    rows = []
    for label, make, B in (("arm", arm_handle, 1024), ("quadrotor", lambda B, lib=None: closed_form_handle(3, 0, B, lib), 4096)):
        s, xa, t0, el, g = make(B)
        p = make(B, parent_lib)[0] if parent_lib else s
        idx = np.arange(B, dtype=np.int32)
        plan = s.store()
        hp = dict(x=plan["x"], u=plan["u"], KT=plan["KT"])     # host-plan rows: both libraries follow these; device-plan rows: each handle the solution it holds itself (same inputs)
        for mode, kw_b, kw_p in (("device-resident plans", {}, {}), ("host plans", hp, hp)):
            (old, old_sp), (new, new_sp) = pair_ms(lambda: p.simulate_batch(t0, el, SUBSTEPS, g, xa, **kw_b), lambda: s.simulate_problems(idx, t0, el, SUBSTEPS, g, xa, family=1, **kw_p))
            ok = same(p.simulate_batch(t0, el, SUBSTEPS, g, xa, **hp), s.simulate_problems(idx, t0, el, SUBSTEPS, g, xa, family=1, **hp))
            rows.append(dict(plant=label, batch=B, mode=mode, parent_ms=old, parent_spread=old_sp, new_ms=new, new_spread=new_sp, same_bits_host_plans=ok,
                             inside=bool(new <= old + old_sp)))
            print(f"{label:9s} B {B}: {mode:22s} parent pddp_simulate_batch {old:8.3f} ms (spread {old_sp:.3f})   pddp_simulate_problems, wave {new:8.3f} ms (spread {new_sp:.3f})"
                  f"   same bits {ok}", flush=True)
        s.close()
        if p is not s:
            p.close()
    out["against_parent"] = rows
    out["parent_lib"] = "a build of the parent commit" if parent_lib else "this tree's own library (pddp_simulate_batch's code path is unchanged)"
    return rows


def write_tables(f, out):
    f.write("## Measured (tools/sim_problems_time.py, one MI355X)\n\n")
    f.write(f"Wall time of one call in ms; figure = median of {ROUNDS} round medians of {CALLS} calls, the two rows of a pair alternating round by round; spread = largest minus\n"
            f"smallest round median.  {SUBSTEPS} sub-steps over about one knot, N = {CF_KW['N']}, M = {CF_KW['M']}, A = {CF_KW['A']}, RK3, device-resident plans, idx = 0 .. count - 1 of 16384 slots.\n\n")
    f.write("| plant | type | count | wave family | spread | thread family | spread | thread faster by more than the spread | same bits |\n|---|---|---|---|---|---|---|---|---|\n")
    for r in out["families"]:
        f.write(f"| {NAMES[r['plant']]} | float{32 if r['dtype'] == 0 else 64} | {r['count']} | {r['wave_ms']:.3f} | {r['wave_spread']:.3f} | {r['thread_ms']:.3f} | {r['thread_spread']:.3f} | "
                f"{'yes' if r['thread_faster'] else 'no'} | {'yes' if r['same_bits'] else 'NO'} |\n")
    f.write("\nChosen thresholds (`sim_ts_threshold`, csrc/sim_slots.hpp): the smallest measured count from which the thread family stays faster.\n\n| plant | float32 | float64 |\n|---|---|---|\n")
    for plant in (1, 2, 3):
        cell = [out["thresholds"][f"{plant}/{d}"] for d in (0, 1)]
        f.write(f"| {NAMES[plant]} | {cell[0] if cell[0] else 'never'} | {cell[1] if cell[1] else 'never'} |\n")
    f.write(f"\nAgainst `pddp_simulate_batch` of {out['parent_lib']}, whole handle, no step table, `idx = 0 .. batch - 1`, family 1:\n\n")
    f.write("| plant | batch | plans | parent `pddp_simulate_batch` | its spread | `pddp_simulate_problems` | its spread | inside parent + spread | same bits |\n|---|---|---|---|---|---|---|---|---|\n")
    for r in out["against_parent"]:
        f.write(f"| {r['plant']} | {r['batch']} | {r['mode']} | {r['parent_ms']:.3f} | {r['parent_spread']:.3f} | {r['new_ms']:.3f} | {r['new_spread']:.3f} | {'yes' if r['inside'] else 'NO'} | "
                f"{'yes' if r['same_bits_host_plans'] else 'NO'} |\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None, help="file for the markdown tables (default: printed)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = {}
    families(out)
    against_parent(out, a.parent_lib)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            write_tables(f, out)
    else:
        write_tables(sys.stdout, out)
    return 0 if all(r["same_bits"] for r in out["families"]) else 1


if __name__ == "__main__":
    sys.exit(main())
