#!/usr/bin/env python3
"""What a control cycle costs with one build of the library, for comparing two builds (profiles/mpc_record.md).

    python tools/mpc_record_time.py --lib PATH/libpddp.so --label NAME [--rounds 5] [--slots 1]

One process, one library.  (1) The loop of bench.py's two mpc_cycle_published_shape_* rows -- the same handle, bench.ee_inputs with seed 77, warm start, 24 cycles of
max_iter = 4, median of cycles 2.. -- `--rounds` times on fresh handles, with a digest over every output of every cycle (the inputs are seeded: two builds that compute
the same print the same digest).  bench.py --rows itself takes no --lib.  (2) The named-slot path through tools/mpc_slots_time.py's Cycle on a handle of 4096 problems:
pddp_mpc_solve on the whole handle and pddp_mpc_solve_problems for 1 / 16 / 256 slots, medians of 25 calls after 3 untimed ones (the tool's own main times the slot
path for the tree's library only).  Prints one JSON line; run the two builds in alternation, every run a process of its own."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "parallel-ddp_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import pyddp  # noqa: E402
import bench  # noqa: E402
import mpc_slots_time as mst  # noqa: E402


def published(lib, ee, rng):
    N = 64
    kw = dict(wafr_urdf=1, mpc_mode=1, tol_cost=1e-5, total_time=0.5, ignore_max_rho_exit=0, device=0, use_graph=1)
    s = pyddp.Solver(pyddp.default_config(4, N=N, M=4, A=16, batch=1, max_iter=100, ee_cost=ee, _lib_path=lib, **kw), _lib_path=lib)
    x0, u0, xg = bench.ee_inputs(N, rng, 1)
    if not ee:
        xg[0, :7] = [0.5, 0.6, -0.3, -0.9, 0.2, 0.7, 0.1]
    s.load(x0, u0, xg)
    first = s.mpc_solve(x0[0, 0], xg, 0, clear_vars=1, max_iter=100)
    cyc_ms, h = [], hashlib.sha256()
    xa = first["x"][0][1]
    for c in range(24):
        t0 = time.perf_counter()
        r = s.mpc_solve(xa + rng.normal(0, 0.0005, 14).astype(np.float32), xg, 1, max_iter=4)
        cyc_ms.append((time.perf_counter() - t0) * 1e3)
        xa = r["x"][0][1]
        for k in ("x", "u", "KT", "Jout", "alphaOut", "success", "iters"):
            h.update(r[k].tobytes())
    s.close()
    return float(np.median(cyc_ms[2:])), h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--label", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1)
    a = ap.parse_args()
    lib = os.path.abspath(a.lib)
    out = {"label": a.label}
    for name, ee in (("ee_cost", 1), ("joint_cost", 0)):
        rows = [published(lib, ee, np.random.default_rng(77)) for _ in range(a.rounds)]
        out[name + "_median_cycle_ms"] = [round(m, 4) for m, _ in rows]
        out[name + "_bits"] = sorted({d for _, d in rows})
    if a.slots:
        big = mst.Cycle(4096, lib)
        out["whole_4096_ms"] = round(mst.median_ms(big.whole(), 25), 4)
        for count in mst.COUNTS:
            call = big.slots(np.random.default_rng(count).permutation(4096)[:count])
            out["slots_%d_ms" % count] = round(mst.median_ms(call, 25), 4)
        big.s.close()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
