#!/usr/bin/env python3
"""What per-problem cost weights cost the sweeps, as a same-process A/B/C: three handles of the same workload, timed in turn, repetition by repetition.

    python tools/problem_costs_time.py --parent-lib PATH/libpddp.so [--out profiles/problem_costs.md] [--batch 16384] [--ee-batch 4096] [--reps 7] [--sweeps 20]

  (a) --parent-lib: a library built from the commit BEFORE pddp_set_cost_problems existed
  (b) this tree's library, no table (the handle never calls pddp_set_cost_problems)
  (c) this tree's library with a table whose rows all equal the handle-wide record (pddp_set_cost_problems with get_cost_problems' own answer): the same numbers,
      fetched per problem
Workloads: the headline (arm, N = 128, M = 4, A = 8, float32, --batch problems, benchmark mode) and the end-effector shape of bench.py's `widening` row (N = 64,
M = 4, A = 8, --ee-batch problems).  Per workload: pddp_time_sweeps (ms per sweep, the graph replay) and pddp_time_kernels (ms per kernel), each as the median over
--reps repetitions with (a)'s own spread beside it, twice: max - min over its repetitions, and their interquartile range (one slow repetition -- another tenant of
the box -- widens the first, not the second): boxes differ by several per cent, so only figures of ONE call compare.
Without --parent-lib column (a) is left out and the table says so.  The output file's text in front of the line MARK (the resource table, written with the build's
-Rpass-analysis=kernel-resource-usage remarks) is kept; everything from MARK on is replaced."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
import pyddp  # noqa: E402

PI = 3.14159
MARK = "<!-- timing: written by tools/problem_costs_time.py -->"


def joint_inputs(N, rng, B):
    x = np.zeros((B, N, 14), np.float32)
    x[:, :, :7] = np.asarray([-0.5 * PI, 0.25 * PI, 0.167 * PI, -0.167 * PI, 0.125 * PI, 0.167 * PI, 0.5 * PI], np.float32)
    x[:, :, 7:] = rng.normal(0, 0.001, (B, N, 7)).astype(np.float32)
    u = np.zeros((B, N, 7), np.float32)
    u[:] = np.asarray([0.0, -102.9832, 11.1968, 47.0724, 2.5993, -7.0290, -0.0907], np.float32)
    g = np.zeros((B, 14), np.float32)
    g[:, :7] = np.asarray([0, 0, 0, -0.25 * PI, 0, 0.25 * PI, 0.5 * PI], np.float32)
    return x, u, g


def ee_inputs(N, rng, B):
    x = np.zeros((B, N, 14), np.float32); x[:, :, 1] = 0.7; x[:, :, 3] = -0.8; x[:, :, 5] = 0.75
    u = np.full((B, N, 7), 0.01, np.float32)
    g = np.zeros((B, 14), np.float32); g[:, :3] = np.array([0.45, 0.15, 0.75]) + rng.uniform(-0.03, 0.03, (B, 3))
    return x, u, g


WORKLOADS = {
    "headline": (dict(N=128, M=4, A=8, wafr_urdf=1, tol_cost=0.0, total_time=0.5, max_iter=1000, use_graph=1), joint_inputs),
    "end-effector": (dict(N=64, M=4, A=8, wafr_urdf=1, mpc_mode=1, tol_cost=1e-5, total_time=0.5, ignore_max_rho_exit=0, max_iter=1000, ee_cost=1, use_graph=1), ee_inputs),
}


def column(lib, kw, inputs, B, table):
    s = pyddp.Solver(pyddp.default_config(4, _lib_path=lib, dtype=0, batch=B, **kw), _lib_path=lib)
    if table:
        idx = list(range(B))
        s.set_cost_problems(idx, s.get_cost_problems(idx))
    x0, u0, xg = inputs(kw["N"], np.random.default_rng(1234), B)
    s.load(x0, u0, xg)
    s.set_benchmark_mode(1)
    s.iterate(5); s.sync()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "problem_costs.md"))
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--ee-batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=20)
    a = ap.parse_args()
    lines = ["## Timing: parent library / this tree without a table / this tree with a table of handle-wide rows", "",
             "`tools/problem_costs_time.py`, one process, the columns alternated repetition by repetition (%d repetitions of %d sweeps); ms, medians; spread = max - min of (a)'s own repetitions, IQR = their interquartile range."
             % (a.reps, a.sweeps), ""]
    if not a.parent_lib:
        lines += ["Column (a) was NOT measured (no --parent-lib given).", ""]
    for name, (kw, inputs) in WORKLOADS.items():
        B = a.batch if name == "headline" else a.ee_batch
        cols = {}
        if a.parent_lib:
            cols["a"] = column(a.parent_lib, kw, inputs, B, False)
        cols["b"] = column(None, kw, inputs, B, False)
        cols["c"] = column(None, kw, inputs, B, True)
        sweep = {c: [] for c in cols}
        kern = {c: {} for c in cols}
        for _ in range(a.reps):
            for c, s in cols.items():
                sweep[c].append(s.time_sweeps(a.sweeps, phases=False)[0] / a.sweeps)
        for _ in range(a.reps):
            for c, s in cols.items():
                for nm, ms in s.time_kernels(a.sweeps):
                    if nm:
                        kern[c].setdefault(nm, []).append(ms)
        for s in cols.values():
            s.close()
        med = lambda v: statistics.median(v)
        ref = "a" if "a" in cols else "b"
        lines += ["### %s: arm, N = %d, M = %d, A = %d, float32, %d problems, benchmark mode" % (name, kw["N"], kw["M"], kw["A"], B), "",
                  "| row | (a) parent | spread of (a) | IQR of (a) | (b) no table | (b) - (a) | (c) table | (c) - (a) |", "|---|---|---|---|---|---|---|---|"]

        def row(label, va, vb, vc):
            r = va if va is not None else vb
            spread = max(r) - min(r)
            q = statistics.quantiles(r, n=4) if len(r) >= 2 else [r[0]] * 3
            fa = "%.4f" % med(va) if va is not None else "not measured"
            lines.append("| %s | %s | %.4f%s | %.4f | %.4f | %+.4f | %.4f | %+.4f |" % (label, fa, spread, "" if va is not None else " (of b)", q[2] - q[0], med(vb), med(vb) - med(r), med(vc), med(vc) - med(r)))

        row("sweep (pddp_time_sweeps)", sweep.get("a"), sweep["b"], sweep["c"])
        for nm in kern[ref]:
            row(nm, kern["a"].get(nm) if "a" in cols else None, kern["b"][nm], kern["c"][nm])
        lines.append("")
        print("\n".join(lines[-(len(kern[ref]) + 5):]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else "# Per-problem cost weights\n\n"
    with open(a.out, "w") as f:
        f.write(head + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
