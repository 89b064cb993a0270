#!/usr/bin/env python3
"""What run-time diagonal cost weights cost the sweeps of the cart-pole and the quadrotor, as a same-process A/B/C: three handles of the same workload, timed in turn,
repetition by repetition (tools/problem_costs_time.py is the arm's).

    python tools/diag_costs_time.py --parent-lib PATH/libpddp.so [--out profiles/diag_costs.md] [--reps 7] [--sweeps 10] [--scale 1.0]

  (a) --parent-lib: a library built from the commit BEFORE pddp_set_diag_cost existed
  (b) this tree's library, no table (the handle never calls a setter): the instantiations on the literals
  (c) this tree's library with a table whose rows are the built-in record (pddp_set_diag_cost with the getter's own answer): the same numbers, read per problem by the
      DiagTab instantiations
  (a2) a second handle of --parent-lib, created last: the control.  The kernels of (a) and (b) that take no weight are the same machine code, and so are (a)'s and
      (a2)'s; what (a2) differs from (a) by is what two handles of one library differ by in this call (where their buffers lie), beside which (b) - (a) is read
Workloads: BASELINE configs[1] (cart-pole N = 128, M = 4, A = 8, RK3, float32, 16384 problems) and configs[4] (quadrotor N = 256, M = 4, A = 16, RK3, float32 with
16384 and float64 with 8192 problems), the shapes and inputs of bench.py's `other_configs` rows, in benchmark mode (no problem exits while it is timed).  --scale shrinks the batches (a smoke run).  Per workload pddp_time_sweeps (ms per
sweep, the graph replay) and pddp_time_kernels (ms per kernel), medians over --reps repetitions with (a)'s own spread (max - min) and interquartile range beside them:
boxes differ by several per cent, so only figures of ONE call compare.  The required property is on column (b): no kernel slower than (a) by more than (a)'s spread;
the last column says so per row.  Column (c) is reported, not bounded.
The output file's text in front of the line MARK (the resource table) is kept; everything from MARK on is replaced."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
import pyddp  # noqa: E402

MARK = "<!-- timing: written by tools/diag_costs_time.py -->"
WORKLOADS = [("configs[1] cart-pole float32", 2, 0, 16384, dict(N=128, M=4, A=8, integrator=3, total_time=4.0)),
             ("configs[4] quadrotor float32", 3, 0, 16384, dict(N=256, M=4, A=16, integrator=3, total_time=4.0)),
             ("configs[4] quadrotor float64", 3, 1, 8192, dict(N=256, M=4, A=16, integrator=3, total_time=4.0))]


def inputs(plant, N, rng, count):
    """bench.py closed_form_inputs: start, nominal control and goal of the example + N(0, 1e-3) noise on the velocities"""
    n, m = {2: (4, 1), 3: (12, 4)}[plant]
    x = np.zeros((count, N, n), np.float32)
    x[:, :, n // 2:] = rng.normal(0, 0.001, (count, N, n // 2)).astype(np.float32)
    if plant == 3:
        x[:, :, 2] = 0.5
    u = np.full((count, N, m), 1.22625 if plant == 3 else 0.01, np.float32)
    g = np.zeros((count, n), np.float32)
    g[:] = {2: [0.0, 3.1416, 0.0, 0.0], 3: [7.0, 10.0, 0.5] + [0.0] * 9}[plant]
    return x, u, g


def column(lib, plant, dtype, B, kw, table):
    s = pyddp.Solver(pyddp.default_config(plant, _lib_path=lib, batch=B, max_iter=1000, tol_cost=0.0, dtype=dtype, use_graph=1, **kw), _lib_path=lib)
    if table:
        s.set_diag_cost(s.get_diag_cost_problems([0])[0])
    x0, u0, xg = inputs(plant, kw["N"], np.random.default_rng(99), B)
    s.load(x0, u0, xg)
    s.set_benchmark_mode(1)                                   # no problem exits: every repetition times sweeps that do the full work
    s.iterate(3); s.sync()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_costs.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    lines = ["## Timing: parent library / this tree without a table / this tree with a table of built-in rows", "",
             "`tools/diag_costs_time.py`, one process, the columns alternated repetition by repetition (%d repetitions of %d sweeps); ms, medians; spread = max - min of (a)'s own repetitions, IQR = their interquartile range."
             % (a.reps, a.sweeps), ""]
    if not a.parent_lib:
        lines += ["Column (a) was NOT measured (no --parent-lib given).", ""]
    for name, plant, dtype, batch, kw in WORKLOADS:
        B = max(64, int(batch * a.scale))
        cols = {}
        if a.parent_lib:
            cols["a"] = column(a.parent_lib, plant, dtype, B, kw, False)
        cols["b"] = column(None, plant, dtype, B, kw, False)
        cols["c"] = column(None, plant, dtype, B, kw, True)
        if a.parent_lib:
            cols["a2"] = column(a.parent_lib, plant, dtype, B, kw, False)      # control: a SECOND handle of the parent's library -- what two handles of the same code differ by
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
        med = statistics.median
        ref = "a" if "a" in cols else "b"
        lines += ["### %s: N = %d, M = %d, A = %d, RK3, %d problems" % (name, kw["N"], kw["M"], kw["A"], B), "",
                  "| row | (a) parent | spread of (a) | IQR of (a) | (b) no table | (b) - (a) | (c) table | (c) - (a) | (b) within (a)'s spread | (a2) parent, second handle | (a2) - (a) |", "|---|---|---|---|---|---|---|---|---|---|---|"]

        def row(label, va, vb, vc, va2=None):
            r = va if va is not None else vb
            spread = max(r) - min(r)
            q = statistics.quantiles(r, n=4) if len(r) >= 2 else [r[0]] * 3
            fa = "%.4f" % med(va) if va is not None else "not measured"
            ok = "n/a" if va is None else ("yes" if med(vb) - med(va) <= spread else "NO")
            ctl = "%.4f | %+.4f" % (med(va2), med(va2) - med(va)) if va2 is not None else "not measured | n/a"
            lines.append("| %s | %s | %.4f%s | %.4f | %.4f | %+.4f | %.4f | %+.4f | %s | %s |" % (label, fa, spread, "" if va is not None else " (of b)", q[2] - q[0], med(vb), med(vb) - med(r), med(vc),
                                                                                               med(vc) - med(r), ok, ctl))

        row("sweep (pddp_time_sweeps)", sweep.get("a"), sweep["b"], sweep["c"], sweep.get("a2"))
        for nm in kern[ref]:
            row(nm, kern["a"].get(nm) if "a" in cols else None, kern["b"][nm], kern["c"][nm], kern["a2"].get(nm) if "a2" in cols else None)
        lines.append("")
        print("\n".join(lines[-(len(kern[ref]) + 5):]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else "# Run-time diagonal cost weights\n\n"
    with open(a.out, "w") as f:
        f.write(head + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
