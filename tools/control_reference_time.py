#!/usr/bin/env python3
"""What the table of control references costs the sweeps of the cart-pole and the quadrotor, as a same-process comparison: four handles of the same workload, timed in
turn, repetition by repetition (the protocol of tools/horizon_time_time.py, which this tool is modelled on).

    python tools/control_reference_time.py --parent-lib PATH/libpddp.so [--out profiles/control_reference.md] [--reps 7] [--sweeps 10] [--scale 1.0]

  (a) --parent-lib: a library built from the commit BEFORE pddp_set_control_reference_problems existed, with the cost, goal and step tables at their defaults
  (b) this tree's library with those three tables and NO reference table (the handle never calls the setter): the StepTab instantiations, which this change does not touch
  (c) this tree's library with every problem flagged on a reference of zeros (the same numbers; the RefTab instantiations fetch a row per knot and subtract it)
  (a2) a second handle of --parent-lib, created last: the control.  (a) and (a2) run the same machine code; what they differ by is what two handles of one library
      differ by in this call, and that difference is the margin (b) - (a) is read against
Workloads: BASELINE configs[1] (cart-pole, float32, 16384 problems) and configs[4] (quadrotor, float32 with 16384 and float64 with 8192 problems) in benchmark mode.
--scale shrinks the batches (a smoke run).  Per workload pddp_time_sweeps (ms per sweep, the graph replay) and pddp_time_kernels (ms per kernel), medians over --reps
repetitions, with (a)'s own spread (max - min) beside them.  Bar 1 is on column (b): no row slower than (a) by more than the larger of |(a2) - (a)| and (a)'s spread.
Column (c) against (b) -- what a reference costs, per kernel -- is reported, not bounded.
The output file's text in front of the line MARK is kept; everything from MARK on is replaced."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyddp  # noqa: E402
from diag_costs_time import WORKLOADS, inputs  # noqa: E402  (WORKLOADS: BASELINE configs[1] and configs[4] as named in the docstring; inputs: their seeded problems)

MARK = "<!-- timing: written by tools/control_reference_time.py -->"


def column(lib, plant, dtype, B, kw, reference_table):
    s = pyddp.Solver(pyddp.default_config(plant, _lib_path=lib, batch=B, max_iter=1000, tol_cost=0.0, dtype=dtype, use_graph=1, **kw), _lib_path=lib)
    s.set_diag_cost(s.get_diag_cost_problems([0])[0])
    x0, u0, xg = inputs(plant, kw["N"], np.random.default_rng(99), B)
    s.set_goal_trajectory_problems([0], np.repeat(xg[:1, None, :], kw["N"], axis=1))      # the goal table, then no problem flagged
    s.clear_goal_trajectory_problems([0])
    s.set_horizon_time_problems(np.arange(B), np.full(B, s.cfg.total_time))                # the step table, every entry the handle's
    if reference_table:
        s.set_control_reference_problems(np.arange(B), np.zeros((B, kw["N"], s.m), s.dtype))      # every problem flagged, every row zero
    s.load(x0, u0, xg)
    s.set_benchmark_mode(1)                                   # no problem exits: every repetition times sweeps that do the full work
    s.iterate(3); s.sync()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "control_reference.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    lines = ["## Timing: parent with a step table / this tree with a step table and no reference table / this tree with every problem on a zero reference", "",
             "`tools/control_reference_time.py`, one process, the columns alternated repetition by repetition (%d repetitions of %d sweeps); ms, medians; spread = max - min of (a)'s own repetitions."
             % (a.reps, a.sweeps), ""]
    if not a.parent_lib:
        lines += ["Column (a) was NOT measured (no --parent-lib given).", ""]
    misses = []
    for name, plant, dtype, batch, kw in WORKLOADS:
        B = max(64, int(batch * a.scale))
        cols = {}
        if a.parent_lib:
            cols["a"] = column(a.parent_lib, plant, dtype, B, kw, False)
        cols["b"] = column(None, plant, dtype, B, kw, False)
        cols["c"] = column(None, plant, dtype, B, kw, True)
        if a.parent_lib:
            cols["a2"] = column(a.parent_lib, plant, dtype, B, kw, False)
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
                  "| row | (a) parent, step table | spread of (a) | (b) step table, no reference table | (b) - (a) | (c) every problem on a zero reference | (c) - (b) | (a2) parent, second handle | (a2) - (a) | (b) within the margin |",
                  "|---|---|---|---|---|---|---|---|---|---|"]

        def row(label, va, vb, vc, va2=None):
            r = va if va is not None else vb
            spread = max(r) - min(r)
            fa = "%.4f" % med(va) if va is not None else "not measured"
            ctl = "%.4f | %+.4f" % (med(va2), med(va2) - med(va)) if va2 is not None else "not measured | n/a"
            if va is None or va2 is None:
                ok = "n/a"
            else:
                ok = "yes" if med(vb) - med(va) <= max(abs(med(va2) - med(va)), spread) else "NO"
                if ok == "NO":
                    misses.append("%s, %s: (a) %.4f / (b) %.4f ms, margin %.4f" % (name, label, med(va), med(vb), max(abs(med(va2) - med(va)), spread)))
            lines.append("| %s | %s | %.4f%s | %.4f | %+.4f | %.4f | %+.4f | %s | %s |" % (label, fa, spread, "" if va is not None else " (of b)", med(vb), med(vb) - med(r), med(vc), med(vc) - med(vb), ctl, ok))

        row("sweep (pddp_time_sweeps)", sweep.get("a"), sweep["b"], sweep["c"], sweep.get("a2"))
        for nm in kern[ref]:
            row(nm, kern["a"].get(nm) if "a" in cols else None, kern["b"][nm], kern["c"][nm], kern["a2"].get(nm) if "a2" in cols else None)
        lines.append("")
        print("\n".join(lines[-(len(kern[ref]) + 5):]), flush=True)
    lines += ["Rows of (b) outside the margin: " + ("none." if not misses else str(len(misses)) + "."), ""] + ["- " + m for m in misses]
    print("\n".join(lines[-(len(misses) + 2):]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else "# Control references\n\n"
    with open(a.out, "w") as f:
        f.write(head + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
