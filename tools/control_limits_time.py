#!/usr/bin/env python3
"""What control limits cost a backward pass and the rollouts, as a same-process comparison of handles of this tree's library timed in turn, repetition by repetition.

    python tools/control_limits_time.py [--out FILE] [--reps 7] [--sweeps 10] [--scale 1.0] [--only-hover]

Per workload two handles: (a) no limit table -- the selection's own kernels (quadrotor: k_bp_mq, and with kernels.cf_bp = cl k_bp_cl; cart-pole: k_bp_ts) and the
RefTab-free rollouts --, (b) every problem at infinite limits -- k_bp_box, the LimTab rollouts, the per-knot sweep.  Infinite limits clamp nothing, so (b) computes
what (a) computes and the difference is the price of the path, not of a different solve.  Workloads: 16384 quadrotor problems, N = 256, M = 4, A = 16, float and
double; 16384 cart-pole problems, N = 128, float.  --scale shrinks the batches (a smoke run).  pddp_time_kernels, medians over --reps repetitions of --sweeps sweeps;
slot 0 of (b) carries the SELECTION's name (include/pddp.h) and is k_bp_box's time where the handle's limits do not run on k_bp_mq.

The last table (hover_rows) is the full-device quadrotor with limits that BIND: every problem's upper limit at 1.3 x hover, benchmark mode (no problem exits), against
the same handle without a table -- per slot and per sweep.  Another commit's figures come from this script run on that commit's build in a process of its own, the
two alternating (two builds of the library in one process share their kernel stubs' names: the second one's launches look their kernels up in the first one's code)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyddp  # noqa: E402
from diag_costs_time import inputs  # noqa: E402  (seeded problems of a plant)

WORKLOADS = [("quadrotor f32 mq", 3, 0, 16384, dict(N=256, M=4, A=16, integrator=3), {}), ("quadrotor f32 cl", 3, 0, 16384, dict(N=256, M=4, A=16, integrator=3), dict(cf_bp="cl")),
             ("quadrotor f64 mq", 3, 1, 16384, dict(N=256, M=4, A=16, integrator=3), {}), ("cart-pole f32 ts", 2, 0, 16384, dict(N=128, M=4, A=16, integrator=3), {})]


def handle(plant, dtype, B, kw, sel, limits):
    s = pyddp.Solver(pyddp.default_config(plant, batch=B, max_iter=1000, tol_cost=0.0, dtype=dtype, use_graph=1, kernels=sel, **kw))
    if limits:
        m = s.m
        s.set_control_limits(np.arange(B), np.tile(np.concatenate([np.full(m, -np.inf), np.full(m, np.inf)]), (B, 1)))
    x0, u0, xg = inputs(plant, kw["N"], np.random.default_rng(99), B)
    s.load(x0, u0, xg)
    s.iterate(2)
    s.sync()
    return s


def hover_rows(a):
    """16384 quadrotor problems at BASELINE configs[4]'s geometry: a handle without a table and one with hi = 1.3 x hover on every problem"""
    plant, B, kw = 3, max(64, int(16384 * a.scale)), dict(N=256, M=4, A=16, integrator=3)
    hs = []
    for limited in (False, True):
        s = pyddp.Solver(pyddp.default_config(plant, batch=B, max_iter=1000, tol_cost=0.0, dtype=0, use_graph=1, **kw))
        if limited:
            s.set_control_limits(np.arange(B), np.tile(np.concatenate([np.full(s.m, -np.inf), np.full(s.m, 1.3 * 9.81 / 8)]), (B, 1)))
        x0, u0, xg = inputs(plant, kw["N"], np.random.default_rng(99), B)
        s.load(x0, u0, xg)
        s.set_benchmark_mode(1)
        s.iterate(3); s.sync()
        hs.append(("hi = 1.3 x hover" if limited else "no table", s))
    runs = [[] for _ in hs]
    for _ in range(a.reps):
        for i, (_, s) in enumerate(hs):
            runs[i].append(s.time_kernels(a.sweeps))
    lines = [f"quadrotor f32, {B} problems, N 256, M 4, A 16: the named slots of one sweep, ms; ms per sweep", ""]
    for (name, s), r in zip(hs, runs):
        med = [statistics.median(x[slot][1] for x in r) for slot in range(len(r[0]))]
        lines.append(f"| {name} | " + " | ".join(f"{r[0][slot][0]} {med[slot]:.4f}" for slot in range(len(r[0]))) + f" | {statistics.median(sum(t for _, t in x) for x in r):.4f} |")
        s.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--sweeps", type=int, default=10); ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only-hover", action="store_true")
    a = ap.parse_args()
    lines = ["| workload | slot | kernel (no table) | ms | with limits: ms |", "|---|---|---|---|---|"]
    for name, plant, dtype, B, kw, sel in ([] if a.only_hover else WORKLOADS):
        B = max(64, int(B * a.scale))
        hs = [handle(plant, dtype, B, kw, sel, lim) for lim in (False, True)]
        runs = [[], []]
        for _ in range(a.reps):
            for i, s in enumerate(hs):
                runs[i].append(s.time_kernels(a.sweeps))
        for slot, (nm, _) in enumerate(runs[0][0]):                  # (the named slots of one sweep, in launch order)
            med = [statistics.median(r[slot][1] for r in runs[i]) for i in (0, 1)]
            lines.append(f"| {name}, {B} problems | {slot} | {nm} | {med[0]:.4f} | {med[1]:.4f} |")
        for s in hs:
            s.close()
    lines += [""] + hover_rows(a)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
