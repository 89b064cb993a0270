#!/usr/bin/env python3
"""What a control cycle of a tracking fleet costs with goal paths against today's way (the caller uploads every cycle's window with the trajectory setter), as a
same-process comparison: handles of the same workload, timed in turn, repetition by repetition (the protocol of tools/goal_trajectory_time.py).

    python tools/goal_path_time.py --parent-lib PATH/libpddp.so [--out profiles/goal_path.md] [--reps 7] [--scale 1.0]

Per workload, wall time in ms of one call sequence on the host clock (everything a caller waits for), medians over --reps repetitions with the spread (max - min);
the variants take turns at leading a repetition:
  path        this tree, every problem on a goal path (WRAP, len = capacity = N + 64, every row of a problem the same numbers): pddp_mpc_solve
  today       this tree, every problem on a plain trajectory: pddp_set_goal_trajectory_problems with the new window (B * N * n numbers from host memory), then pddp_mpc_solve
  plain       the same handle, pddp_mpc_solve alone (the window stays): a handle with plain trajectories only; `setter`: the setter call of `today` alone
  none        this tree, a handle without any trajectory: pddp_mpc_solve
  parent ...  the same three on --parent-lib, a library built from the commit before goal paths, twice (the second handle is the control: two handles of one library
              differ by where their buffers lie, and that difference is part of the margin)
and the stream time of k_goal_window by HIP events (pddp_goal_path_profile) against the bytes it moves, 2 * B * N * n * sizeof(T).
Cycles: shift 1, max_iter 2 of config.max_iter 4, clear_vars 0, no time budget (one synchronisation per cycle), outputs into preallocated arrays.
The named-slot row runs pddp_mpc_solve_problems on 256 slots of the float32 quadrotor handles.
Merge conditions: `plain` and `none` within the margin of the parent's (the larger of |parent 2 - parent| and the parent's own spread); `path` not slower than `today`.
The output file's text in front of the line MARK is kept; everything from MARK on is replaced."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pyddp  # noqa: E402
from diag_costs_time import WORKLOADS, inputs  # noqa: E402

MARK = "<!-- timing: written by tools/goal_path_time.py -->"
WRAP = 2
NAMED = 256


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Fleet:
    """one handle with its inputs and preallocated outputs; cycle() / cycle_named() are the C calls alone"""

    def __init__(self, lib, plant, dtype, B, kw, x0, u0, xg):
        self.s = s = pyddp.Solver(pyddp.default_config(plant, _lib_path=lib, batch=B, max_iter=4, tol_cost=0.0, dtype=dtype, use_graph=1, **kw), _lib_path=lib)
        self.B, self.N, self.n, self.m = B, kw["N"], s.n, s.m
        T = s.dtype
        self.xg, self.xa = np.ascontiguousarray(xg, T), np.ascontiguousarray(x0[:, 1], T)
        self.x0, self.u0 = x0, u0
        self.shift = np.ones(B, np.int32)
        mi = s.cfg.max_iter
        self.out = [np.zeros((B, self.N, self.n), T), np.zeros((B, self.N, self.m), T), np.zeros((B, self.N, self.m, self.n), T), np.zeros((B, mi + 2), T),
                    np.zeros((B, mi + 2), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)]
        self.idx = np.arange(B, dtype=np.int32)
        self.named = np.ascontiguousarray(np.random.default_rng(3).permutation(B)[:NAMED].astype(np.int32))
        s.lib.pddp_mpc_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 7
        s.lib.pddp_mpc_solve_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 7
        s.lib.pddp_set_goal_trajectory_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]

    def seed(self):
        self.s.load(self.x0, self.u0, self.xg)
        self.s.iterate(2); self.s.sync()
        self.cycle(); self.cycle()                                    # warm: staging areas, the graph of an MPC handle

    def cycle(self):
        s = self.s
        s._chk(s.lib.pddp_mpc_solve(s.h, ptr(self.xa), ptr(self.xg), ptr(self.shift), 0, 1, 1, 2, 0.0, 4, *(ptr(a) for a in self.out)))

    def cycle_named(self):
        s, q = self.s, self.named
        if not hasattr(self, "named_in"):
            self.named_in = (np.ascontiguousarray(self.xa[q]), np.ascontiguousarray(self.xg[q]), np.ones(NAMED, np.int32))
        xa, xg, sh = self.named_in
        s._chk(s.lib.pddp_mpc_solve_problems(s.h, NAMED, ptr(q), ptr(xa), ptr(xg), ptr(sh), 0, 1, 1, 2, 0.0, 4, *(ptr(a) for a in self.out)))

    def write_window(self, G, idx):
        s = self.s
        s._chk(s.lib.pddp_set_goal_trajectory_problems(s.h, idx.size, ptr(idx), ptr(G)))


def timed(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "goal_path.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    med = statistics.median
    lines = ["## Timing: a control cycle with goal paths, with caller-written windows, and on the parent commit", "",
             "`tools/goal_path_time.py`, one process, the variants alternated repetition by repetition (%d repetitions); wall ms of the calls on the host clock, medians, spread = max - min." % a.reps, ""]
    if not a.parent_lib:
        lines += ["The parent columns were NOT measured (no --parent-lib given).", ""]
    misses, slower = [], []
    order = [w for w in WORKLOADS if w[1] == 3] + [w for w in WORKLOADS if w[1] != 3]      # configs[4] first
    for name, plant, dtype, batch, kw in order:
        B = max(512, int(batch * a.scale))
        N = kw["N"]
        x0, u0, xg = inputs(plant, N, np.random.default_rng(99), B)
        cap = N + 64
        T = np.float32 if dtype == 0 else np.float64
        n = x0.shape[2]
        # every row of a problem's path is the same (its goal plus an offset of its own): the window holds the same numbers at every cursor, so all handles solve the
        # same problems cycle after cycle and a repetition's times compare -- how long a cycle takes depends on what its problems do (a problem whose backward pass
        # fails is polled on after the iteration limit); what the mover and the upload cost does not depend on the numbers
        path = np.repeat((xg.astype(np.float64) + np.random.default_rng(5).normal(0, 0.01, (B, n)))[:, None, :], cap, axis=1).astype(T)
        wins = [np.ascontiguousarray(path[:, c: c + N]) for c in (1, 2)]      # today's way: two host buffers of the caller's, alternated
        res = {}

        def note(key, ms):
            res.setdefault(key, []).append(ms)

        # ---- group 1: trajectories
        P = Fleet(None, plant, dtype, B, kw, x0, u0, xg)
        P.s.reserve_goal_path(cap)
        P.s.set_goal_path_problems(P.idx, path, WRAP)
        Tt = Fleet(None, plant, dtype, B, kw, x0, u0, xg)
        group = {"path": P, "today": Tt}
        if a.parent_lib:
            group["parent today"] = Fleet(a.parent_lib, plant, dtype, B, kw, x0, u0, xg)
            group["parent 2 today"] = Fleet(a.parent_lib, plant, dtype, B, kw, x0, u0, xg)
        for k, f in group.items():
            if k != "path":
                f.write_window(wins[0], f.idx)
            f.seed()
        P.s.lib.pddp_goal_path_profile.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        P.s._chk(P.s.lib.pddp_goal_path_profile(P.s.h, 1, None))
        kms = np.zeros(1, np.float32)
        named_row = plant == 3 and dtype == 0 and B >= 2 * NAMED
        def rotated(r):                                               # every variant leads a repetition in turn: what ran just before a call is part of its time
            ks = list(group)
            return [(k, group[k]) for k in ks[r % len(ks):] + ks[:r % len(ks)]]

        for r in range(a.reps):
            for k, f in rotated(r):
                if k == "path":
                    note("path", timed(f.cycle))
                    P.s._chk(P.s.lib.pddp_goal_path_profile(P.s.h, -1, ptr(kms)))
                    note("k_goal_window", float(kms[0]))
                else:
                    t_set = timed(lambda: f.write_window(wins[r & 1], f.idx))
                    note(k, t_set + timed(f.cycle))
                    note(k.replace("today", "setter"), t_set)
            for k, f in rotated(r):                                    # (the path handle too: every handle runs the same number of cycles, so their problems stay in step)
                note("path, second cycle" if k == "path" else k.replace("today", "plain"), timed(f.cycle))
            if named_row:
                for k, f in rotated(r):
                    if k == "path":
                        note("named path", timed(f.cycle_named))
                        P.s._chk(P.s.lib.pddp_goal_path_profile(P.s.h, -1, ptr(kms)))
                        note("named k_goal_window", float(kms[0]))
                    else:
                        w = np.ascontiguousarray(wins[r & 1][f.named])
                        t_set = timed(lambda: f.write_window(w, f.named))
                        note("named " + k, t_set + timed(f.cycle_named))
                        note("named " + k.replace("today", "setter"), t_set)
        for f in group.values():
            f.s.close()
        # ---- group 2: no trajectory at all
        group = {"none": Fleet(None, plant, dtype, B, kw, x0, u0, xg)}
        if a.parent_lib:
            group["parent none"] = Fleet(a.parent_lib, plant, dtype, B, kw, x0, u0, xg)
            group["parent 2 none"] = Fleet(a.parent_lib, plant, dtype, B, kw, x0, u0, xg)
        for f in group.values():
            f.seed()
        for r in range(a.reps):
            for k, f in group.items():
                note(k, timed(f.cycle))
        for f in group.values():
            f.s.close()

        spread = lambda v: max(v) - min(v)
        win_bytes = 2.0 * B * N * n * np.dtype(T).itemsize
        lines += ["### %s: N = %d, M = %d, A = %d, RK3, %d problems (window: %.1f MB per cycle)" % (name, N, kw["M"], kw["A"], B, win_bytes / 2e6), "",
                  "| call sequence | this tree | spread | parent | spread | parent, second handle | this tree - parent | margin | inside |", "|---|---|---|---|---|---|---|---|---|"]
        for label, key in (("path: pddp_mpc_solve", "path"), ("path: pddp_mpc_solve, the repetition's second cycle", "path, second cycle"), ("today: setter + pddp_mpc_solve", "today"), ("plain trajectories: pddp_mpc_solve", "plain"), ("no trajectory: pddp_mpc_solve", "none")):
            v = res[key]
            if not key.startswith("path") and a.parent_lib:
                pa, pa2 = res["parent " + key], res["parent 2 " + key]
                margin = max(abs(med(pa2) - med(pa)), spread(pa))
                ok = med(v) - med(pa) <= margin
                if key in ("plain", "none") and not ok:
                    misses.append("%s, %s: this tree %.3f / parent %.3f ms, margin %.3f" % (name, label, med(v), med(pa), margin))
                lines.append("| %s | %.3f | %.3f | %.3f | %.3f | %.3f | %+.3f | %.3f | %s |" % (label, med(v), spread(v), med(pa), spread(pa), med(pa2), med(v) - med(pa), margin, "yes" if ok else "NO"))
            else:
                lines.append("| %s | %.3f | %.3f | n/a | n/a | n/a | n/a | n/a | n/a |" % (label, med(v), spread(v)))
        d = med(res["path"]) - med(res["today"])
        lines += ["", "path - today: %+.3f ms (%.1f %% of today's way).  The setter call alone (today's upload of the window, wall): %.3f ms (spread %.3f)."
                  % (d, 100.0 * d / med(res["today"]), med(res["setter"]), spread(res["setter"]))]
        if d > 0:
            slower.append("%s: path %.3f / today %.3f ms" % (name, med(res["path"]), med(res["today"])))
        k = res["k_goal_window"]
        lines += ["k_goal_window: %.4f ms of stream time (spread %.4f) for %.1f MB read + written: %.0f GB/s." % (med(k), spread(k), win_bytes / 1e6, win_bytes / (med(k) * 1e-3) / 1e9), ""]
        if named_row:
            nb = 2.0 * NAMED * N * n * np.dtype(T).itemsize
            lines += ["Named slots, pddp_mpc_solve_problems on %d of %d slots:" % (NAMED, B), "", "| call sequence | ms | spread |", "|---|---|---|"]
            for label, key in (("path", "named path"), ("today: setter + cycle", "named today"), ("parent: setter + cycle", "named parent today"), ("parent, second handle", "named parent 2 today")):
                if key in res:
                    lines.append("| %s | %.3f | %.3f |" % (label, med(res[key]), spread(res[key])))
            lines += ["", "The setter call alone on the %d slots: %.3f ms (spread %.3f)." % (NAMED, med(res["named setter"]), spread(res["named setter"]))]
            k = res["named k_goal_window"]
            lines += ["", "k_goal_window on the %d slots: %.4f ms (spread %.4f), %.2f MB: %.0f GB/s." % (NAMED, med(k), spread(k), nb / 1e6, nb / (med(k) * 1e-3) / 1e9), ""]
            d = med(res["named path"]) - med(res["named today"])
            if d > 0:
                slower.append("%s, named slots: path %.3f / today %.3f ms" % (name, med(res["named path"]), med(res["named today"])))
        print("\n".join(lines[-26:]), flush=True)
        for key, v in res.items():                                   # the repetitions themselves, for the log
            print("raw %s: %s" % (key, " ".join("%.3f" % t for t in v)), flush=True)
    lines += ["Rows of `plain` / `none` outside the margin of the parent's: " + ("none." if not misses else str(len(misses)) + "."), ""] + ["- " + m for m in misses]
    lines += ["Workloads where the path cycle is slower than today's way: " + ("none." if not slower else str(len(slower)) + "."), ""] + ["- " + m for m in slower]
    print("\n".join(lines[-(len(misses) + len(slower) + 4):]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    head = open(a.out).read().split(MARK)[0] if os.path.exists(a.out) else "# Goal paths\n\n"
    with open(a.out, "w") as f:
        f.write(head + MARK + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
