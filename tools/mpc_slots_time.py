#!/usr/bin/env python3
"""What a control cycle for named slots costs (pddp_mpc_solve_problems), next to the two things a caller could do before it existed.

    python tools/mpc_slots_time.py [--out FILE.md] [--lib PATH/libpddp.so] [--batch 4096] [--reps 25]      (profiles/mpc_slots.md: its tables + what they say)

Arm, the MPC example's shape: N = 64, M = 4, A = 8, float32, max_iter = 4, no time budget, full rollout.  A handle of `batch` problems is solved once; every timed call
is a warm-started cycle with shift 1 from knot 1 of the slot's own plan plus a little noise.  For count in {1, 16, 256}:

  slots      pddp_mpc_solve_problems(count) on the big handle, the named slots a random draw: wall time of the C call (outputs preallocated), and its in / cycle / out
             stages (HIP events on the solver's stream, pddp_mpc_slots_profile; a separate series of calls, so that the events do not sit in the wall time)
  small      pddp_mpc_solve on a handle of `count` problems   (every robot, or every group of robots that reports together, a handle of its own)
  whole      pddp_mpc_solve on the big handle                 (a whole-handle cycle whenever anyone reports)

Medians over --reps calls after 3 untimed ones.  --lib runs `small` and `whole` against another build of the library (the commit before this call existed has nothing
else to measure); the binding of THIS tree drives it, the entry points it uses there are old ones."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
import pyddp  # noqa: E402

KW = dict(N=64, M=4, A=8, wafr_urdf=1, mpc_mode=1, total_time=0.5, tol_cost=1e-5, max_iter=4, ignore_max_rho_exit=0)
COUNTS = (1, 16, 256)
MAX_ITER = 4
N, NX, NU = KW["N"], 14, 7


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Cycle:
    """a solved handle of B problems + preallocated inputs / outputs of a cycle for `count` of them"""

    def __init__(self, B, lib_path):
        self.B = B
        self.s = pyddp.Solver(pyddp.default_config(4, dtype=0, batch=B, _lib_path=lib_path, **KW), _lib_path=lib_path)
        rng = np.random.default_rng(7)
        PI = 3.14159
        x0 = np.zeros((B, N, NX), np.float32)
        x0[:, :, :7] = [-0.5 * PI, 0.25 * PI, 0.167 * PI, -0.167 * PI, 0.125 * PI, 0.167 * PI, 0.5 * PI]
        u0 = np.full((B, N, NU), 0.01, np.float32)
        self.goal = np.zeros((B, NX), np.float32)
        self.goal[:, :7] = np.array([0, 0, 0, -0.25 * PI, 0, 0.25 * PI, 0.5 * PI]) + rng.normal(0, 0.05, (B, 7))
        self.plan = self.s.solve(x0, u0, self.goal)["x"]
        self.noise = rng.normal(0, 0.002, (B, NX)).astype(np.float32)
        lib = self.s.lib
        lib.pddp_mpc_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 7
        if hasattr(lib, "pddp_mpc_solve_problems"):
            lib.pddp_mpc_solve_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int] + [C.c_void_p] * 7

    def buffers(self, count):
        o = MAX_ITER + 2
        return [np.zeros((count, N, NX), np.float32), np.zeros((count, N, NU), np.float32), np.zeros((count, N, NX * NU), np.float32), np.zeros((count, o), np.float32),
                np.zeros((count, o), np.int32), np.zeros(count, np.int32), np.zeros(count, np.int32)]

    def whole(self):
        xa = np.ascontiguousarray(self.plan[:, 1] + self.noise)
        shift, out = np.ones(self.B, np.int32), self.buffers(self.B)

        def call():
            rc = self.s.lib.pddp_mpc_solve(self.s.h, ptr(xa), ptr(self.goal), ptr(shift), 0, 1, 1, MAX_ITER, 0.0, MAX_ITER, *[ptr(a) for a in out])
            assert rc == 0, self.s.lib.pddp_last_error()
        return call

    def slots(self, idx):
        idx = np.ascontiguousarray(idx, np.int32)
        xa, goal = np.ascontiguousarray(self.plan[idx, 1] + self.noise[idx]), np.ascontiguousarray(self.goal[idx])
        shift, out = np.ones(idx.size, np.int32), self.buffers(idx.size)

        def call():
            rc = self.s.lib.pddp_mpc_solve_problems(self.s.h, idx.size, ptr(idx), ptr(xa), ptr(goal), ptr(shift), 0, 1, 1, MAX_ITER, 0.0, MAX_ITER, *[ptr(a) for a in out])
            assert rc == 0, self.s.lib.pddp_last_error()
        return call


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def stages_ms(c, fn, reps):
    c.s.mpc_slots_profile(timing=1)
    for _ in range(3):
        fn()
    rows = []
    for _ in range(reps):
        fn(); rows.append(c.s.mpc_slots_profile())
    c.s.mpc_slots_profile(timing=0)
    return np.median(np.asarray(rows), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=25)
    a = ap.parse_args()
    assert a.reps >= 20
    lib_path = a.lib or pyddp.library_path()
    what = "another build of the library (%s)" % os.path.relpath(lib_path, ROOT) if a.lib else "this tree"
    lines = ["# Control cycles for named slots (tools/mpc_slots_time.py): %s\n\n" % what,
             "Arm, float32, N = %d, M = %d, A = %d, max_iter = %d, no budget, shift 1, full rollout; handle of %d problems; ms, medians of %d calls after 3 untimed ones.\n\n" % (N, KW["M"], KW["A"], MAX_ITER, a.batch, a.reps)]
    big = Cycle(a.batch, lib_path)
    have = hasattr(big.s.lib, "pddp_mpc_solve_problems") and not a.lib
    t_whole = median_ms(big.whole(), a.reps)
    print("pddp_mpc_solve on the %d-problem handle: %.3f ms" % (a.batch, t_whole), flush=True)
    rows = []
    for count in COUNTS:
        small = Cycle(count, lib_path)
        t_small = median_ms(small.whole(), a.reps)
        small.s.close()
        r = dict(count=count, small=t_small)
        if have:
            call = big.slots(np.random.default_rng(count).permutation(a.batch)[:count])
            r["slots"] = median_ms(call, a.reps)
            r["stages"] = stages_ms(big, call, a.reps)
        rows.append(r)
        print(r, flush=True)
    big.s.close()
    if have:
        lines += ["| count | `pddp_mpc_solve_problems`, wall | in | cycle | out | `pddp_mpc_solve`, handle of `count` | `pddp_mpc_solve`, handle of %d |\n|---|---|---|---|---|---|---|\n" % a.batch]
        lines += ["| %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f |\n" % (r["count"], r["slots"], r["stages"][0], r["stages"][1], r["stages"][2], r["small"], t_whole) for r in rows]
        lines += ["\nin / cycle / out: stream time between HIP events (in = movers + load stage kernel; cycle = initial cost, setup, %d sweeps, fall-back and result records; out = movers).\n" % MAX_ITER]
    else:
        lines += ["| count | `pddp_mpc_solve`, handle of `count` | `pddp_mpc_solve`, handle of %d |\n|---|---|---|\n" % a.batch]
        lines += ["| %d | %.3f | %.3f |\n" % (r["count"], r["small"], t_whole) for r in rows]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(lines)
    print("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
