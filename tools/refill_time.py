#!/usr/bin/env python3
"""What refilling slots costs and what it buys (pddp_load_problems / pddp_store_problems / pyddp.solve_stream).  Arm, float32, N = 64, M = 4, A = 8.

    python tools/refill_time.py [--out profiles/refill.md] [--stream-batch 4096]

(a) wall time of pddp_load_problems(count = 64) into handles of 256 and 4096 problems, next to pddp_load of a whole 64-problem handle: the two refill figures show
    whether the cost follows `count` and not `batch`;
(b) pddp_store_problems(count = 64) next to pddp_store, on the 4096-problem handle;
(c) problems per second for a stream of 4 * batch problems whose exit iterations are spread (noise levels and goal distances drawn from the recipes of
    tests/test_mixed_states.py ARM_RECIPE, kinds a, b, c; tol_cost = 5e-3, max_iter = 20): once through solve_stream, once as four full waves of pddp_solve -- what the
    handle could do before the two calls existed, through unchanged code.
Every figure of (a), (b) is the median over the repetitions of the time between entering and leaving the Python call, after one untimed warm-up call (the first refill
also creates the intake area); (c) is one pass each, after a warm-up wave."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyddp  # noqa: E402
from test_mixed_states import ARM_RECIPE, make_problem  # noqa: E402

KW = dict(N=64, M=4, A=8, wafr_urdf=1, total_time=0.5, tol_cost=5e-3, max_iter=20, ignore_max_rho_exit=0)
DISTINCT = 128


def solver(B):
    return pyddp.Solver(pyddp.default_config(4, dtype=0, batch=B, **KW))


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def problems(count):
    """`count` problems: DISTINCT different ones (kind, noise and goal drawn from the recipes), repeated in a shuffled order"""
    rng = np.random.default_rng(11)
    entries = [(k, e) for k in "abc" for e in ARM_RECIPE[k]]
    base = []
    for i in range(DISTINCT):
        kind, (noise, goal, _) = entries[rng.integers(len(entries))]
        p = make_problem(4, KW, 0, kind, noise, goal, 0, 50000 + i)
        base.append((p["x0"], p["u0"], p["xg"]))
    return [base[i] for i in rng.integers(DISTINCT, size=count)]


def stacked(probs):
    return tuple(np.concatenate([p[k] for p in probs]) for k in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refill.md"))
    ap.add_argument("--stream-batch", type=int, default=4096)
    a = ap.parse_args()
    lines = ["# Refilling slots of a running batch (tools/refill_time.py)\n", "Arm, float32, N = %d, M = %d, A = %d; wall time of the Python call in ms, median over repetitions.\n" % (KW["N"], KW["M"], KW["A"])]
    count = 64
    some = problems(count)
    x64, u64, g64 = stacked(some)
    # ---- (a)
    s64 = solver(count)
    t_load = median_ms(lambda: s64.load(x64, u64, g64), 20)
    s64.close()
    refill = {}
    handles = {}
    for B in (256, 4096):
        s = solver(B)
        fill = stacked([some[i % count] for i in range(B)])
        s.load(*fill)
        s.iterate(8); s.sync()
        idx = np.random.default_rng(B).permutation(B)[:count]
        refill[B] = median_ms(lambda: s.load_problems(idx, x64, u64, g64), 20)
        handles[B] = (s, idx)
        print("pddp_load_problems(count = 64) into a handle of %4d: %.3f ms   (pddp_load of a 64-problem handle: %.3f ms)" % (B, refill[B], t_load), flush=True)
    lines += ["\n## (a) loading 64 problems\n\n| call | ms |\n|---|---|\n", "| `pddp_load` of a whole 64-problem handle | %.3f |\n" % t_load]
    lines += ["| `pddp_load_problems(count = 64)` into a handle of %d problems | %.3f |\n" % (B, refill[B]) for B in (256, 4096)]
    # ---- (b)
    s, idx = handles[4096]
    t_rows = median_ms(lambda: s.store_problems(idx), 20)
    t_all = median_ms(lambda: s.store(), 5)
    print("pddp_store_problems(count = 64): %.3f ms   pddp_store of the 4096-problem handle: %.3f ms" % (t_rows, t_all), flush=True)
    lines += ["\n## (b) fetching results from the 4096-problem handle\n\n| call | ms |\n|---|---|\n", "| `pddp_store_problems(count = 64)` | %.3f |\n" % t_rows,
              "| `pddp_store` (all 4096 problems) | %.3f |\n" % t_all]
    for h, _ in handles.values():
        h.close()
    # ---- (c)
    B = a.stream_batch
    probs = problems(4 * B)
    s = solver(B)
    waves = [stacked(probs[w * B: (w + 1) * B]) for w in range(4)]
    s.solve_timed(*waves[0])                                   # warm-up: graph capture, first-use allocations
    t0 = time.perf_counter()
    wave_iters = []
    for w in range(4):
        r = s.solve_timed(*waves[w])
        wave_iters.append(np.asarray(r["iters"]).copy())
    t_waves = time.perf_counter() - t0
    wave_iters = np.concatenate(wave_iters)
    list(pyddp.solve_stream(s, probs[:B], sweeps_per_poll=4))  # warm-up of the refill path (intake area)
    t0 = time.perf_counter()
    got = dict(pyddp.solve_stream(s, probs, sweeps_per_poll=4))
    t_stream = time.perf_counter() - t0
    stream_iters = np.array([got[i]["iters"] for i in range(4 * B)])
    s.close()
    same = bool((stream_iters == wave_iters).all())
    q = [int(v) for v in np.percentile(wave_iters, [0, 25, 50, 75, 100])]
    print("stream of %d problems through %d slots: solve_stream %.1f ms = %.0f problems/s, four waves of pddp_solve %.1f ms = %.0f problems/s; same exit iterations: %s; "
          "exit iterations min / quartiles / max %s" % (4 * B, B, t_stream * 1e3, 4 * B / t_stream, t_waves * 1e3, 4 * B / t_waves, same, list(q)), flush=True)
    lines += ["\n## (c) a stream of %d problems through a handle of %d slots\n\n" % (4 * B, B),
              "tol_cost = 5e-3, max_iter = 20; exit iterations of the problems: min / quartiles / max = %s; the two ways end every problem at the same iteration: %s.\n\n" % (list(q), "yes" if same else "NO"),
              "| way | wall time, ms | problems / s |\n|---|---|---|\n", "| `pyddp.solve_stream` (sweeps_per_poll = 4) | %.1f | %.0f |\n" % (t_stream * 1e3, 4 * B / t_stream),
              "| four full waves of `pddp_solve` | %.1f | %.0f |\n" % (t_waves * 1e3, 4 * B / t_waves)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.writelines(lines)
    return 0


if __name__ == "__main__":
    sys.exit(main())
