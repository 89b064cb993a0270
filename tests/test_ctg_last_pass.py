"""Interior cost-to-go slots are written only by the passes a caller can observe: one iterate(n) == n calls of iterate(1), bit for bit.

Between two calls that enqueue sweeps a caller can read both halves of the cost-to-go double buffer: the interiors of every problem's last two backward passes.  A call
that enqueues n sweeps (pddp_iterate(n), a chunk of pddp_solve, an MPC cycle) therefore keeps every slot in its last two sweeps; in the sweeps in front of them the
matrix-core backward pass leaves the interior [P | p] out for the problems that provably run on for two more sweeps (no exit by max_iter or by the maximum rho within
two sweeps; handles on which an exit by tolerance is impossible: tol_cost <= 0, no negative cost weight).

The yardstick is the same build driven so that every pass keeps: iterate(1) enqueues one sweep, which is its call's last, so a handle advanced by single-sweep calls
writes every slot in every pass -- the behaviour before the split.  Everything a caller can read afterwards must be the same bits (np.array_equal, NaNs equal): both
halves of the cost-to-go double buffer, x, u, KT, du, Jout, alphaOut, dmax, dJexp and the solver states.

Shapes (the smallest at which the knot loop's branches differ): float32 with the benched kernels at N = 32 and N = 16 (M = 4: blocks of 8 and 4 knots), M = 1, 70 problems
(a ragged last wavefront of the line search), one problem on the library's own selection (line search inside the rollout kernel k_fp_tl4), and one float64 handle with
bp = "mx".  The single-problem shape has nobody to be "still running", so where a case asks for a mix of exits it asks that problem to exit strictly inside the chunk.
The cases with a positive tolerance hold the other side of the rule: such a handle must go on keeping every slot in every pass.
"""
import os
import sys

import numpy as np
import pytest

import pyddp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from bench import example_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

KRHOMAX = 10000000.0                                            # solver_state.hpp kRhoMax
BENCHED = dict(bp="mx", fp="tl")
SHAPES = {
    "f32-N32-M4-b70": dict(dtype=0, N=32, M=4, batch=70, kernels=BENCHED),
    "f32-N16-M4-b70": dict(dtype=0, N=16, M=4, batch=70, kernels=BENCHED),
    "f32-N32-M1-b70": dict(dtype=0, N=32, M=1, batch=70, kernels=BENCHED),
    "f32-N32-M4-b1-auto": dict(dtype=0, N=32, M=4, batch=1, kernels=None),
    "f64-N32-M4-b70": dict(dtype=1, N=32, M=4, batch=70, kernels=dict(bp="mx")),
}
STATE_FIELDS = ("done", "iter", "rho", "drho", "prevJ", "dJ", "z", "alphaIndex", "ignore_defect", "accepted", "cur", "cur2", "bp_retries", "pw")
ARRAYS = ("P", "p", "Pp", "pp", "du", "dJexp")


def make(shape, **over):
    sh = dict(SHAPES[shape])
    kw = dict(A=8, wafr_urdf=1, total_time=0.5, tol_cost=0.0, max_iter=40)
    kw.update(sh); kw.update(over)
    s = pyddp.Solver(pyddp.default_config(4, **kw))
    return s


def inputs(shape, seed=11):
    """bench.example_inputs with per-problem noise: the velocity noise of problem i is scaled by a factor between 1 and 60, so the problems converge at different rates"""
    sh = SHAPES[shape]
    B, N = sh["batch"], sh["N"]
    x, u, g = example_inputs(N, np.random.default_rng(seed), B)
    scale = np.geomspace(1.0, 60.0, B).astype(np.float32)
    np.random.default_rng(seed + 1).shuffle(scale)
    x[:, :, 7:] *= scale[:, None, None]
    T = np.float32 if sh["dtype"] == 0 else np.float64
    return x.astype(T), u.astype(T), g.astype(T)


def states(s):
    st = s.get_state()
    return {f: np.array([getattr(v, f) for v in st]) for f in STATE_FIELDS}


def snapshot(s):
    s.sync()
    out = dict(s.store())
    for k in ARRAYS:
        out[k] = s.get(k)
    out.update({"state." + f: v for f, v in states(s).items()})
    return out


def assert_same(ref, got, what):
    assert ref.keys() == got.keys()
    bad = [k for k in ref if not np.array_equal(ref[k], got[k], equal_nan=ref[k].dtype.kind == "f")]
    assert not bad, f"{what}: {bad} differ between single-sweep calls and chunked calls"


def check_selection(s):
    """the handle runs the matrix-core backward pass (on a scratch handle: time_kernels advances the solve)"""
    names = [nm for nm, _ in s.time_kernels(1)]
    assert "k_bp_mfma" in names, names
    return names


def run(shape, chunks, over=None, probe=None):
    """(reference snapshot, subject snapshot, per-sweep `done` of the reference [sweeps][B]).  chunks: the subject's iterate() calls; the reference runs their sum in
    single-sweep calls."""
    x, u, g = inputs(shape)
    ref, sub = make(shape, **(over or {})), make(shape, **(over or {}))
    try:
        ref.load(x, u, g); sub.load(x, u, g)
        trace = []
        for _ in range(sum(chunks)):
            ref.iterate(1)
            if probe is not None:
                ref.sync(); trace.append(probe(ref))
        for c in chunks:
            sub.iterate(c)
        return snapshot(ref), snapshot(sub), trace
    finally:
        ref.close(); sub.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_selection_is_the_matrix_core_pass(shape):
    s = make(shape)
    try:
        s.load(*inputs(shape))
        names = check_selection(s)
        if SHAPES[shape]["kernels"] is None:
            assert "k_fp_tl4" in names and not any(n.startswith("k_ls") for n in names), names      # the line search runs inside the rollout kernel
    finally:
        s.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_no_exit(shape):
    ref, sub, tr = run(shape, [12], probe=lambda s: states(s)["done"].copy())
    assert not np.any(tr[-1]), "mis-configured: no problem may exit in this case"
    assert_same(ref, sub, "iterate(12)")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_chunks(shape):
    ref, sub, _ = run(shape, [3, 5])
    assert_same(ref, sub, "iterate(3); iterate(5)")


def tol_candidates(shape, n):
    """tol_cost candidates from a single-sweep handle's own run with tol_cost = 0: the relative decreases of its accepted iterations, sweep by sweep.  A problem leaves at
    the first accepted sweep whose decrease is below the tolerance; the candidates sit 20 % above observed decreases, and those predicted to meet the case's condition
    come back ordered by the number of different sweeps the exits fall on.  (A prediction only: the handle under test starts from prevJ = J + 2 tol_cost, so the case
    itself is judged on the reference handle's own trace.)"""
    x, u, g = inputs(shape)
    s = make(shape)
    try:
        s.load(x, u, g)
        acc, dJ = [], []
        for _ in range(n):
            s.iterate(1); s.sync()
            st = states(s)
            acc.append(st["accepted"] == 1); dJ.append(st["dJ"].astype(np.float64))
    finally:
        s.close()
    acc, dJ = np.array(acc), np.array(dJ)                       # [n][B]
    B = acc.shape[1]
    found = []
    for tol in np.unique(dJ[acc]) * 1.2:
        hit = acc & (dJ < tol)
        first = np.where(hit.any(axis=0), hit.argmax(axis=0), n)                      # sweep index (0-based) of the exit; n: still running after n sweeps
        early, running = int(np.sum(first < n - 1)), int(np.sum(first >= n - 1))      # exits strictly before sweep n | still running when sweep n starts
        if (early >= -(-B // 4) + 2 and running >= 3) if B > 1 else early == 1:
            found.append((len(np.unique(first[first < n - 1])) if B > 1 else -abs(int(first[0]) - n // 2), float(tol)))
    return [t for _, t in sorted(found, reverse=True)][:5]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_exit_by_tolerance_inside_a_chunk(shape):
    """The handle-unchanged side of the rule: with tol_cost > 0 an exit cannot be foreseen, so such a handle enqueues no lean sweep at all and this case runs no new
    kernel code -- it holds that the split stays OFF there (a lean pass in front of one of these exits would leave a stale interior in one of the halves)."""
    n = 12
    seen = []
    for tol in tol_candidates(shape, n):
        ref, sub, tr = run(shape, [n], over=dict(tol_cost=tol), probe=lambda s: states(s)["done"].copy())
        tr = np.array(tr)                                       # [n][B] done after sweep i + 1
        B = tr.shape[1]
        early, running = int(np.sum(tr[n - 2] != 0)), int(np.sum(tr[n - 2] == 0))      # exited strictly before sweep n | still running at sweep n
        seen.append((tol, early, running))
        if early >= max(1, -(-B // 4)) and (running >= 1 or B == 1):
            assert np.all(tr[n - 2][tr[n - 2] != 0] == 1)
            assert_same(ref, sub, f"iterate({n}) with tol_cost {tol}")
            return
    pytest.fail(f"mis-configured: no tolerance makes a quarter of the problems exit before sweep {n} with one still running: (tol, exited, running) {seen}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_exit_by_max_iter_inside_the_chunk(shape):
    n = 9
    ref, sub, tr = run(shape, [n], over=dict(max_iter=n - 3), probe=lambda s: states(s)["done"].copy())
    assert np.all(tr[-1] == 2) and not np.any(tr[n - 5]), "mis-configured: every problem exits by max_iter at sweep n - 3"
    assert_same(ref, sub, f"iterate({n}) with max_iter {n - 3}")


@pytest.mark.parametrize("below", [1.25, 6.0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exit_by_max_rho(shape, below):
    # rho_init a factor 1.25 below kRhoMax: one rejection ends a problem.  Rejections need no staging: at this regularisation the steps are so short that the actual
    # decrease falls outside the acceptance window (the host emulation rejects every line search), and the reference handle has to show it.  A factor 6 below: the growing
    # factor of rho_increase (1.25, 1.5625, 1.95, 2.44) reaches the maximum at the fourth rejection, so the first two passes see no exit within two sweeps.
    n = 6
    ref, sub, tr = run(shape, [n], over=dict(ignore_max_rho_exit=0, rho_init=KRHOMAX / below), probe=lambda s: states(s)["done"].copy())
    tr = np.array(tr)
    assert np.any(ref["state.done"] == 3), "mis-configured: no problem of the reference handle exits by max rho"
    assert np.any(tr[n - 2] == 3), "mis-configured: no problem exits by max rho strictly inside the chunk"
    if below > 2:
        assert not np.any(tr[1]) and np.any(tr[3] == 3), "mis-configured: the exits by max rho come at the fourth sweep"
    assert_same(ref, sub, f"iterate({n}) from rho_init = kRhoMax / {below}")


@pytest.mark.parametrize("shape", ["f32-N32-M4-b70", "f32-N32-M4-b1-auto"])
def test_reload_after_an_exit(shape):
    x, u, g = inputs(shape)
    x2, u2, g2 = inputs(shape, seed=23)
    over = dict(max_iter=4)                                     # every problem exits at sweep 4 of 6: in front of the call's last two sweeps
    ref, sub = make(shape, **over), make(shape, **over)
    try:
        for s, chunks in ((ref, [1] * 6), (sub, [6])):
            s.load(x, u, g)
            for c in chunks:
                s.iterate(c)
        first = snapshot(ref), snapshot(sub)
        assert np.all(first[0]["state.done"] == 2)
        assert_same(first[0], first[1], "first solve")
        for s, chunks in ((ref, [1] * 6), (sub, [6])):
            s.load(x2, u2, g2)
            for c in chunks:
                s.iterate(c)
        second = snapshot(ref), snapshot(sub)
        assert np.all(second[0]["state.done"] == 2)
        assert_same(second[0], second[1], "second solve, after the reload")
        assert not np.array_equal(first[0]["P"], second[0]["P"])
    finally:
        ref.close(); sub.close()


@pytest.mark.parametrize("tol,per_cycle", [(0.0, 4), (0.0, 6), (1e-5, 4)], ids=["fixed-budget-4", "fixed-budget-6", "tolerance-1e-5"])
def test_mpc_cycles(tol, per_cycle):
    """Three control cycles at the published MPC shape (N = 64, end-effector cost, 4 iterations per cycle; 6 as well).  poll_every = 1 makes the cycle enqueue its sweeps
    one per call (every pass keeps); poll_every = per_cycle enqueues the cycle's whole budget in one call.  tol_cost = 0 (a fixed budget per cycle) is the handle on
    which that call splits: the cycle's iteration limit is the lowered max_iter the lean passes are launched with, so of 4 sweeps the first two are lean (iter 1, 2 <
    max_iter - 1) and the warm start of the next cycle shifts both halves of a double buffer that lean sweeps have written to.  tol_cost = 1e-5: the published setting,
    no split."""
    B, N, n = 6, 64, 14
    kw = dict(N=N, wafr_urdf=1, mpc_mode=1, ee_cost=1, tol_cost=tol, max_iter=10, ignore_max_rho_exit=0, batch=B, dtype=0, kernels=BENCHED)
    rng = np.random.default_rng(3)
    x0 = np.zeros((B, N, n), np.float32); x0[:, :, 1] = 0.7; x0[:, :, 3] = -0.8; x0[:, :, 5] = 0.75
    x0[:, :, 7:] = rng.normal(0, 0.01, (B, N, 7)) * np.geomspace(1, 20, B)[:, None, None]
    u0 = np.full((B, N, 7), 0.01, np.float32)
    C = 3
    goals = np.zeros((C, B, n), np.float32)
    goals[:, :, :3] = np.array([0.45, 0.15, 0.75]) + rng.normal(0, 0.05, (C, B, 3))
    noise = rng.normal(0, 0.004, (C, B, n)).astype(np.float32)
    ref, sub = (pyddp.Solver(pyddp.default_config(4, **kw)) for _ in range(2))
    try:
        check = pyddp.Solver(pyddp.default_config(4, **kw))
        try:
            check.load(x0, u0, goals[0]); check_selection(check)
        finally:
            check.close()
        plans = []
        for s in (ref, sub):
            plans.append(s.solve(x0, u0, goals[0], chunk=1 if s is ref else 8)["x"])
        assert np.array_equal(plans[0], plans[1])
        for c in range(C):
            xa = (plans[0][:, 1] + noise[c]).astype(np.float32)
            want = ref.mpc_solve(xa, goals[c], 1, max_iter=per_cycle, poll_every=1)
            got = sub.mpc_solve(xa, goals[c], 1, max_iter=per_cycle, poll_every=per_cycle)
            if tol == 0.0:
                assert np.all(want["iters"] == per_cycle) or np.any(snapshot(ref)["state.done"] == 3), "mis-configured: a fixed budget runs every cycle to its limit"
            for k in want:
                assert np.array_equal(want[k], got[k], equal_nan=want[k].dtype.kind == "f"), (c, k)
            assert_same(snapshot(ref), snapshot(sub), f"cycle {c}")
            plans = [want["x"], got["x"]]
        # every later cycle's warm start shifted every [P | p] slot of the one before: its outputs are compared above
    finally:
        ref.close(); sub.close()
