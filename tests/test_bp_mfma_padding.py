"""The matrix-core backward pass reads the zeros of its tiles instead of selecting them: a padding lane must never see a neighbour's data.

The LDS-prefetching instantiations of k_bp_mfma (float, compact [A B]) point every lane whose tile element must be zero -- or the cost Hessian's diagonal weight -- at
constant cells of the wave's operand buffer, decided once per lane (csrc/bp_mfma.hpp, mx_lds_knot / mx_cost_base).  A wrong address there does not fault: it reads the
next column, the next knot or -- the compact [A B] keeps 64 knots of consecutive problems in one chunk -- the next problem.  So:

* neighbour poisoning: problem 1 of three is the example input, problems 0 and 2 the same input scaled by +1e3 and -1e3 (finite, and a thousand times anything problem 1
  holds).  Everything a caller can read of problem 1 is, bit for bit, what the same problem gives alone in a one-problem handle pinned to the same kernels -- for
  M = 4 / 2 / 1 (fused sweep maps, forward-sweep operands, single shooting), with every pass keeping the interior cost-to-go, with no pass keeping it
  (boundary_cost_to_go_only) and with lean passes followed by keeping ones (tol_cost = 0, iterate(4)); once with the end-effector cost (the compact position block).
* first and last knot of a block: at N = 8 and N = 16 with M = 4 every knot is a block's first or last one; the gains K | du are held under the float32 bar of
  tests/test_fp32_bar.py for this kernel, with that file's own machinery (the float32 evaluations of the reference pass it is measured against include the one the
  lane-group pass reproduces bit for bit).
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import pyddp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from bench import ee_inputs, example_inputs  # noqa: E402
from test_fp32_bar import KUKA, run_bar  # noqa: E402

pytestmark = pytest.mark.gpu

BENCHED = dict(bp="mx", fp="tl")                                # the large-batch selection bench.py runs; it can be pinned onto one problem
KEYS = ("x", "u", "KT", "Jout", "alphaOut", "P", "p")
MODES = {
    "every-pass-keeps": (dict(tol_cost=1e-5), 3),               # a positive tolerance: no lean pass is ever enqueued
    "no-pass-keeps": (dict(tol_cost=1e-5, boundary_cost_to_go_only=1), 3),
    "lean-then-keeping": (dict(tol_cost=0.0), 4),               # iterate(4): two lean sweeps in front of the call's last two
}


def config(N, M, batch, ee, over):
    kw = dict(N=N, M=M, A=2, wafr_urdf=1, total_time=0.5, max_iter=12, batch=batch, dtype=0, kernels=BENCHED)
    if ee:
        kw.update(ee_cost=1, mpc_mode=1, ignore_max_rho_exit=0)
    kw.update(over)
    return pyddp.default_config(4, **kw)


def three_problems(N, ee):
    """problem 1: the example input; problems 0 and 2: the same scaled by +1e3 / -1e3 (different from each other, finite)"""
    x, u, g = (ee_inputs if ee else example_inputs)(N, np.random.default_rng(5), 1)
    x, u, g = (np.repeat(a, 3, axis=0) for a in (x, u, g))
    for b, f in ((0, 1e3), (2, -1e3)):
        x[b] *= np.float32(f); u[b] *= np.float32(f)
    assert np.isfinite(x).all() and np.isfinite(u).all()
    return x, u, g


def kernel_names(cfg, x, u, g):
    """(kernel names of one sweep, which of the compact arrays ABc / Hc the handle keeps) -- on a scratch handle: time_kernels advances the solve.  pddp_time_kernels
    reports bare names; which instantiation of k_bp_mfma a float handle launches follows from the arrays (mx_launch: compact [A B] <=> ABc, the position block <=> Hc)."""
    s = pyddp.Solver(cfg)
    try:
        s.load(x, u, g)
        have = []
        for name in ("ABc", "Hc"):
            nb = ctypes.c_size_t(0)
            have.append(s.lib.pddp_array_bytes(s.h, name.encode(), ctypes.byref(nb)) == 0 and nb.value != 0)
        return [nm for nm, _ in s.time_kernels(1) if nm], have
    finally:
        s.close()


def run(cfg, x, u, g, sweeps):
    s = pyddp.Solver(cfg)
    try:
        s.load(x, u, g); s.iterate(sweeps); s.sync()
        out = dict(s.store())
        out["P"], out["p"] = s.get_cost_to_go()[:2]
        return out
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def pair(N, M, ee, mode):
    """(problem 1 inside the poisoned batch, the same problem alone, kernel names of the two handles)"""
    over, sweeps = MODES[mode]
    x, u, g = three_problems(N, ee)
    c3, c1 = config(N, M, 3, ee, over), config(N, M, 1, ee, over)
    names = kernel_names(c3, x, u, g), kernel_names(c1, x[1:2], u[1:2], g[1:2])
    return run(c3, x, u, g, sweeps), run(c1, x[1:2], u[1:2], g[1:2], sweeps), names


def assert_problem_1_alone(N, M, ee, mode):
    batch, alone, names = pair(N, M, ee, mode)
    assert names[0] == names[1] and "k_bp_mfma" in names[0][0], names   # the one-problem handle resolves to the same kernels ...
    assert names[0][1] == [True, bool(ee)], names                       # ... and both to the LDS-prefetching instantiation: float, compact [A B] (+ the position block)
    assert np.any(alone["KT"] != 0) and np.isfinite(alone["KT"]).all() and np.isfinite(alone["P"]).all(), "mis-configured: the backward pass of problem 1 must run and stay finite"
    bad = [k for k in KEYS if not np.array_equal(batch[k][1], alone[k][0], equal_nan=batch[k].dtype.kind == "f")]
    assert not bad, f"problem 1 between two problems scaled by 1e3 differs from the same problem alone in {bad}"


@pytest.mark.parametrize("M", [4, 2, 1])
def test_neighbour_poisoning(M):
    assert_problem_1_alone(16, M, False, "every-pass-keeps")


@pytest.mark.parametrize("mode", ["no-pass-keeps", "lean-then-keeping"])
@pytest.mark.parametrize("M", [4, 2, 1])
def test_neighbour_poisoning_both_pass_modes(M, mode):
    assert_problem_1_alone(16, M, False, mode)


def test_neighbour_poisoning_end_effector_cost():
    assert_problem_1_alone(16, 4, True, "every-pass-keeps")


@pytest.mark.parametrize("N", [8, 16])
def test_first_and_last_knot_of_a_block_under_the_float32_bar(N):
    """The gains of the first six iterations of a solve, each backward pass teacher-forced from the float64 iteration (test_fp32_bar.run_bar), under that file's bar for
    this kernel: err(kernel, float64) <= max(1e-4, 1.5 x the worst of its eight float32 evaluations of the reference pass).  The lane-group pass is bit-identical to the
    first member of that ensemble (the strict float32 oracle).  Held against the lane-group HANDLE's single evaluation of a free-running first sweep instead, the same
    bits of this kernel and of its parent commit miss: du 1.87e-2 against 5.5e-3 at N = 16, KT 4.3e-4 against 1.8e-4 at N = 8 (errors against a double handle) -- the
    factor of 2 - 6 between two valid float32 evaluations of this pass that test_fp32_bar.py's header describes, which is why the bar there is the ensemble's."""
    rows, _, _ = run_bar("hip", 4, {**KUKA, "N": N}, BENCHED, 5, 6, ensemble=True)
    gains = [r for r in rows if r[1] == "bp" and r[2] in ("KT", "du")]
    assert len(gains) == 12, [r[:3] for r in rows if r[1] == "bp"]
    for it, ph, name, ek, eo, ok in gains:
        print(f"N {N} iteration {it} {name}: err(matrix-core, float64) {ek:.3e}  err(strict float32 oracle, float64) {eo:.3e}  inside {ok}")
    assert all(r[5] for r in gains), [(it, name, f"{ek:.2e}", f"{eo:.2e}") for it, ph, name, ek, eo, ok in gains if not ok]
