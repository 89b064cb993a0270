"""Control limits of the quadrotor on the matrix-core backward pass: k_bp_mq's BOX instantiations (csrc/bp_mq.hpp), reached through
kernels.cf_bp = mq with the record rollouts, which pins the plan at any batch.  The yardsticks, batches and limit rows are tests/test_control_limits.py's."""
import numpy as np
import pytest

import pyddp
from backends import make_solver
from test_control_limits import B6, batch_limits, device_pass, loaded, np_type, problem_set, reference_pass, rel_err, tight_limits

SEL = dict(cf_bp="mq", cf_fp="cf")
FIVE = ("KT", "du", "P", "p", "dJexp")
DTYPES = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]


@pytest.mark.gpu
@pytest.mark.parametrize("N,M", [(8, 1), (8, 2), (16, 4)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_pass_against_the_enumeration(dtype, N, M):
    """1: the table-less pass (k_bp_mq as it was), then the six rows: slots 0-2 bit for bit, all six against the float64 recursion over the 3^4 active sets"""
    m = 4
    s, _ = loaded(3, dtype, N, M, B6, A=8, kernels=SEL)
    lim, free = batch_limits(s, m)
    plain = device_pass(s, pyddp.PHASE_BP)
    s.set_control_limits([2, 3, 4, 5], lim[2:])
    ref = reference_pass(s, lim)
    nc = ref["nclamp"][3:, :-1]
    hist = np.bincount(nc.ravel(), minlength=m + 1)
    assert (nc == 0).any() and (nc == m).any() and ((nc >= 1) & (nc < m)).any(), hist
    keep = ref["margin"] >= 1e-6
    keep[:, -1] = True
    assert (~keep).sum() <= 0.05 * B6 * (N - 1), (~keep).sum()
    box = device_pass(s, pyddp.PHASE_BP)
    assert not box["err"].any() and not plain["err"].any()
    for k in FIVE + (("ApBK", "Bdu") if M > 1 else ()):
        assert np.array_equal(box[k][:3], plain[k][:3]), k
    mq_err = rel_err(plain, free, (0, 1))
    tol = 1e-9 if dtype == 1 else 4 * mq_err
    err = rel_err(box, ref, range(B6), keep)
    print(f"dtype {dtype} N {N} M {M}: k_bp_mq without a table {mq_err:.3e}  with the rows {err:.3e}  tolerance {tol:.3e}  clamped-count histogram {hist}")
    assert err <= tol, (err, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("N,M", [(16, 4), (8, 2)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_form_keeps_the_sweep_maps(dtype, N, M):
    """2: PHASE_BP_FUSED on a handle with limits: the plain form's gains and cost-to-go bit for bit, the maps' boundary states and the rebuilt A - B K | B du at 1e-5"""
    n, m, A = 12, 4, 16                                              # (the record rollouts hold whole 12-state problems per wavefront at 16 step sizes only: at 8 no plan fuses)
    s, _ = loaded(3, dtype, N, M, B6, A=A, kernels=SEL)
    lim, _ = batch_limits(s, m)
    s.set_control_limits([2, 3, 4, 5], lim[2:])
    ref = device_pass(s, pyddp.PHASE_BP)
    s.run_phase(pyddp.PHASE_FP)
    xs = s.get("xs").reshape(B6, A, N, n).astype(np.float64)
    fused = device_pass(s, pyddp.PHASE_BP_FUSED)
    assert not ref["err"].any() and not fused["err"].any()
    for k in FIVE:
        assert np.array_equal(fused[k], ref[k], equal_nan=True), k
    s.set("xw", np.zeros(B6 * N * A * (n + m), np_type(dtype)))
    s.run_phase(pyddp.PHASE_SWEEP_FUSED)
    xw = s.get("xw").reshape(B6, N, A, n + m).astype(np.float64)
    bnd = [k + 1 for k in range(N - 1) if (k + 1) % (N // M) == 0]
    got, want = xw[:, bnd, :, :n].transpose(0, 2, 1, 3), xs[:, :, bnd]
    assert np.isfinite(want).all() and np.isfinite(got).all()
    worst = np.abs(got - want).max() / np.abs(want).max()
    print(f"dtype {dtype} N {N} M {M}: boundary states from the maps against the per-knot sweep {worst:.2e} of the trajectory's size")
    assert worst <= 1e-5, worst
    for k in ("ApBK", "Bdu"):
        s.set(k, np.full(ref[k].size, np.nan, np_type(dtype)))
    s.refresh_reference_views()
    for k in ("ApBK", "Bdu"):
        a, b = s.get(k).reshape(B6, N, -1)[:, :-1].astype(np.float64), ref[k].reshape(B6, N, -1)[:, :-1].astype(np.float64)
        assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), k


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_solves_stay_inside_and_cost_no_more_than_k_bp_box(dtype):
    """3: one solve and two control cycles with tight limits: controls inside exactly, accepted costs never rise, final costs no worse than the k_bp_box handle's beyond
    the relative difference the two selections show without a table"""
    N, M, A, B, m, T = 16, 4, 16, 4, 4, np_type(dtype)
    lim = tight_limits(3, B)
    lo, hi = lim[:, None, :m].astype(T), lim[:, None, m:].astype(T)
    x0, u0, xg = problem_set(3, N, dtype, B, 2)
    u0 = np.clip(u0, lo, hi)

    def run(sel, limited):
        s = make_solver("hip", 3, dtype=dtype, batch=B, N=N, M=M, A=A, integrator=3, total_time=N / 32.0, max_iter=8, kernels=sel)
        if limited:
            s.set_control_limits(np.arange(B), lim)
        outs = [s.solve(x0, u0, xg)]
        for _ in range(2):
            outs.append(s.mpc_solve(outs[-1]["x"][:, 1], xg, 1))
        return outs, np.array([[o["Jout"][b, int(o["iters"][b])] for b in range(B)] for o in outs], np.float64)

    (_, Jp), (_, Jc) = run(SEL, False), run(dict(SEL, cf_bp="coop"), False)
    assert np.isfinite(Jp[0]).all() and np.array_equal(np.isfinite(Jp), np.isfinite(Jc))
    tol = np.nanmax(np.abs(Jp - Jc) / np.abs(Jc))                    # (without limits the second control cycle of two of these problems ends without a finite cost on either selection)
    (outs, Jmq), (_, Jbox) = run(SEL, True), run(dict(SEL, cf_bp="coop"), True)
    for o in outs:
        u = o["u"][:, :-1]
        assert (u >= lo).all() and (u <= hi).all()
        for b in range(B):
            acc = [0] + [k for k in range(1, int(o["iters"][b]) + 1) if o["alphaOut"][b, k] >= 0]
            assert (np.diff(o["Jout"][b, acc]) <= 0).all(), (b, o["Jout"][b, acc])
    assert np.isfinite(Jmq).all() and np.isfinite(Jbox).all()
    excess = ((Jmq - Jbox) / np.abs(Jbox)).max()
    print(f"dtype {dtype}: final costs, k_bp_mq with limits over k_bp_box {excess:.3e}; the two selections without a table differ by {tol:.3e}")
    assert excess <= tol, (excess, tol)
