"""Control limits of the pendulum, cart-pole and quadrotor: pddp_set_control_limits_problems / pddp_get_control_limits_problems / pddp_clear_control_limits_problems
(csrc/control_limit_table.hpp, csrc/bp_box.hpp k_bp_box, csrc/plants.hpp LimTab).

Yardsticks:
  * a float64 NumPy recursion over the arrays the handle holds after a load (AB, H, g, the state records ...) that solves every knot's box problem by enumerating all
    3^m active sets -- it shares nothing with the library;
  * the cooperative backward pass k_bp (PDDP_PHASE_BP_COOP) and a handle without a table pinned to it, bit for bit, wherever no limit is active;
  * np.clip in the element type for the rollouts' control law.
The batch of the backward-pass tests: slots 0, 1 without limits, slot 2 with limits far outside reach, slots 3, 4, 5 with limits taken from quantiles of the
REFERENCE'S unconstrained new controls ucur - du (batch_limits), so that some knots clamp one control, some all and some none.
"""
import itertools
import os
import subprocess

import numpy as np
import pytest

import pyddp
from backends import make_solver
from oracle_binding import example_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = {1: (1, 2, 1), 2: (2, 4, 1), 3: (6, 12, 4)}                 # npos, n, m
SHAPES = [(8, 1), (8, 2), (16, 4)]
CASES = [pytest.param(p, d, N, M, id=f"plant{p}-{'f32' if d == 0 else 'f64'}-N{N}-M{M}") for p in (1, 2, 3) for d in (0, 1) for N, M in SHAPES]
B6 = 6
HOVER = 9.81 / 8


def np_type(dtype):
    return np.float32 if dtype == 0 else np.float64


def inputs(plant, N, dtype, B, seed=0):
    """B problems: the example's inputs with noise, controls around the plant's trim, and warm-start arrays (SPD cost-to-go, small defects, small gains)"""
    npos, n, m = DIMS[plant]
    rng = np.random.default_rng(100 * plant + seed)
    T = np_type(dtype)
    x0, u0, xg, P0, p0, d0, KT0 = [], [], [], [], [], [], []
    for _ in range(B):
        x, u, g = example_inputs(plant, N, np.float64, noise=rng.normal(0, 0.01, (N, n)))
        x0.append(x.reshape(N, n)); xg.append(g)
        u0.append((HOVER if plant == 3 else 0.0) + rng.normal(0, 0.3, (N, m)))
        L = rng.normal(0, 1, (N, n, n)); P0.append(np.einsum("kij,klj->kil", L, L) + 2.0 * np.eye(n)); p0.append(rng.normal(0, 1, (N, n)))
        d0.append(rng.normal(0, 0.01, (N, n))); KT0.append(rng.normal(0, 0.1, (N, m, n)))
    return {k: np.asarray(v).astype(T) for k, v in dict(x0=x0, u0=u0, xg=xg, P0=P0, p0=p0, d0=d0, KT0=KT0).items()}


def loaded(plant, dtype, N, M, B, A=4, **kw):
    s = make_solver("hip", plant, dtype=dtype, batch=B, N=N, M=M, A=A, integrator=3, total_time=N / 32.0, max_iter=8, use_graph=0, **kw)
    i = inputs(plant, N, dtype, B)
    s.load(i["x0"], i["u0"], i["xg"], clear_vars=0, KT0=i["KT0"], P0=i["P0"], p0=i["p0"], d0=i["d0"])
    return s, i


def box_enum(Q, q, lo, hi):
    """argmin 1/2 x'Qx - q'x over [lo, hi] by enumerating the 3^m active sets: (x, clamped mask, smallest margin in units of |q|)"""
    m = q.size
    for sides in itertools.product((0, -1, 1), repeat=m):
        sides = np.asarray(sides)
        if np.any((sides == -1) & np.isinf(lo)) or np.any((sides == 1) & np.isinf(hi)):
            continue
        c = sides != 0
        x = np.where(sides == -1, lo, np.where(sides == 1, hi, 0.0))
        if (~c).any():
            x[~c] = np.linalg.solve(Q[np.ix_(~c, ~c)], q[~c] - Q[np.ix_(~c, c)] @ x[c])
        grad = Q @ x - q
        slack = np.minimum(x - lo, hi - x) * np.diag(Q)            # (in the multipliers' units)
        margins = np.where(c, np.where(sides == -1, grad, -grad), slack)
        if margins.min() >= 0:
            return x, c, margins.min() / max(np.linalg.norm(q), 1e-300)
    raise AssertionError("no active set satisfies the conditions")


def reference_pass(s, lim):
    """bp_block (csrc/bp.hpp) in float64 with the box step: KT, du, P, p of every written slot, dJexp, and per knot the number of clamped controls and the margin"""
    c = s.cfg
    B, N, M, n, m = c.batch, c.N, c.M, s.n, s.m
    NM, NB = n + m, c.N // c.M
    f = lambda k, *sh: s.get(k).astype(np.float64).reshape(B, *sh)
    AB, H, g, xb, dcur, ucur = f("AB", N, NM, n), f("H", N, NM, NM), f("g", N, NM), f("xb", 2, N, n), f("dcur", N, n), f("ucur", N, m)
    st = s.get_state()
    Pw, pw, Pr, pr = s.get_cost_to_go()                          # (written halves, then the halves the pass reads)
    Pr, pr = Pr.astype(np.float64).reshape(B, N, n, n), pr.astype(np.float64).reshape(B, N, n)
    out = dict(KT=np.zeros((B, N, m, n)), du=np.zeros((B, N, m)), P=np.full((B, N, n, n), np.nan), p=np.full((B, N, n), np.nan), dJexp=np.zeros((B, 2 * M)),
               nclamp=np.full((B, N), -1), margin=np.full((B, N), np.inf))
    for b in range(B):
        rho, xcur, xprev2 = st[b].rho, xb[b, st[b].cur], xb[b, st[b].cur2]
        lo, hi = lim[b, :m], lim[b, m:]
        for blk in range(M):
            ks = NB * (blk + 1) - 1
            if ks == N - 1:
                Pm, pv = H[b, ks][:n, :n].copy(), g[b, ks][:n].copy()
                out["P"][b, ks - 1], out["p"][b, ks - 1] = Pm, pv
                ks, iters = ks - 1, NB - 2
            else:
                Pm, iters = Pr[b, ks].copy(), NB - 1
                pv = Pm.T @ (xcur[ks + 1] - xprev2[ks + 1]) + pr[b, ks]
            for it in range(iters, -1, -1):
                ABm = AB[b, ks].T
                AB2 = np.concatenate([Pm @ ABm[:, :n], (Pm + rho * np.eye(n)) @ ABm[:, n:]], axis=1)
                if M > 1 and (it + 1) % NB == 0 and it < N - 1:
                    pv = pv + Pm.T @ dcur[b, ks]
                Hm, gm = AB2.T @ ABm + H[b, ks], ABm.T @ pv + g[b, ks]
                Quu, qu, Qux = Hm[n:, n:].T, gm[n:], Hm[:n, n:].T
                du, cl, margin = box_enum(Quu, qu, ucur[b, ks] - hi, ucur[b, ks] - lo)
                K = np.zeros((m, n))
                if (~cl).any():
                    K[~cl] = np.linalg.solve(Quu[np.ix_(~cl, ~cl)], Qux[~cl])
                W = K.T @ Hm[n:, n:].T - Hm[n:, :n].T
                out["KT"][b, ks], out["du"][b, ks], out["nclamp"][b, ks], out["margin"][b, ks] = K, du, cl.sum(), margin
                out["dJexp"][b, 2 * blk] += du @ qu
                out["dJexp"][b, 2 * blk + 1] += du @ (Quu @ du)
                if it != 0 or blk != 0:
                    Pm, pv = Hm[:n, :n] + (W @ K).T - Hm[:n, n:] @ K, gm[:n] + W @ du - K.T @ qu
                    out["P"][b, ks - 1], out["p"][b, ks - 1] = Pm, pv
                ks -= 1
    return out


def device_pass(s, phase):
    s.run_phase(phase)
    B, N, M, n, m = s.cfg.batch, s.cfg.N, s.cfg.M, s.n, s.m
    Pw, pw, _, _ = s.get_cost_to_go()
    return dict(KT=s.get("KT").reshape(B, N, m, n), du=s.get("du").reshape(B, N, m), P=Pw.reshape(B, N, n, n), p=pw.reshape(B, N, n), dJexp=s.get("dJexp").reshape(B, 2 * M),
                ApBK=s.get("ApBK").reshape(B, N, n, n), Bdu=s.get("Bdu").reshape(B, N, n), err=s.get("err"))


def rel_err(dev, ref, rows, keep=None):
    """largest error of the written slots of problems `rows`, relative to each array's largest reference entry of the problem"""
    worst = 0.0
    for b in rows:
        for k in ("KT", "du", "P", "p", "dJexp"):
            r, d = ref[k][b], dev[k][b].astype(np.float64)
            ok = np.isfinite(r)
            if keep is not None and k in ("KT", "du"):
                ok = ok & keep[b].reshape((-1,) + (1,) * (r.ndim - 1))
            if k in ("KT", "du"):
                ok[-1] = False                                       # (knot N - 1 has no control step)
            worst = max(worst, np.abs(d - r)[ok].max() / max(np.abs(r[ok]).max(), 1e-300))
    return worst


def batch_limits(s, m):
    """the six rows (see the module docstring), from the reference's own unconstrained pass"""
    B, N = s.cfg.batch, s.cfg.N
    open_rows = np.concatenate([np.full((B, m), -np.inf), np.full((B, m), np.inf)], axis=1)
    free = reference_pass(s, open_rows)
    unew = s.get("ucur").astype(np.float64).reshape(B, N, m)[:, :-1] - free["du"][:, :-1]
    lim = open_rows.copy()
    lim[2] = np.concatenate([np.full(m, -1e6), np.full(m, 1e6)])
    # slot 3: a window per control, wide for the first and narrow for the last, so that knots clamp some controls and not others; slot 4: narrow for all; slot 5: just
    # outside everything its knots k >= 1 reach -- no clamped knot in front of it changes the recursion, so those knots clamp nothing, and knot 0 may
    wins = [(5, 95), (25, 75), (40, 60), (45, 55)] if m > 1 else [(25, 75)]
    lim[3] = np.concatenate([[np.percentile(unew[3][:, j], wins[j][0]) for j in range(m)], [np.percentile(unew[3][:, j], wins[j][1]) for j in range(m)]])
    lim[4] = np.concatenate([np.percentile(unew[4], 45, axis=0), np.percentile(unew[4], 55, axis=0)])
    span = unew[5][1:].max(axis=0) - unew[5][1:].min(axis=0)
    lim[5] = np.concatenate([unew[5][1:].min(axis=0) - 0.1 * span, unew[5][1:].max(axis=0) + 0.1 * span])
    return lim, free


@pytest.mark.gpu
@pytest.mark.parametrize("plant,dtype,N,M", CASES)
def test_backward_pass_against_brute_force_and_k_bp(plant, dtype, N, M):
    """1: k_bp_box against the enumeration, float64 at 1e-9, float32 at 4x the error k_bp itself shows against the same recursion on the problems without limits;
    2 (first half): where no limit is active, k_bp_box is k_bp bit for bit"""
    m = DIMS[plant][2]
    s, _ = loaded(plant, dtype, N, M, B6)
    lim, free = batch_limits(s, m)
    coop = device_pass(s, pyddp.PHASE_BP_COOP)                       # (no table yet: k_bp)
    s.set_control_limits([2, 3, 4, 5], lim[2:])
    ref = reference_pass(s, lim)
    nc = ref["nclamp"][3:, :-1]
    assert (nc == 0).any() and (nc == m).any() and ((nc >= 1) & (nc <= m)).any(), np.bincount(nc.ravel(), minlength=m + 1)
    if m > 1:
        assert ((nc >= 1) & (nc < m)).any(), np.bincount(nc.ravel(), minlength=m + 1)
    keep = ref["margin"] >= 1e-6
    keep[:, -1] = True
    assert (~keep).sum() <= 0.05 * B6 * (N - 1), (~keep).sum()
    box = device_pass(s, pyddp.PHASE_BP)
    assert not box["err"].any() and not coop["err"].any()
    bp_err = rel_err(coop, free, (0, 1))
    tol = 1e-9 if dtype == 1 else 4 * bp_err
    err = rel_err(box, ref, range(B6), keep)
    print(f"plant {plant} dtype {dtype} N {N} M {M}: k_bp {bp_err:.3e}  k_bp_box {err:.3e}  tolerance {tol:.3e}  clamped-count histogram {np.bincount(nc.ravel(), minlength=m + 1)}")
    assert err <= tol, (err, tol)
    again = device_pass(s, pyddp.PHASE_BP_COOP)                      # the same handle, its cooperative kernel: no limits
    for k in ("KT", "du", "P", "p", "dJexp") + (("ApBK", "Bdu") if M > 1 else ()):
        assert np.array_equal(box[k][:3], again[k][:3]), k


ROLLOUT_FAMILIES = [pytest.param(dict(cf_fp="coop"), 4, id="k_fp"), pytest.param(dict(cf_fp="ts"), 4, id="k_fp_ts"), pytest.param(dict(cf_fp="cf"), 16, id="k_fp_cf")]


def problem_set(plant, N, dtype, B, seed):
    """the example's own inputs with a little noise: solves that accept steps"""
    npos, n, m = DIMS[plant]
    rng = np.random.default_rng(10 * plant + seed)
    T = np_type(dtype)
    x0, u0, xg = zip(*[example_inputs(plant, N, np.float64, noise=rng.normal(0, 0.002, (N, n))) for _ in range(B)])
    return np.asarray(x0).astype(T).reshape(B, N, n), np.asarray(u0).astype(T).reshape(B, N, m), np.asarray(xg).astype(T).reshape(B, n)


@pytest.mark.gpu
@pytest.mark.parametrize("sel,A", ROLLOUT_FAMILIES)
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("plant", [1, 2, 3])
def test_infinite_limits_solve_like_k_bp(plant, dtype, sel, A):
    """2 (second half): a whole solve with every problem at infinite limits against a handle without a table pinned to the cooperative backward pass"""
    N, M, B, m = 16, 4, 5, DIMS[plant][2]
    kw = dict(dtype=dtype, batch=B, N=N, M=M, A=A, integrator=3, total_time=N / 32.0, max_iter=8)
    x0, u0, xg = problem_set(plant, N, dtype, B, 1)
    plain = make_solver("hip", plant, kernels=dict(sel, cf_bp="coop"), **kw)
    lim = make_solver("hip", plant, kernels=dict(sel, cf_bp="coop"), **kw)
    lim.set_control_limits(np.arange(B), np.tile(np.concatenate([np.full(m, -np.inf), np.full(m, np.inf)]), (B, 1)))
    a, b = plain.solve(x0, u0, xg), lim.solve(x0, u0, xg)
    for k in ("x", "u", "KT", "Jout", "alphaOut"):
        assert np.array_equal(a[k], b[k]), k


def tight_limits(plant, B, scale=None):
    m = DIMS[plant][2]
    c = HOVER if plant == 3 else 0.0
    w = np.linspace(0.02, 0.2, B)[:, None] * (scale if scale is not None else 1.0 if plant == 3 else 5.0)
    return np.concatenate([c - w * np.ones(m), c + 1.3 * w * np.ones(m)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("sel,A", ROLLOUT_FAMILIES)
@pytest.mark.parametrize("N,M", [(8, 4), (8, 1)])
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("plant", [1, 2, 3])
def test_rollouts_clamp_the_control_law(plant, dtype, N, M, sel, A):
    """3 (rollouts): teacher-forced PDDP_PHASE_ROLLOUT.  Two-knot segments: the candidates' controls are the clipped control law in the element type and the next states
    pddp_plant_eval(what = 2) on them; both shapes: every stored running-knot control inside the limits exactly, a third of them or more on a bound"""
    B, (npos, n, m), T = 4, DIMS[plant], np_type(dtype)
    s, i = loaded(plant, dtype, N, M, B, A=A, kernels=sel)
    lim = tight_limits(plant, B, 1.0)                                # (half-widths 0.02 .. 0.2 around the trim: the teacher-forced law below spreads over +- 0.5 and more)
    s.set_control_limits(np.arange(B), lim)
    lo, hi = lim[:, None, None, :m].astype(T), lim[:, None, None, m:].astype(T)
    rng = np.random.default_rng(5)
    du = rng.normal(0, 0.5, (B, N, m)).astype(T)
    xs = np.repeat(i["x0"][:, None], A, axis=1) + rng.normal(0, 0.05, (B, A, N, n)).astype(T)
    xs[:, :, 0] = i["x0"][:, None, 0]                                # (segment 0 starts from the current trajectory)
    s.set("du", du); s.set("xs", xs)
    s.run_phase(pyddp.PHASE_ROLLOUT)
    us, xo = s.get("us").reshape(B, A, N, m)[:, :, :-1], s.get("xs").reshape(B, A, N, n)
    assert (us >= lo).all() and (us <= hi).all()
    assert ((us == lo) | (us == hi)).mean() >= 1 / 3
    if N // M == 2:
        alpha = s.get("alpha").astype(T)[None, :, None, None]
        k0 = np.arange(0, N, 2)                                      # the segments' first knots: one control each from the given start state
        st, xb = s.get_state(), s.get("xb").reshape(B, 2, N, n)
        xcur, ucur, KT = np.stack([xb[b, st[b].cur] for b in range(B)]), i["u0"], i["KT0"]
        dx = xs[:, :, k0] - xcur[:, None, k0]
        Kdx = np.zeros((B, A, k0.size, m), T)
        for c in range(n):                                           # (the kernels' order: the sum over the state index ascending, in the element type)
            Kdx = Kdx + KT[:, k0][:, None, :, :, c] * dx[..., c:c + 1]
        law = ucur[:, None, k0] - (alpha * du[:, None, k0] + Kdx)
        want = np.clip(law, lo, hi)
        assert np.array_equal(us[:, :, k0], want)
        xn = s.plant_eval(2, xs[:, :, k0].reshape(-1, n), want.reshape(-1, m)).reshape(B, A, k0.size, n)
        assert np.array_equal(xo[:, :, k0 + 1], xn)


@pytest.mark.gpu
@pytest.mark.parametrize("sel,A", ROLLOUT_FAMILIES)
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("plant", [1, 2, 3])
def test_solves_and_control_cycles_stay_inside_the_limits(plant, dtype, sel, A):
    """3 (solves): after pddp_solve with tight limits and after two control cycles every running-knot control is inside the limits exactly and the cost never rises"""
    N, M, B, m = 16, 4, 4, DIMS[plant][2]
    s = make_solver("hip", plant, dtype=dtype, batch=B, N=N, M=M, A=A, integrator=3, total_time=N / 32.0, max_iter=8, kernels=sel)
    lim = tight_limits(plant, B)
    s.set_control_limits(np.arange(B), lim)
    T = np_type(dtype)
    lo, hi = lim[:, None, :m].astype(T), lim[:, None, m:].astype(T)
    x0, u0, xg = problem_set(plant, N, dtype, B, 2)
    u0 = np.clip(u0, lo, hi)                                         # (a load does not clamp the caller's u0)
    out = s.solve(x0, u0, xg)
    outs = [out]
    for _ in range(2):
        outs.append(s.mpc_solve(outs[-1]["x"][:, 1], xg, 1))
    for o in outs:
        u = o["u"][:, :-1]
        assert (u >= lo).all() and (u <= hi).all()
        iters = o["iters"]
        for b in range(B):
            # (a rejected iteration repeats prevJ, which starts out as the loaded cost + 2 tol_cost: the accepted entries are the costs)
            acc = [0] + [k for k in range(1, int(iters[b]) + 1) if o["alphaOut"][b, k] >= 0]
            J = o["Jout"][b, acc]
            assert (np.diff(J) <= 0).all(), (b, J)


QUAD_W = np.array([0.01] * 3 + [0.001] * 3 + [2.0] * 6 + [5.0] * 4 + [1000.0] * 12)      # the quadrotor's built-in diagonal: q | r | qf


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1])
def test_limited_quadrotor_beats_clipping_after_the_fact(dtype):
    """3 (the point of it): a quadrotor 1 m below its goal with hi at 1.3 x hover.  The plan made WITH the limit, flown open loop by pddp_simulate_problems, ends cheaper
    than the unconstrained plan with its controls clipped after the fact and flown the same way: the box step and the zeroed gains are worth more than a clamp"""
    N, n, m, T, total = 32, 12, 4, np_type(dtype), 0.5
    kw = dict(dtype=dtype, batch=1, N=N, M=4, A=8, integrator=3, total_time=total, max_iter=40)
    x0, xg = np.zeros((1, N, n), T), np.zeros((1, n), T)
    xg[0, 2] = 1.0
    u0 = np.full((1, N, m), HOVER, T)
    hi = 1.3 * HOVER
    free, box = make_solver("hip", 3, **kw), make_solver("hip", 3, **kw)
    box.set_control_limits([0], np.concatenate([np.full(m, -np.inf), np.full(m, hi)])[None])
    plan, lplan = free.solve(x0, u0, xg), box.solve(x0, u0, xg)
    assert (lplan["u"][0, :-1] <= T(hi)).all() and (plan["u"][0, :-1] > T(hi)).any()      # the limit binds: the free plan asks for more
    dt_us = total / (N - 1) * 1e6

    def flown_cost(u):
        """the controls u [N][m] flown open loop from the start: the state at every knot from one simulator call (entry k: slot 0 after k steps), the built-in cost on them"""
        k = np.arange(1, N - 1)                                      # (the simulator flies up to knot N - 2; the last step is the handle's own integrator step)
        plan_x, plan_K = np.zeros((N - 2, N, n), T), np.zeros((N - 2, N, m, n), T)
        xk, _, failed = box.simulate_problems(np.zeros(N - 2, np.int32), 0.0, k * dt_us, 8 * k, xActual=x0[0, 0], x=plan_x, u=np.repeat(u[None], N - 2, axis=0), KT=plan_K)
        assert not failed.any()
        x = np.concatenate([x0[0, :1], xk, box.plant_eval(2, xk[-1:], u[N - 2:N - 1])]).astype(np.float64)
        d = x - xg[0].astype(np.float64)
        return 0.5 * ((QUAD_W[:n] * d[:-1] ** 2).sum() + (QUAD_W[n:n + m] * u[:-1].astype(np.float64) ** 2).sum() + (QUAD_W[n + m:] * d[-1] ** 2).sum())
    limited, clipped = flown_cost(lplan["u"][0]), flown_cost(np.minimum(plan["u"][0], T(hi)))
    print(f"dtype {dtype}: flown cost with the limit planned {limited:.4f}, clipped after the fact {clipped:.4f}, unconstrained plan {flown_cost(plan['u'][0]):.4f}")
    assert limited < clipped


def test_host_only_code_as_a_stand_alone_program(tmp_path):
    """tests/native/control_limit_host_check.cpp (its own main, -fsanitize=address,undefined): every argument check, the rounding and the open row"""
    exe = str(tmp_path / "control_limit_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "control_limit_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "control_limit_host_check: ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_surface_and_named_slots():
    """4: setter, getter and clear, every refusal, the arm refusing all four; a row rewritten between two control cycles of 5 named slots out of 9 equals
    single-problem handles bit for bit, and the slots that are not named are untouched"""
    plant, dtype, N, B = 3, 0, 16, 9
    m, inf = DIMS[plant][2], np.inf
    kw = dict(dtype=dtype, N=N, M=4, A=8, integrator=3, total_time=N / 32.0, max_iter=6, kernels=dict(cf="coop"))
    s = make_solver("hip", plant, batch=B, **kw)
    assert s.control_limits_size() == 2 * m
    s.clear_control_limits([0, 1])                                   # no table yet: a successful no-op
    got, has = s.get_control_limits([0, 8])
    assert not has.any() and (got[:, :m] == -inf).all() and (got[:, m:] == inf).all()
    row = np.concatenate([np.full(m, 0.1), np.full(m, 2.0)])
    rows = np.stack([row, np.concatenate([np.full(m, -inf), np.full(m, inf)])])
    s.set_control_limits([4, 2], rows)
    got, has = s.get_control_limits([2, 3, 4])
    assert list(has) == [1, 0, 1] and np.array_equal(got[0], rows[1]) and np.array_equal(got[2], rows[0].astype(np.float32).astype(np.float64)) and (got[1, :m] == -inf).all()
    s.clear_control_limits([4])
    assert list(s.get_control_limits([4, 2])[1]) == [0, 1]
    bad = row.copy(); bad[0] = np.nan
    closed = row.copy(); closed[m] = closed[0]
    rounded = row.copy(); rounded[0] = 1.0; rounded[m] = 1.0 + 2.0 ** -40
    for idx, lim in (([0], bad), ([0], closed), ([0], rounded), ([B], row), ([-1], row), ([1, 1], np.stack([row, row]))):
        with pytest.raises(pyddp.PddpError):
            s.set_control_limits(idx, lim)
    for call in (lambda: s.lib.pddp_set_control_limits_problems(s.h, 0, None, None), lambda: s.lib.pddp_set_control_limits_problems(s.h, 1, None, None),
                 lambda: s.lib.pddp_get_control_limits_problems(s.h, 1, None, None, None), lambda: s.lib.pddp_clear_control_limits_problems(s.h, 0, None)):
        assert call() != 0
    assert list(s.get_control_limits([4, 2])[1]) == [0, 1]          # the handle is unchanged
    arm = make_solver("hip", 4, dtype=0, batch=1, N=16, M=4, A=4)
    for call in (arm.control_limits_size, lambda: arm.set_control_limits([0], np.zeros(14)), lambda: arm.get_control_limits([0]), lambda: arm.clear_control_limits([0])):
        with pytest.raises(pyddp.PddpError):
            call()
    # named slots with their own rows
    x0, u0, xg = problem_set(plant, N, dtype, B, 3)
    lims = tight_limits(plant, B)
    s.set_control_limits(np.arange(B), lims)
    u0 = np.clip(u0, lims[:, None, :m], lims[:, None, m:]).astype(np.float32)
    s.solve(x0, u0, xg)
    named = np.array([7, 1, 4, 0, 5])
    singles = []
    for b in named:
        one = make_solver("hip", plant, batch=1, **kw)
        one.set_control_limits([0], lims[b:b + 1])
        one.solve(x0[b:b + 1], u0[b:b + 1], xg[b:b + 1])
        singles.append(one)
    before = s.store()
    xa = before["x"][named, 1]
    c1 = s.mpc_solve_problems(named, xa, xg[named], 1)
    new = lims[named].copy()                                         # rewritten between the cycles: the upper limits a tenth of the box lower
    new[:, m:] = new[:, :m] + 0.9 * (new[:, m:] - new[:, :m])
    s.set_control_limits(named, new)
    c2 = s.mpc_solve_problems(named, c1["x"][:, 1], xg[named], 1)
    for i, (b, one) in enumerate(zip(named, singles)):
        o1 = one.mpc_solve(xa[i:i + 1], xg[b:b + 1], 1)
        one.set_control_limits([0], new[i:i + 1])
        o2 = one.mpc_solve(o1["x"][:, 1], xg[b:b + 1], 1)
        for k in ("x", "u", "KT", "Jout", "alphaOut"):
            assert np.array_equal(c1[k][i], o1[k][0]) and np.array_equal(c2[k][i], o2[k][0]), (b, k)
    after = s.store()
    rest = np.setdiff1d(np.arange(B), named)
    for k in ("x", "u", "KT", "Jout", "alphaOut"):
        assert np.array_equal(before[k][rest], after[k][rest]), k
