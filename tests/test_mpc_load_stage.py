"""The load stage of an MPC control cycle (k_mpc_load: csrc/mpc.hpp, csrc/fp_pipe.hpp) alone, array by array, against a numpy restatement.

pddp_mpc_load runs what pddp_mpc_solve runs up to and including the k_mpc_load launch and stops: no sweep has overwritten P, p, KT, xb or AB yet.  Before every call
EVERY array the stage reads or writes is set to distinct non-zero random values for every problem, so a copy from the wrong knot, problem, half or array cannot give
the right value.  After the call every one of them is fetched again and compared with

  * the numpy shift / clear of the very values that were set -- bit for bit -- for everything that is data movement (the documented layout of mpc.hpp: half 0 of
    xb = the rolled-out trajectory, half 1 = x_old = the shifted previous trajectory including knot N-1; u_old = the shifted controls BEFORE the closed-loop tail;
    KT_old = the shifted gains; knots N-2, N-1 of ucur / KT and knot N-1 of dcur, P, p, Pp, pp are not touched by a shift; du, dmax, err zero; AB zero at knot N-2
    only), for arrays the stage has no business with (H, g, J, Jout, alphaOut) and for every knot of xb / ucur the rollout does not write;
  * a float64 rollout (Oracle(...).integrator from the float32 inputs converted exactly) for the rolled-out knots and, without FULL_ROLLOUT, the controls of the
    closed-loop tail: 1e-9 for float64 handles, err(kernel32, ref64) <= max(1e-4, 1.5 x err(oracle32, ref64)) for float32 ones, oracle32 = the same
    restatement in float32 (for the 512-thread pipeline, whose Euler update is an explicit fused multiply-add: the worse of the strict and the FMA-contracted oracle).

Nothing here compares the kernel with a value the kernel produced.  The three kernel forms: the 512-thread role pipeline (float arm, built-in robot model, V = 1 / 0),
the 256-thread kernel with the lane-group rollout (float arm with kernels.fp = lg or another robot model; double arm), the 256-thread kernel with the generic rollout
(integrator_step: cart-pole, RK3).  The host emulation runs the 256-thread body with one lane.

The float32 ratios err(kernel32) / err(oracle32) are printed per rollout and per case (pytest -s); DESIGN.md section 2 carries the measured figures."""
import numpy as np
import pytest

import pyddp
from backends import BACKENDS, make_solver
from oracle_binding import Oracle, OracleMpc, default_cfg, example_inputs, PLANT_DIMS

ARM = dict(wafr_urdf=1, mpc_mode=1, total_time=0.5, A=8)
CASES = {
    # name: (plant, dtype (0 float / 1 double), batch, config, kernel selection, runs the 512-thread pipeline on the GPU)
    "arm-f32-pipe-v1": (4, 0, 3, dict(ARM, N=32, M=4), None, True),
    "arm-f32-pipe-v0": (4, 0, 3, dict(ARM, N=32, M=4, wafr_urdf=0), None, True),
    "arm-f32-pipe-nroll2": (4, 0, 2, dict(ARM, N=32, M=16), None, True),            # NB = 2: without FULL_ROLLOUT the chain stores x_1, factor wave 1 has no job
    "arm-f32-pipe-nroll4": (4, 0, 2, dict(ARM, N=64, M=16), None, True),            # NB = 4: factor wave 0 stores x_1, the chain x_2 and x_3
    "arm-f32-pipe-m1": (4, 0, 2, dict(ARM, N=16, M=1), None, True),                 # single shooting: no tail even without FULL_ROLLOUT, NB = N
    "arm-f32-lg": (4, 0, 3, dict(ARM, N=32, M=4), dict(fp="lg"), False),            # 256 threads, lane-group rollout
    "arm-f32-other-model": (4, 0, 2, dict(ARM, N=32, M=4, wafr_urdf=0, ee_type=2), None, False),   # not a built-in robot model: 256 threads as well
    "arm-f64": (4, 1, 2, dict(ARM, N=32, M=4), None, False),
    "cart-f32-rk3": (2, 0, 2, dict(N=32, M=2, A=8, integrator=3, total_time=2.0), None, False),   # generic rollout through integrator_step
    "cart-f64-rk3": (2, 1, 2, dict(N=32, M=2, A=8, integrator=3, total_time=2.0), None, False),
    "arm-f32-ee-shift": (4, 0, 2, dict(ARM, N=32, M=4, ee_cost=1, ee_cost_shift=1), None, True),  # tshift = shift
}
SET = ("xb", "ucur", "dcur", "P", "Pp", "p", "pp", "KT", "du", "dmax", "err", "AB", "x_old", "u_old", "KT_old", "xGoal", "tshift")
BYSTANDERS = ("H", "g", "J", "Jout", "alphaOut")
ORACLE_KEYS = ("N", "M", "A", "integrator", "wafr_urdf", "mpc_mode", "total_time", "ee_type", "ee_cost", "ee_cost_shift")


def nrel(a, ref):
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))


def shift_knots(a, shift, dim_n, zero_fill):
    """shiftAndCopy on [N][...]: out[k] = a[min(k + shift, dim_n - 1)] (0 beyond the data when zero_fill) for k < dim_n - 1; the other knots keep their values"""
    out = a.copy()
    for k in range(dim_n - 1):
        ks = k + shift
        out[k] = 0 if (zero_fill and ks >= dim_n - 1) else a[min(ks, dim_n - 1)]
    return out


def rollout(step, dtype, x_shifted, x_prev, u, KT, xact, N, NB, M, shift, full):
    """rolloutMPC (+ rolloutMPC2 without FULL_ROLLOUT) in `dtype` with `step` as the integrator; returns (half 0 of xb, ucur)"""
    x, u = x_shifted.astype(dtype), u.astype(dtype).copy()
    x_prev, KT = x_prev.astype(dtype), KT.astype(dtype)
    m, n = u.shape[1], x.shape[1]
    x[0] = xact
    for k in range((N if full else NB) - 1):
        x[k + 1] = step(x[k], u[k])
    if not full and M > 1 and shift > 0:
        ks = N - 1 - shift
        for kn in range(ks, ks + shift):
            dx = x[kn] - x_prev[kn]
            K = KT[kn].reshape(m, n)
            for r in range(m):
                acc = dtype(0)
                for c in range(n):
                    acc = dtype(acc + dtype(K[r, c] * dx[c]))
                u[kn, r] = dtype(u[kn, r] - acc)
            x[kn + 1] = step(x[kn], u[kn])
    return x, u


def expected_of(inp, cur, xact, goal, shifts, clear, full, dims, ee_shift, oracles):
    """What every array holds after the stage: exp[name] for the bit-for-bit part, plus per problem the rolled-out knots / tail controls and their references"""
    B, N, M, NB, n, m, A = dims
    dtype = inp["xb"].dtype.type
    exp = {k: v.copy() for k, v in inp.items()}
    rolled = []
    for pb in range(B):
        s = int(shifts[pb])
        xs = shift_knots(inp["xb"][pb, cur[pb]], s, N, False)
        exp["xb"][pb, 0] = xs; exp["xb"][pb, 1] = xs; exp["x_old"][pb] = xs
        if s > 0:
            exp["dcur"][pb] = shift_knots(inp["dcur"][pb], s, N, False)
        for name, dim_n, zero_fill in (("P", N, False), ("p", N, False), ("Pp", N, False), ("pp", N, False), ("ucur", N - 1, True), ("KT", N - 1, True)):
            if clear:
                exp[name][pb] = 0
            elif s > 0:
                exp[name][pb] = shift_knots(inp[name][pb], s, dim_n, zero_fill)
        exp["u_old"][pb] = exp["ucur"][pb]; exp["KT_old"][pb] = exp["KT"][pb]
        exp["du"][pb] = 0; exp["dmax"][pb] = 0; exp["err"][pb] = 0; exp["AB"][pb, N - 2] = 0
        exp["xGoal"][pb] = goal[pb]; exp["tshift"][pb] = s if ee_shift else 0
        exp["xb"][pb, 0, 0] = xact[pb]
        # the knots the rollout writes
        xmask, umask = np.zeros(N, bool), np.zeros(N, bool)
        xmask[1:(N if full else NB)] = True
        if not full and M > 1 and s > 0:
            xmask[N - s:N] = True; umask[N - 1 - s:N - 1] = True
        runs = {}
        for key, (step, dt_) in oracles.items():
            runs[key] = rollout(step, dt_, xs, xs, exp["ucur"][pb], exp["KT"][pb], xact[pb].astype(dt_), N, NB, M, s, full)
        rolled.append((xmask, umask, runs))
    return exp, rolled


def fill_inputs(rng, plant, dtype, dims):
    """distinct non-zero random values for every array of every problem; xb and ucur tame (the example pose plus small noise, controls around 0.01); the gains the
    closed-loop tail multiplies by are small, everything that is only moved is arbitrary"""
    B, N, M, NB, n, m, A = dims
    x0 = example_inputs(plant, N, np.float64)[0].reshape(N, n)
    f = lambda *sh: rng.normal(0, 1, sh)
    inp = dict(xb=x0[None, None] + rng.normal(0, 0.002, (B, 2, N, n)), ucur=0.01 + rng.normal(0, 0.002, (B, N, m)), dcur=f(B, N, n),
               P=f(B, N, n, n), Pp=f(B, N, n, n), p=f(B, N, n), pp=f(B, N, n), KT=0.05 * f(B, N, m * n), du=f(B, N, m), dmax=f(B, A),
               err=rng.integers(1, 1000, (B, M)), AB=f(B, N, n * (n + m)), x_old=f(B, N, n), u_old=f(B, N, m), KT_old=f(B, N, m * n),
               xGoal=f(B, n), tshift=rng.integers(1, 1000, (B,)))
    out = {k: np.ascontiguousarray(v, np.int32 if k in ("err", "tshift") else dtype) for k, v in inp.items()}
    for k, v in out.items():
        assert np.all(v != 0), k
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(CASES))
def test_load_stage_array_by_array(backend, case):
    plant, dt_code, B, kw, sel, piped = CASES[case]
    dtype = np.float64 if dt_code else np.float32
    N, M, A = kw["N"], kw["M"], kw["A"]
    NB = N // M
    npos, n, m = PLANT_DIMS[plant]
    dims = (B, N, M, NB, n, m, A)
    s = make_solver(backend, plant, dtype=dt_code, batch=B, max_iter=4, kernels=sel, **kw)
    if backend == "hip" and plant == 4:
        # which kernel form the handle launches, read from the library's behaviour: the thread-lane plant evaluation exists only for the built-in robot models
        x1 = example_inputs(4, 2, dtype)[0][:14]
        if case == "arm-f32-other-model":
            with pytest.raises(pyddp.PddpError):
                s.plant_eval(7, x1, np.zeros(7, dtype))
        else:
            s.plant_eval(7, x1, np.zeros(7, dtype))
    okw = {k: v for k, v in kw.items() if k in ORACLE_KEYS}
    mk = lambda dt_, variant="strict": Oracle(default_cfg(plant, cores=1, spawn_threads=0, **okw), dt_, variant=variant).integrator
    oracles = {"ref64": (mk(np.float64), np.float64)}
    if not dt_code:
        oracles["o32"] = (mk(np.float32), np.float32)
        if piped and backend == "hip":
            oracles["o32fma"] = (mk(np.float32, "fma"), np.float32)
    ee_shift = bool(kw.get("ee_cost") and kw.get("ee_cost_shift"))
    rng = np.random.default_rng([77, sorted(CASES).index(case)])
    S = sorted(v for v in {0, 1, NB - 1, NB, N - 2} if 0 <= v <= N - 2)      # (single shooting: NB - 1 and NB are beyond what the ABI accepts)
    before = {k: s.get(k).copy() for k in BYSTANDERS}
    ratios, call = [], 0
    for rot in range(len(S)):
        shifts = np.asarray([S[(rot + i) % len(S)] for i in range(B)], np.int32)
        for clear in (0, 1):
            for full in (0, 1):
                inp = fill_inputs(rng, plant, dtype, dims)
                for k in SET:
                    s.set(k, inp[k])
                cur = [(call + i) % 2 for i in range(B)]
                st = s.get_state()
                for i in range(B):
                    st[i].cur = cur[i]
                s.set_state(st)
                goal = rng.normal(0, 1, (B, n)).astype(dtype)
                xact = np.stack([inp["xb"][i, cur[i], shifts[i]] for i in range(B)]) + rng.normal(0, 0.0005, (B, n)).astype(dtype)
                exp, rolled = expected_of(inp, cur, xact, goal, shifts, clear, full, dims, ee_shift, oracles)
                s.mpc_load(xact, goal, shifts, clear_vars=clear, full_rollout=full)
                tag = (case, backend, list(shifts), clear, full, cur)
                got = {k: s.get(k).reshape(inp[k].shape) for k in SET}
                assert [st_.cur for st_ in s.get_state()] == cur, tag
                for k in BYSTANDERS:
                    assert np.array_equal(s.get(k), before[k]), (tag, k)
                xmask = np.stack([r[0] for r in rolled]); umask = np.stack([r[1] for r in rolled])
                for k in SET:
                    g, e = got[k], exp[k]
                    if k == "xb":
                        assert np.array_equal(g[:, 1], e[:, 1]), (tag, "xb half 1")
                        assert np.array_equal(g[:, 0][~xmask], e[:, 0][~xmask]), (tag, "xb half 0, knots the rollout does not write", np.argwhere(g[:, 0][~xmask] != e[:, 0][~xmask])[:4])
                    elif k == "ucur":
                        assert np.array_equal(g[~umask], e[~umask]), (tag, "ucur, knots the tail does not write")
                    else:
                        assert np.array_equal(g, e), (tag, k, np.argwhere(g != e)[:4])
                for pb, (xm, um, runs) in enumerate(rolled):
                    for what, gk, mask, idx in (("x", got["xb"][pb, 0], xm, 0), ("u", got["ucur"][pb], um, 1)):
                        if not mask.any():
                            continue
                        ref = runs["ref64"][idx][mask]
                        ek = nrel(gk[mask], ref)
                        if dt_code:
                            assert ek <= 1e-9, (tag, pb, what, ek)
                            continue
                        eo = max(nrel(runs[key][idx][mask], ref) for key in runs if key != "ref64")
                        ratios.append(ek / max(eo, 1e-30))
                        print("%s[%s] shift %d clear %d full %d problem %d %s: err(kernel32) %.3g err(oracle32) %.3g ratio %.3g" % (case, backend, shifts[pb], clear, full, pb, what, ek, eo, ratios[-1]))
                        if not ek <= max(1e-4, 1.5 * eo):
                            assert eo < 1e-3, (tag, pb, what, "the inputs are not tame", eo)
                        assert ek <= max(1e-4, 1.5 * eo), (tag, pb, what, ek, eo)
                call += 1
    if ratios:
        print("%s[%s]: err(kernel32) / err(oracle32) over %d rollouts: median %.3g worst %.3g" % (case, backend, len(ratios), float(np.median(ratios)), max(ratios)))
    s.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_arm_has_no_generic_rollout_to_reach(backend):
    """The generic rollout (integrator_step) is reached through the cart-pole cases only: the arm is Euler-only (config.cuh:58), a handle with integrator = 3 is refused."""
    with pytest.raises(pyddp.PddpError):
        make_solver(backend, 4, batch=2, max_iter=4, **dict(ARM, N=16, M=2, integrator=3))


# ---------------------------------------------------------------------------------------------------------------- one whole cycle: the store side in float32
CYCLE_KW = dict(N=32, M=4, A=8, wafr_urdf=1, mpc_mode=1, total_time=0.5, tol_cost=1e-5, max_iter=3)
_CYCLE = {}


def cycle_problems():
    """Four problems picked on the CPU from a small pool by what OracleMpc makes of them in float32 (cold cycle, then a warm-started one with the candidate's shift):
    two whose warm cycle takes a step and two whose warm cycle falls back (a start at its goal takes no step of index > 0).  The batch under test has no part in it."""
    if "picked" in _CYCLE:
        return _CYCLE["picked"]
    rng = np.random.default_rng([78, 1])
    pool = []
    for i in range(10):
        x0, _, _ = example_inputs(4, 32, np.float32, noise=rng.normal(0, 0.001, (32, 14)) if i % 2 == 0 else None)
        xg = x0[:14].copy()
        if i % 2 == 0:
            xg[:7] += np.float32(0.05 + 0.02 * i); xg[7:] = 0        # a nearby goal: progress
        pool.append(dict(x0=x0, u0=np.full(32 * 7, 0.01, np.float32), xg=xg, xact=x0[:14] + (rng.normal(0, 0.002, 14).astype(np.float32) if i % 2 == 0 else 0), shift=1 + i % 3))
    for p in pool:
        for dt_ in (np.float32, np.float64):
            o = OracleMpc(default_cfg(4, cores=1, spawn_threads=0, **CYCLE_KW), dt_)
            o.set_traj(p["x0"], p["u0"])
            cold = o.mpc_solve(p["xact"], p["xg"], 0, clear_vars=1, max_iter=3)
            if dt_ == np.float32:
                warm = o.mpc_solve(cold["x"].reshape(32, 14)[p["shift"]], p["xg"], p["shift"], clear_vars=0, max_iter=2)
                p["success"] = (cold["success"], warm["success"])
            p["J0_%d" % np.dtype(dt_).itemsize] = float(cold["Jout"][0])
    steps = [p for p in pool if p["success"] == (1, 1)][:2]
    falls = [p for p in pool if p["success"][1] == 0][:2]
    assert len(steps) == 2 and len(falls) == 2, [p["success"] for p in pool]
    _CYCLE["picked"] = [steps[0], falls[0], steps[1], falls[1]]
    return _CYCLE["picked"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_whole_float32_cycle_returns_the_arrays_or_the_fall_back(backend):
    """k_mpc_store's packed record against the arrays: for a problem that took a step the returned x, u, K are xb[cur], ucur, KT; for one that did not they are x_old,
    u_old, KT_old -- bit for bit, both kinds in one batch.  Jout[0] of the cold cycle (the cost of the load stage's rolled-out trajectory) against OracleMpc in float64."""
    probs = cycle_problems()
    B, N = len(probs), 32
    s = make_solver(backend, 4, batch=B, **CYCLE_KW)
    s.load(np.concatenate([p["x0"] for p in probs]), np.concatenate([p["u0"] for p in probs]), np.stack([p["xg"] for p in probs]))
    goals = np.stack([p["xg"] for p in probs])
    shifts = np.asarray([p["shift"] for p in probs], np.int32)
    assert len(set(shifts.tolist())) > 1
    cold = s.mpc_solve(np.stack([p["xact"] for p in probs]), goals, 0, clear_vars=1, max_iter=3)
    checked = []
    for r in (cold, None):
        if r is None:
            r = s.mpc_solve(cold["x"][np.arange(B), shifts], goals, shifts, clear_vars=0, max_iter=2)
        cur = [st.cur for st in s.get_state()]
        arr = {k: s.get(k) for k in ("xb", "ucur", "KT", "x_old", "u_old", "KT_old")}
        xb = arr["xb"].reshape(B, 2, N, 14)
        for pb in range(B):
            names = ("x_old", "u_old", "KT_old") if not r["success"][pb] else ("xb", "ucur", "KT")
            want = [xb[pb, cur[pb]] if k == "xb" else arr[k].reshape(B, -1)[pb] for k in names]
            for out, w in zip(("x", "u", "KT"), want):
                assert np.array_equal(r[out][pb].ravel(), w.ravel()), (pb, out, int(r["success"][pb]))
        checked.append([int(v) for v in r["success"]])
        assert 0 in checked[-1] and 1 in checked[-1], checked
    j64 = np.asarray([p["J0_8"] for p in probs]); j32 = np.asarray([p["J0_4"] for p in probs])
    ek, eo = nrel(cold["Jout"][:, 0], j64), nrel(j32, j64)
    print("whole cycle[%s]: success flags %s, Jout[0] err(kernel32) %.3g err(oracle32) %.3g" % (backend, checked, ek, eo))
    if not ek <= max(1e-4, 1.5 * eo):
        assert eo < 1e-3, eo
    assert ek <= max(1e-4, 1.5 * eo), (ek, eo)
    s.close()
