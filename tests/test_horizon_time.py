"""Per-problem horizon times of the pendulum, cart-pole and quadrotor: pddp_set_horizon_time_problems / pddp_get_horizon_time_problems
(csrc/horizon_time_table.hpp, csrc/plants.hpp StepTab and problem_dt).

A problem given the horizon time t integrates with the step T(t / (N - 1)) -- the expression the handle-wide step is formed with -- wherever a kernel integrates: rollouts,
the setup's [A B], the warm start of a control cycle.

Yardsticks:
  * a handle with cost and goal tables and NO step table for a step table whose entries are all the default -- bit for bit, every array pddp_get_array names;
  * a SINGLE-PROBLEM handle created with cfg.total_time = t_b, with no table at all and pinned to the same kernels, for slot b of a batch with mixed times -- bit for bit
    (tests/test_diag_costs.py and tests/test_goal_trajectory.py hold a handle with the other two tables bit for bit to one without);
  * the oracle, which takes total_time directly: Oracle(default_cfg(plant, total_time = t_b, ...)) per problem.

The structure (FAMILIES pinned through pddp_config.kernels and asserted by name, problem(), solve_single, collect, assert_rows_equal) is that of
tests/test_goal_trajectory.py, restated here.  Shapes: N 16 / 32, M 1 / 4, A 4 / 8, A = 16 for the quadrotor families with k_fp_cf; batches 3, 5 and 67 (67: a wave of the
thread-serial and staged kernels holds several problems with different steps, the last wave is partial).  Problem b gets total_time = (N / 32) x LADDER[b % 5]; the
handle's own time is N / 32, so every fifth problem keeps the default.

The inputs were checked on the CPU: with problem() seeds 0-4 and the settings of base_kw, the float64 and float32 oracles at every (plant, shape, integrator) of FAMILIES
and these times keep the cost finite, accept at least one iteration per problem and exit at two or more different iterations.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyddp
from backends import make_solver
from oracle_binding import Oracle, default_cfg, example_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = {1: (1, 2, 1), 2: (2, 4, 1), 3: (6, 12, 4)}                 # npos, n, m
# cost_pend.cuh:19-24, cost_cart.cuh:19-38 (N != 512), cost_quad.cuh:19-25 as [q | r | qf]
BUILTIN = {1: np.array([1.0, 0.1, 0.1, 1000.0, 1000.0]),
           2: np.array([0.01, 0.01, 0.001, 0.001, 0.0001] + [1000.0] * 4),
           3: np.array([0.01] * 3 + [0.001] * 3 + [2.0] * 6 + [5.0] * 4 + [1000.0] * 12)}
STATE_ALL = tuple(name for name, _ in pyddp.binding.PddpState._fields_)
ARRAYS = ("xs", "us", "ds", "xb", "ucur", "dcur", "P", "Pp", "p", "pp", "AB", "H", "g", "KT", "du", "ApBK", "Bdu", "J", "dmax", "dJexp", "alpha", "xGoal", "Jout", "err",
          "alphaOut", "x_old", "u_old", "KT_old", "xTarget", "costk", "tshift", "Jpart", "dpart", "parts_fresh")
CTG = ("P", "Pp", "p", "pp")
OUT_KEYS = ("x", "u", "KT", "Jout", "alphaOut", "dmax")
MPC_KEYS = ("x", "u", "KT", "Jout", "alphaOut", "success", "iters")
EXTRA_SWEEPS = 3
LADDER = (1.0, 0.6, 1.37, 0.8, 1.5)


def np_type(dtype):
    return np.float32 if dtype == 0 else np.float64


def horizon_time(N, b):
    return (N / 32.0) * LADDER[b % 5]


def horizon_times(N, B, skip=0):
    return [horizon_time(N, skip + b) for b in range(B)]


def base_kw(plant, N, M, A, integ, **more):
    return dict(dict(N=N, M=M, A=A, integrator=integ, total_time=N / 32.0, tol_cost=0.05 if plant == 2 else 1e-3, max_iter=8, ignore_max_rho_exit=0), **more)      # (the cart-pole's cost moves by more per iteration)


# (id, plant, keywords, selection, kernel names, batch)
def _families():
    out = []
    for plant, tag in ((1, "pend"), (2, "cart"), (3, "quad")):
        out.append((tag + "-coop", plant, base_kw(plant, 16, 4, 4, 3), dict(cf="coop"), ("k_bp", "k_fp", "k_nis"), 3))
        out.append((tag + "-coop-M1-euler", plant, base_kw(plant, 16, 1, 4, 1), dict(cf="coop"), ("k_bp", "k_fp", "k_nis"), 3))
        out.append((tag + "-ts", plant, base_kw(plant, 16, 4, 4, 2), dict(cf="ts"), ("k_bp_ts", "k_fp_ts", "k_nis_ts"), 67))
        if plant != 3:
            out.append((tag + "-cf-gl-kb16", plant, base_kw(plant, 32, 4, 8, 3), dict(cf_bp="gl", cf_fp="cf", cf_nis="kb16"), ("k_bp_gl", "k_sweep_cf", "k_fp_cf", "k_nis_kb"), 67))
            out.append((tag + "-gl32-ts-gl8", plant, base_kw(plant, 16, 4, 4, 1), dict(cf_bp="gl32", cf_fp="ts", cf_nis="gl8"), ("k_bp_gl", "k_fp_ts", "k_nis_gl"), 5))
    q = 3
    out.append(("quad-mq-fused-cf-kb16", q, base_kw(q, 16, 4, 16, 3), dict(cf_bp="mq", cf_fp="cf", cf_nis="kb16"), ("k_bp_mq", "k_sweep_maps", "k_fp_cf", "k_nis_kb"), 67))
    out.append(("quad-cl-cf-kb20", q, base_kw(q, 16, 4, 16, 3), dict(cf_bp="cl", cf_fp="cf", cf_nis="kb20"), ("k_bp_cl", "k_sweep_cf", "k_fp_cf", "k_nis_kb"), 5))
    out.append(("quad-mq-ts-kb32", q, base_kw(q, 32, 4, 8, 3), dict(cf_bp="mq", cf_fp="ts", cf_nis="kb32"), ("k_bp_mq", "k_fp_ts", "k_nis_kb"), 5))
    out.append(("quad-mq-M1-cf-kb64", q, base_kw(q, 16, 1, 16, 3), dict(cf_bp="mq", cf_fp="cf", cf_nis="kb64"), ("k_bp_mq", "k_fp_cf", "k_nis_kb"), 5))
    out.append(("quad-gl-cf-gl", q, base_kw(q, 16, 4, 16, 2), dict(cf_bp="gl", cf_fp="cf", cf_nis="gl"), ("k_bp_gl", "k_sweep_cf", "k_fp_cf", "k_nis_gl"), 5))
    out.append(("quad-gl32-ts-gl8", q, base_kw(q, 16, 4, 4, 1), dict(cf_bp="gl32", cf_fp="ts", cf_nis="gl8"), ("k_bp_gl", "k_fp_ts", "k_nis_gl"), 5))
    return [dict(key=k, plant=p, kw=kw, sel=sel, names=names, B=B) for k, p, kw, sel, names, B in out]


FAMILIES = _families()
FAMILY_PARAMS = [pytest.param(f, id=f["key"]) for f in FAMILIES]


def family(key):
    return next(f for f in FAMILIES if f["key"] == key)


def kernel_names(s):
    return [n for n, _ in s.time_kernels(1)]


def handle(fam, dtype, batch, use_graph=1, **more):
    s = make_solver("hip", fam["plant"], dtype=dtype, batch=batch, use_graph=use_graph, kernels=dict(fam["sel"]), **dict(fam["kw"], **more))
    have = kernel_names(s)
    assert all(any(h.startswith(n) for h in have) for n in fam["names"]), (fam["key"], fam["names"], have)
    return s


def problem(plant, N, dtype, seed):
    """the example's inputs with velocity noise and the goal moved along the line from the start: near goals exit by tolerance early, far ones run on"""
    npos, n, m = DIMS[plant]
    rng = np.random.default_rng(1000 * plant + seed)
    x0, u0, xg = example_inputs(plant, N, np.float64, noise=rng.normal(0, 0.002, (N, n)))
    start = x0.reshape(N, n)[0, :npos]
    frac = (0.02, 1.0, 0.3, 0.08, 0.6)[seed % 5] * (1.0 + 0.01 * (seed // 5))
    xg = xg.copy(); xg[:npos] = start + frac * (xg[:npos] - start)
    T = np_type(dtype)
    return dict(x0=x0.astype(T), u0=u0.astype(T), xg=xg.astype(T))


def problems(plant, N, dtype, B, skip=0):
    return [problem(plant, N, dtype, skip + b) for b in range(B)]


def stack(probs, key):
    return np.concatenate([p[key].ravel() for p in probs])


def set_times(s, times, slots=None):
    slots = list(range(len(times))) if slots is None else list(slots)
    s.set_horizon_time_problems(slots[::-1], list(times)[::-1])      # unsorted on purpose


def cost_and_goal_tables(s, plant, N, dtype):
    """the two tables a step table is layered on, with nothing in them: built-in cost rows, no problem flagged"""
    n = DIMS[plant][1]
    s.set_diag_cost(BUILTIN[plant])
    s.set_goal_trajectory_problems([0], np.zeros((1, N, n), np_type(dtype)))
    s.clear_goal_trajectory_problems([0])


def state_rows(s, slots):
    st = s.get_state()
    return {f: np.array([getattr(st[b], f) for b in slots]) for f in STATE_ALL}


def collect(s):
    B = s.cfg.batch
    out = s.store()
    out.update(state_rows(s, range(B)))
    for k in CTG:
        out[k] = s.get(k).reshape(B, -1)
    return out


def reset_like_fresh(s):
    B, mi = s.cfg.batch, s.cfg.max_iter
    st = s.get_state()
    for b in range(B):
        st[b].pw = 0
    s.set_state(st)
    s.set("Jout", np.zeros(B * (mi + 2))); s.set("alphaOut", np.zeros(B * (mi + 2), np.int32))


def run_until_done(s, extra=EXTRA_SWEEPS):
    for _ in range(200):
        s.iterate(4)
        done, _ = s.status()
        if done.all():
            break
    assert done.all()
    s.iterate(extra); s.sync()


def solve_single(s1, prob, **load_kw):
    """the yardstick: one problem on a single-problem handle in the state of a fresh one -- its horizon time is the handle's cfg.total_time --, sweep by sweep until it exits"""
    reset_like_fresh(s1)
    s1.load(prob["x0"], prob["u0"], prob["xg"], clear_vars=1, **load_kw)
    first = {k + "0": s1.get(k).copy() for k in ("AB", "H", "g")}
    for _ in range(4 * s1.cfg.max_iter + 40):
        s1.iterate(1)
        done, _ = s1.status()
        if done[0]:
            break
    assert done[0], "the yardstick problem did not exit"
    res = {k: v[0] for k, v in collect(s1).items()}
    res.update(first)
    return res


def single_refs(fam, dtype, probs, times, **load_kw):
    """per problem: solve_single on a handle created with cfg.total_time = its time (one handle per distinct time), no table of any kind"""
    refs = [None] * len(probs)
    for t in sorted(set(times)):
        s1 = handle(fam, dtype, 1, total_time=t)
        for b, p in enumerate(probs):
            if times[b] == t:
                refs[b] = solve_single(s1, p, **load_kw)
        s1.close()
    return refs


def assert_rows_equal(got, j, ref, label, keys=OUT_KEYS + STATE_ALL + CTG):
    for k in keys:
        assert np.array_equal(np.asarray(got[k][j]).ravel(), np.asarray(ref[k]).ravel(), equal_nan=True), (label, k)


def oracle(plant, kw, t, dtype=np.float64):
    return Oracle(default_cfg(plant, cores=1, spawn_threads=0, **dict(kw, total_time=t)), dtype)


# ---------------------------------------------------------------------------------------------------------------- CPU 1: the surface
def test_entry_points_are_exported_declared_and_bound():
    lib = C.CDLL(pyddp.library_path())
    header = open(os.path.join(ROOT, "include", "pddp.h")).read()
    for sym in ("pddp_set_horizon_time_problems", "pddp_get_horizon_time_problems"):
        assert getattr(lib, sym) is not None
    assert "int pddp_set_horizon_time_problems(pddp_handle h, int count, const int* idx, const double* total_time" in header
    assert "int pddp_get_horizon_time_problems(pddp_handle h, int count, const int* idx, double* total_time" in header
    assert "double* time_step" in header
    for name in ("set_horizon_time_problems", "get_horizon_time_problems"):
        assert callable(getattr(pyddp.Solver, name))


# ---------------------------------------------------------------------------------------------------------------- CPU 2: the host-only code under the sanitizers
def test_host_only_code_as_a_stand_alone_program(tmp_path):
    """tests/native/horizon_time_host_check.cpp (its own main, -fsanitize=address,undefined): every refusal, the step of a given time against time_step<T> of a
    configuration with that total_time for both element types, and problem_dt on exactly-sized buffers for a StepTab policy and the policies below it"""
    exe = str(tmp_path / "horizon_time_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "horizon_time_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "horizon_time_host_check: ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------- CPU 3: the float32 yardstick can be met
F32_SEED = {1: 1, 2: 1, 3: 1}                                       # the problem of each plant's float32 GPU test (checked on the CPU: the two oracles agree on every iteration of it)
F32_TIME = horizon_time(32, 1)                                      # 0.6 s: not the handle's 1.0 s
_F32 = {}


def f32_case(plant):
    """the float32 GPU test's problem and the two oracles' solves at the non-default time, computed once"""
    if plant not in _F32:
        kw = dict(base_kw(plant, 32, 4, 8, 3), tol_cost=0.0)
        p32 = problem(plant, 32, 0, F32_SEED[plant])
        p64 = {k: v.astype(np.float64) for k, v in p32.items()}
        r32 = oracle(plant, kw, F32_TIME, np.float32).run_ilqr_gpusem(p32["x0"], p32["u0"], p32["xg"])
        r64 = oracle(plant, kw, F32_TIME, np.float64).run_ilqr_gpusem(p64["x0"], p64["u0"], p64["xg"])
        agree = next((i for i in range(r64["iters"] + 1) if r32["alphaOut"][i] != r64["alphaOut"][i]), r64["iters"] + 1)
        _F32[plant] = dict(kw=kw, p32=p32, r32=r32, r64=r64, agree=agree)
    return _F32[plant]


@pytest.mark.parametrize("plant", [1, 2, 3])
def test_float32_and_float64_oracles_agree_on_the_leading_iterations(plant):
    c = f32_case(plant)
    print("plant %d: the oracles agree on %d leading entries of alphaOut: %s / %s" % (plant, c["agree"], list(c["r32"]["alphaOut"]), list(c["r64"]["alphaOut"])))
    assert c["agree"] >= 3 + 1, (c["r32"]["alphaOut"], c["r64"]["alphaOut"])      # entry 0 is the load; at least 3 iterations behind it
    assert sum(a >= 0 for a in c["r64"]["alphaOut"][1: c["agree"]]) >= 2, "the case must accept iterations"
    # the time matters: the same problem at the handle's default time takes other steps
    kw, p = c["kw"], {k: v.astype(np.float64) for k, v in c["p32"].items()}
    other = oracle(plant, kw, kw["total_time"]).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
    assert not np.array_equal(other["Jout"], c["r64"]["Jout"])


# ---------------------------------------------------------------------------------------------------------------- GPU 4: a table of default entries is no table
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("fam", FAMILY_PARAMS)
def test_a_step_table_of_default_entries_solves_bit_for_bit_like_a_handle_without_one(fam, dtype):
    B, plant, N = min(fam["B"], 5), fam["plant"], fam["kw"]["N"]
    probs = problems(plant, N, dtype, B)
    outs, names = [], []
    for with_table in (False, True):
        s = handle(fam, dtype, B)
        cost_and_goal_tables(s, plant, N, dtype)                     # both: cost and goal tables, built-in rows, no problem flagged
        if with_table:
            s.set_horizon_time_problems(list(range(B)), [fam["kw"]["total_time"]] * B)
            t, st = s.get_horizon_time_problems(list(range(B)))
            assert t.tolist() == [fam["kw"]["total_time"]] * B and st.tolist() == [float(np_type(dtype)(fam["kw"]["total_time"] / (N - 1)))] * B
        names.append(kernel_names(s))
        assert all(any(h.startswith(n) for h in names[-1]) for n in fam["names"])
        reset_like_fresh(s)
        s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
        after_load = {k: s.get(k).copy() for k in ("H", "g", "AB", "Jout")}
        run_until_done(s)
        res = collect(s)
        res.update({"load_" + k: v for k, v in after_load.items()})
        res.update({"arr_" + k: s.get(k) for k in ARRAYS})
        outs.append(res)
        s.close()
    assert names[0] == names[1], "the step table changed the kernel family"
    plain, table = outs
    assert len(set(plain["iter"])) >= 2, ("the problems must exit at different iterations", plain["iter"])
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(table[k]), equal_nan=True), (fam["key"], dtype, k)


# ---------------------------------------------------------------------------------------------------------------- GPU 5: a batch with mixed times is B single-problem handles
def mixed_batch_against_singles(fam, dtype, B, **load_kw):
    plant, N = fam["plant"], fam["kw"]["N"]
    probs, times = problems(plant, N, dtype, B), horizon_times(N, B)
    refs = single_refs(fam, dtype, probs, times, **load_kw)
    s1 = handle(fam, dtype, 1)
    plain = solve_single(s1, probs[1], **load_kw)                    # problem 1 at the default time
    s1.close()
    assert len({int(r["iter"]) for r in refs}) >= 2, "the problems must exit at different iterations"
    assert not np.array_equal(refs[1]["Jout"], plain["Jout"]) and not np.array_equal(refs[1]["AB0"], plain["AB0"]), "the horizon time changed nothing"
    for use_graph in (1, 0):
        label = "%s dtype=%d use_graph=%d" % (fam["key"], dtype, use_graph)
        s = handle(fam, dtype, B, use_graph)
        set_times(s, times)
        reset_like_fresh(s)
        s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1, **load_kw)
        first = {k: s.get(k).reshape(B, -1) for k in ("AB", "H", "g")}
        for b in range(B):
            for k in ("AB", "H", "g"):
                assert np.array_equal(first[k][b], refs[b][k + "0"].ravel(), equal_nan=True), (label, k, "after the load, slot", b)
        run_until_done(s)
        got = collect(s)
        for b in range(B):
            assert_rows_equal(got, b, refs[b], (label, "slot", b))
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("fam", FAMILY_PARAMS)
def test_batch_with_mixed_times_equals_single_problem_handles(fam, dtype):
    mixed_batch_against_singles(fam, dtype, fam["B"])


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [pytest.param(family(k), id=k) for k in ("pend-coop", "cart-ts", "quad-mq-fused-cf-kb16")])
def test_mixed_times_with_the_initial_rollout_of_the_load(fam):
    """pddp_load_ex(forward_rollout = 1): the load's own rollout integrates with the problem's step too"""
    mixed_batch_against_singles(fam, 1, 5, forward_rollout=1)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["cart-coop-M1-euler", "quad-gl32-ts-gl8"])
def test_mixed_times_with_the_finite_difference_jacobian(key):
    """use_finite_diff = 1 (the Euler rule's [A B] by central differences): the quotient is scaled by the problem's own step"""
    fam = family(key)
    fam = dict(fam, kw=dict(fam["kw"], use_finite_diff=1, finite_diff_epsilon=1e-5))
    mixed_batch_against_singles(fam, 1, 5)


# ---------------------------------------------------------------------------------------------------------------- GPU 6: float64 against the oracle
def check_against_oracle(out, b, ref, label):
    """the bounds of tests/test_solver_parity.py test_other_plants_float64 (as tests/test_goal_trajectory.py takes them)"""
    it = ref["iters"]
    assert out["iters"][b] == it, (label, out["iters"][b], it)
    assert list(out["alphaOut"][b][: it + 1]) == list(ref["alphaOut"][: it + 1]), (label, out["alphaOut"][b], ref["alphaOut"])
    np.testing.assert_allclose(out["Jout"][b][: it + 1], ref["Jout"][: it + 1], rtol=1e-7)
    np.testing.assert_allclose(out["x"][b].ravel(), ref["x"], rtol=0, atol=1e-7 * max(np.abs(ref["x"]).max(), 1))


ORACLE_CASES = [pytest.param(1, base_kw(1, 16, 4, 4, 1), None, id="pend-M4-euler"), pytest.param(1, base_kw(1, 32, 1, 4, 3), None, id="pend-M1-rk3"),
                pytest.param(2, base_kw(2, 32, 4, 8, 3), None, id="cart-M4-rk3"), pytest.param(2, base_kw(2, 16, 1, 4, 2), None, id="cart-M1-midpoint"),
                pytest.param(3, base_kw(3, 16, 4, 8, 1), None, id="quad-M4-euler"), pytest.param(3, base_kw(3, 16, 1, 4, 2), None, id="quad-M1-midpoint"),
                pytest.param(3, base_kw(3, 32, 4, 8, 3), None, id="quad-M4-rk3"), pytest.param(3, base_kw(3, 16, 1, 8, 3), None, id="quad-M1-rk3")]
PINNED_ORACLE = [pytest.param(f["plant"], f["kw"], f["sel"], id=f["key"] + "-pinned") for f in (family("pend-ts"), family("cart-cf-gl-kb16"), family("quad-mq-fused-cf-kb16"))]


@pytest.mark.gpu
@pytest.mark.parametrize("plant,kw,sel", ORACLE_CASES + PINNED_ORACLE)
def test_float64_batch_with_mixed_times_follows_the_oracle(plant, kw, sel):
    """B = 4 problems with four different times, on the library's own selection for the shape or a pinned family: after pddp_load [A B], H, g and the initial cost
    against the oracle's ora_next_iteration_setup / ora_total_cost at total_time = t_b knot by knot, at the float64 bound of tests/test_phase_parity.py (1e-9 of the
    largest magnitude), then the whole solves decision for decision at the bounds of tests/test_solver_parity.py."""
    npos, n, m = DIMS[plant]
    N, B = kw["N"], 4
    kw = dict(kw, tol_cost=0.0)
    probs, times = problems(plant, N, 1, B), horizon_times(N, B)
    s = make_solver("hip", plant, dtype=1, batch=B, **(dict(kw, kernels=dict(sel)) if sel else kw))
    set_times(s, times)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    AB, H, g, st = s.get("AB").reshape(B, N, n * (n + m)), s.get("H").reshape(B, N, n + m, n + m), s.get("g").reshape(B, N, n + m), s.get_state()
    for b in range(B):
        o = oracle(plant, kw, times[b])
        ABo, Ho, go = o.next_iteration_setup(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        ABo, Ho, go = ABo.reshape(N, n * (n + m)), Ho.reshape(N, n + m, n + m), go.reshape(N, n + m)
        for k in range(N):
            if k < N - 1:
                assert np.abs(AB[b][k] - ABo[k]).max() <= 1e-9 * np.abs(ABo[: N - 1]).max(), (b, k, "[A B] after the load")
            assert np.abs(H[b][k] - Ho[k]).max() <= 1e-9 * max(np.abs(Ho[k]).max(), 1e-30) or not Ho[k].any(), (b, k, "H after the load")
            assert np.abs(g[b][k] - go[k]).max() <= 1e-9 * np.abs(go).max(), (b, k, "g after the load")
        J0 = o.total_cost(1, probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        assert abs(st[b].prevJ - J0) <= 1e-9 * abs(J0), (b, st[b].prevJ, J0)
    # the steps differ, so must the Jacobians of two problems' first knots (same plant, nearly the same state)
    assert not np.array_equal(AB[0][0], AB[1][0])
    run_until_done(s)
    out = s.store()
    out["iters"] = np.array([x.iter for x in s.get_state()])
    accepted = 0
    for b in range(B):
        ref = oracle(plant, kw, times[b]).run_ilqr_gpusem(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        accepted += sum(a >= 0 for a in ref["alphaOut"][1: ref["iters"] + 1])
        check_against_oracle(out, b, ref, (plant, b))
    assert accepted >= 3, "the cases must accept iterations"
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 7: float32 against the oracles
@pytest.mark.gpu
@pytest.mark.parametrize("plant", [1, 2, 3])
def test_float32_with_a_non_default_time_follows_the_oracles_over_the_leading_iterations(plant):
    """the rule of tests/test_diag_costs.py / tests/test_goal_trajectory.py: alphaOut equal to the float32 AND the float64 oracle over the leading iterations, J there
    inside max(1e-4, 5 x the float32 oracle's own error).  The number of leading iterations required is exactly what the two ORACLES agree on for the problem
    (test_float32_and_float64_oracles_agree_on_the_leading_iterations holds that to at least 3).  Slot 1 of a batch of two carries the time; slot 0 keeps the default."""
    c = f32_case(plant)
    kw, p32, r32, r64, agree = c["kw"], c["p32"], c["r32"], c["r64"], c["agree"]
    s = make_solver("hip", plant, dtype=0, batch=2, kernels=dict(cf="coop"), **kw)
    s.set_horizon_time_problems([1], [F32_TIME])
    out = s.solve(stack([p32, p32], "x0"), stack([p32, p32], "u0"), stack([p32, p32], "xg"))
    lead = next((i for i in range(r64["iters"] + 1) if not (out["alphaOut"][1][i] == r32["alphaOut"][i] == r64["alphaOut"][i])), r64["iters"] + 1)
    print("plant %d: alphaOut %s, oracle32 %s, oracle64 %s" % (plant, list(out["alphaOut"][1]), list(r32["alphaOut"]), list(r64["alphaOut"])))
    assert lead >= agree, (out["alphaOut"][1], r32["alphaOut"], r64["alphaOut"])
    for i in range(lead):
        ek, eo = abs(float(out["Jout"][1][i]) - r64["Jout"][i]) / r64["Jout"][i], abs(float(r32["Jout"][i]) - r64["Jout"][i]) / r64["Jout"][i]
        print("  iteration %d: J error %.3g, the float32 oracle's %.3g" % (i, ek, eo))
        assert ek <= max(1e-4, 5 * eo), (i, ek, eo)
    assert not np.array_equal(out["Jout"][0], out["Jout"][1]), "slot 0 runs at the default time"
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 8: named slots
QUAD_SLOTS = dict(key="quad-slots", plant=3, kw=base_kw(3, 16, 4, 16, 3, max_iter=10), sel=dict(cf_bp="mq", cf_fp="cf", cf_nis="kb16"),
                  names=("k_bp_mq", "k_sweep_maps", "k_fp_cf", "k_nis_kb"), B=5)
UNTOUCHED = ("xb", "ucur", "dcur", "P", "Pp", "p", "pp", "AB", "H", "g", "KT", "du", "xGoal", "Jout", "alphaOut")


def snapshot(s):
    B = s.cfg.batch
    snap = {k: s.get(k).reshape(B, -1).copy() for k in UNTOUCHED}
    snap.update(state_rows(s, range(B)))
    return snap


def tables(s):
    """what the handle's three tables hold for every slot"""
    idx = list(range(s.cfg.batch))
    t, st = s.get_horizon_time_problems(idx)
    G, has = s.get_goal_trajectory_problems(idx)
    return dict(times=t, steps=st, cost=s.get_diag_cost_problems(idx), goal=G, has=has)


def assert_same(a, b, rows, label, keys=None):
    for k in (keys or a):
        assert np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k])[rows], equal_nan=True), (label, k)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_refill_of_named_slots_with_their_own_times(dtype):
    """load_problems into slots of a running batch: the named slots run with the times the setter just gave them and equal fresh single-problem handles created with
    those times; the unnamed slots -- running or exited -- are unchanged bit for bit by the setter and the refill, and finish as they would have"""
    fam, B, N = QUAD_SLOTS, QUAD_SLOTS["B"], 16
    first, late = problems(3, N, dtype, B), problems(3, N, dtype, 2, skip=11)
    first_times, late_times = horizon_times(N, B), [0.45 * N / 32.0, N / 32.0]      # one refilled slot gets a new time, the other returns to the default
    ref_first = single_refs(fam, dtype, first, first_times)
    ref_late = single_refs(fam, dtype, late, late_times)
    s = handle(fam, dtype, B)
    set_times(s, first_times)
    reset_like_fresh(s)
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    s.iterate(2); s.sync()
    done, _ = s.status()
    slots = [4, 1]
    others = [b for b in range(B) if b not in slots]
    assert any(not done[b] for b in others), "no running slot among the others"
    before, tab_before = snapshot(s), tables(s)
    s.set_horizon_time_problems(slots, late_times)
    assert_same(before, snapshot(s), slice(None), "the setter changed a slot", UNTOUCHED + STATE_ALL)      # [A B] and the trajectory in a slot are not rebuilt
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    assert_same(before, snapshot(s), others, "another slot changed", UNTOUCHED + STATE_ALL)
    tab_after = tables(s)
    assert_same(tab_before, tab_after, others, "another slot's table entries changed")
    assert tab_after["times"][slots].tolist() == late_times
    assert tab_after["steps"][slots].tolist() == [float(np_type(dtype)(t / (N - 1))) for t in late_times]
    run_until_done(s)
    got = collect(s)
    for j, b in enumerate(slots):
        assert_rows_equal(got, b, ref_late[j], ("refilled slot", b))
    for b in others:
        assert_rows_equal(got, b, ref_first[b], ("unnamed slot", b))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift,clear_vars", [(1, 0), (0, 0), (1, 1), (0, 1)])
def test_control_cycles_of_named_slots_run_with_their_own_times(shift, clear_vars):
    """float32 quadrotor on k_fp_cf, B = 4 with four different times: a solve seeds every slot of the subject and of a twin; then pddp_mpc_load_problems and two
    pddp_mpc_solve_problems cycles on slots [3, 0] against pddp_mpc_load / pddp_mpc_solve of the WHOLE twin (which test 9 holds to single-problem handles): the named
    rows equal the twin's, the slots that are not named keep every array, their state and their table entries."""
    fam, B, dtype, N = QUAD_SLOTS, 4, 0, 16
    kw = dict(fam["kw"], tol_cost=0.0, max_iter=4)
    probs, times = problems(3, N, dtype, B), horizon_times(N, B)
    named, others = [3, 0], [1, 2]
    xg = stack(probs, "xg").reshape(B, -1)
    subj, twin = [make_solver("hip", 3, dtype=dtype, batch=B, kernels=dict(fam["sel"]), **kw) for _ in range(2)]
    seeds = []
    for s in (subj, twin):
        set_times(s, times)
        seeds.append(s.solve(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg")))
    assert_same(seeds[0], seeds[1], slice(None), "seed solve", OUT_KEYS)
    seed = seeds[0]
    before, tab_before = snapshot(subj), tables(subj)
    xa = seed["x"][:, 1].copy()
    # the load stage alone
    subj.mpc_load_problems(named, xa[named], xg[named], [shift, shift], clear_vars=clear_vars)
    twin.mpc_load(xa, xg, shift, clear_vars=clear_vars)
    a, t = snapshot(subj), snapshot(twin)
    assert_same(a, t, named, "load stage, named slots", ("xb", "ucur", "dcur", "P", "Pp", "p", "pp", "KT", "du", "xGoal"))
    assert_same(before, a, others, "load stage: another slot changed", UNTOUCHED + STATE_ALL)
    # two cycles from there (the load stage shifted once more: the same on both sides)
    for cycle in range(2):
        got = subj.mpc_solve_problems(named, xa[named], xg[named], [shift, shift], clear_vars=clear_vars, max_iter=4)
        ref = twin.mpc_solve(xa, xg, shift, clear_vars=clear_vars, max_iter=4)
        for j, b in enumerate(named):
            for k in MPC_KEYS:
                assert np.array_equal(np.asarray(got[k][j]), np.asarray(ref[k][b]), equal_nan=True), ("cycle", cycle, "slot", b, k)
        a, t = snapshot(subj), snapshot(twin)
        assert_same(a, t, named, ("cycle", cycle, "named slots"), UNTOUCHED + STATE_ALL)
        xa = ref["x"][:, 1].copy()
    assert_same(before, snapshot(subj), others, "another slot changed", UNTOUCHED + STATE_ALL)
    assert_same(tab_before, tables(subj), slice(None), "a cycle changed a table")
    subj.close(); twin.close()


@pytest.mark.gpu
def test_260_named_slots_of_300_with_their_own_times_go_through_two_chunks():
    """float32 cart-pole, thread-serial kernels: 260 of 300 slots in shuffled order cross the 256-slot chunks of the intake area; slot b runs at horizon_time(N, b)"""
    fam, B, P, K, dtype = family("cart-ts"), 300, 11, 260, 0
    N = fam["kw"]["N"]
    kw = dict(fam["kw"], tol_cost=0.0, max_iter=4)
    base = problems(2, N, dtype, P)
    probs, times = [base[b % P] for b in range(B)], horizon_times(N, B)
    rng = np.random.default_rng(93)
    left_out = set(int(v) for v in rng.permutation(np.arange(1, B - 1))[: B - K])      # (the first and the last slot are named)
    slots = [int(v) for v in rng.permutation(B) if int(v) not in left_out]
    others = sorted(left_out)
    assert len(slots) == K and slots != sorted(slots) and B - 1 in slots and 0 in slots
    shift = rng.integers(0, 3, B).astype(np.int32)
    xg = stack(probs, "xg").reshape(B, -1)
    subj, twin = [make_solver("hip", 2, dtype=dtype, batch=B, kernels=dict(fam["sel"]), **kw) for _ in range(2)]
    for s in (subj, twin):
        set_times(s, times)
        seed = s.solve(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"))
    before, tab_before = snapshot(subj), tables(subj)
    xa = seed["x"][:, 1].copy()
    got = subj.mpc_solve_problems(slots, xa[slots], xg[slots], shift[slots], clear_vars=0, max_iter=4)
    ref = twin.mpc_solve(xa, xg, shift, clear_vars=0, max_iter=4)
    for k in MPC_KEYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k])[slots], equal_nan=True), k
    a, t = snapshot(subj), snapshot(twin)
    assert_same(a, t, slots, "named slots", UNTOUCHED + STATE_ALL)
    assert_same(before, a, others, "another slot changed", UNTOUCHED + STATE_ALL)
    assert_same(tab_before, tables(subj), slice(None), "the cycle changed a table")
    # slots that differ only in their time solve differently: slots b and b + 55 share inputs AND time, b and b + 11 only the inputs
    assert np.array_equal(seed["x"][0], seed["x"][55]) and not np.array_equal(seed["x"][0], seed["x"][11])
    subj.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 9: whole-handle control cycles
@pytest.mark.gpu
@pytest.mark.parametrize("fam,dtype", [pytest.param(QUAD_SLOTS, 0, id="quad-cf-f32"), pytest.param(family("cart-ts"), 1, id="cart-ts-f64"),
                                       pytest.param(family("pend-coop"), 0, id="pend-coop-f32")])
def test_whole_handle_control_cycles_equal_single_problem_handles(fam, dtype):
    """three pddp_mpc_solve cycles (shifts 1, 0, 2) on a batch of 5 with mixed times against single-problem handles created with those cfg.total_time: outputs and state
    records bit for bit.  Problem 2 also follows a goal path on both sides: the cursor and the window move by the shift in knots, whatever the step is."""
    plant, N, B = fam["plant"], fam["kw"]["N"], 5
    npos, n, m = DIMS[plant]
    T = np_type(dtype)
    kw = dict(fam["kw"], tol_cost=0.0, max_iter=4)
    probs, times = problems(plant, N, dtype, B), horizon_times(N, B)
    xg = stack(probs, "xg").reshape(B, n)
    shifts, cap = (1, 0, 2), N + 6
    path = (np.tile(probs[2]["xg"], (cap, 1)) + 0.003 * np.arange(1, cap + 1)[:, None] * (1.0 + 0.1 * np.arange(n))[None, :]).astype(T)

    def with_path(s, slot):
        s.reserve_goal_path(cap)
        s.set_goal_path_problems([slot], path[None], s.GOAL_PATH_HOLD)

    s = make_solver("hip", plant, dtype=dtype, batch=B, kernels=dict(fam["sel"]), **kw)
    set_times(s, times)
    with_path(s, 2)
    outs = [s.solve(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"))]
    states = [state_rows(s, range(B))]
    for sh in shifts:
        outs.append(s.mpc_solve(outs[-1]["x"][:, 1].copy(), xg, sh, clear_vars=0, max_iter=4))
        states.append(state_rows(s, range(B)))
    cursor = s.get_goal_path_problems([2], rows=False)[2][0]
    assert cursor == sum(shifts), "the cursor advances by the shifts in knots"
    s.close()
    for b in range(B):
        s1 = make_solver("hip", plant, dtype=dtype, batch=1, kernels=dict(fam["sel"]), **dict(kw, total_time=times[b]))
        if b == 2:
            with_path(s1, 0)
        one = s1.solve(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        for k in OUT_KEYS:
            assert np.array_equal(np.asarray(one[k][0]), np.asarray(outs[0][k][b]), equal_nan=True), ("seed solve", b, k)
        for c, sh in enumerate(shifts):
            one = s1.mpc_solve(one["x"][:, 1].copy(), xg[[b]], sh, clear_vars=0, max_iter=4)
            for k in MPC_KEYS:
                assert np.array_equal(np.asarray(one[k][0]), np.asarray(outs[c + 1][k][b]), equal_nan=True), ("cycle", c, "problem", b, k)
            st1 = state_rows(s1, [0])
            for f in STATE_ALL:
                assert np.array_equal(st1[f][0], states[c + 1][f][b], equal_nan=True), ("cycle", c, "problem", b, "state", f)
        s1.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 10: setter semantics, round trip, refusals
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_setter_semantics_round_trip_and_refusals(dtype):
    fam = family("cart-ts")
    B, plant, N, n = 5, 2, fam["kw"]["N"], 4
    T = np_type(dtype)
    default = fam["kw"]["total_time"]
    probs, times = problems(plant, N, dtype, B), horizon_times(N, B)
    step = lambda t: float(T(t / (N - 1)))
    s = handle(fam, dtype, B)
    t, st = s.get_horizon_time_problems([4, 0])                      # before the first setter call (and before any load)
    assert t.tolist() == [default] * 2 and st.tolist() == [step(default)] * 2 and t.dtype == st.dtype == np.float64
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    s.iterate(1); s.sync()
    lib, EINVAL = s.lib, -1
    lib.pddp_set_horizon_time_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_get_horizon_time_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good_idx, tw = np.array([3, 0], np.int32), np.array([0.7, 0.3])
    tiny, huge = float(np.finfo(T).tiny) * (N - 1) * 0.25, (1e39 * (N - 1) if dtype == 0 else np.inf)
    bad = [("count 0", 0, good_idx, tw), ("count < 0", -2, good_idx, tw), ("idx null", 2, None, tw), ("times null", 2, good_idx, None),
           ("index == batch", 2, np.array([0, B], np.int32), tw), ("index < 0", 2, np.array([-1, 2], np.int32), tw), ("index twice", 2, np.array([2, 2], np.int32), tw),
           ("nan", 2, good_idx, np.array([0.7, np.nan])), ("inf", 2, good_idx, np.array([np.inf, 0.3])), ("-inf", 2, good_idx, np.array([0.7, -np.inf])),
           ("zero", 2, good_idx, np.array([0.0, 0.3])), ("negative", 2, good_idx, np.array([0.7, -0.5])),
           ("step underflows", 2, good_idx, np.array([0.7, tiny])), ("step overflows", 2, good_idx, np.array([huge, 0.3]))]
    values_only = ("times null", "nan", "inf", "-inf", "zero", "negative", "step underflows", "step overflows")

    def refused_everywhere(label):
        before = snapshot(s)
        rows = s.get_horizon_time_problems(list(range(B)))
        for what, count, idx, t_ in bad:
            assert lib.pddp_set_horizon_time_problems(s.h, count, ptr(idx), ptr(t_)) == EINVAL, (label, what)
            assert len(lib.pddp_last_error()) > 0, (label, what, "a refusal carries a message")
            if what not in values_only:
                o1, o2 = np.zeros(2), np.zeros(2)
                assert lib.pddp_get_horizon_time_problems(s.h, count, ptr(idx), ptr(o1), ptr(o2)) == EINVAL, (label, what)
                assert not o1.any() and not o2.any()
        after = snapshot(s)
        for k in UNTOUCHED + STATE_ALL:
            assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), (label, "a refused call changed", k)
        again = s.get_horizon_time_problems(list(range(B)))
        assert np.array_equal(again[0], rows[0]) and np.array_equal(again[1], rows[1]), (label, "a refused call changed the table")

    refused_everywhere("without a table")
    names = kernel_names(s)
    # pddp_simulate_batch works on a handle without a step table
    xa0 = s.store()["x"][:, 0].copy()
    sim = s.simulate_batch(0.0, 1000.0, substeps=4, xActual=xa0)
    assert np.isfinite(sim[0]).all()
    reset_like_fresh(s)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    s.iterate(1); s.sync()
    # the setter on loaded slots changes neither [A B], the trajectory nor the state record until the next load
    before = snapshot(s)
    s.set_horizon_time_problems([3, 1], [times[3], times[1]])
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), ("the setter changed", k)
    assert kernel_names(s) == names                                 # (runs a sweep: the slots are reloaded below)
    assert np.array_equal(s.get_diag_cost_problems(list(range(B))), np.tile(np.asarray(BUILTIN[plant], T).astype(np.float64), (B, 1)))      # the cost table it brought: built-in rows
    assert s.get_goal_trajectory_problems(list(range(B)))[1].tolist() == [0] * B                                                           # the goal table it brought: no problem flagged
    t, st = s.get_horizon_time_problems(list(range(B)))              # the round trip: times exactly, steps NumPy's T(t / (N - 1)); unnamed entries the default
    want = [default, times[1], default, times[3], default]
    assert t.tolist() == want and st.tolist() == [step(v) for v in want]
    t, st = s.get_horizon_time_problems([3, 2])
    assert t.tolist() == [times[3], default] and st.tolist() == [step(times[3]), step(default)]
    assert lib.pddp_get_horizon_time_problems(s.h, 1, ptr(good_idx), None, None) == 0      # both outputs may be NULL
    o = np.zeros(1)
    assert lib.pddp_get_horizon_time_problems(s.h, 1, ptr(good_idx), None, ptr(o)) == 0 and o[0] == step(times[3])
    assert lib.pddp_get_horizon_time_problems(s.h, 1, ptr(good_idx), ptr(o), None) == 0 and o[0] == times[3]
    refused_everywhere("with a table")
    # pddp_simulate_batch refuses on a handle with a table, with a message that names the reason
    with pytest.raises(pyddp.PddpError, match="horizon time"):
        s.simulate_batch(0.0, 1000.0, substeps=4, xActual=xa0)
    # pddp_get_config keeps reporting the handle-wide time
    cfg = pyddp.PddpConfig()
    lib.pddp_get_config.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.pddp_get_config(s.h, C.byref(cfg)) == 0 and cfg.total_time == default
    # the next load reads the entries: [A B] differs from a handle without a table exactly in the named problems
    never = handle(fam, dtype, B)
    never.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    AB0 = never.get("AB").reshape(B, -1)
    reset_like_fresh(s)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    AB = s.get("AB").reshape(B, -1)
    assert [bool(np.array_equal(AB[b], AB0[b])) for b in range(B)] == [True, False, True, False, True]
    # setting cfg.total_time again is how a problem returns to the default
    s.set_horizon_time_problems([1, 3], [default, default])
    assert np.array_equal(s.get("AB").reshape(B, -1), AB), "the setter rebuilt [A B] of a loaded slot"
    reset_like_fresh(s); reset_like_fresh(never)
    for h in (s, never):
        h.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
        run_until_done(h)
    a, b_ = collect(s), collect(never)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b_[k]), equal_nan=True), ("back at the default", k)
    s.close(); never.close()


@pytest.mark.gpu
def test_arm_handles_refuse_both():
    EINVAL = -1
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    arm = make_solver("hip", 4, dtype=0, batch=2, N=32, M=4, A=8, wafr_urdf=1, total_time=0.5)
    idx, t, o1, o2 = np.array([0, 1], np.int32), np.array([0.4, 0.6]), np.zeros(2), np.zeros(2)
    lib = arm.lib
    lib.pddp_set_horizon_time_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_get_horizon_time_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.pddp_set_horizon_time_problems(arm.h, 2, ptr(idx), ptr(t)) == EINVAL
    assert lib.pddp_get_horizon_time_problems(arm.h, 2, ptr(idx), ptr(o1), ptr(o2)) == EINVAL
    assert not o1.any() and not o2.any()
    arm.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 11: the captured graph
@pytest.mark.gpu
@pytest.mark.parametrize("fam", [pytest.param(family(k), id=k) for k in ("cart-cf-gl-kb16", "quad-mq-fused-cf-kb16", "pend-coop")])
def test_graph_replay_follows_the_step_table(fam):
    """use_graph = 1: iterate, set a first time, reload and iterate, set another, reload and iterate -- bit for bit a use_graph = 0 handle given the same calls.
    The first setter call drops the captured graph (other kernels); the second only writes an entry, which the re-captured graph reads."""
    dtype, B, plant, N = 0, 3, fam["plant"], fam["kw"]["N"]
    probs = problems(plant, N, dtype, B)
    outs = []
    for use_graph in (1, 0):
        s = handle(fam, dtype, B, use_graph)
        stages = []
        for t in (None, horizon_time(N, 1), horizon_time(N, 2)):
            if t is not None:
                s.set_horizon_time_problems([1], [t])
            reset_like_fresh(s)
            s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
            s.iterate(2); s.iterate(3); s.sync()
            stages.append(collect(s))
        outs.append(stages)
        s.close()
    graph, plain = outs
    for i in range(3):
        for k in plain[i]:
            assert np.array_equal(np.asarray(graph[i][k]), np.asarray(plain[i][k]), equal_nan=True), (fam["key"], "stage", i, k)
    for i, j in ((0, 1), (1, 2)):
        assert not np.array_equal(plain[i]["Jout"][1], plain[j]["Jout"][1]), "the time changed nothing"
        assert np.array_equal(plain[i]["Jout"][0], plain[j]["Jout"][0]) and np.array_equal(plain[i]["Jout"][2], plain[j]["Jout"][2])
