"""Per-knot goal trajectories of the pendulum, cart-pole and quadrotor: pddp_goal_trajectory_size / pddp_set_goal_trajectory_problems /
pddp_get_goal_trajectory_problems / pddp_clear_goal_trajectory_problems (csrc/goal_traj_table.hpp, csrc/plants.hpp GoalTab).

A problem with a trajectory G[N][n] reads G[k] wherever the cost, its gradient or the initial cost of knot k read xGoal; one without reads xGoal as always.

Yardsticks:
  * a handle with a table of built-in cost rows and NO trajectory for a trajectory whose rows all equal xGoal -- bit for bit, every array pddp_get_array names
    (tests/test_diag_costs.py holds such a handle bit for bit to one without a table);
  * a SINGLE-PROBLEM handle pinned to the same kernels and given the problem's trajectory (or none) for a batch with mixed trajectories -- bit for bit;
  * the oracle's plug-in plant with tests/plugin_goal_traj/goal_traj_shim.cpp (the "shim-oracle"): dynamics forwarded to the oracle's own plant 1, 2 or 3, the
    diagonal cost formulas with the goal taken from a table at the knot index the oracle passes.  The CPU test first holds the shim-oracle with every row equal to
    xGoal against the oracle's own plants.

The structure (FAMILIES pinned through pddp_config.kernels and asserted by name, problem(), solve_single, collect, assert_rows_equal) is that of
tests/test_diag_costs.py, restated here.  Shapes: N 16 / 32, M 1 / 4, A 4 / 8, A = 16 for the quadrotor families with k_fp_cf; batches 3, 5 and 67 (67: a wave of the
thread-serial and staged kernels holds several problems, the last wave is partial, problems with and without a trajectory share a wavefront).  Odd-numbered problems
get a trajectory, even-numbered ones none.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyddp
import oracle_binding
from backends import make_solver
from oracle_binding import Oracle, default_cfg, example_inputs, register_plugin

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
EXTRA_SWEEPS = 3
ENTRY_POINTS = ("pddp_goal_trajectory_size", "pddp_set_goal_trajectory_problems", "pddp_get_goal_trajectory_problems", "pddp_clear_goal_trajectory_problems")


def np_type(dtype):
    return np.float32 if dtype == 0 else np.float64


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


def handle(fam, dtype, batch, use_graph=1, **more):
    s = make_solver("hip", fam["plant"], dtype=dtype, batch=batch, use_graph=use_graph, kernels=dict(fam["sel"]), **dict(fam["kw"], **more))
    have = [n for n, _ in s.time_kernels(1)]
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


def trajectory(plant, N, dtype, prob, seed=0):
    """G[N][n] in the element type.  Positions move from the start state to xg along sin^2 (smooth, not linear in k); EVERY entry -- the velocities and the positions --
    carries a small offset that grows with k and differs per entry, so every row differs from both neighbours in every entry and row N - 1 is xg plus an offset of its
    own: an off-by-one knot, a segment-local index or a missed final row changes numbers."""
    npos, n, m = DIMS[plant]
    x0 = prob["x0"].astype(np.float64).reshape(N, n)[0]
    xg = prob["xg"].astype(np.float64)
    k = np.arange(N)
    s = np.sin(0.5 * np.pi * (k + 1) / N) ** 2
    G = np.tile(xg, (N, 1))
    G[:, :npos] = x0[:npos] + s[:, None] * (xg[:npos] - x0[:npos])
    G += 0.004 * (1.0 + 0.13 * np.arange(n) + 0.07 * seed)[None, :] * ((k + 1.0) / N)[:, None]
    G = G.astype(np_type(dtype))
    assert all((np.diff(G, axis=0) != 0).all(axis=0)) and (G[N - 1] != prob["xg"]).all()
    return G


def with_trajectory(b):
    return b % 2 == 1


def trajectories(plant, N, dtype, probs, skip=0):
    """per problem of the list: its trajectory (odd-numbered ones) or None"""
    return [trajectory(plant, N, dtype, p, skip + b) if with_trajectory(b) else None for b, p in enumerate(probs)]


def set_trajectories(s, trajs, slots=None):
    slots = list(range(len(trajs))) if slots is None else list(slots)
    named = [(q, G) for q, G in zip(slots, trajs) if G is not None]
    named.reverse()                                                  # unsorted on purpose
    if named:
        s.set_goal_trajectory_problems([q for q, _ in named], np.stack([G for _, G in named]))


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


def solve_single(s1, prob, G=None):
    """the yardstick: one problem on a single-problem handle in the state of a fresh one, given the problem's trajectory (or none), sweep by sweep until it exits"""
    if G is not None:
        s1.set_goal_trajectory_problems([0], G)
    else:
        s1.clear_goal_trajectory_problems([0])
    reset_like_fresh(s1)
    s1.load(prob["x0"], prob["u0"], prob["xg"], clear_vars=1)
    H0, g0 = s1.get("H").copy(), s1.get("g").copy()
    for _ in range(4 * s1.cfg.max_iter + 40):
        s1.iterate(1)
        done, _ = s1.status()
        if done[0]:
            break
    assert done[0], "the yardstick problem did not exit"
    res = {k: v[0] for k, v in collect(s1).items()}
    res["H0"], res["g0"] = H0, g0
    return res


def assert_rows_equal(got, j, ref, label, keys=OUT_KEYS + STATE_ALL + CTG):
    for k in keys:
        assert np.array_equal(np.asarray(got[k][j]).ravel(), np.asarray(ref[k]).ravel(), equal_nan=True), (label, k)


# ---------------------------------------------------------------------------------------------------------------- the shim-oracle
_SHIM = {}


def shim():
    if "lib" not in _SHIM:
        src = os.path.join(ROOT, "tests", "plugin_goal_traj", "goal_traj_shim.cpp")
        out = os.path.join(ROOT, "tests", "plugin_goal_traj", "libgoal_traj_shim.so")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", out, src])
        _SHIM["lib"], _SHIM["path"] = C.CDLL(out), out
    return _SHIM["lib"], _SHIM["path"]


def shim_oracle(plant, kw, G=None, dtype=np.float64, rec=None):
    """the oracle's plant 5 = plant `plant` with the diagonal record `rec` (default: the built-in one) and the goal trajectory G (None: the cost reads xg): same solver
    configuration as Oracle(default_cfg(plant, **kw))"""
    lib, path = shim()
    L = oracle_binding.lib()
    base = default_cfg(plant, cores=1, spawn_threads=0, **kw)
    npos, n, m = DIMS[plant]
    rec = np.ascontiguousarray(BUILTIN[plant] if rec is None else rec, np.float64)
    Gd = None if G is None else np.ascontiguousarray(G, np.float64)
    assert Gd is None or Gd.shape == (kw["N"], n)
    addr = lambda f: C.cast(f, C.c_void_p)
    lib.goal_traj_shim_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_void_p] * 4
    lib.goal_traj_shim_set(C.byref(base), n, m, kw["N"], rec.ctypes.data_as(C.c_void_p), None if Gd is None else Gd.ctypes.data_as(C.c_void_p), addr(L.ora_dynamics_f32),
                           addr(L.ora_dynamics_gradient_f32), addr(L.ora_dynamics_f64), addr(L.ora_dynamics_gradient_f64))
    register_plugin(path)
    cfg = default_cfg(plant, cores=1, spawn_threads=0, **kw)
    cfg.plant = 5
    return Oracle(cfg, dtype)


ORACLE_CASES = [pytest.param(1, base_kw(1, 16, 4, 4, 1), id="pend-M4-euler"), pytest.param(1, base_kw(1, 32, 1, 4, 3), id="pend-M1-rk3"),
                pytest.param(2, base_kw(2, 32, 4, 8, 3), id="cart-M4-rk3"), pytest.param(2, base_kw(2, 16, 1, 4, 2), id="cart-M1-midpoint"),
                pytest.param(3, base_kw(3, 16, 4, 8, 1), id="quad-M4-euler"), pytest.param(3, base_kw(3, 16, 1, 4, 2), id="quad-M1-midpoint"),
                pytest.param(3, base_kw(3, 32, 4, 8, 3), id="quad-M4-rk3"), pytest.param(3, base_kw(3, 16, 1, 8, 3), id="quad-M1-rk3")]


# ---------------------------------------------------------------------------------------------------------------- CPU 1: the surface
def test_entry_points_are_exported_declared_and_bound():
    lib = C.CDLL(pyddp.library_path())
    header = open(os.path.join(ROOT, "include", "pddp.h")).read()
    for sym in ENTRY_POINTS:
        assert getattr(lib, sym) is not None
    assert "int pddp_goal_trajectory_size(pddp_handle h);" in header
    assert "int pddp_set_goal_trajectory_problems(pddp_handle h, int count, const int* idx, const void* G" in header
    assert "int pddp_get_goal_trajectory_problems(pddp_handle h, int count, const int* idx, void* G" in header
    assert "int pddp_clear_goal_trajectory_problems(pddp_handle h, int count, const int* idx);" in header
    for name in ("goal_trajectory_size", "set_goal_trajectory_problems", "get_goal_trajectory_problems", "clear_goal_trajectory_problems", "has_goal_trajectory"):
        assert callable(getattr(pyddp.Solver, name))


# ---------------------------------------------------------------------------------------------------------------- CPU 2: the host-only code under the sanitizers
def test_host_only_code_as_a_stand_alone_program(tmp_path):
    """tests/native/goal_traj_host_check.cpp (its own main, -fsanitize=address,undefined): every argument check, the getter's block for a problem without a
    trajectory, and base / stride / row of problem_goal and goal_at on exactly-sized buffers"""
    exe = str(tmp_path / "goal_traj_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "goal_traj_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "goal_traj_host_check: ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------- CPU 3: the shim-oracle is the oracle
@pytest.mark.parametrize("plant,kw", ORACLE_CASES)
def test_shim_oracle_with_every_row_equal_to_the_goal_reproduces_the_oracles_own_plant(plant, kw):
    """Whole solves (ora_run_ilqr_gpusem, float64): identical iteration counts and alphaOut; J, x, u, KT with exact equality -- the shim's cost sums are the oracle's
    own statements (weight * pow(d, 2) in index order, 0.5 * sum) and its dynamics ARE the oracle's, as for tests/plugin_diag/diag_shim.cpp (measured deviation there:
    0).  Also: with a trajectory, g and the cost of knot k against a NumPy restatement that reads row k."""
    npos, n, m = DIMS[plant]
    N = kw["N"]
    kw = dict(kw, tol_cost=0.0)
    for seed in (1, 2):
        p = problem(plant, N, 1, seed)
        own = Oracle(default_cfg(plant, cores=1, spawn_threads=0, **kw), np.float64).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
        for G in (np.tile(p["xg"], (N, 1)), None):
            via = shim_oracle(plant, kw, G).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
            assert via["iters"] == own["iters"] and list(via["alphaOut"]) == list(own["alphaOut"])
            for k in ("Jout", "x", "u", "KT"):
                dev = float(np.abs(via[k] - own[k]).max())
                print("shim-oracle against the oracle's plant %d, problem %d, %s: max deviation %.3g" % (plant, seed, k, dev))
                assert dev == 0.0, (k, dev)
        assert sum(a >= 0 for a in own["alphaOut"][1: own["iters"] + 1]) >= 2, "the case must accept iterations"
    p = problem(plant, N, 1, 1)
    G = trajectory(plant, N, 1, p)
    o = shim_oracle(plant, kw, G)
    rec = BUILTIN[plant]
    q, r, qf = rec[:n], rec[n: n + m], rec[n + m:]
    rng = np.random.default_rng(5 + plant)
    for k in (0, 3, N - 2, N - 1):
        x, u = rng.normal(0, 1.5, n), rng.normal(0, 2.0, m)
        H, g = o.cost_grad(x, u, p["xg"], k)
        fin = k == N - 1
        gw = np.concatenate([qf * (x - G[k]), np.zeros(m)]) if fin else np.concatenate([q * (x - G[k]), r * u])
        cw = 0.5 * np.sum(qf * (x - G[k]) ** 2) if fin else 0.5 * (np.sum(q * (x - G[k]) ** 2) + np.sum(r * u ** 2))
        assert np.array_equal(g, gw) and np.array_equal(H.reshape(n + m, n + m), np.diag(np.concatenate([qf, np.zeros(m)]) if fin else np.concatenate([q, r])))
        assert abs(o.cost_func(x, u, p["xg"], k) - cw) <= 1e-14 * abs(cw)
    # the trajectory changes the solve
    a = shim_oracle(plant, kw, G).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
    b = shim_oracle(plant, kw, None).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
    assert not np.array_equal(a["Jout"], b["Jout"])


# ---------------------------------------------------------------------------------------------------------------- CPU 4: the float32 yardstick can be met
F32_SEED = {1: 1, 2: 1, 3: 1}                                       # the problem of each plant's float32 GPU test (chosen so that the two oracles agree on >= 3 leading iterations)
_F32 = {}


def f32_case(plant):
    """the float32 GPU test's problem, trajectory and the two shim-oracles' solves, computed once"""
    if plant not in _F32:
        kw = dict(base_kw(plant, 32, 4, 8, 3), tol_cost=0.0)
        p32 = problem(plant, 32, 0, F32_SEED[plant])
        G = trajectory(plant, 32, 0, p32)
        p64 = {k: v.astype(np.float64) for k, v in p32.items()}
        r32 = shim_oracle(plant, kw, G, np.float32).run_ilqr_gpusem(p32["x0"], p32["u0"], p32["xg"])
        r64 = shim_oracle(plant, kw, G, np.float64).run_ilqr_gpusem(p64["x0"], p64["u0"], p64["xg"])
        agree = next((i for i in range(r64["iters"] + 1) if r32["alphaOut"][i] != r64["alphaOut"][i]), r64["iters"] + 1)
        _F32[plant] = dict(kw=kw, p32=p32, G=G, r32=r32, r64=r64, agree=agree)
    return _F32[plant]


@pytest.mark.parametrize("plant", [1, 2, 3])
def test_float32_and_float64_shim_oracles_agree_on_the_leading_iterations(plant):
    c = f32_case(plant)
    print("plant %d: the oracles agree on %d leading entries of alphaOut: %s / %s" % (plant, c["agree"], list(c["r32"]["alphaOut"]), list(c["r64"]["alphaOut"])))
    assert c["agree"] >= 3 + 1, (c["r32"]["alphaOut"], c["r64"]["alphaOut"])      # entry 0 is the load; at least 3 iterations behind it
    assert sum(a >= 0 for a in c["r64"]["alphaOut"][1: c["agree"]]) >= 2, "the case must accept iterations"


# ---------------------------------------------------------------------------------------------------------------- GPU 5: a constant trajectory is no trajectory
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("fam", FAMILY_PARAMS)
def test_a_trajectory_of_xgoal_rows_solves_bit_for_bit_like_a_handle_without_a_trajectory(fam, dtype):
    B, plant, N = min(fam["B"], 5), fam["plant"], fam["kw"]["N"]
    probs = problems(plant, N, dtype, B)
    outs = []
    for with_traj in (False, True):
        s = handle(fam, dtype, B)
        s.set_diag_cost(BUILTIN[plant])                              # both: a table of built-in cost rows
        if with_traj:
            G = np.stack([np.tile(p["xg"], (N, 1)) for p in probs])
            s.set_goal_trajectory_problems(list(range(B)), G)
            got, has = s.get_goal_trajectory_problems(list(range(B)))
            assert np.array_equal(got, G) and has.tolist() == [1] * B
            names = [n for n, _ in s.time_kernels(1)]                 # (same names with a trajectory table: the family did not change)
            assert all(any(h.startswith(n) for h in names) for n in fam["names"])
        reset_like_fresh(s)
        s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
        after_load = {k: s.get(k).copy() for k in ("H", "g", "AB", "Jout")}
        run_until_done(s)
        res = collect(s)
        res.update({"load_" + k: v for k, v in after_load.items()})
        res.update({"arr_" + k: s.get(k) for k in ARRAYS})
        outs.append(res)
        s.close()
    plain, traj = outs
    assert len(set(plain["iter"])) >= 2, ("the problems must exit at different iterations", plain["iter"])
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(traj[k]), equal_nan=True), (fam["key"], dtype, k)


# ---------------------------------------------------------------------------------------------------------------- GPU 6: a batch with mixed trajectories is B single-problem handles
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("fam", FAMILY_PARAMS)
def test_batch_with_mixed_trajectories_equals_single_problem_handles(fam, dtype):
    B, plant, N = fam["B"], fam["plant"], fam["kw"]["N"]
    probs = problems(plant, N, dtype, B)
    trajs = trajectories(plant, N, dtype, probs)
    s1 = handle(fam, dtype, 1)
    refs = [solve_single(s1, probs[b], trajs[b]) for b in range(B)]      # (problem 0 runs before the handle's first setter call: no table at all)
    plain = solve_single(s1, probs[1], None)
    s1.close()
    assert len({int(r["iter"]) for r in refs}) >= 2, "the problems must exit at different iterations"
    assert not np.array_equal(refs[1]["Jout"], plain["Jout"]) and not np.array_equal(refs[1]["g0"], plain["g0"]), "the trajectory changed nothing"
    for use_graph in (1, 0):
        label = "%s dtype=%d use_graph=%d" % (fam["key"], dtype, use_graph)
        s = handle(fam, dtype, B, use_graph)
        set_trajectories(s, trajs)
        reset_like_fresh(s)
        s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
        H, g = s.get("H").reshape(B, -1), s.get("g").reshape(B, -1)
        for b in range(B):
            assert np.array_equal(H[b], refs[b]["H0"].ravel(), equal_nan=True), (label, "H after the load, slot", b)
            assert np.array_equal(g[b], refs[b]["g0"].ravel(), equal_nan=True), (label, "g after the load, slot", b)
        run_until_done(s)
        got = collect(s)
        for b in range(B):
            assert_rows_equal(got, b, refs[b], (label, "slot", b))
        assert np.array_equal(s.get("xGoal"), stack(probs, "xg")), (label, "xGoal is what the load put there")
        s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 7: float64 against the shim-oracle
def check_against_oracle(out, b, ref, label):
    """the bounds of tests/test_solver_parity.py test_other_plants_float64"""
    it = ref["iters"]
    assert out["iters"][b] == it, (label, out["iters"][b], it)
    assert list(out["alphaOut"][b][: it + 1]) == list(ref["alphaOut"][: it + 1]), (label, out["alphaOut"][b], ref["alphaOut"])
    np.testing.assert_allclose(out["Jout"][b][: it + 1], ref["Jout"][: it + 1], rtol=1e-7)
    np.testing.assert_allclose(out["x"][b].ravel(), ref["x"], rtol=0, atol=1e-7 * max(np.abs(ref["x"]).max(), 1))


def nrel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64).ravel() - ref.ravel()).max() / max(np.abs(ref).max(), 1e-30))


PINNED_ORACLE = [pytest.param(f["plant"], f["kw"], f["sel"], id=f["key"] + "-pinned") for f in (family("pend-ts"), family("cart-cf-gl-kb16"), family("quad-mq-fused-cf-kb16"))]
ORACLE_GPU_CASES = [pytest.param(*c.values, None, id=c.id) for c in ORACLE_CASES] + PINNED_ORACLE


@pytest.mark.gpu
@pytest.mark.parametrize("plant,kw,sel", ORACLE_GPU_CASES)
def test_float64_batch_with_trajectories_follows_the_shim_oracle(plant, kw, sel):
    """B = 4 problems, the odd ones with a trajectory, on the library's own selection for the shape or a pinned family: after pddp_load H, g and the initial cost
    against the shim-oracle's ora_next_iteration_setup / ora_total_cost knot by knot at the float64 bound of tests/test_phase_parity.py (1e-9 of the largest
    magnitude), then the whole solves decision for decision at the bounds of tests/test_solver_parity.py."""
    npos, n, m = DIMS[plant]
    N, B = kw["N"], 4
    kw = dict(kw, tol_cost=0.0)
    probs = problems(plant, N, 1, B)
    trajs = trajectories(plant, N, 1, probs)
    s = make_solver("hip", plant, dtype=1, batch=B, **(dict(kw, kernels=dict(sel)) if sel else kw))
    set_trajectories(s, trajs)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    H, g, st = s.get("H").reshape(B, N, n + m, n + m), s.get("g").reshape(B, N, n + m), s.get_state()
    for b in range(B):
        o = shim_oracle(plant, kw, trajs[b])
        _, Ho, go = o.next_iteration_setup(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        Ho, go = Ho.reshape(N, n + m, n + m), go.reshape(N, n + m)
        for k in range(N):
            assert nrel(H[b][k], Ho[k]) <= 1e-9 or not Ho[k].any(), (b, k, "H after the load")
            assert np.abs(g[b][k] - go[k]).max() <= 1e-9 * np.abs(go).max(), (b, k, "g after the load")
        J0 = o.total_cost(1, probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        assert abs(st[b].prevJ - J0) <= 1e-9 * abs(J0), (b, st[b].prevJ, J0)
    run_until_done(s)
    out = s.store()
    out["iters"] = np.array([x.iter for x in s.get_state()])
    accepted = 0
    for b in range(B):
        ref = shim_oracle(plant, kw, trajs[b]).run_ilqr_gpusem(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        accepted += sum(a >= 0 for a in ref["alphaOut"][1: ref["iters"] + 1])
        check_against_oracle(out, b, ref, (plant, b))
    assert accepted >= 3, "the cases must accept iterations"
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 8: float32 against the shim-oracles
@pytest.mark.gpu
@pytest.mark.parametrize("plant", [1, 2, 3])
def test_float32_with_a_trajectory_follows_the_shim_oracles_over_the_leading_iterations(plant):
    """the rule of tests/test_diag_costs.py / tests/test_ref_plugin.py: alphaOut equal to the float32 AND the float64 shim-oracle over the leading iterations, J there
    inside max(1e-4, 5 x the float32 oracle's own error).  The number of leading iterations required is exactly what the two ORACLES agree on for the problem
    (test_float32_and_float64_shim_oracles_agree_on_the_leading_iterations holds that to at least 3)."""
    c = f32_case(plant)
    kw, p32, r32, r64, agree = c["kw"], c["p32"], c["r32"], c["r64"], c["agree"]
    s = make_solver("hip", plant, dtype=0, batch=1, kernels=dict(cf="coop"), **kw)
    s.set_goal_trajectory_problems([0], c["G"])
    out = s.solve(p32["x0"], p32["u0"], p32["xg"])
    lead = next((i for i in range(r64["iters"] + 1) if not (out["alphaOut"][0][i] == r32["alphaOut"][i] == r64["alphaOut"][i])), r64["iters"] + 1)
    print("plant %d: alphaOut %s, oracle32 %s, oracle64 %s" % (plant, list(out["alphaOut"][0]), list(r32["alphaOut"]), list(r64["alphaOut"])))
    assert lead >= agree, (out["alphaOut"][0], r32["alphaOut"], r64["alphaOut"])
    for i in range(lead):
        ek, eo = abs(float(out["Jout"][0][i]) - r64["Jout"][i]) / r64["Jout"][i], abs(float(r32["Jout"][i]) - r64["Jout"][i]) / r64["Jout"][i]
        print("  iteration %d: J error %.3g, the float32 oracle's %.3g" % (i, ek, eo))
        assert ek <= max(1e-4, 5 * eo), (i, ek, eo)
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 9: named slots
QUAD_SLOTS = dict(key="quad-slots", plant=3, kw=base_kw(3, 16, 4, 16, 3, max_iter=10), sel=dict(cf_bp="mq", cf_fp="cf", cf_nis="kb16"),
                  names=("k_bp_mq", "k_sweep_maps", "k_fp_cf", "k_nis_kb"), B=5)
UNTOUCHED = ("xb", "ucur", "dcur", "P", "Pp", "p", "pp", "AB", "H", "g", "KT", "du", "xGoal", "Jout", "alphaOut")


def snapshot(s):
    B = s.cfg.batch
    snap = {k: s.get(k).reshape(B, -1).copy() for k in UNTOUCHED}
    snap.update(state_rows(s, range(B)))
    return snap


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_refill_of_named_slots_with_trajectories(dtype):
    """load_problems into slots of a running batch: the named slots run with their trajectories and equal fresh single-problem handles; the unnamed slots -- running
    or exited -- are unchanged bit for bit by the setter and the refill, and finish as they would have"""
    fam, B = QUAD_SLOTS, QUAD_SLOTS["B"]
    first, late = problems(3, 16, dtype, B), problems(3, 16, dtype, 2, skip=11)
    first_trajs = trajectories(3, 16, dtype, first)
    late_trajs = [trajectory(3, 16, dtype, late[0], 21), None]         # one refilled slot with a trajectory, one without
    s1 = handle(fam, dtype, 1)
    ref_first = [solve_single(s1, p, G) for p, G in zip(first, first_trajs)]
    ref_late = [solve_single(s1, p, G) for p, G in zip(late, late_trajs)]
    s1.close()
    s = handle(fam, dtype, B)
    set_trajectories(s, first_trajs)
    reset_like_fresh(s)
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    s.iterate(2); s.sync()
    done, _ = s.status()
    slots = [4, 1]                                                   # slot 4 (no trajectory so far) gets one, slot 1 loses its own
    others = [b for b in range(B) if b not in slots]
    assert any(not done[b] for b in others), "no running slot among the others"
    before = snapshot(s)
    s.set_goal_trajectory_problems([4], late_trajs[0])
    s.clear_goal_trajectory_problems([1])
    mid = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k]), np.asarray(mid[k]), equal_nan=True), ("the setter changed a slot", k)
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k])[others], np.asarray(after[k])[others], equal_nan=True), ("another slot changed", k)
    G, has = s.get_goal_trajectory_problems(list(range(B)))
    assert has.tolist() == [0, 0, 0, 1, 1] and np.array_equal(G[3], first_trajs[3]) and np.array_equal(G[4], late_trajs[0])
    run_until_done(s)
    got = collect(s)
    for j, b in enumerate(slots):
        assert_rows_equal(got, b, ref_late[j], ("refilled slot", b))
    for b in others:
        assert_rows_equal(got, b, ref_first[b], ("unnamed slot", b))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift,clear_vars", [(1, 0), (0, 0), (1, 1), (0, 1)])
def test_control_cycles_of_named_slots_run_with_their_own_trajectories_and_do_not_shift_them(shift, clear_vars):
    """float32 quadrotor on k_fp_cf, B = 4, slots 1 and 3 with a trajectory: a solve seeds every slot, then a pddp_mpc_solve_problems cycle on slots [3, 0] against
    single-problem handles holding the same previous solution and the same trajectory, driven through pddp_solve + pddp_mpc_solve.  Then the test rewrites slot 3's
    window with the setter (the old rows moved up by `shift`, its own business) and a second cycle again equals the single-problem handles given the same rows: the
    library used the rows as they stood, unshifted, both times.  The slots that are not named keep every array and their state."""
    fam, B, dtype = QUAD_SLOTS, 4, 0
    kw = dict(fam["kw"], tol_cost=0.0, max_iter=4)
    probs = problems(3, 16, dtype, B)
    trajs = trajectories(3, 16, dtype, probs)
    keys = ("x", "u", "KT", "Jout", "alphaOut", "success", "iters")
    s = make_solver("hip", 3, dtype=dtype, batch=B, kernels=dict(fam["sel"]), **kw)
    set_trajectories(s, trajs)
    seed = s.solve(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"))
    named, others = [3, 0], [1, 2]
    xg = stack(probs, "xg").reshape(B, -1)
    window2 = np.roll(trajs[3], -1, axis=0).copy(); window2[-1] = trajs[3][-1] + np.float32(0.002)      # the caller's next window
    before = snapshot(s)
    got1 = s.mpc_solve_problems(named, seed["x"][named, 1].copy(), xg[named], [shift, shift], clear_vars=clear_vars, max_iter=4)
    s.set_goal_trajectory_problems([3], window2)
    got2 = s.mpc_solve_problems(named, got1["x"][:, 1].copy(), xg[named], [shift, shift], clear_vars=clear_vars, max_iter=4)
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k])[others], np.asarray(after[k])[others], equal_nan=True), ("another slot changed", k)
    G, has = s.get_goal_trajectory_problems([3, 1])
    assert has.tolist() == [1, 1] and np.array_equal(G[0], window2) and np.array_equal(G[1], trajs[1]), "a cycle changed a trajectory"
    s.close()
    changed = False
    for j, b in enumerate(named):
        s1 = make_solver("hip", 3, dtype=dtype, batch=1, kernels=dict(fam["sel"]), **kw)
        if trajs[b] is not None:
            s1.set_goal_trajectory_problems([0], trajs[b])
        one = s1.solve(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        for k in ("x", "u", "Jout", "alphaOut"):
            assert np.array_equal(np.asarray(one[k][0]), np.asarray(seed[k][b]), equal_nan=True), ("seed solve", b, k)
        ref1 = s1.mpc_solve(one["x"][:, 1].copy(), xg[[b]], shift, clear_vars=clear_vars, max_iter=4)
        for k in keys:
            assert np.array_equal(np.asarray(got1[k][j]), np.asarray(ref1[k][0]), equal_nan=True), ("first cycle, slot", b, k)
        if b == 3:
            s1.set_goal_trajectory_problems([0], window2)
        ref2 = s1.mpc_solve(ref1["x"][:, 1].copy(), xg[[b]], shift, clear_vars=clear_vars, max_iter=4)
        for k in keys:
            assert np.array_equal(np.asarray(got2[k][j]), np.asarray(ref2[k][0]), equal_nan=True), ("second cycle, slot", b, k)
        if b == 3:                                                   # the rewritten window matters: the same cycle with the old rows gives other numbers
            s1.close()
            s1 = make_solver("hip", 3, dtype=dtype, batch=1, kernels=dict(fam["sel"]), **kw)
            s1.set_goal_trajectory_problems([0], trajs[b])
            s1.solve(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
            s1.mpc_solve(one["x"][:, 1].copy(), xg[[b]], shift, clear_vars=clear_vars, max_iter=4)
            old = s1.mpc_solve(ref1["x"][:, 1].copy(), xg[[b]], shift, clear_vars=clear_vars, max_iter=4)
            changed = not np.array_equal(old["Jout"][0], ref2["Jout"][0])
        s1.close()
    assert changed, "the second window changed nothing"


# ---------------------------------------------------------------------------------------------------------------- GPU 10: setter semantics, round trip, refusals
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_setter_semantics_round_trip_and_refusals(dtype):
    fam = family("cart-ts")
    B, plant, N, n = 5, 2, fam["kw"]["N"], 4
    T = np_type(dtype)
    probs = problems(plant, N, dtype, B)
    trajs = trajectories(plant, N, dtype, probs)
    xg = stack(probs, "xg").reshape(B, n)
    # the yardstick for "clear restores xGoal behaviour": a handle that never had a trajectory
    never = handle(fam, dtype, B)
    reset_like_fresh(never)
    never.load(stack(probs, "x0"), stack(probs, "u0"), xg.ravel(), clear_vars=1)
    never_load = {k: never.get(k).copy() for k in ("H", "g", "Jout")}
    run_until_done(never)
    never_res = collect(never)
    never.close()

    s = handle(fam, dtype, B)
    assert s.has_goal_trajectory() and s.goal_trajectory_size() == N * n
    s.clear_goal_trajectory_problems([0, 2])                         # never had a trajectory: a successful no-op
    s.load(stack(probs, "x0"), stack(probs, "u0"), xg.ravel(), clear_vars=1)
    G, has = s.get_goal_trajectory_problems([4, 0])                  # before the first setter call: answered from xGoal
    assert has.tolist() == [0, 0] and np.array_equal(G, np.stack([np.tile(xg[4], (N, 1)), np.tile(xg[0], (N, 1))])) and G.dtype == T
    s.iterate(1); s.sync()
    lib, EINVAL = s.lib, -1
    lib.pddp_set_goal_trajectory_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_get_goal_trajectory_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pddp_clear_goal_trajectory_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good_idx, Gw = np.array([3, 0], np.int32), np.stack([trajs[3], trajs[1]]).astype(T)

    def bad_at(e, v):
        a = Gw.copy().ravel(); a[e] = v
        return a

    bad = [("count 0", 0, good_idx, Gw), ("count < 0", -2, good_idx, Gw), ("idx null", 2, None, Gw), ("G null", 2, good_idx, None),
           ("index == batch", 2, np.array([0, B], np.int32), Gw), ("index < 0", 2, np.array([-1, 2], np.int32), Gw), ("index twice", 2, np.array([2, 2], np.int32), Gw),
           ("nan", 2, good_idx, bad_at(N * n + 5, np.nan)), ("inf", 2, good_idx, bad_at(2 * N * n - 1, np.inf)), ("-inf", 2, good_idx, bad_at(0, -np.inf))]
    values_only = ("nan", "inf", "-inf")

    def refused_everywhere(label):
        before = snapshot(s)
        rows = s.get_goal_trajectory_problems(list(range(B)))
        for what, count, idx, G_ in bad:
            assert lib.pddp_set_goal_trajectory_problems(s.h, count, ptr(idx), ptr(G_)) == EINVAL, (label, what)
            if what not in values_only:
                out, hs = np.zeros(2 * N * n, T), np.zeros(2, np.int32)
                assert lib.pddp_get_goal_trajectory_problems(s.h, count, ptr(idx), None if G_ is None else ptr(out), ptr(hs)) == EINVAL, (label, what)
                if what != "G null":
                    assert lib.pddp_clear_goal_trajectory_problems(s.h, count, ptr(idx)) == EINVAL, (label, what)
        after = snapshot(s)
        for k in UNTOUCHED + STATE_ALL:
            assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), (label, "a refused call changed", k)
        again = s.get_goal_trajectory_problems(list(range(B)))
        assert np.array_equal(again[0], rows[0]) and np.array_equal(again[1], rows[1]), (label, "a refused call changed the table")

    refused_everywhere("without a table")
    # the setter on loaded slots changes neither H, g nor the state record until the next load
    before = snapshot(s)
    set_trajectories(s, trajs)
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), ("the setter changed", k)
    assert np.array_equal(s.get_diag_cost_problems(list(range(B))), np.tile(np.asarray(BUILTIN[plant], T).astype(np.float64), (B, 1)))      # the cost table it brought: built-in rows
    G, has = s.get_goal_trajectory_problems(list(range(B)))
    assert has.tolist() == [0, 1, 0, 1, 0] and has.dtype == np.int32
    for b in range(B):
        assert np.array_equal(G[b], trajs[b] if trajs[b] is not None else np.tile(xg[b], (N, 1))), ("round trip", b)
    G, has = s.get_goal_trajectory_problems([3, 2])
    assert has.tolist() == [1, 0] and np.array_equal(G[0], trajs[3]) and np.array_equal(G[1], np.tile(xg[2], (N, 1)))
    assert lib.pddp_get_goal_trajectory_problems(s.h, 1, ptr(good_idx), ptr(np.zeros(N * n, T)), None) == 0      # has may be NULL
    refused_everywhere("with a table")
    # the next load reads the rows: g differs from the handle without a trajectory exactly in the odd problems
    reset_like_fresh(s)
    s.load(stack(probs, "x0"), stack(probs, "u0"), xg.ravel(), clear_vars=1)
    g, g0 = s.get("g").reshape(B, -1), never_load["g"].reshape(B, -1)
    assert [bool(np.array_equal(g[b], g0[b])) for b in range(B)] == [True, False, True, False, True]
    assert np.array_equal(s.get("H"), never_load["H"]), "H does not depend on the goal"
    # clear: from the next load on, bit for bit the handle that never had a trajectory
    s.clear_goal_trajectory_problems([3, 1, 0])
    assert s.get_goal_trajectory_problems(list(range(B)))[1].tolist() == [0] * B
    assert np.array_equal(s.get("g").reshape(B, -1), g), "clear rebuilt g of a loaded slot"
    reset_like_fresh(s)
    s.load(stack(probs, "x0"), stack(probs, "u0"), xg.ravel(), clear_vars=1)
    for k, v in never_load.items():
        assert np.array_equal(s.get(k), v, equal_nan=True), ("after clear, the load", k)
    run_until_done(s)
    got = collect(s)
    for k in never_res:
        assert np.array_equal(np.asarray(got[k]), np.asarray(never_res[k]), equal_nan=True), ("after clear", k)
    s.close()
    for p, size in ((1, 16 * 2), (3, 16 * 12)):
        h = make_solver("hip", p, dtype=dtype, batch=1, **base_kw(p, 16, 4, 4, 1))
        assert h.goal_trajectory_size() == size
        h.close()


@pytest.mark.gpu
def test_arm_handles_refuse_all_four():
    EINVAL = -1
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    arm = make_solver("hip", 4, dtype=0, batch=2, N=32, M=4, A=8, wafr_urdf=1, total_time=0.5)
    assert not arm.has_goal_trajectory()
    G, idx, has = np.zeros(2 * 32 * 14, np.float32), np.array([0, 1], np.int32), np.zeros(2, np.int32)
    lib = arm.lib
    lib.pddp_set_goal_trajectory_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_get_goal_trajectory_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pddp_clear_goal_trajectory_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.pddp_goal_trajectory_size.argtypes = [C.c_void_p]
    assert lib.pddp_goal_trajectory_size(arm.h) == EINVAL
    assert lib.pddp_set_goal_trajectory_problems(arm.h, 2, ptr(idx), ptr(G)) == EINVAL
    assert lib.pddp_get_goal_trajectory_problems(arm.h, 2, ptr(idx), ptr(G), ptr(has)) == EINVAL
    assert lib.pddp_clear_goal_trajectory_problems(arm.h, 2, ptr(idx)) == EINVAL
    assert not G.any() and not has.any()
    arm.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 11: the captured graph
@pytest.mark.gpu
@pytest.mark.parametrize("fam", [pytest.param(family(k), id=k) for k in ("cart-cf-gl-kb16", "quad-mq-fused-cf-kb16", "pend-coop")])
def test_graph_replay_follows_the_trajectory_table(fam):
    """use_graph = 1: iterate, set a first trajectory, reload and iterate, set another, reload and iterate -- bit for bit a use_graph = 0 handle given the same calls.
    The first setter call drops the captured graph (other kernels, other arguments); the second only writes rows, which the re-captured graph reads."""
    dtype, B, plant, N = 0, 3, fam["plant"], fam["kw"]["N"]
    probs = problems(plant, N, dtype, B)
    first = trajectory(plant, N, dtype, probs[1], 1)
    second = trajectory(plant, N, dtype, probs[1], 9)
    outs = []
    for use_graph in (1, 0):
        s = handle(fam, dtype, B, use_graph)
        stages = []
        for G in (None, first, second):
            if G is not None:
                s.set_goal_trajectory_problems([1], G)
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
        assert not np.array_equal(plain[i]["Jout"][1], plain[j]["Jout"][1]), "the trajectory changed nothing"
        assert np.array_equal(plain[i]["Jout"][0], plain[j]["Jout"][0]) and np.array_equal(plain[i]["Jout"][2], plain[j]["Jout"][2])
