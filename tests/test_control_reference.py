"""Control references of the pendulum, cart-pole and quadrotor: pddp_set_control_reference_problems / pddp_get_control_reference_problems /
pddp_clear_control_reference_problems (csrc/control_ref_table.hpp, csrc/plants.hpp RefTab).

A problem with a reference U[N][m] pays for u_k - U[k] at every running knot k < N - 1 -- in the cost, in its gradient g and in the initial cost -- where a problem
without one pays for u_k.  k is the absolute knot of the horizon.  Row N - 1 is stored and returned and never read.

Yardsticks:
  * a handle with step, goal and cost tables at their defaults and NO reference table for a handle whose problems are unflagged or flagged with zeros -- bit for bit,
    every array pddp_get_array names and the state records, with and without the captured graph;
  * a SINGLE-PROBLEM handle carrying problem b's reference, pinned to the same kernels, for slot b of a mixed batch -- bit for bit;
  * the oracle's plug-in plant with tests/plugin_control_ref/control_ref_shim.cpp (the "shim-oracle"): tests/plugin_goal_traj/goal_traj_shim.cpp with
    pow(uk[j] - U[k][j], 2) and r (uk[j] - U[k][j]).  It shares nothing with the library.

The structure (FAMILIES pinned through pddp_config.kernels and asserted by name, problem(), solve_single, collect, assert_rows_equal) is that of
tests/test_horizon_time.py, restated here.  Shapes: N 16 / 32, M 1 / 4, A 4 / 8, A = 16 for the quadrotor families with k_fp_cf; batches 3, 5 and 67 (67: a wave of the
thread-serial and staged kernels holds several problems with different flags, the last wave is partial).

A batch holds the five kinds of problem, slot b being of kind b % 5:
  0  unflagged                               3  flagged, a per-knot ramp plus seeded noise (an index taken inside a shooting segment instead of the absolute knot shows
  1  flagged, every row zero                    at M = 4)
  2  flagged, constant (the quadrotor:       4  the problem AND the reference of the slot before it (kind 3), with row N - 1 set to 1e3: it has to equal that slot
     9.81 / 8 per rotor, the hover trim)        bit for bit

The inputs were checked on the CPU (test_the_inputs_keep_the_shim_oracle_busy, below, holds it): with problem() seeds 0-4, reference() and the settings of base_kw,
the float64 shim-oracle at every (plant, shape, integrator) of ORACLE_CASES gives, for each problem, a finite cost and at least one accepted iteration, and the batch
exits at two or more different iterations.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_binding
import pyddp
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
MPC_KEYS = ("x", "u", "KT", "Jout", "alphaOut", "success", "iters")
EXTRA_SWEEPS = 3
ENTRY_POINTS = ("pddp_control_reference_size", "pddp_set_control_reference_problems", "pddp_get_control_reference_problems", "pddp_clear_control_reference_problems")
HOVER = 9.81 / 8                                                    # thrust per rotor that holds the quadrotor still: 2 (u_0 + u_1 + u_2 + u_3) = 9.81
TRIM = {1: 0.05, 2: 0.05, 3: HOVER}                                 # the constant reference of kind 2


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


def kernel_names(s):
    return [n for n, _ in s.time_kernels(1)]


def handle(fam, dtype, batch, use_graph=1, **more):
    s = make_solver("hip", fam["plant"], dtype=dtype, batch=batch, use_graph=use_graph, kernels=dict(fam["sel"]), **dict(fam["kw"], **more))
    have = kernel_names(s)
    assert all(any(h.startswith(n) for h in have) for n in fam["names"]), (fam["key"], fam["names"], have)
    return s


def seed_of(b):
    """slot b's problem: its own, except that a slot of kind 4 repeats the problem of the slot before it"""
    return b - 1 if b % 5 == 4 else b


def problem(plant, N, dtype, seed):
    """the example's inputs with velocity noise and the goal moved along the line from the start: near goals exit by tolerance early, far ones run on"""
    npos, n, m = DIMS[plant]
    rng = np.random.default_rng(1000 * plant + seed)
    x0, u0, xg = example_inputs(plant, N, np.float64, noise=rng.normal(0, 0.002, (N, n)))
    start = x0.reshape(N, n)[0, :npos]
    frac = (0.02, 0.6, 1.0, 0.08, 0.3)[seed % 5] * (1.0 + 0.01 * (seed // 5))      # (the farthest goal in the slot of kind 2: a batch of 3 -- kinds 2, 3, 4 -- exits at different iterations)
    xg = xg.copy(); xg[:npos] = start + frac * (xg[:npos] - start)
    T = np_type(dtype)
    return dict(x0=x0.astype(T), u0=u0.astype(T), xg=xg.astype(T))


def problems(plant, N, dtype, B, skip=0):
    return [problem(plant, N, dtype, seed_of(skip + b)) for b in range(B)]


def stack(probs, key):
    return np.concatenate([p[key].ravel() for p in probs])


def reference(plant, N, dtype, b):
    """slot b's control reference [N][m] in the element type, or None (kind 0)"""
    m, T, kind = DIMS[plant][2], np_type(dtype), b % 5
    if kind == 0:
        return None
    if kind == 1:
        return np.zeros((N, m), T)
    if kind == 2:
        return np.full((N, m), TRIM[plant], T)
    s = seed_of(b)
    rng = np.random.default_rng(7000 * plant + s)
    ramp = np.arange(N)[:, None] / (N - 1.0)
    U = TRIM[plant] * (0.8 + 0.5 * ramp + 0.1 * (s % 3)) + rng.normal(0, 0.1 * TRIM[plant], (N, m))
    if kind == 4:
        U[N - 1] = 1e3
    return U.astype(T)


def references(plant, N, dtype, B, skip=0):
    return [reference(plant, N, dtype, skip + b) for b in range(B)]


def set_references(s, refs, slots=None):
    """flags the slots that have a reference, clears the others"""
    slots = list(range(len(refs))) if slots is None else list(slots)
    on = [(b, U) for b, U in zip(slots, refs) if U is not None][::-1]      # unsorted on purpose
    off = [b for b, U in zip(slots, refs) if U is None]
    if on:
        s.set_control_reference_problems([b for b, _ in on], np.stack([U for _, U in on]))
    if off:
        s.clear_control_reference_problems(off)


def default_tables(s, plant, N, dtype):
    """the three tables a reference table is layered on, with nothing in them: built-in cost rows, no goal flagged, every step the handle's"""
    n = DIMS[plant][1]
    s.set_diag_cost(BUILTIN[plant])
    s.set_goal_trajectory_problems([0], np.zeros((1, N, n), np_type(dtype)))
    s.clear_goal_trajectory_problems([0])
    s.set_horizon_time_problems([0], [s.cfg.total_time])


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


def solve_single(s1, prob, U=None, **load_kw):
    """the yardstick: one problem on a single-problem handle in the state of a fresh one, sweep by sweep until it exits"""
    if U is not None:
        s1.set_control_reference_problems([0], U)
    else:
        s1.clear_control_reference_problems([0])                   # (a no-op before the handle's first setter call)
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


def assert_rows_equal(got, j, ref, label, keys=OUT_KEYS + STATE_ALL + CTG):
    for k in keys:
        assert np.array_equal(np.asarray(got[k][j]).ravel(), np.asarray(ref[k]).ravel(), equal_nan=True), (label, k)


# ---------------------------------------------------------------------------------------------------------------- the shim-oracle
_SHIM = {}


def shim():
    if "lib" not in _SHIM:
        src = os.path.join(ROOT, "tests", "plugin_control_ref", "control_ref_shim.cpp")
        out = os.path.join(ROOT, "tests", "plugin_control_ref", "libcontrol_ref_shim.so")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", out, src])
        _SHIM["lib"], _SHIM["path"] = C.CDLL(out), out
    return _SHIM["lib"], _SHIM["path"]


def shim_oracle(plant, kw, U=None, dtype=np.float64, G=None):
    """the oracle's plant 5 = plant `plant` with the built-in diagonal record, the control reference U (None: the control term is taken on u) and the goal trajectory G
    (None: the cost reads xg): same solver configuration as Oracle(default_cfg(plant, **kw))"""
    lib, path = shim()
    L = oracle_binding.lib()
    base = default_cfg(plant, cores=1, spawn_threads=0, **kw)
    npos, n, m = DIMS[plant]
    rec = np.ascontiguousarray(BUILTIN[plant], np.float64)
    Ud = None if U is None else np.ascontiguousarray(U, np.float64)
    Gd = None if G is None else np.ascontiguousarray(G, np.float64)
    assert Ud is None or Ud.shape == (kw["N"], m)
    assert Gd is None or Gd.shape == (kw["N"], n)
    addr = lambda f: C.cast(f, C.c_void_p)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    lib.control_ref_shim_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_void_p] * 4
    lib.control_ref_shim_set(C.byref(base), n, m, kw["N"], ptr(rec), ptr(Gd), ptr(Ud), addr(L.ora_dynamics_f32), addr(L.ora_dynamics_gradient_f32), addr(L.ora_dynamics_f64),
                             addr(L.ora_dynamics_gradient_f64))
    register_plugin(path)
    cfg = default_cfg(plant, cores=1, spawn_threads=0, **kw)
    cfg.plant = 5
    return Oracle(cfg, dtype)


ORACLE_CASES = [pytest.param(1, base_kw(1, 16, 4, 4, 1), None, id="pend-M4-euler"), pytest.param(1, base_kw(1, 32, 1, 4, 3), None, id="pend-M1-rk3"),
                pytest.param(2, base_kw(2, 32, 4, 8, 3), None, id="cart-M4-rk3"), pytest.param(2, base_kw(2, 16, 1, 4, 2), None, id="cart-M1-midpoint"),
                pytest.param(3, base_kw(3, 16, 4, 8, 1), None, id="quad-M4-euler"), pytest.param(3, base_kw(3, 16, 1, 4, 2), None, id="quad-M1-midpoint"),
                pytest.param(3, base_kw(3, 32, 4, 8, 3), None, id="quad-M4-rk3"), pytest.param(3, base_kw(3, 16, 1, 8, 3), None, id="quad-M1-rk3")]
PINNED_ORACLE = [pytest.param(f["plant"], f["kw"], f["sel"], id=f["key"] + "-pinned") for f in (family("pend-ts"), family("cart-cf-gl-kb16"), family("quad-mq-fused-cf-kb16"))]


# ---------------------------------------------------------------------------------------------------------------- CPU 1: the surface
def test_entry_points_are_exported_declared_and_bound():
    lib = C.CDLL(pyddp.library_path())
    header = open(os.path.join(ROOT, "include", "pddp.h")).read()
    for sym in ENTRY_POINTS:
        assert getattr(lib, sym) is not None
    assert "int pddp_control_reference_size(pddp_handle h);" in header
    assert "int pddp_set_control_reference_problems(pddp_handle h, int count, const int* idx, const void* U" in header
    assert "int pddp_get_control_reference_problems(pddp_handle h, int count, const int* idx, void* U" in header
    assert "int pddp_clear_control_reference_problems(pddp_handle h, int count, const int* idx);" in header
    assert "CARRY NO CONTROL" in header                             # goal paths: said in the header
    for name in ("control_reference_size", "set_control_reference_problems", "get_control_reference_problems", "clear_control_reference_problems", "has_control_reference"):
        assert callable(getattr(pyddp.Solver, name))


# ---------------------------------------------------------------------------------------------------------------- CPU 2: the host-only code under the sanitizers
def test_host_only_code_as_a_stand_alone_program(tmp_path):
    """tests/native/control_ref_host_check.cpp (its own main, -fsanitize=address,undefined): every argument check, the layout of the allocation, and goal / reference
    base, stride and row of problem_goal and goal_at with RefTab's cost routines on exactly-sized buffers"""
    exe = str(tmp_path / "control_ref_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "control_ref_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "control_ref_host_check: ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------- CPU 3: the shim-oracle, and what the inputs do to it
_ORACLE_RUNS = {}


def oracle_runs(plant, kw, B=5):
    """float64 shim-oracle solves of the batch's first B problems with their references (tol_cost as given), computed once per case"""
    key = (plant, tuple(sorted(kw.items())), B)
    if key not in _ORACLE_RUNS:
        N = kw["N"]
        probs, refs = problems(plant, N, 1, B), references(plant, N, 1, B)
        _ORACLE_RUNS[key] = [shim_oracle(plant, kw, refs[b]).run_ilqr_gpusem(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"]) for b in range(B)]
    return _ORACLE_RUNS[key]


@pytest.mark.parametrize("plant,kw,sel", ORACLE_CASES)
def test_shim_oracle_without_a_reference_is_the_oracles_own_plant_and_with_one_reads_row_k(plant, kw, sel):
    npos, n, m = DIMS[plant]
    N = kw["N"]
    kw = dict(kw, tol_cost=0.0)
    p = problem(plant, N, 1, 1)
    own = Oracle(default_cfg(plant, cores=1, spawn_threads=0, **kw), np.float64).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
    for U in (None, np.zeros((N, m))):
        via = shim_oracle(plant, kw, U).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
        assert via["iters"] == own["iters"] and list(via["alphaOut"]) == list(own["alphaOut"])
        for k in ("Jout", "x", "u", "KT"):
            assert float(np.abs(via[k] - own[k]).max()) == 0.0, k
    U = reference(plant, N, 1, 3)
    o = shim_oracle(plant, kw, U)
    rec = BUILTIN[plant]
    q, r, qf = rec[:n], rec[n: n + m], rec[n + m:]
    rng = np.random.default_rng(5 + plant)
    for k in (0, 3, N - 2, N - 1):
        x, u = rng.normal(0, 1.5, n), rng.normal(0, 2.0, m)
        H, g = o.cost_grad(x, u, p["xg"], k)
        fin = k == N - 1
        gw = np.concatenate([qf * (x - p["xg"]), np.zeros(m)]) if fin else np.concatenate([q * (x - p["xg"]), r * (u - U[k])])
        cw = 0.5 * np.sum(qf * (x - p["xg"]) ** 2) if fin else 0.5 * (np.sum(q * (x - p["xg"]) ** 2) + np.sum(r * (u - U[k]) ** 2))
        assert np.array_equal(g, gw) and np.array_equal(H.reshape(n + m, n + m), np.diag(np.concatenate([qf, np.zeros(m)]) if fin else np.concatenate([q, r])))
        assert abs(o.cost_func(x, u, p["xg"], k) - cw) <= 1e-14 * abs(cw)
    a = shim_oracle(plant, kw, U).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
    assert not np.array_equal(a["Jout"], own["Jout"]), "the reference changes the solve"
    U5 = reference(plant, N, 1, 4)                                  # kind 4 = kind 3 of the same seed with row N - 1 at 1e3: never read
    assert np.array_equal(U5[: N - 1], U[: N - 1]) and (U5[N - 1] == 1e3).all()
    b = shim_oracle(plant, kw, U5).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
    for k in ("Jout", "x", "u", "KT", "alphaOut"):
        assert np.array_equal(a[k], b[k]), ("row N - 1 was read", k)


def _shapes():
    """every (plant, shape, integrator) of FAMILIES once, with the smallest batch a family runs it at"""
    seen = {}
    for f in FAMILIES:
        key = (f["plant"], tuple(sorted(f["kw"].items())))
        seen[key] = (f, min(f["B"], seen[key][1]) if key in seen else f["B"])
    return [pytest.param(f["plant"], f["kw"], B, id="%s-N%d-M%d-A%d-integ%d" % (f["key"].split("-")[0], f["kw"]["N"], f["kw"]["M"], f["kw"]["A"], f["kw"]["integrator"]))
            for f, B in seen.values()]


@pytest.mark.parametrize("plant,kw,B", _shapes())
def test_the_inputs_keep_the_shim_oracle_busy(plant, kw, B):
    """what the module docstring states about the inputs, at every (plant, shape, integrator) of FAMILIES: per problem a finite cost and at least one accepted
    iteration; two or more different exits across the five kinds, and where a family runs the shape at batch 3 across kinds 2, 3, 4 alone (what that batch holds)"""
    runs = oracle_runs(plant, kw)
    iters = [r["iters"] for r in runs]
    print("plant %d %s: exits at %s, accepted %s" % (plant, kw, iters, [int(sum(a >= 0 for a in r["alphaOut"][1: r["iters"] + 1])) for r in runs]))
    for b, r in enumerate(runs):
        assert np.isfinite(r["Jout"][: r["iters"] + 1]).all(), (b, r["Jout"])
        assert sum(a >= 0 for a in r["alphaOut"][1: r["iters"] + 1]) >= 1, (b, r["alphaOut"])
    assert len(set(iters)) >= 2 and (B > 3 or len(set(iters[2:])) >= 2), iters
    assert iters[3] == iters[4] and np.array_equal(runs[3]["Jout"], runs[4]["Jout"]), "kind 4 is kind 3"


F32_SLOT = 3                                                        # the float32 GPU test's problem: kind 3, the ramp
_F32 = {}


def f32_case(plant):
    """the float32 GPU test's problem, reference and the two shim-oracles' solves, computed once"""
    if plant not in _F32:
        kw = dict(base_kw(plant, 32, 4, 8, 3), tol_cost=0.0)
        p32 = problem(plant, 32, 0, F32_SLOT)
        U = reference(plant, 32, 0, F32_SLOT)
        p64 = {k: v.astype(np.float64) for k, v in p32.items()}
        r32 = shim_oracle(plant, kw, U, np.float32).run_ilqr_gpusem(p32["x0"], p32["u0"], p32["xg"])
        r64 = shim_oracle(plant, kw, U, np.float64).run_ilqr_gpusem(p64["x0"], p64["u0"], p64["xg"])
        agree = next((i for i in range(r64["iters"] + 1) if r32["alphaOut"][i] != r64["alphaOut"][i]), r64["iters"] + 1)
        _F32[plant] = dict(kw=kw, p32=p32, U=U, r32=r32, r64=r64, agree=agree)
    return _F32[plant]


@pytest.mark.parametrize("plant", [1, 2, 3])
def test_float32_and_float64_shim_oracles_agree_on_the_leading_iterations(plant):
    c = f32_case(plant)
    print("plant %d: the oracles agree on %d leading entries of alphaOut: %s / %s" % (plant, c["agree"], list(c["r32"]["alphaOut"]), list(c["r64"]["alphaOut"])))
    assert c["agree"] >= 3 + 1, (c["r32"]["alphaOut"], c["r64"]["alphaOut"])      # entry 0 is the load; at least 3 iterations behind it
    assert sum(a >= 0 for a in c["r64"]["alphaOut"][1: c["agree"]]) >= 2, "the case must accept iterations"


# ---------------------------------------------------------------------------------------------------------------- GPU 1: zero is nothing
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("fam", FAMILY_PARAMS)
def test_unflagged_and_zero_references_solve_bit_for_bit_like_a_handle_without_a_table(fam, dtype):
    B, plant, N = min(fam["B"], 5), fam["plant"], fam["kw"]["N"]
    m = DIMS[plant][2]
    probs = problems(plant, N, dtype, B)
    for use_graph in (1, 0):
        outs, names = [], []
        for with_table in (False, True):
            s = handle(fam, dtype, B, use_graph)
            default_tables(s, plant, N, dtype)                       # both: step, goal and cost tables at their defaults
            if with_table:
                s.set_control_reference_problems(list(range(B)), np.zeros((B, N, m), np_type(dtype)))
                s.clear_control_reference_problems(list(range(0, B, 2)))      # even slots unflagged, odd slots flagged with zeros
                U, has = s.get_control_reference_problems(list(range(B)))
                assert not U.any() and has.tolist() == [b % 2 for b in range(B)]
            names.append(kernel_names(s))
            assert all(any(h.startswith(n) for h in names[-1]) for n in fam["names"])
            reset_like_fresh(s)
            s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
            res = {"load_" + k: s.get(k).copy() for k in ARRAYS}
            res.update({"load_" + k: v for k, v in state_rows(s, range(B)).items()})
            s.iterate(fam["kw"]["max_iter"]); s.sync()                # max_iter sweeps
            res.update({"sweeps_" + k: s.get(k).copy() for k in ARRAYS})
            res.update({"sweeps_" + k: v for k, v in state_rows(s, range(B)).items()})
            run_until_done(s)
            res.update(collect(s))
            res.update({"arr_" + k: s.get(k) for k in ARRAYS})
            outs.append(res)
            s.close()
        assert names[0] == names[1], "the reference table changed the kernel family"
        plain, table = outs
        assert len(set(plain["iter"])) >= 2, ("the problems must exit at different iterations", plain["iter"])
        for k in plain:
            assert np.array_equal(np.asarray(plain[k]), np.asarray(table[k]), equal_nan=True), (fam["key"], dtype, use_graph, k)


# ---------------------------------------------------------------------------------------------------------------- GPU 2: a mixed batch is B single-problem handles
def single_refs(fam, dtype, probs, refs, **load_kw):
    s1 = handle(fam, dtype, 1)
    out = [solve_single(s1, p, U, **load_kw) for p, U in zip(probs, refs)]      # (problem 0 runs before the handle's first setter call: no table at all)
    s1.close()
    return out


def mixed_batch_against_singles(fam, dtype, B, **load_kw):
    """(a batch of 3 holds kinds 2, 3, 4 -- the constant, the ramp and the ramp's copy; larger batches start at kind 0 and hold all five)"""
    plant, N = fam["plant"], fam["kw"]["N"]
    skip = 2 if B == 3 else 0
    P = min(B, 15)                                                   # the batch repeats its first 15 slots (three of each kind): one yardstick solve per distinct slot
    base_p, base_r = problems(plant, N, dtype, P, skip), references(plant, N, dtype, P, skip)
    base_s = single_refs(fam, dtype, base_p, base_r, **load_kw)
    probs, refs, singles = [base_p[b % P] for b in range(B)], [base_r[b % P] for b in range(B)], [base_s[b % P] for b in range(B)]
    r3 = 3 - skip                                                    # the first slot of kind 3
    copies = [b for b in range(1, B) if (skip + b) % 5 == 4]
    s1 = handle(fam, dtype, 1)
    plain = solve_single(s1, probs[r3], None, **load_kw)             # the ramp's problem without its reference
    s1.close()
    assert len({int(r["iter"]) for r in singles}) >= 2, "the problems must exit at different iterations"
    assert not np.array_equal(singles[r3]["Jout"], plain["Jout"]) and not np.array_equal(singles[r3]["g0"], plain["g0"]), "the reference changed nothing"
    assert np.array_equal(singles[r3]["H0"], plain["H0"]) and np.array_equal(singles[r3]["AB0"], plain["AB0"]), "H and [A B] do not depend on the reference"
    assert copies
    for b in copies:                                                 # kind 4 equals kind 3 bit for bit: row N - 1 is never read
        for k in singles[b]:
            assert np.array_equal(np.asarray(singles[b][k]), np.asarray(singles[b - 1][k]), equal_nan=True), ("kind 4 against kind 3, yardsticks", b, k)
    for use_graph in (1, 0):
        label = "%s dtype=%d use_graph=%d" % (fam["key"], dtype, use_graph)
        s = handle(fam, dtype, B, use_graph)
        set_references(s, refs)
        reset_like_fresh(s)
        s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1, **load_kw)
        first = {k: s.get(k).reshape(B, -1) for k in ("AB", "H", "g")}
        for b in range(B):
            for k in ("AB", "H", "g"):
                assert np.array_equal(first[k][b], singles[b][k + "0"].ravel(), equal_nan=True), (label, k, "after the load, slot", b)
        run_until_done(s)
        got = collect(s)
        for b in range(B):
            assert_rows_equal(got, b, singles[b], (label, "slot", b))
        for b in copies:
            assert_rows_equal(got, b, {k: got[k][b - 1] for k in OUT_KEYS + STATE_ALL + CTG}, (label, "kind 4 against kind 3, slot", b))
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("fam", FAMILY_PARAMS)
def test_mixed_batch_equals_single_problem_handles(fam, dtype):
    mixed_batch_against_singles(fam, dtype, fam["B"])


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [pytest.param(family(k), id=k) for k in ("pend-coop", "cart-ts", "quad-mq-fused-cf-kb16")])
def test_mixed_batch_with_the_initial_rollout_of_the_load(fam):
    """pddp_load_ex(forward_rollout = 1): the load's own rollout forms its cost on u - U[k] too"""
    mixed_batch_against_singles(fam, 1, 5, forward_rollout=1)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["cart-coop-M1-euler", "quad-gl32-ts-gl8"])
def test_mixed_batch_with_the_finite_difference_jacobian(key):
    """use_finite_diff = 1: k_nis / k_nis_gl on the finite-difference path form g on u - U[k]"""
    fam = family(key)
    fam = dict(fam, kw=dict(fam["kw"], use_finite_diff=1, finite_diff_epsilon=1e-5))
    mixed_batch_against_singles(fam, 1, 5)


# ---------------------------------------------------------------------------------------------------------------- GPU 3: float64 against the shim-oracle
def check_against_oracle(out, b, ref, label):
    """the bounds of tests/test_solver_parity.py test_other_plants_float64 (as tests/test_goal_trajectory.py takes them)"""
    it = ref["iters"]
    assert out["iters"][b] == it, (label, out["iters"][b], it)
    assert list(out["alphaOut"][b][: it + 1]) == list(ref["alphaOut"][: it + 1]), (label, out["alphaOut"][b], ref["alphaOut"])
    np.testing.assert_allclose(out["Jout"][b][: it + 1], ref["Jout"][: it + 1], rtol=1e-7)
    np.testing.assert_allclose(out["x"][b].ravel(), ref["x"], rtol=0, atol=1e-7 * max(np.abs(ref["x"]).max(), 1))


def nrel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64).ravel() - ref.ravel()).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("plant,kw,sel", ORACLE_CASES + PINNED_ORACLE)
def test_float64_batch_with_references_follows_the_shim_oracle(plant, kw, sel):
    """B = 5 problems, one of each kind, on the library's own selection for the shape or a pinned family: after pddp_load H, g and the initial cost against the
    shim-oracle's ora_next_iteration_setup / ora_total_cost knot by knot at the float64 bound tests/test_goal_trajectory.py uses (1e-9 of the largest magnitude), then
    the whole solves decision for decision at the bounds of tests/test_solver_parity.py."""
    npos, n, m = DIMS[plant]
    N, B = kw["N"], 5
    kw = dict(kw, tol_cost=0.0)
    probs, refs = problems(plant, N, 1, B), references(plant, N, 1, B)
    s = make_solver("hip", plant, dtype=1, batch=B, **(dict(kw, kernels=dict(sel)) if sel else kw))
    set_references(s, refs)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    H, g, st = s.get("H").reshape(B, N, n + m, n + m), s.get("g").reshape(B, N, n + m), s.get_state()
    for b in range(B):
        o = shim_oracle(plant, kw, refs[b])
        _, Ho, go = o.next_iteration_setup(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        Ho, go = Ho.reshape(N, n + m, n + m), go.reshape(N, n + m)
        for k in range(N):
            assert nrel(H[b][k], Ho[k]) <= 1e-9 or not Ho[k].any(), (b, k, "H after the load")
            assert np.abs(g[b][k] - go[k]).max() <= 1e-9 * np.abs(go).max(), (b, k, "g after the load")
        J0 = o.total_cost(1, probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        assert abs(st[b].prevJ - J0) <= 1e-9 * abs(J0), (b, st[b].prevJ, J0)
    assert not np.array_equal(g[3][:, n:], g[0][:, n:])             # the ramp is in g's control rows
    run_until_done(s)
    out = s.store()
    out["iters"] = np.array([x.iter for x in s.get_state()])
    accepted = 0
    for b in range(B):
        ref = shim_oracle(plant, kw, refs[b]).run_ilqr_gpusem(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        accepted += sum(a >= 0 for a in ref["alphaOut"][1: ref["iters"] + 1])
        check_against_oracle(out, b, ref, (plant, b))
    assert accepted >= 3, "the cases must accept iterations"
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plant", [1, 2, 3])
def test_float32_with_a_reference_follows_the_shim_oracles_over_the_leading_iterations(plant):
    """the rule of tests/test_goal_trajectory.py: alphaOut equal to the float32 AND the float64 shim-oracle over the leading iterations, J there inside
    max(1e-4, 5 x the float32 oracle's own error).  The number of leading iterations required is exactly what the two ORACLES agree on for the problem
    (test_float32_and_float64_shim_oracles_agree_on_the_leading_iterations holds that to at least 3).  Slot 1 of a batch of two carries the reference."""
    c = f32_case(plant)
    kw, p32, r32, r64, agree = c["kw"], c["p32"], c["r32"], c["r64"], c["agree"]
    s = make_solver("hip", plant, dtype=0, batch=2, kernels=dict(cf="coop"), **kw)
    s.set_control_reference_problems([1], c["U"])
    out = s.solve(stack([p32, p32], "x0"), stack([p32, p32], "u0"), stack([p32, p32], "xg"))
    lead = next((i for i in range(r64["iters"] + 1) if not (out["alphaOut"][1][i] == r32["alphaOut"][i] == r64["alphaOut"][i])), r64["iters"] + 1)
    print("plant %d: alphaOut %s, oracle32 %s, oracle64 %s" % (plant, list(out["alphaOut"][1]), list(r32["alphaOut"]), list(r64["alphaOut"])))
    assert lead >= agree, (out["alphaOut"][1], r32["alphaOut"], r64["alphaOut"])
    for i in range(lead):
        ek, eo = abs(float(out["Jout"][1][i]) - r64["Jout"][i]) / r64["Jout"][i], abs(float(r32["Jout"][i]) - r64["Jout"][i]) / r64["Jout"][i]
        print("  iteration %d: J error %.3g, the float32 oracle's %.3g" % (i, ek, eo))
        assert ek <= max(1e-4, 5 * eo), (i, ek, eo)
    assert not np.array_equal(out["Jout"][0], out["Jout"][1]), "slot 0 has no reference"
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 4: what it is for
@pytest.mark.gpu
def test_a_quadrotor_hovering_on_its_goal_pays_nothing_with_the_trim_as_reference():
    """one float64 quadrotor problem resting on its goal at the hover thrust.  With the trim as reference the initial cost is exactly 0 and the solve stays on the goal
    inside the float64 oracle tolerance of test 3 (1e-7 of max(|x|, 1)); without it the initial cost is (N - 1) 1/2 5 4 (9.81 / 8)^2 as float64 rounds it -- rebuilt
    here operation by operation and held with equality -- and the solved trajectory sags: its altitude error at mid-horizon is strictly larger."""
    N, n, m = 16, 12, 4
    kw = base_kw(3, N, 4, 8, 3)
    xg = np.zeros(n); xg[:3] = [0.3, -0.2, 0.5]
    x0, u0 = np.tile(xg, (N, 1)), np.full((N, m), HOVER)
    res = {}
    for with_ref in (True, False):
        s = make_solver("hip", 3, dtype=1, batch=1, **kw)
        if with_ref:
            s.set_control_reference_problems([0], np.full((1, N, m), HOVER))
        out = s.solve(x0.ravel(), u0.ravel(), xg)
        res[with_ref] = dict(J0=float(out["Jout"][0][0]), x=np.asarray(out["x"][0]).reshape(N, n))
        s.close()
    assert res[True]["J0"] == 0.0, res[True]["J0"]
    dev = np.abs(res[True]["x"] - xg).max()
    print("with the trim: max |x - goal| = %.3g; without: altitude error at mid-horizon %.3g" % (dev, abs(res[False]["x"][N // 2, 2] - xg[2])))
    assert dev <= 1e-7 * max(np.abs(xg).max(), 1.0), dev
    # (N - 1) 1/2 5 4 (9.81 / 8)^2 as float64 rounds it on the way the library takes: the knot's cost as DiagTab::cost accumulates it (the state terms are exact
    # zeros), the N knots summed in tree_sum's pairing (fp.hpp), Jout[0] = (J + 2 tol_cost) - 2 tol_cost (init_cost_body)
    c = 0.0
    for _ in range(m):
        c += 5.0 * (HOVER * HOVER)
    vals = [0.5 * c] * (N - 1) + [0.0]
    h = N // 2
    while h >= 2:
        for t in range(h):
            vals[t] += vals[t + h]
        h //= 2
    want = ((vals[0] + vals[1]) + 2 * kw["tol_cost"]) - 2 * kw["tol_cost"]
    assert abs(want - (N - 1) * 0.5 * 5.0 * 4 * HOVER ** 2) <= N * np.finfo(np.float64).eps * want
    assert res[False]["J0"] == want, (res[False]["J0"], want)
    assert abs(res[False]["x"][N // 2, 2] - xg[2]) > abs(res[True]["x"][N // 2, 2] - xg[2])


# ---------------------------------------------------------------------------------------------------------------- GPU 5: named slots
QUAD_SLOTS = dict(key="quad-slots", plant=3, kw=base_kw(3, 16, 4, 16, 3, max_iter=10), sel=dict(cf_bp="mq", cf_fp="cf", cf_nis="kb16"),
                  names=("k_bp_mq", "k_sweep_maps", "k_fp_cf", "k_nis_kb"), B=5)
UNTOUCHED = ("xb", "ucur", "dcur", "P", "Pp", "p", "pp", "AB", "H", "g", "KT", "du", "xGoal", "Jout", "alphaOut")


def snapshot(s):
    B = s.cfg.batch
    snap = {k: s.get(k).reshape(B, -1).copy() for k in UNTOUCHED}
    snap.update(state_rows(s, range(B)))
    return snap


def tables(s):
    """what the handle's four tables hold for every slot"""
    idx = list(range(s.cfg.batch))
    t, st = s.get_horizon_time_problems(idx)
    G, has = s.get_goal_trajectory_problems(idx)
    U, uhas = s.get_control_reference_problems(idx)
    return dict(times=t, steps=st, cost=s.get_diag_cost_problems(idx), goal=G, has=has, ref=U, ref_has=uhas)


def assert_same(a, b, rows, label, keys=None):
    for k in (keys or a):
        assert np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k])[rows], equal_nan=True), (label, k)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_refill_of_named_slots_with_their_own_references(dtype):
    """load_problems into slots of a running batch: the named slots run with the references the setter just gave them and equal fresh single-problem handles carrying
    those; the unnamed slots -- running or exited -- , their rows and their flags are unchanged bit for bit by the setter and the refill, and finish as they would have"""
    fam, B, N = QUAD_SLOTS, QUAD_SLOTS["B"], 16
    first, late = problems(3, N, dtype, B), problems(3, N, dtype, 2, skip=11)
    first_refs, late_refs = references(3, N, dtype, B), [reference(3, N, dtype, 13), None]      # one refilled slot gets a new ramp, the other loses its reference
    ref_first = single_refs(fam, dtype, first, first_refs)
    ref_late = single_refs(fam, dtype, late, late_refs)
    s = handle(fam, dtype, B)
    set_references(s, first_refs)
    reset_like_fresh(s)
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    s.iterate(2); s.sync()
    done, _ = s.status()
    slots = [4, 1]
    others = [b for b in range(B) if b not in slots]
    assert any(not done[b] for b in others), "no running slot among the others"
    before, tab_before = snapshot(s), tables(s)
    set_references(s, late_refs, slots)
    assert_same(before, snapshot(s), slice(None), "the setter changed a slot", UNTOUCHED + STATE_ALL)      # g and the cost of what is in a slot are not rebuilt
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    assert_same(before, snapshot(s), others, "another slot changed", UNTOUCHED + STATE_ALL)
    tab_after = tables(s)
    assert_same(tab_before, tab_after, others, "another slot's table entries changed")
    assert tab_after["ref_has"][slots].tolist() == [1, 0] and np.array_equal(tab_after["ref"][4], late_refs[0]) and not tab_after["ref"][1].any()
    run_until_done(s)
    got = collect(s)
    for j, b in enumerate(slots):
        assert_rows_equal(got, b, ref_late[j], ("refilled slot", b))
    for b in others:
        assert_rows_equal(got, b, ref_first[b], ("unnamed slot", b))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift,clear_vars", [(1, 0), (0, 0), (1, 1), (0, 1)])
def test_control_cycles_of_named_slots_run_with_their_own_references(shift, clear_vars):
    """float32 quadrotor on k_fp_cf, B = 5 with the five kinds: a solve seeds every slot of the subject and of a twin; then pddp_mpc_load_problems and two
    pddp_mpc_solve_problems cycles on slots [3, 0, 2] against pddp_mpc_load / pddp_mpc_solve of the WHOLE twin (which
    test_whole_handle_control_cycles_equal_single_problem_handles holds to single-problem handles): the named rows equal the twin's, the slots that are not named keep
    every array, their state and their table entries.  Between the two cycles the caller rewrites slot 3's reference on both sides: the second cycle runs with it, and
    no cycle shifts a row."""
    fam, B, dtype, N = QUAD_SLOTS, 5, 0, 16
    kw = dict(fam["kw"], tol_cost=0.0, max_iter=4)
    probs, refs = problems(3, N, dtype, B), references(3, N, dtype, B)
    named, others = [3, 0, 2], [1, 4]
    xg = stack(probs, "xg").reshape(B, -1)
    subj, twin = [make_solver("hip", 3, dtype=dtype, batch=B, kernels=dict(fam["sel"]), **kw) for _ in range(2)]
    seeds = []
    for s in (subj, twin):
        set_references(s, refs)
        seeds.append(s.solve(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg")))
    assert_same(seeds[0], seeds[1], slice(None), "seed solve", OUT_KEYS)
    seed = seeds[0]
    before, tab_before = snapshot(subj), tables(subj)
    xa = seed["x"][:, 1].copy()
    sh = [shift] * len(named)
    # the load stage alone
    subj.mpc_load_problems(named, xa[named], xg[named], sh, clear_vars=clear_vars)
    twin.mpc_load(xa, xg, shift, clear_vars=clear_vars)
    a, t = snapshot(subj), snapshot(twin)
    assert_same(a, t, named, "load stage, named slots", ("xb", "ucur", "dcur", "P", "Pp", "p", "pp", "KT", "du", "xGoal"))
    assert_same(before, a, others, "load stage: another slot changed", UNTOUCHED + STATE_ALL)
    for cycle in range(2):
        if cycle == 1:                                               # the caller's new window for slot 3
            new = reference(3, N, dtype, 8)
            assert not np.array_equal(new, refs[3])
            for s in (subj, twin):
                s.set_control_reference_problems([3], new)
            tab_before = tables(subj)
            assert np.array_equal(tab_before["ref"][3], new) and tab_before["ref_has"].tolist() == [0, 1, 1, 1, 1], "the getter returns the rewritten rows"
        got = subj.mpc_solve_problems(named, xa[named], xg[named], sh, clear_vars=clear_vars, max_iter=4)
        ref = twin.mpc_solve(xa, xg, shift, clear_vars=clear_vars, max_iter=4)
        for j, b in enumerate(named):
            for k in MPC_KEYS:
                assert np.array_equal(np.asarray(got[k][j]), np.asarray(ref[k][b]), equal_nan=True), ("cycle", cycle, "slot", b, k)
        a, t = snapshot(subj), snapshot(twin)
        assert_same(a, t, named, ("cycle", cycle, "named slots"), UNTOUCHED + STATE_ALL)
        assert_same(tab_before, tables(subj), slice(None), ("cycle", cycle, "changed a table"))
        xa = ref["x"][:, 1].copy()
    assert_same(before, snapshot(subj), others, "another slot changed", UNTOUCHED + STATE_ALL)
    subj.close(); twin.close()


@pytest.mark.gpu
def test_260_named_slots_of_300_with_their_own_references_go_through_two_chunks():
    """float32 cart-pole, thread-serial kernels: 260 of 300 slots in shuffled order cross the 256-slot chunks of the intake area; slot b carries reference(b)"""
    fam, B, K, dtype = family("cart-ts"), 300, 260, 0
    N = fam["kw"]["N"]
    kw = dict(fam["kw"], tol_cost=0.0, max_iter=4)
    base_p, base_r = problems(2, N, dtype, 15), references(2, N, dtype, 15)
    probs, refs = [base_p[b % 15] for b in range(B)], [base_r[b % 15] for b in range(B)]
    rng = np.random.default_rng(93)
    left_out = set(int(v) for v in rng.permutation(np.arange(1, B - 1))[: B - K])      # (the first and the last slot are named)
    slots = [int(v) for v in rng.permutation(B) if int(v) not in left_out]
    others = sorted(left_out)
    assert len(slots) == K and slots != sorted(slots) and B - 1 in slots and 0 in slots
    shift = rng.integers(0, 3, B).astype(np.int32)
    xg = stack(probs, "xg").reshape(B, -1)
    subj, twin = [make_solver("hip", 2, dtype=dtype, batch=B, kernels=dict(fam["sel"]), **kw) for _ in range(2)]
    for s in (subj, twin):
        set_references(s, refs)
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
    # slots that differ only in their reference solve differently: slots 2 and 3 share nothing, 3 and 4 everything that is read, 0 and 15 everything
    assert np.array_equal(seed["x"][0], seed["x"][15]) and np.array_equal(seed["x"][3], seed["x"][4]) and not np.array_equal(seed["u"][1], seed["u"][2])
    subj.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 6: whole-handle control cycles
@pytest.mark.gpu
@pytest.mark.parametrize("fam,dtype", [pytest.param(QUAD_SLOTS, 0, id="quad-cf-f32"), pytest.param(family("cart-ts"), 1, id="cart-ts-f64"),
                                       pytest.param(family("cart-ts"), 0, id="cart-ts-f32"),      # (the family and element type of the 260-of-300 test's twin)
                                       pytest.param(family("pend-coop"), 0, id="pend-coop-f32")])
def test_whole_handle_control_cycles_equal_single_problem_handles(fam, dtype):
    """three pddp_mpc_solve cycles (shifts 1, 0, 2) on a batch of 5 with the five kinds against single-problem handles carrying those references: outputs and state
    records bit for bit.  Problem 2 also follows a goal path on both sides, problem 3 carries the ramp: the path's window moves by the shifts and the reference's rows do
    not move -- neither call touches the other's table."""
    plant, N, B = fam["plant"], fam["kw"]["N"], 5
    npos, n, m = DIMS[plant]
    T = np_type(dtype)
    kw = dict(fam["kw"], tol_cost=0.0, max_iter=4)
    probs, refs = problems(plant, N, dtype, B), references(plant, N, dtype, B)
    xg = stack(probs, "xg").reshape(B, n)
    shifts, cap = (1, 0, 2), N + 6
    path = (np.tile(probs[2]["xg"], (cap, 1)) + 0.003 * np.arange(1, cap + 1)[:, None] * (1.0 + 0.1 * np.arange(n))[None, :]).astype(T)

    def with_path(s, slot):
        s.reserve_goal_path(cap)
        s.set_goal_path_problems([slot], path[None], s.GOAL_PATH_HOLD)

    s = make_solver("hip", plant, dtype=dtype, batch=B, kernels=dict(fam["sel"]), **kw)
    set_references(s, refs)
    with_path(s, 2)
    U0, has0 = s.get_control_reference_problems(list(range(B)))
    outs = [s.solve(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"))]
    states = [state_rows(s, range(B))]
    for sh in shifts:
        outs.append(s.mpc_solve(outs[-1]["x"][:, 1].copy(), xg, sh, clear_vars=0, max_iter=4))
        states.append(state_rows(s, range(B)))
    cursor = s.get_goal_path_problems([2], rows=False)[2][0]
    assert cursor == sum(shifts), "the cursor advances by the shifts in knots"
    U1, has1 = s.get_control_reference_problems(list(range(B)))
    assert np.array_equal(U0, U1) and np.array_equal(has0, has1) and has0.tolist() == [0, 1, 1, 1, 1], "the cycles and the path left the references alone"
    G, ghas = s.get_goal_trajectory_problems(list(range(B)))
    assert ghas.tolist() == [0, 0, 1, 0, 0]
    s.close()
    for b in range(B):
        s1 = make_solver("hip", plant, dtype=dtype, batch=1, kernels=dict(fam["sel"]), **kw)
        if refs[b] is not None:
            s1.set_control_reference_problems([0], refs[b])
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
        if b == 2:                                                   # the path's window is where a handle without any reference leaves it
            assert np.array_equal(s1.get_goal_trajectory_problems([0])[0][0], G[2]), "the references moved the path's window"
        s1.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 7: setter, getter, clear, refusals
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_setter_getter_clear_and_every_refusal(dtype):
    fam = family("cart-ts")
    B, plant, N, m = 5, 2, fam["kw"]["N"], 1
    T = np_type(dtype)
    probs, refs = problems(plant, N, dtype, B), references(plant, N, dtype, B)
    s = handle(fam, dtype, B)
    assert s.has_control_reference() and s.control_reference_size() == N * m
    U, has = s.get_control_reference_problems([4, 0])                # before the first setter call (and before any load): zeros, has = 0
    assert U.shape == (2, N, m) and U.dtype == T and not U.any() and has.tolist() == [0, 0]
    s.clear_control_reference_problems([1, 3])                       # a successful no-op on a handle that never had a table
    names = kernel_names(s)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    s.iterate(1); s.sync()
    lib, EINVAL = s.lib, -1
    lib.pddp_set_control_reference_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_get_control_reference_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pddp_clear_control_reference_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good_idx, good = np.array([3, 0], np.int32), np.stack([refs[3], refs[1]])

    def poisoned(at, v):
        u = good.copy(); u.reshape(-1)[at] = v
        return u

    bad = [("count 0", 0, good_idx, good), ("count < 0", -2, good_idx, good), ("idx null", 2, None, good), ("U null", 2, good_idx, None),
           ("index == batch", 2, np.array([0, B], np.int32), good), ("index < 0", 2, np.array([-1, 2], np.int32), good), ("index twice", 2, np.array([2, 2], np.int32), good),
           ("nan", 2, good_idx, poisoned(0, np.nan)), ("inf", 2, good_idx, poisoned(N * m, np.inf)), ("-inf in row N - 1", 2, good_idx, poisoned(2 * N * m - 1, -np.inf))]
    values_only = ("nan", "inf", "-inf in row N - 1")

    def refused_everywhere(label):
        before = snapshot(s)
        rows = s.get_control_reference_problems(list(range(B)))
        for what, count, idx, U_ in bad:
            assert lib.pddp_set_control_reference_problems(s.h, count, ptr(idx), ptr(U_)) == EINVAL, (label, what)
            assert len(lib.pddp_last_error()) > 0, (label, what, "a refusal carries a message")
            if what not in values_only:
                o, h_ = np.zeros((2, N, m), T), np.zeros(2, np.int32)
                assert lib.pddp_get_control_reference_problems(s.h, count, ptr(idx), None if what == "U null" else ptr(o), ptr(h_)) == EINVAL, (label, what)
                assert not o.any() and not h_.any()
                if what != "U null":
                    assert lib.pddp_clear_control_reference_problems(s.h, count, ptr(idx)) == EINVAL, (label, what)
        after = snapshot(s)
        for k in UNTOUCHED + STATE_ALL:
            assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), (label, "a refused call changed", k)
        again = s.get_control_reference_problems(list(range(B)))
        assert np.array_equal(again[0], rows[0]) and np.array_equal(again[1], rows[1]), (label, "a refused call changed the table")

    refused_everywhere("without a table")
    assert kernel_names(s) == names
    reset_like_fresh(s)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    s.iterate(1); s.sync()
    # the setter on loaded slots changes neither g, the trajectory nor the state record until the next load
    before = snapshot(s)
    s.set_control_reference_problems([3, 1], np.stack([refs[3], refs[1]]))
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), ("the setter changed", k)
    assert kernel_names(s) == names                                 # (runs a sweep: the slots are reloaded below)
    # the tables it brought: built-in cost rows, no goal flagged, every step the handle's
    assert np.array_equal(s.get_diag_cost_problems(list(range(B))), np.tile(np.asarray(BUILTIN[plant], T).astype(np.float64), (B, 1)))
    assert s.get_goal_trajectory_problems(list(range(B)))[1].tolist() == [0] * B
    assert s.get_horizon_time_problems(list(range(B)))[0].tolist() == [fam["kw"]["total_time"]] * B
    U, has = s.get_control_reference_problems(list(range(B)))        # the round trip: rows exactly, unnamed slots zero and unflagged
    assert has.tolist() == [0, 1, 0, 1, 0] and np.array_equal(U[1], refs[1]) and np.array_equal(U[3], refs[3]) and not U[[0, 2, 4]].any()
    U, has = s.get_control_reference_problems([3, 2])
    assert has.tolist() == [1, 0] and np.array_equal(U[0], refs[3]) and not U[1].any()
    o = np.zeros((1, N, m), T)
    assert lib.pddp_get_control_reference_problems(s.h, 1, ptr(good_idx), ptr(o), None) == 0 and np.array_equal(o[0], refs[3])      # has may be NULL
    refused_everywhere("with a table")
    # the next load reads the rows: g differs from a handle without a table exactly in the named problems (slot 1's rows are zero: flagged, and still nothing)
    never = handle(fam, dtype, B)
    never.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    g0, H0, AB0 = (never.get(k).reshape(B, -1) for k in ("g", "H", "AB"))
    reset_like_fresh(s)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    g, H, AB = (s.get(k).reshape(B, -1) for k in ("g", "H", "AB"))
    assert [bool(np.array_equal(g[b], g0[b])) for b in range(B)] == [True, True, True, False, True]
    assert np.array_equal(H, H0) and np.array_equal(AB, AB0), "H and [A B] do not depend on a reference"
    # clear: the flag goes, the getter answers zeros; a loaded slot is not rebuilt; after the next load the handle is back where a handle without a table is
    s.clear_control_reference_problems([3, 1])
    U, has = s.get_control_reference_problems(list(range(B)))
    assert has.tolist() == [0] * B and not U.any()
    assert np.array_equal(s.get("g").reshape(B, -1), g), "the clear call rebuilt g of a loaded slot"
    reset_like_fresh(s); reset_like_fresh(never)
    for h in (s, never):
        h.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
        run_until_done(h)
    a, b_ = collect(s), collect(never)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b_[k]), equal_nan=True), ("after the clear", k)
    # the binding's shape check
    with pytest.raises(pyddp.PddpError, match="numbers"):
        s.set_control_reference_problems([0, 1], np.zeros((1, N, m), T))
    s.close(); never.close()


@pytest.mark.gpu
def test_arm_handles_refuse_all_four():
    EINVAL = -1
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    arm = make_solver("hip", 4, dtype=0, batch=2, N=32, M=4, A=8, wafr_urdf=1, total_time=0.5)
    idx, U, has = np.array([0, 1], np.int32), np.zeros((2, 32, 7), np.float32), np.zeros(2, np.int32)
    lib = arm.lib
    lib.pddp_control_reference_size.argtypes = [C.c_void_p]
    lib.pddp_set_control_reference_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_get_control_reference_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pddp_clear_control_reference_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    assert not arm.has_control_reference()
    assert lib.pddp_control_reference_size(arm.h) == EINVAL
    assert lib.pddp_set_control_reference_problems(arm.h, 2, ptr(idx), ptr(U)) == EINVAL
    assert lib.pddp_get_control_reference_problems(arm.h, 2, ptr(idx), ptr(U), ptr(has)) == EINVAL
    assert lib.pddp_clear_control_reference_problems(arm.h, 2, ptr(idx)) == EINVAL
    assert not U.any() and not has.any()
    with pytest.raises(pyddp.PddpError):
        arm.control_reference_size()
    arm.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 8: the captured graph
@pytest.mark.gpu
@pytest.mark.parametrize("fam", [pytest.param(family(k), id=k) for k in ("cart-cf-gl-kb16", "quad-mq-fused-cf-kb16", "pend-coop")])
def test_graph_replay_follows_the_reference_table(fam):
    """use_graph = 1: iterate, set a first reference, reload and iterate, set another, reload and iterate -- bit for bit a use_graph = 0 handle given the same calls.
    The first setter call drops the captured graph (other kernels); the second only writes rows, which the graph captured after the first call reads without a new
    capture."""
    dtype, B, plant, N = 0, 3, fam["plant"], fam["kw"]["N"]
    probs = problems(plant, N, dtype, B)
    outs = []
    for use_graph in (1, 0):
        s = handle(fam, dtype, B, use_graph)
        stages = []
        for U in (None, reference(plant, N, dtype, 3), reference(plant, N, dtype, 8)):
            if U is not None:
                s.set_control_reference_problems([1], U)
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
        assert not np.array_equal(plain[i]["Jout"][1], plain[j]["Jout"][1]), "the reference changed nothing"
        assert np.array_equal(plain[i]["Jout"][0], plain[j]["Jout"][0]) and np.array_equal(plain[i]["Jout"][2], plain[j]["Jout"][2])
