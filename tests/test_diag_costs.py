"""Run-time diagonal cost weights of the pendulum, cart-pole and quadrotor: pddp_diag_cost_size / pddp_set_diag_cost / pddp_set_diag_cost_problems /
pddp_get_diag_cost_problems (csrc/diag_cost_table.hpp, csrc/plants.hpp DiagTab).

The record of a problem is [ q_0..q_{n-1} | r_0..r_{m-1} | qf_0..qf_{n-1} ].  BUILTIN below restates the constants of plants/cost_{pend,cart,quad}.cuh; nothing here reads
them from the library except where the getter itself is under test.

Yardsticks:
  * a handle that never called a setter (the literals' instantiations) for a table of built-in rows -- bit for bit, every array pddp_get_array names;
  * a SINGLE-PROBLEM handle pinned to the same kernels and given the problem's record with pddp_set_diag_cost for a batch with a table -- bit for bit;
  * the oracle for run-time weights.  Its plants 1-3 have fixed weights, its plant 5 takes a plug-in: tests/plugin_diag/diag_shim.cpp forwards dynamics to the
    oracle's own plant 1, 2 or 3 and evaluates the diagonal formulas with a record the test sets (the "shim-oracle").  The CPU test first holds the shim-oracle with the
    built-in record against the oracle's own plants.

Kernel families are pinned through pddp_config.kernels and asserted by name (time_kernels).  Shapes: N 16 / 32, M 1 / 4, A 4 / 8 -- and A = 16 for the quadrotor
families that include the staged rollouts (k_fp_cf serves 8 or 16 step sizes, and a wavefront has to hold whole 12-state problems: 16 only); batches 3, 5 and 67
(67: a wave of the thread-serial kernels holds problems with different records and the last wave is partial).
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


def typed(a, dtype):
    return np.asarray(a, np.float32 if dtype == 0 else np.float64).astype(np.float64)


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
    T = np.float32 if dtype == 0 else np.float64
    return dict(x0=x0.astype(T), u0=u0.astype(T), xg=xg.astype(T))


def problems(plant, N, dtype, B, skip=0):
    return [problem(plant, N, dtype, skip + b) for b in range(B)]


def stack(probs, key):
    return np.concatenate([p[key].ravel() for p in probs])


def records(plant, B, seed):
    """[B][2 n + m] positive records, multiples of the built-in one in [0.3, 3] per entry (so qf differs per state in every row); row 1 has zeros in q (first and last
    state), row 2 a qf that spans two decades over the states, row 0 is the built-in record"""
    npos, n, m = DIMS[plant]
    rng = np.random.default_rng(77 * plant + seed)
    w = BUILTIN[plant] * np.exp(rng.uniform(np.log(0.3), np.log(3.0), (B, 2 * n + m)))
    w[0] = BUILTIN[plant]
    if B > 1:
        w[1, 0] = w[1, n - 1] = 0.0
    if B > 2:
        w[2, n + m:] = BUILTIN[plant][n + m:] * np.logspace(-1, 1, n)
    return w


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


def solve_single(s1, prob, rec=None):
    """the yardstick: one problem on a single-problem handle in the state of a fresh one, its record set handle-wide, sweep by sweep until it exits"""
    if rec is not None:
        s1.set_diag_cost(rec)
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
        src = os.path.join(ROOT, "tests", "plugin_diag", "diag_shim.cpp")
        out = os.path.join(ROOT, "tests", "plugin_diag", "libdiag_shim.so")
        if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-o", out, src])
        _SHIM["lib"], _SHIM["path"] = C.CDLL(out), out
    return _SHIM["lib"], _SHIM["path"]


def shim_oracle(plant, kw, rec, dtype=np.float64):
    """the oracle's plant 5 = plant `plant` with the diagonal record `rec`: same solver configuration as Oracle(default_cfg(plant, **kw))"""
    lib, path = shim()
    L = oracle_binding.lib()
    base = default_cfg(plant, cores=1, spawn_threads=0, **kw)
    npos, n, m = DIMS[plant]
    rec = np.ascontiguousarray(rec, np.float64)
    addr = lambda f: C.cast(f, C.c_void_p)
    lib.diag_shim_set.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_void_p] * 4
    lib.diag_shim_set(C.byref(base), n, m, kw["N"], rec.ctypes.data_as(C.c_void_p), addr(L.ora_dynamics_f32), addr(L.ora_dynamics_gradient_f32), addr(L.ora_dynamics_f64),
                      addr(L.ora_dynamics_gradient_f64))
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
    for sym in ("pddp_diag_cost_size", "pddp_set_diag_cost", "pddp_set_diag_cost_problems", "pddp_get_diag_cost_problems"):
        assert getattr(lib, sym) is not None
    assert "int pddp_diag_cost_size(pddp_handle h);" in header
    assert "int pddp_set_diag_cost(pddp_handle h, const double* w" in header
    assert "int pddp_set_diag_cost_problems(pddp_handle h, int count, const int* idx, const double* w" in header
    assert "int pddp_get_diag_cost_problems(pddp_handle h, int count, const int* idx, double* w" in header
    for name in ("diag_cost_size", "set_diag_cost", "set_diag_cost_problems", "get_diag_cost_problems", "has_diag_cost"):
        assert callable(getattr(pyddp.Solver, name))


# ---------------------------------------------------------------------------------------------------------------- CPU 2: the host-only code under the sanitizers
def test_host_only_code_as_a_stand_alone_program(tmp_path):
    """tests/native/diag_cost_host_check.cpp (its own main, -fsanitize=address,undefined): every argument check, the built-in record, the packing, and the DiagTab
    policy on the built-in record against the literal policy, bit for bit"""
    exe = str(tmp_path / "diag_cost_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "diag_cost_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "diag_cost_host_check: ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------- CPU 3: the shim-oracle is the oracle
@pytest.mark.parametrize("plant,kw", ORACLE_CASES)
def test_shim_oracle_with_the_builtin_record_reproduces_the_oracles_own_plant(plant, kw):
    """Whole solves (ora_run_ilqr_gpusem, float64): identical iteration counts and alphaOut are required; J, x, u, KT in float64.
    Measured deviation: 0 in every case of ORACLE_CASES, every array (max |a - b| == 0.0) -- the shim's cost sums are the oracle's own statements (weight * pow(d, 2) in
    index order, 0.5 * sum) and its dynamics ARE the oracle's, so nothing differs; the bound asserted is therefore exact equality (10 x 0).
    Also: g, H and the per-knot cost of the shim for a random positive record against a NumPy restatement of the formulas."""
    npos, n, m = DIMS[plant]
    N = kw["N"]
    kw = dict(kw, tol_cost=0.0)
    for seed in (1, 2):
        p = problem(plant, N, 1, seed)
        own = Oracle(default_cfg(plant, cores=1, spawn_threads=0, **kw), np.float64).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
        via = shim_oracle(plant, kw, BUILTIN[plant]).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
        assert via["iters"] == own["iters"] and list(via["alphaOut"]) == list(own["alphaOut"])
        assert sum(a >= 0 for a in own["alphaOut"][1: own["iters"] + 1]) >= 2, "the case must accept iterations"
        for k in ("Jout", "x", "u", "KT"):
            dev = float(np.abs(via[k] - own[k]).max())
            print("shim-oracle against the oracle's plant %d, problem %d, %s: max deviation %.3g" % (plant, seed, k, dev))
            assert dev == 0.0, (k, dev)
    rng = np.random.default_rng(5 + plant)
    rec = BUILTIN[plant] * np.exp(rng.uniform(np.log(0.2), np.log(5.0), 2 * n + m))
    o = shim_oracle(plant, kw, rec)
    q, r, qf = rec[:n], rec[n: n + m], rec[n + m:]
    for k in (0, 3, N - 2, N - 1):
        x, u, xg = rng.normal(0, 1.5, n), rng.normal(0, 2.0, m), rng.normal(0, 1.0, n)
        H, g = o.cost_grad(x, u, xg, k)
        fin = k == N - 1
        Hw = np.diag(np.concatenate([qf, np.zeros(m)]) if fin else np.concatenate([q, r]))
        gw = np.concatenate([qf * (x - xg), np.zeros(m)]) if fin else np.concatenate([q * (x - xg), r * u])
        cw = 0.5 * np.sum(qf * (x - xg) ** 2) if fin else 0.5 * (np.sum(q * (x - xg) ** 2) + np.sum(r * u ** 2))
        assert np.array_equal(H.reshape(n + m, n + m), Hw) and np.array_equal(g, gw)
        assert abs(o.cost_func(x, u, xg, k) - cw) <= 1e-14 * abs(cw)


# ---------------------------------------------------------------------------------------------------------------- CPU 4: the scheduler picks the diagonal methods
def test_scheduler_uses_the_diagonal_methods_on_a_solver_that_has_diagonal_records():
    from test_refill import FakeSolver

    class DiagFake(FakeSolver):
        WIDE = np.arange(9.0)

        def __init__(self, batch, exit_sweeps):
            super().__init__(batch, exit_sweeps)
            self.calls, self.rows = [], [self.WIDE.copy() for _ in range(batch)]

        def has_diag_cost(self):
            return True

        def get_diag_cost_problems(self, idx):
            self.calls.append("get")
            return np.array([self.rows[i] for i in idx])

        def set_diag_cost_problems(self, idx, w):
            self.calls.append("set")
            for i, r in zip(idx, np.asarray(w, np.float64).reshape(len(idx), -1)):
                self.rows[int(i)] = r.copy()

        def set_cost_problems(self, idx, w):
            raise AssertionError("the arm's setter on a handle with diagonal records")

        def load_problems(self, idx, x0, u0, xg, ignore_first_defect=1):
            super().load_problems(idx, x0, u0, xg, ignore_first_defect)
            for slot, tag in zip(idx, x0):
                self.at_load[int(tag)] = self.rows[int(slot)].copy()

        def load(self, x0, u0, xg, clear_vars=1, ignore_first_defect=1):
            super().load(x0, u0, xg, clear_vars, ignore_first_defect)
            self.at_load = {int(x0[s]): self.rows[s].copy() for s in range(self.B)}

    fake = DiagFake(2, [2, 1, 3, 1, 2])
    tag = lambda p: np.array([p])
    probs = [(tag(p), tag(p), tag(p), np.arange(9.0) + 10 * (p + 1)) if p != 3 else (tag(p), tag(p), tag(p)) for p in range(5)]
    got = list(pyddp.SlotScheduler(fake, iter(probs), 2, sweeps_per_poll=1).run())
    assert sorted(i for i, _ in got) == list(range(5)) and fake.calls.count("get") == 1
    for p in range(5):
        assert np.array_equal(fake.at_load[p], DiagFake.WIDE if p == 3 else np.arange(9.0) + 10 * (p + 1)), p


# ---------------------------------------------------------------------------------------------------------------- GPU 1: defaults are the constants
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("fam", FAMILY_PARAMS)
def test_a_table_of_builtin_rows_solves_bit_for_bit_like_a_handle_without_a_table(fam, dtype):
    B = min(fam["B"], 5)
    probs = problems(fam["plant"], fam["kw"]["N"], dtype, B)
    outs = []
    for with_table in (False, True):
        s = handle(fam, dtype, B)
        if with_table:
            rows = s.get_diag_cost_problems(list(range(B)))
            assert np.array_equal(rows, np.tile(typed(BUILTIN[fam["plant"]], dtype), (B, 1)))
            s.set_diag_cost(rows[0])
            assert np.array_equal(s.get_diag_cost_problems(list(range(B))), rows)
            handle_names = [n for n, _ in s.time_kernels(1)]                       # (same names with a table: the family did not change)
            assert all(any(h.startswith(n) for h in handle_names) for n in fam["names"])
        reset_like_fresh(s)
        s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
        after_load = {k: s.get(k).copy() for k in ("H", "g", "AB", "Jout")}
        run_until_done(s)
        res = collect(s)
        res.update({"load_" + k: v for k, v in after_load.items()})
        res.update({"arr_" + k: s.get(k) for k in ARRAYS})
        outs.append(res)
        s.close()
    plain, table = outs
    assert len(set(plain["iter"])) >= 2, ("the problems must exit at different iterations", plain["iter"])
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(table[k]), equal_nan=True), (fam["key"], dtype, k)


# ---------------------------------------------------------------------------------------------------------------- GPU 2: a batch with a table is B single-problem handles
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("fam", FAMILY_PARAMS)
def test_batch_with_a_table_equals_single_problem_handles(fam, dtype):
    B, plant = fam["B"], fam["plant"]
    probs = problems(plant, fam["kw"]["N"], dtype, B)
    recs = records(plant, B, 41)
    s1 = handle(fam, dtype, 1)
    refs = [solve_single(s1, probs[b], recs[b]) for b in range(B)]
    plain = solve_single(s1, probs[B - 1], BUILTIN[plant])
    s1.close()
    assert len({int(r["iter"]) for r in refs}) >= 2, "the problems must exit at different iterations"
    assert not np.array_equal(refs[B - 1]["Jout"], plain["Jout"]), "the records changed nothing"
    for use_graph in (1, 0):
        label = "%s dtype=%d use_graph=%d" % (fam["key"], dtype, use_graph)
        s = handle(fam, dtype, B, use_graph)
        named = [b for b in reversed(range(B)) if b != 0]                              # unsorted on purpose; slot 0 keeps the built-in row (recs[0])
        s.set_diag_cost_problems(named, recs[named])
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
        s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 3: against the reference
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


@pytest.mark.gpu
@pytest.mark.parametrize("plant,kw", ORACLE_CASES)
def test_float64_batch_with_a_table_follows_the_shim_oracle(plant, kw):
    """B = 3 problems with three records on the library's own selection for the shape: after pddp_load H, g and the initial cost against the shim-oracle's
    ora_next_iteration_setup / ora_total_cost at the float64 bound of tests/test_phase_parity.py (1e-9 of the largest magnitude), then the whole solves decision for
    decision at the bounds of tests/test_solver_parity.py.  (The array "costk" is not written for these plants -- only the end-effector cost leaves per-knot costs --
    so the per-knot cost is held on the CPU side, shim against NumPy.)"""
    npos, n, m = DIMS[plant]
    N, B = kw["N"], 3
    kw = dict(kw, tol_cost=0.0)
    probs = problems(plant, N, 1, B)
    recs = records(plant, B, 53)
    s = make_solver("hip", plant, dtype=1, batch=B, **kw)
    s.set_diag_cost_problems([2, 1], recs[[2, 1]])
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    H, g, st = s.get("H").reshape(B, N, n + m, n + m), s.get("g").reshape(B, -1), s.get_state()
    for b in range(B):
        o = shim_oracle(plant, kw, recs[b])
        _, Ho, go = o.next_iteration_setup(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        Ho = Ho.reshape(N, n + m, n + m)
        assert nrel(H[b], Ho) <= 1e-9 and nrel(g[b], go) <= 1e-9, (b, "H / g after the load")      # every knot whole: the final knot's control rows and columns are zeros on both sides
        assert np.array_equal(H[b][N - 1, n:, :], np.zeros((m, n + m))) and np.array_equal(H[b][N - 1, :, n:], np.zeros((n + m, m))), (b, "final knot, control block")
        J0 = o.total_cost(1, probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        assert abs(st[b].prevJ - J0) <= 1e-9 * abs(J0), (b, st[b].prevJ, J0)
    run_until_done(s)
    out = s.store()
    out["iters"] = np.array([x.iter for x in s.get_state()])
    accepted = 0
    for b in range(B):
        ref = shim_oracle(plant, kw, recs[b]).run_ilqr_gpusem(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        accepted += sum(a >= 0 for a in ref["alphaOut"][1: ref["iters"] + 1])
        check_against_oracle(out, b, ref, (plant, b))
    assert accepted >= 3, "the cases must accept iterations"
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plant", [1, 2, 3])
def test_float32_with_a_record_follows_the_shim_oracle_over_the_leading_iterations(plant):
    """the way tests/test_ref_plugin.py does it: alphaOut equal to the float32 AND the float64 shim-oracle over the leading iterations, J there inside
    max(1e-4, 5 x the float32 oracle's own error).  The number of leading iterations required is what the two ORACLES agree on for the problem (their own float32
    error decides how long a float32 solve can follow), at least 3: the wave-cooperative kernels execute the reference's operations one for one."""
    kw = dict(base_kw(plant, 32, 4, 8, 3), tol_cost=0.0)
    rec = typed(records(plant, 4, 61)[3], 0)
    p32 = problem(plant, 32, 0, 1)
    p64 = {k: v.astype(np.float64) for k, v in p32.items()}
    r32 = shim_oracle(plant, kw, rec, np.float32).run_ilqr_gpusem(p32["x0"], p32["u0"], p32["xg"])
    r64 = shim_oracle(plant, kw, rec, np.float64).run_ilqr_gpusem(p64["x0"], p64["u0"], p64["xg"])
    agree = next((i for i in range(r64["iters"] + 1) if r32["alphaOut"][i] != r64["alphaOut"][i]), r64["iters"] + 1)
    assert agree >= 3, (r32["alphaOut"], r64["alphaOut"])
    s = make_solver("hip", plant, dtype=0, batch=1, kernels=dict(cf="coop"), **kw)
    s.set_diag_cost(rec)
    out = s.solve(p32["x0"], p32["u0"], p32["xg"])
    lead = next((i for i in range(r64["iters"] + 1) if not (out["alphaOut"][0][i] == r32["alphaOut"][i] == r64["alphaOut"][i])), r64["iters"] + 1)
    assert lead >= agree, (out["alphaOut"][0], r32["alphaOut"], r64["alphaOut"])
    for i in range(lead):
        ek, eo = abs(float(out["Jout"][0][i]) - r64["Jout"][i]) / r64["Jout"][i], abs(float(r32["Jout"][i]) - r64["Jout"][i]) / r64["Jout"][i]
        assert ek <= max(1e-4, 5 * eo), (i, ek, eo)
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 4: slots
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
def test_refill_of_named_slots_with_records(dtype):
    fam, B = QUAD_SLOTS, QUAD_SLOTS["B"]
    first, late = problems(3, 16, dtype, B), problems(3, 16, dtype, 2, skip=11)
    recs = records(3, 4, 59)[[3, 1]]
    s1 = handle(fam, dtype, 1)
    ref_first = [solve_single(s1, p, BUILTIN[3]) for p in first]
    ref_late = [solve_single(s1, p, r) for p, r in zip(late, recs)]
    s1.close()
    s = handle(fam, dtype, B)
    reset_like_fresh(s)
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    s.iterate(2); s.sync()
    done, _ = s.status()
    slots = [3, 0]
    others = [b for b in range(B) if b not in slots]
    assert any(not done[b] for b in others), "no running slot among the others"
    before = snapshot(s)
    s.set_diag_cost_problems(slots, recs)                       # the handle's first setter call: the table appears under running problems
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k])[others], np.asarray(after[k])[others], equal_nan=True), ("another slot changed", k)
    assert np.array_equal(s.get_diag_cost_problems(others), np.tile(typed(BUILTIN[3], dtype), (len(others), 1)))
    assert np.array_equal(s.get_diag_cost_problems(slots), typed(recs, dtype))
    run_until_done(s)
    got = collect(s)
    for j, b in enumerate(slots):
        assert_rows_equal(got, b, ref_late[j], ("refilled slot", b))
    for b in others:
        assert_rows_equal(got, b, ref_first[b], ("unnamed slot", b))
    s.close()


@pytest.mark.gpu
def test_a_control_cycle_of_named_slots_runs_with_their_own_records():
    """float32 quadrotor, B = 4 with four records: a solve seeds every slot, then ONE pddp_mpc_solve_problems cycle on slots [2, 0] (shift 1, clear_vars 0, 4 iterations, the
    measured state = knot 1 of the slot's plan) against single-problem handles given the record with pddp_set_diag_cost and driven through pddp_solve + pddp_mpc_solve;
    the slots that are not named keep every array and their state."""
    fam, B, dtype = QUAD_SLOTS, 4, 0
    kw = dict(fam["kw"], tol_cost=0.0, max_iter=4)
    probs = problems(3, 16, dtype, B)
    recs = records(3, B, 67)
    keys = ("x", "u", "KT", "Jout", "alphaOut", "success", "iters")
    s = make_solver("hip", 3, dtype=dtype, batch=B, kernels=dict(fam["sel"]), **kw)
    s.set_diag_cost_problems([3, 2, 1], recs[[3, 2, 1]])
    seed = s.solve(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"))
    named = [2, 0]
    before = snapshot(s)
    xg = stack(probs, "xg").reshape(B, -1)
    got = s.mpc_solve_problems(named, seed["x"][named, 1].copy(), xg[named], [1, 1], clear_vars=0, max_iter=4)
    after = snapshot(s)
    others = [1, 3]
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k])[others], np.asarray(after[k])[others], equal_nan=True), ("another slot changed", k)
    s.close()
    for j, b in enumerate(named):
        s1 = make_solver("hip", 3, dtype=dtype, batch=1, kernels=dict(fam["sel"]), **kw)
        s1.set_diag_cost(recs[b])
        one = s1.solve(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        for k in ("x", "u", "Jout", "alphaOut"):
            assert np.array_equal(np.asarray(one[k][0]), np.asarray(seed[k][b]), equal_nan=True), ("seed solve", b, k)
        ref = s1.mpc_solve(one["x"][:, 1].copy(), xg[[b]], 1, clear_vars=0, max_iter=4)
        s1.close()
        for k in keys:
            assert np.array_equal(np.asarray(got[k][j]), np.asarray(ref[k][0]), equal_nan=True), ("cycle, slot", b, k)


@pytest.mark.gpu
def test_solve_stream_with_records_returns_every_problems_own_solution():
    cart = next(f for f in FAMILIES if f["key"] == "cart-ts")
    count, B, dtype = 7, 3, 0
    probs = problems(2, cart["kw"]["N"], dtype, count)
    recs = records(2, count, 71)
    has_rec = lambda p: p != 4                                                      # problem 4 is a plain 3-tuple: it gets the built-in record
    s1 = handle(cart, dtype, 1)
    refs = [solve_single(s1, probs[p], recs[p] if has_rec(p) else BUILTIN[2]) for p in range(count)]
    s1.close()
    s = handle(cart, dtype, B)
    stream = ((probs[p]["x0"], probs[p]["u0"], probs[p]["xg"], recs[p]) if has_rec(p) else (probs[p]["x0"], probs[p]["u0"], probs[p]["xg"]) for p in range(count))
    got = dict(pyddp.solve_stream(s, stream, sweeps_per_poll=2))
    s.close()
    assert sorted(got) == list(range(count))
    for p in range(count):
        for k in ("x", "u", "KT", "Jout", "alphaOut"):
            assert np.array_equal(np.asarray(got[p][k]).ravel(), np.asarray(refs[p][k]).ravel(), equal_nan=True), ("stream problem", p, k)


# ---------------------------------------------------------------------------------------------------------------- GPU 5: round trip and refusals
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_round_trip_and_refusals(dtype):
    fam = next(f for f in FAMILIES if f["key"] == "cart-ts")
    B, rec = 5, 9
    probs = problems(2, fam["kw"]["N"], dtype, B)
    s = handle(fam, dtype, B)
    assert s.diag_cost_size() == rec
    assert np.array_equal(s.get_diag_cost_problems(list(range(B))), np.tile(typed(BUILTIN[2], dtype), (B, 1)))      # before any setter call
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    s.iterate(1); s.sync()
    lib, EINVAL = s.lib, -1
    lib.pddp_set_diag_cost_problems.argtypes = lib.pddp_get_diag_cost_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_set_diag_cost.argtypes = [C.c_void_p, C.c_void_p]
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good_idx, w = np.array([3, 0], np.int32), np.arange(1.0, 2 * rec + 1)

    def bad_at(e, v):
        a = w.copy(); a[rec + e] = v
        return a

    bad = [("count 0", 0, good_idx, w), ("count < 0", -2, good_idx, w), ("idx null", 2, None, w), ("w null", 2, good_idx, None),
           ("index == batch", 2, np.array([0, B], np.int32), w), ("index < 0", 2, np.array([-1, 2], np.int32), w), ("index twice", 2, np.array([2, 2], np.int32), w),
           ("nan", 2, good_idx, bad_at(7, np.nan)), ("inf", 2, good_idx, bad_at(2, np.inf)), ("negative q", 2, good_idx, bad_at(1, -0.5)),
           ("negative qf", 2, good_idx, bad_at(8, -1e-9)), ("r == 0", 2, good_idx, bad_at(4, 0.0)), ("negative r", 2, good_idx, bad_at(4, -1.0))]
    values_only = ("nan", "inf", "negative q", "negative qf", "r == 0", "negative r")

    def refused_everywhere(label):
        before = snapshot(s)
        rows = s.get_diag_cost_problems(list(range(B)))
        for what, count, idx, ww in bad:
            assert lib.pddp_set_diag_cost_problems(s.h, count, ptr(idx), ptr(ww)) == EINVAL, (label, what)
            if what in values_only:
                assert lib.pddp_set_diag_cost(s.h, ptr(ww[rec:])) == EINVAL, (label, what)
            else:
                out = np.zeros(2 * rec)
                assert lib.pddp_get_diag_cost_problems(s.h, count, ptr(idx), None if ww is None else ptr(out)) == EINVAL, (label, what)
        assert lib.pddp_set_diag_cost(s.h, None) == EINVAL
        after = snapshot(s)
        for k in UNTOUCHED + STATE_ALL:
            assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), (label, "a refused call changed", k)
        assert np.array_equal(s.get_diag_cost_problems(list(range(B))), rows), (label, "a refused call changed the table")

    refused_everywhere("without a table")
    recs = records(2, B, 41)
    named = [4, 2, 1]
    s.set_diag_cost_problems(named, recs[named])
    want = np.tile(typed(BUILTIN[2], dtype), (B, 1)); want[named] = typed(recs[named], dtype)
    assert np.array_equal(s.get_diag_cost_problems(list(range(B))), want)
    assert np.array_equal(s.get_diag_cost_problems([B - 1, 0]), want[[B - 1, 0]])
    refused_everywhere("with a table")
    s.set_diag_cost(recs[3])                                                         # the handle-wide call overwrites every row
    assert np.array_equal(s.get_diag_cost_problems(list(range(B))), np.tile(typed(recs[3], dtype), (B, 1)))
    # q = 0 and qf = 0 are accepted
    zero = recs[3].copy(); zero[:4] = 0.0; zero[5:] = 0.0
    s.set_diag_cost(zero)
    assert np.array_equal(s.get_diag_cost_problems([1])[0], typed(zero, dtype))
    s.close()
    for plant, size in ((1, 5), (3, 28)):
        h = make_solver("hip", plant, dtype=dtype, batch=1, **base_kw(plant, 16, 4, 4, 1))
        assert h.diag_cost_size() == size and np.array_equal(h.get_diag_cost_problems([0])[0], typed(BUILTIN[plant], dtype))
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plant", [1, 2, 3])
def test_set_cost_leaves_a_table_of_diagonal_records_alone(plant):
    """pddp_set_cost is the arm's call; on plants 1-3 it has always returned 0 and changed nothing the kernels read.  With a table of diagonal records it must stay so:
    the rows, and H / g / the initial cost of the next load, are what they were before the call (the numbers passed are nothing like the records, and R = 0)."""
    npos, n, m = DIMS[plant]
    B, dtype = 3, 0
    kw = base_kw(plant, 16, 4, 4, 3)
    probs, recs = problems(plant, 16, dtype, B), records(plant, B, 83)
    s = make_solver("hip", plant, dtype=dtype, batch=B, **kw)
    s.set_diag_cost_problems([2, 1], recs[[2, 1]])
    rows = s.get_diag_cost_problems(list(range(B)))
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    before = {k: s.get(k).copy() for k in ("H", "g", "Jout")}
    s.set_cost(7.0, 0.25, 0.0, -3.0, 11.0)
    assert np.array_equal(s.get_diag_cost_problems(list(range(B))), rows), "pddp_set_cost wrote into the table of diagonal records"
    reset_like_fresh(s)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    for k, v in before.items():
        assert np.array_equal(s.get(k), v, equal_nan=True), ("pddp_set_cost changed what the next load computes", k)
    s.set_diag_cost_problems([0], recs[[1]])                     # the table still takes rows afterwards
    want = rows.copy(); want[0] = typed(recs[1], dtype)
    assert np.array_equal(s.get_diag_cost_problems(list(range(B))), want)
    plain = make_solver("hip", plant, dtype=dtype, batch=B, **kw)          # and without a table the call is as inert as ever
    plain.set_cost(7.0, 0.25, 0.0, -3.0, 11.0)
    assert np.array_equal(plain.get_diag_cost_problems(list(range(B))), np.tile(typed(BUILTIN[plant], dtype), (B, 1)))
    plain.close()
    s.close()


@pytest.mark.gpu
def test_arm_and_plugin_handles_refuse_all_four():
    EINVAL = -1
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    w, idx, out = np.arange(1.0, 71.0), np.array([0, 1], np.int32), np.zeros(70)
    from test_ref_plugin import HIPLIB, KW as PLUGIN_KW
    arm = make_solver("hip", 4, dtype=0, batch=2, N=32, M=4, A=8, wafr_urdf=1, total_time=0.5)
    plug = pyddp.Solver(pyddp.default_config(5, _lib_path=HIPLIB, dtype=0, batch=2, **PLUGIN_KW), _lib_path=HIPLIB)
    for h in (arm, plug):
        lib = h.lib
        lib.pddp_set_diag_cost_problems.argtypes = lib.pddp_get_diag_cost_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.pddp_set_diag_cost.argtypes = [C.c_void_p, C.c_void_p]
        assert lib.pddp_diag_cost_size(h.h) == EINVAL
        assert lib.pddp_set_diag_cost(h.h, ptr(w)) == EINVAL
        assert lib.pddp_set_diag_cost_problems(h.h, 2, ptr(idx), ptr(w)) == EINVAL
        assert lib.pddp_get_diag_cost_problems(h.h, 2, ptr(idx), ptr(out)) == EINVAL
        h.close()
