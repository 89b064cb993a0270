"""pddp_simulate_problems: the simulated robots of NAMED slots, each at the knot spacing of its own horizon time (csrc/sim_slots.hpp, csrc/sim.hpp
PlantSimSlotIn, k_plant_sim_slots / k_plant_sim_ts in csrc/kernels.hpp).

Yardsticks:
  * pddp_simulate on a SINGLE-PROBLEM handle created with cfg.total_time = t_b, given slot b's plan -- bit for bit, for an entry of a handle with a step table;
  * the same rows of pddp_simulate_batch -- bit for bit, on a handle without a step table;
  * the wave family (a wavefront per entry) for the thread family (a thread per entry) -- bit for bit;
  * the oracle, which takes total_time directly, with the tolerances tests/test_simulate_batch.py uses for this body.

Shapes: N 16 (RK3) and 32 (Euler), M 2, A 4; batches 5 and 67; counts up to 130; 4 to 40 sub-steps.  Horizon times are test_horizon_time.py's mixture -- slot 0 is never
named and keeps the default, slots 1, 2 and 4 get 0.6 / 1.37 / 1.5 of it -- with slot 3 very short (0.3 of the default).  Start states: a slot's plan's first knot plus
small noise, as in test_simulate_batch.py.  Each handle below is solved once per (plant, element type) and only READ by the tests that share it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyddp
from backends import make_solver
from oracle_binding import Oracle, default_cfg
from test_horizon_time import (ARRAYS, DIMS, MPC_KEYS, OUT_KEYS, STATE_ALL, UNTOUCHED, base_kw, collect, horizon_time, np_type, problems, set_times, snapshot, stack,
                               state_rows, tables)
from test_simulate_batch import KW as ARM_KW, SIGMA, T0_US as ARM_T0_US, KNOTS as ARM_KNOTS, STEP_US as ARM_STEP_US, solved as arm_solved

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PLANTS = [pytest.param(1, id="pend"), pytest.param(2, id="cart"), pytest.param(3, id="quad")]
DTYPES = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
FAMILIES = [pytest.param(1, id="wave"), pytest.param(2, id="thread")]
PLANS = [pytest.param(False, id="device-plans"), pytest.param(True, id="host-plans")]
SWEEPS = 3
SUBSTEPS = (4, 7, 40, 13, 5, 22)


def kw_small(plant):
    return base_kw(plant, 16, 2, 4, 3)                       # N 16, RK3


def kw_big(plant):
    return base_kw(plant, 32, 2, 4, 1)                       # N 32, Euler


def spacing_us(t, N):
    return t / (N - 1) * 1000.0 * 1000.0                     # the expression of step_us (csrc/handle_setup.hpp)


def mixed_times(N, B):
    """test_horizon_time.py's mixture; every slot b with b % 5 == 3 very short"""
    return [0.3 * N / 32.0 if b % 5 == 3 else horizon_time(N, b) for b in range(B)]


def solved_handle(plant, dtype, kw, B, table, **more):
    """a handle of B different problems after a load and SWEEPS sweeps; table: mixed horizon times, slots with b % 5 == 0 never named"""
    N = kw["N"]
    s = make_solver("hip", plant, dtype=dtype, batch=B, **dict(kw, **more))
    times = mixed_times(N, B) if table else [kw["total_time"]] * B
    if table:
        named = [b for b in range(B) if b % 5]
        set_times(s, [times[b] for b in named], named)
    probs = problems(plant, N, dtype, B)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    s.iterate(SWEEPS); s.sync()
    plan = s.store_problems(list(range(B)), only=("x", "u", "KT"))
    assert all(np.isfinite(plan[k]).all() for k in ("x", "u", "KT"))
    rng = np.random.default_rng(77 + plant)
    xa = np.stack([plan["x"][b][0] + rng.normal(0, SIGMA[b % 5], DIMS[plant][1]) for b in range(B)]).astype(np_type(dtype))
    return dict(s=s, plan=plan, xa=xa, times=times, N=N, B=B, probs=probs, kw=kw, plant=plant, dtype=dtype)


_HANDLES = {}


def shared(kind, plant, dtype):
    """"small": batch 5, N 16, RK3, step table; "big": batch 67, N 32, Euler, step table; "plain": batch 67, N 32, Euler, NO table.  Solved once, only read afterwards."""
    key = (kind, plant, dtype)
    if key not in _HANDLES:
        _HANDLES[key] = solved_handle(plant, dtype, kw_small(plant) if kind == "small" else kw_big(plant), 5 if kind == "small" else 67, kind != "plain")
    return _HANDLES[key]


def entry_plans(c, idx):
    return dict(x=c["plan"]["x"][idx], u=c["plan"]["u"][idx], KT=c["plan"]["KT"][idx])


def assert_same(got, want, label=""):
    assert np.array_equal(got[0], want[0]), (label, "state")
    assert np.array_equal(np.asarray(got[1]), np.asarray(want[1])), (label, "error")
    assert np.array_equal(np.asarray(got[2]), np.asarray(want[2])), (label, "failed")


def rows(res, sel):
    return tuple(np.asarray(v)[sel] for v in res)


# ---------------------------------------------------------------------------------------------------------------- CPU 1: the surface
def test_symbol_header_and_binding_exist():
    assert hasattr(C.CDLL(pyddp.library_path()), "pddp_simulate_problems")
    header = open(os.path.join(ROOT, "include", "pddp.h")).read()
    assert "int pddp_simulate_problems(pddp_handle h, int count, const int* idx," in header
    assert "A SLOT MAY BE NAMED MORE THAN ONCE" in header
    assert callable(getattr(pyddp.Solver, "simulate_problems", None))


# ---------------------------------------------------------------------------------------------------------------- CPU 2: the host-only code under the sanitizers
def test_host_only_code_as_a_stand_alone_program(tmp_path):
    """tests/native/sim_slots_host_check.cpp (its own main, -fsanitize=address,undefined): every refusal, the spacing of a given time against step_us of a configuration
    with that total_time, the record fill for duplicate and out-of-order indices on exactly-sized buffers, the family choice for every plant"""
    exe = str(tmp_path / "sim_slots_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "sim_slots_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "sim_slots_host_check: ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU 3: the yardstick
YARD_IDX = np.array([3, 0, 4, 1, 2, 3, 1])                   # out of order, slots 3 and 1 twice
YARD_T0 = np.array([0.0, 250.0, 1000.0, 4000.5, 16129.0, -77.25, 0.0])
YARD_KNOTS = np.array([2.3, 0.6, 1.7, 3.4, 5.0, 0.9, 6.2])   # elapsed time of each entry in knots of its slot's OWN spacing
YARD_SUB = np.array([40, 4, 7, 13, 5, 22, 40], np.int32)
_YARD = {}


def yardstick(plant, dtype):
    """the entries of tests 3 and 7 and what pddp_simulate gives for each on a single-problem handle created with total_time = the slot's time, given the slot's plan
    and the entry's own start state: computed once per (plant, element type), never modified"""
    key = (plant, dtype)
    if key not in _YARD:
        c = shared("small", plant, dtype)
        N, times = c["N"], c["times"]
        own = np.array([spacing_us(times[b], N) for b in YARD_IDX])
        el = YARD_KNOTS * own
        rng = np.random.default_rng(5)
        xa = (c["xa"][YARD_IDX] + rng.normal(0, 0.002, (len(YARD_IDX), DIMS[plant][1]))).astype(np_type(dtype))      # entries of one slot start from different states
        want = [None] * len(YARD_IDX)
        for t in sorted(set(times)):
            s1 = make_solver("hip", plant, dtype=dtype, batch=1, **dict(c["kw"], total_time=t))
            for i, b in enumerate(YARD_IDX):
                if times[b] == t:
                    want[i] = s1.simulate(c["plan"]["x"][b], c["plan"]["u"][b], c["plan"]["KT"][b], YARD_T0[i], el[i], int(YARD_SUB[i]), None, xa[i])
            s1.close()
        _YARD[key] = dict(el=el, xa=xa, own=own, want=(np.stack([w[0] for w in want]), np.array([w[1] for w in want]), np.array([w[2] for w in want])))
    return _YARD[key]


def knots_visited(el, substeps, spacing):
    dt = el / substeps
    tk, out = 0.0, []
    for _ in range(substeps):
        out.append(int(tk / spacing)); tk += dt
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("host_plans", PLANS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plant", PLANTS)
def test_every_entry_is_pddp_simulate_on_a_handle_of_that_horizon_time(plant, dtype, family, host_plans):
    c, y = shared("small", plant, dtype), yardstick(plant, dtype)
    default = spacing_us(c["kw"]["total_time"], c["N"])
    # a kernel that ignored the per-entry spacing would follow other knots: at least one entry visits a knot under its own spacing that the default spacing does not give
    differs = [i for i in range(len(YARD_IDX)) if knots_visited(y["el"][i], int(YARD_SUB[i]), y["own"][i]) != knots_visited(y["el"][i], int(YARD_SUB[i]), default)]
    assert differs and any(c["times"][YARD_IDX[i]] != c["kw"]["total_time"] for i in differs)
    assert (y["want"][2] == 0).all() and not np.array_equal(y["want"][0], y["xa"])
    plans = entry_plans(c, YARD_IDX) if host_plans else {}
    got = c["s"].simulate_problems(YARD_IDX, YARD_T0, y["el"], YARD_SUB, None, y["xa"], family=family, **plans)
    assert_same(got, y["want"])
    assert_same(c["s"].simulate_problems(YARD_IDX, YARD_T0, y["el"], YARD_SUB, None, y["xa"], family=0, **plans), y["want"], "the library's choice")


# ---------------------------------------------------------------------------------------------------------------- GPU 4: no table
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plant", PLANTS)
def test_without_a_table_rows_equal_the_batched_simulator(plant, dtype, family):
    c = shared("plain", plant, dtype)
    s, B, N = c["s"], c["B"], c["N"]
    step = spacing_us(c["kw"]["total_time"], N)
    rng = np.random.default_rng(41)
    t0, el = rng.uniform(0.0, 5000.0, B), rng.uniform(0.3, 6.0, B) * step
    whole = s.simulate_batch(t0, el, 7, None, c["xa"])
    assert (whole[2] == 0).all() and not np.array_equal(whole[0], c["xa"])
    for idx in (np.arange(B), np.arange(B)[::-1], rng.permutation(B)[:23], np.array([B - 1]), np.array([5, 5, 66, 0, 5])):
        assert_same(s.simulate_problems(idx, t0[idx], el[idx], 7, None, c["xa"][idx], family=family), rows(whole, idx), idx[:4])
        assert_same(s.simulate_problems(idx, t0[idx], el[idx], 7, None, c["xa"][idx], family=family, **entry_plans(c, idx)), rows(whole, idx), ("host plans", idx[:4]))


_ARM = {}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_arm_rows_with_tool_point_goals_equal_the_batched_simulator(dtype):
    if dtype not in _ARM:
        _ARM[dtype] = arm_solved(dtype)
    s, out, xg = _ARM[dtype]
    xa = (out["x"][:, 0] + np.random.default_rng(31).normal(0, 0.004, (5, 14))).astype(dtype)
    el = ARM_KNOTS * ARM_STEP_US
    whole = s.simulate_batch(ARM_T0_US, el, 40, xg[:, :3], xa)
    assert (whole[1] > 0).all() and (whole[2] == 0).all()
    for idx in (np.arange(5), np.array([4, 2, 2, 0])):
        assert_same(s.simulate_problems(idx, ARM_T0_US[idx], el[idx], 40, xg[idx, :3], xa[idx], family=1), rows(whole, idx))
        assert_same(s.simulate_problems(idx, ARM_T0_US[idx], el[idx], 40, xg[idx, :3], xa[idx], family=0), rows(whole, idx))
        assert_same(s.simulate_problems(idx, ARM_T0_US[idx], el[idx], 40, xg[idx, :3], xa[idx], family=1, x=out["x"][idx], u=out["u"][idx], KT=out["KT"][idx]), rows(whole, idx))
    with pytest.raises(pyddp.PddpError, match="pddp_simulate_problems"):                    # the arm has no thread family
        s.simulate_problems([0, 1], 0.0, 1000.0, 4, None, xa[:2], family=2)


# ---------------------------------------------------------------------------------------------------------------- GPU 5: thread family edges
@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plant", PLANTS)
def test_thread_family_equals_wave_family_at_the_edges_of_a_wavefront(plant, dtype, count):
    """batch 67 with mixed times: count 130 names slots twice; slot batch - 1 is named last; the sub-step counts differ inside one wavefront; one entry has elapsed 0"""
    c = shared("big", plant, dtype)
    s, B, N = c["s"], c["B"], c["N"]
    rng = np.random.default_rng(100 + count)
    idx = np.concatenate([rng.integers(0, B, count - 1), [B - 1]]).astype(np.int32)
    if count >= 63:
        idx[1] = idx[0]                                       # a duplicate at every count that has room for one
        assert len(set(idx.tolist())) < count
    own = np.array([spacing_us(c["times"][b], N) for b in idx])
    el = rng.uniform(0.3, 6.0, count) * own
    el[count // 2] = 0.0
    t0 = rng.uniform(-500.0, 5000.0, count)
    sub = np.array([SUBSTEPS[i % len(SUBSTEPS)] for i in range(count)], np.int32)
    xa = (c["xa"][idx] + rng.normal(0, 0.002, (count, DIMS[plant][1]))).astype(np_type(dtype))
    wave = s.simulate_problems(idx, t0, el, sub, None, xa, family=1)
    assert (wave[2] == 0).all() and np.isfinite(wave[0]).all()
    assert np.array_equal(wave[0][count // 2], xa[count // 2])                                # no time passed: the state it started from
    if count > 1:
        assert not np.array_equal(wave[0][0], xa[0])
    assert_same(s.simulate_problems(idx, t0, el, sub, None, xa, family=2), wave)
    assert_same(s.simulate_problems(idx, t0, el, sub, None, xa, family=2, **entry_plans(c, idx)), wave, "host plans")


# ---------------------------------------------------------------------------------------------------------------- GPU 6: abort alone
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plant", PLANTS)
def test_an_entry_that_leaves_its_plan_aborts_alone(plant, dtype, family):
    c = shared("small", plant, dtype)
    s, N, times = c["s"], c["N"], c["times"]
    idx = np.array([1, 3, 4, 0])                              # slot 3: the very short horizon
    el = np.full(4, 16.0 * spacing_us(times[3], N))            # the SAME elapsed time for every entry: past knot N - 2 of slot 3 only
    assert el[0] / spacing_us(times[3], N) * 39 / 40 >= N - 2 and all(el[0] / spacing_us(times[b], N) < N - 3 for b in (1, 4, 0))
    t0, sub = np.array([0.0, 100.0, 200.0, 300.0]), np.array([7, 40, 40, 13], np.int32)
    got = s.simulate_problems(idx, t0, el, sub, None, c["xa"][idx], family=family)
    assert got[2].tolist() == [0, 1, 0, 0]
    assert np.array_equal(got[0][1], c["xa"][3]) and got[1][1] == 0.0
    keep = [0, 2, 3]                                          # ... and the others are what they are without the aborting neighbour
    alone = s.simulate_problems(idx[keep], t0[keep], el[keep], sub[keep], None, c["xa"][idx[keep]], family=family)
    assert_same(rows(got, keep), alone)
    assert not np.array_equal(alone[0], c["xa"][idx[keep]])


# ---------------------------------------------------------------------------------------------------------------- GPU 7: oracle parity
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype,tol", [pytest.param(1, 1e-10, id="f64"), pytest.param(0, 2e-5, id="f32")])
@pytest.mark.parametrize("plant", PLANTS)
def test_oracle_parity_per_entry(plant, dtype, tol, family):
    c, y = shared("small", plant, dtype), yardstick(plant, dtype)
    got = c["s"].simulate_problems(YARD_IDX, YARD_T0, y["el"], YARD_SUB, None, y["xa"], family=family)
    for i, b in enumerate(YARD_IDX):
        o = Oracle(default_cfg(plant, cores=1, spawn_threads=0, **dict(c["kw"], total_time=c["times"][b])), np_type(dtype))
        ro = o.simulate(c["plan"]["x"][b].ravel(), c["plan"]["u"][b].ravel(), c["plan"]["KT"][b].ravel(), YARD_T0[i], y["el"][i], int(YARD_SUB[i]), None, y["xa"][i])
        print(f"entry {i} slot {b}: state diff {np.abs(got[0][i] - ro[0]).max():.3e} of |x| {np.abs(ro[0]).max():.3e}")
        assert ro[2] == 0 and got[2][i] == 0
        np.testing.assert_allclose(got[0][i], ro[0], rtol=0, atol=tol * max(1.0, np.abs(ro[0]).max()))
        assert abs(got[1][i] - ro[1]) <= max(tol, 2e-7) * max(1.0, abs(ro[1]))


# ---------------------------------------------------------------------------------------------------------------- GPU 8: read-only
def everything(s):
    """every named array, the state records and the cost, goal and step tables"""
    B = s.cfg.batch
    snap = {k: s.get(k).copy() for k in ARRAYS}
    snap.update(state_rows(s, range(B)))
    snap.update({"table_" + k: v for k, v in tables(s).items()})
    return snap


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plant", PLANTS)
def test_the_call_only_reads(plant, dtype):
    after_sweep = []
    for disturb in (True, False):
        c = solved_handle(plant, dtype, kw_small(plant), 5, True)
        s, N = c["s"], c["N"]
        if disturb:
            idx = np.array([4, 1, 1, 3, 0])
            el = np.array([spacing_us(c["times"][b], N) for b in idx]) * np.array([1.5, 0.7, 20.0, 2.0, 3.1])      # (the third entry aborts)
            before = everything(s)
            for family in (1, 2):
                for plans in ({}, entry_plans(c, idx)):
                    r = s.simulate_problems(idx, 0.0, el, SUBSTEPS[:5], None, c["xa"][idx], family=family, **plans)
                    assert r[2].tolist() == [0, 0, 1, 0, 0]
            after = everything(s)
            for k in before:
                assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), ("the call changed", k)
        s.iterate(1); s.sync()
        after_sweep.append(everything(s))
        s.close()
    for k in after_sweep[0]:
        assert np.array_equal(np.asarray(after_sweep[0][k]), np.asarray(after_sweep[1][k]), equal_nan=True), ("the following sweep differs in", k)


# ---------------------------------------------------------------------------------------------------------------- GPU 9: closed loop
@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plant", PLANTS)
def test_closed_loop_of_named_slots_equals_single_problem_handles(plant, dtype, family):
    """three cycles on batch 5 with mixed times: the named slots' robots advance one knot of their OWN step on the plan their slot holds, then a control cycle with
    shift 1 starts from the simulated states -- against single-problem handles of those total_time driven with pddp_simulate + pddp_mpc_solve, bit for bit"""
    B, N, sel = 5, 16, dict(cf="coop")
    kw = dict(kw_small(plant), tol_cost=0.0, max_iter=4)
    n = DIMS[plant][1]
    probs, times = problems(plant, N, dtype, B), mixed_times(N, B)
    xg = stack(probs, "xg").reshape(B, n)
    named, others = [3, 0, 4], [1, 2]
    sub = np.array([40, 13, 22], np.int32)
    s = make_solver("hip", plant, dtype=dtype, batch=B, kernels=sel, **kw)
    set_times(s, [times[b] for b in (1, 2, 3, 4)], (1, 2, 3, 4))
    seed = s.solve(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"))
    before, tab_before = snapshot(s), tables(s)
    rng = np.random.default_rng(9)
    xa0 = (seed["x"][named, 0] + rng.normal(0, 0.002, (3, n))).astype(np_type(dtype))
    el = np.array([spacing_us(times[b], N) for b in named])
    xa, sims, cycles = xa0, [], []
    for cyc in range(3):
        sim = s.simulate_problems(named, 0.0, el, sub, None, xa, family=family)
        assert (sim[2] == 0).all()
        xa = sim[0]
        sims.append(sim)
        cycles.append(s.mpc_solve_problems(named, xa, xg[named], 1, clear_vars=0, max_iter=4))
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k])[others], np.asarray(after[k])[others], equal_nan=True), ("an unnamed slot changed", k)
    tab_after = tables(s)
    for k in tab_before:
        assert np.array_equal(tab_before[k], tab_after[k], equal_nan=True), ("a table changed", k)
    s.close()
    for j, b in enumerate(named):
        s1 = make_solver("hip", plant, dtype=dtype, batch=1, kernels=sel, **dict(kw, total_time=times[b]))
        one = s1.solve(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
        for k in OUT_KEYS:
            assert np.array_equal(np.asarray(one[k][0]), np.asarray(seed[k][b]), equal_nan=True), ("seed solve", b, k)
        xa1 = xa0[j]
        for cyc in range(3):
            r1 = s1.simulate(one["x"][0], one["u"][0], one["KT"][0], 0.0, el[j], int(sub[j]), None, xa1)
            assert_same(rows(sims[cyc], j), r1, ("cycle", cyc, "slot", b))
            xa1 = r1[0]
            one = s1.mpc_solve(xa1[None], xg[[b]], 1, clear_vars=0, max_iter=4)
            for k in MPC_KEYS:
                assert np.array_equal(np.asarray(one[k][0]), np.asarray(cycles[cyc][k][j]), equal_nan=True), ("cycle", cyc, "slot", b, k)
        s1.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 10: refusals through the ABI
@pytest.mark.gpu
def test_refusals_name_the_call_and_leave_the_handle_usable():
    plant, dtype = 2, 0
    c, y = shared("small", plant, dtype), yardstick(plant, dtype)
    s, B = c["s"], c["B"]
    lib = s.lib
    lib.pddp_simulate_problems.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 11 + [C.c_int]
    lib.pddp_last_error.restype = C.c_char_p
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    before = everything(s)
    good = dict(count=3, idx=np.array([3, 0, 3], np.int32), x=None, u=None, KT=None, t0=np.zeros(3), el=np.full(3, 1000.0), sub=np.array([4, 7, 40], np.int32),
                goal=None, xa=c["xa"][[3, 0, 3]].copy(), family=0)

    def call(handle=s, **change):
        a = dict(good, **change)
        err, failed = np.zeros(8), np.zeros(8, np.int32)
        return handle.lib.pddp_simulate_problems(handle.h, a["count"], ptr(a["idx"]), ptr(a["x"]), ptr(a["u"]), ptr(a["KT"]), ptr(a["t0"]), ptr(a["el"]), ptr(a["sub"]),
                                                 ptr(a["goal"]), ptr(a["xa"]), ptr(err), ptr(failed), a["family"])

    assert call() == 0
    hp = entry_plans(c, good["idx"])
    bad = [("count 0", dict(count=0)), ("count -1", dict(count=-1)), ("null idx", dict(idx=None)), ("null t0", dict(t0=None)), ("null elapsed", dict(el=None)),
           ("null substeps", dict(sub=None)), ("null xActual", dict(xa=None)), ("index == batch", dict(idx=np.array([3, B, 0], np.int32))),
           ("negative index", dict(idx=np.array([-1, 0, 3], np.int32))), ("substeps 0", dict(sub=np.array([4, 0, 40], np.int32))),
           ("elapsed < 0", dict(el=np.array([1000.0, 1000.0, -1.0]))), ("elapsed NaN", dict(el=np.array([np.nan, 1000.0, 1000.0]))),
           ("t0 infinite", dict(t0=np.array([0.0, np.inf, 0.0]))), ("t0 NaN", dict(t0=np.array([0.0, 0.0, np.nan]))), ("family 3", dict(family=3)), ("family -1", dict(family=-1)),
           ("x alone", dict(x=hp["x"])), ("u missing", dict(x=hp["x"], KT=hp["KT"])), ("x missing", dict(u=hp["u"], KT=hp["KT"]))]
    for what, change in bad:
        assert call(**change) == EINVAL, what
        assert b"pddp_simulate_problems" in lib.pddp_last_error(), (what, lib.pddp_last_error())
    assert call(x=hp["x"], u=hp["u"], KT=hp["KT"]) == 0 and call(family=2) == 0 and call(family=1) == 0
    # NULL plans on a handle that was never loaded; host plans are fine there
    fresh = make_solver("hip", plant, dtype=dtype, batch=B, **c["kw"])
    assert call(fresh) == EINVAL and b"pddp_simulate_problems" in lib.pddp_last_error() and b"loaded" in lib.pddp_last_error()
    assert call(fresh, x=hp["x"], u=hp["u"], KT=hp["KT"]) == 0
    fresh.close()
    # the thread family on the arm
    arm = make_solver("hip", 4, dtype=0, batch=2, N=32, M=4, A=8, wafr_urdf=1, total_time=0.5)
    plans = dict(x=np.zeros((3, 32, 14), np.float32), u=np.zeros((3, 32, 7), np.float32), KT=np.zeros((3, 32, 7, 14), np.float32))
    arm_args = dict(idx=np.array([1, 0, 1], np.int32), xa=np.zeros((3, 14), np.float32), **plans)
    assert call(arm, family=2, **arm_args) == EINVAL and b"pddp_simulate_problems" in lib.pddp_last_error()
    assert call(arm, family=1, **arm_args) == 0
    arm.close()
    # pddp_simulate_batch still refuses a handle with a step table
    with pytest.raises(pyddp.PddpError, match="horizon time"):
        s.simulate_batch(0.0, 1000.0, substeps=4, xActual=c["xa"])
    after = everything(s)
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), ("a refused call changed", k)
    assert_same(s.simulate_problems(YARD_IDX, YARD_T0, y["el"], YARD_SUB, None, y["xa"]), y["want"])
