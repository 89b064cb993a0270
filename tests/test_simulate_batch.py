"""pddp_simulate_batch: the simulated robot of the lock-step experiment (tests/test_lockstep_sim.py) for every problem of a handle
in one launch.  Per problem it IS pddp_simulate -- the same double-precision body, one wavefront per problem -- so the batched call is held bit for bit against
serial pddp_simulate calls on the same handle, and through them against the oracle with the tolerances test_lockstep_sim.py uses for that body.  With no plan
arguments every problem follows the solution the handle holds on the device: what pddp_store / pddp_mpc_solve hand out, the fall-back of a cycle that took no
step included."""
import ctypes
import os

import numpy as np
import pytest

import pyddp
from backends import make_solver
from oracle_binding import Oracle, default_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(N=32, M=4, A=8, wafr_urdf=1, mpc_mode=1, tol_cost=1e-5, total_time=0.5, max_iter=10, ee_cost=1, ignore_max_rho_exit=0)   # tests/test_lockstep_sim.py
B = 5
STEP_US = KW["total_time"] / (KW["N"] - 1) * 1e6
T0_US = np.array([0.0, 250.0, 1000.0, 4000.5, 16129.0])
KNOTS = np.array([0.6, 1.7, 2.3, 3.4, 5.0])                  # elapsed time of each problem in knots
SIGMA = np.array([0.002, 0.004, 0.006, 0.008, 0.01])         # start states: the plan's first knot + N(0, sigma)
GOAL_STEP = np.array([[0.0, 0.0, 0.0], [0.03, -0.02, 0.01], [-0.03, 0.02, 0.02], [0.02, 0.03, -0.02], [-0.02, -0.03, -0.01]])


def goals(dtype, moved=0.0):
    xg = np.zeros((B, 14), dtype)
    xg[:, :3] = np.array([0.45, 0.15, 0.75]) + GOAL_STEP + moved
    return xg


def solved(dtype):
    """a handle of five problems after ONE batched solve towards five different tool-point goals"""
    N = KW["N"]
    s = make_solver("hip", 4, dtype=0 if dtype == np.float32 else 1, batch=B, **KW)
    x0 = np.zeros((B, N, 14), dtype); x0[:, :, 1] = 0.7; x0[:, :, 3] = -0.8; x0[:, :, 5] = 0.75
    u0 = np.full((B, N, 7), 0.01, dtype)
    xg = goals(dtype)
    return s, s.solve(x0, u0, xg), xg


_CASES = {}


def case(dtype):
    """the inputs of tests 2, 3 and 7 and the five serial pddp_simulate results they are held against: computed once per element type, never modified"""
    key = np.dtype(dtype).name
    if key not in _CASES:
        s, out, xg = solved(dtype)
        rng = np.random.default_rng(31)
        xa = np.stack([out["x"][b][0] + rng.normal(0, SIGMA[b], 14) for b in range(B)]).astype(dtype)
        c = dict(s=s, out=out, xg=xg, xa=xa, serial={})
        for name, knots, substeps in (("plain40", KNOTS, 40), ("plain150", KNOTS, 150), ("abort40", np.where(np.arange(B) == 2, 31.5, KNOTS), 40)):
            r = [s.simulate(out["x"][b], out["u"][b], out["KT"][b], T0_US[b], knots[b] * STEP_US, substeps, xg[b, :3], xa[b]) for b in range(B)]
            c["serial"][name] = (knots, substeps, np.stack([v[0] for v in r]), np.array([v[1] for v in r]), np.array([v[2] for v in r]))
        _CASES[key] = c
    return _CASES[key]


def batched(c, name, **plans):
    knots, substeps = c["serial"][name][:2]
    return c["s"].simulate_batch(T0_US, knots * STEP_US, substeps, c["xg"][:, :3], c["xa"], **plans)


def host_plans(out):
    return dict(x=out["x"], u=out["u"], KT=out["KT"])


def assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert (np.asarray(got[1]) == np.asarray(want[1])).all() and (np.asarray(got[2]) == np.asarray(want[2])).all()


# ---- 1
def test_symbol_header_and_binding_exist():
    assert hasattr(ctypes.CDLL(pyddp.library_path()), "pddp_simulate_batch")
    assert "int pddp_simulate_batch(pddp_handle h," in open(os.path.join(ROOT, "include", "pddp.h")).read()
    assert callable(getattr(pyddp.Solver, "simulate_batch", None))


# ---- 2
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["plain40", "plain150"])
def test_batched_call_is_bit_identical_to_the_single_problem_call(dtype, name):
    c = case(dtype)
    want = c["serial"][name][2:]
    assert (want[2] == 0).all() and (want[1] > 0).all()
    assert_same(batched(c, name, **host_plans(c["out"])), want)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_problem_that_leaves_its_plan_aborts_alone(dtype):
    c = case(dtype)
    got = batched(c, "abort40", **host_plans(c["out"]))
    assert list(got[2]) == [0, 0, 1, 0, 0]
    assert np.array_equal(got[0][2], c["xa"][2]) and got[1][2] == 0.0
    assert_same(got, c["serial"]["abort40"][2:])
    keep = [0, 1, 3, 4]                                       # ... and the other four are what they are without the aborting neighbour
    assert_same([v[keep] for v in got], [v[keep] for v in c["serial"]["plain40"][2:]])


# ---- 3
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tol,name", [(np.float64, 1e-10, "plain150"), (np.float32, 2e-5, "plain40"), (np.float64, 1e-10, "plain40")])
def test_oracle_parity_per_problem(dtype, tol, name):
    c = case(dtype)
    out, xg = c["out"], c["xg"]
    knots, substeps = c["serial"][name][:2]
    got = batched(c, name, **host_plans(out))
    o = Oracle(default_cfg(4, cores=8, spawn_threads=0, **KW), dtype)
    for b in range(B):
        ro = o.simulate(out["x"][b].ravel(), out["u"][b].ravel(), out["KT"][b].ravel(), T0_US[b], knots[b] * STEP_US, substeps, xg[b, :3], c["xa"][b])
        print(f"problem {b}: state diff {np.abs(got[0][b] - ro[0]).max():.3e}  error {got[1][b]:.9e} oracle {ro[1]:.9e}")
        assert ro[2] == 0 and got[2][b] == 0
        np.testing.assert_allclose(got[0][b], ro[0], rtol=0, atol=tol * max(1.0, np.abs(ro[0]).max()))
        assert abs(got[1][b] - ro[1]) <= max(tol, 2e-7) * max(1.0, abs(ro[1]))
        assert ro[1] > 0


# ---- 4
def mpc_cycles(s, dtype, xa, cycles=3):
    """three control cycles on a solved handle: simulate one knot on the device-resident plan, then warm-start from the simulated states towards goals moved a little.
    Yields (cycle, mpc_solve's result, the simulated states).  These inputs were run through the hostsim backend's mpc_solve on the CPU first (its pddp_simulate per
    problem in place of the batched call): success over the three cycles is 10101 / 01100 / 10101 in float32 and 10101 / 11100 / 00101 in float64 -- several problems
    of every cycle accept and several fall back, as DESIGN.md section 7 row N2 describes for ee_cost = 1 without ee_initial_cost_fix."""
    for cyc in range(cycles):
        xa = s.simulate_batch(0.0, STEP_US, 40, None, xa)[0]
        yield cyc, s.mpc_solve(xa, goals(dtype, moved=0.01 * (cyc + 1)), 1, max_iter=4), xa


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_resident_plan_is_the_solution_the_handle_holds(dtype):
    s, out, xg = solved(dtype)
    rng = np.random.default_rng(32)
    xa = (out["x"][:, 0] + rng.normal(0, 0.004, (B, 14))).astype(dtype)
    args = (T0_US, KNOTS * STEP_US, 40, xg[:, :3], xa)
    assert_same(s.simulate_batch(*args), s.simulate_batch(*args, **host_plans(out)))
    success = []
    for cyc, r, xa_c in mpc_cycles(s, dtype, xa):
        args = (T0_US, KNOTS * STEP_US, 40, goals(dtype, 0.01 * (cyc + 1))[:, :3], xa_c)
        got = s.simulate_batch(*args)
        assert (got[2] == 0).all()
        assert_same(got, s.simulate_batch(*args, **host_plans(r)))
        success += list(r["success"])
    print("success of the 3 x 5 cycles:", success)
    assert 0 in success and 1 in success                      # accepted solutions AND the fall-back branch of k_mpc_store


# ---- 5
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_solver_is_not_disturbed(dtype):
    res = []
    for disturb in (True, False):
        s, out, xg = solved(dtype)
        xa = (out["x"][:, 1] + np.random.default_rng(33).normal(0, 0.004, (B, 14))).astype(dtype)
        if disturb:
            s.simulate_batch(T0_US, KNOTS * STEP_US, 40, xg[:, :3], xa)
        res.append(s.mpc_solve(xa, goals(dtype, 0.01), 1, max_iter=4))
        s.close()
    for k in ("x", "u", "KT", "Jout", "alphaOut", "success", "iters"):
        assert np.array_equal(res[0][k], res[1][k]), k


# ---- 6
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_another_plant_without_a_goal(dtype):
    N, Bq = 16, 3
    s = make_solver("hip", 3, dtype=0 if dtype == np.float32 else 1, batch=Bq, N=N, M=2, A=4)
    rng = np.random.default_rng(34)
    x = np.zeros((Bq, N, 12)); x[:, :, 2] = 0.5; x += rng.normal(0, 0.05, x.shape)
    u = 1.22625 + rng.normal(0, 0.05, (Bq, N, 4))
    KT = rng.normal(0, 0.05, (Bq, N, 4, 12))
    x, u, KT = x.astype(dtype), u.astype(dtype), KT.astype(dtype)
    xa = (x[:, 0] + rng.normal(0, 0.01, (Bq, 12))).astype(dtype)
    step_us = s.cfg.total_time / (N - 1) * 1e6
    t0, el = np.array([0.0, 500.0, 12345.0]), np.array([0.7, 2.2, 4.9]) * step_us
    got = s.simulate_batch(t0, el, 40, None, xa, x=x, u=u, KT=KT)
    want = [s.simulate(x[b], u[b], KT[b], t0[b], el[b], 40, None, xa[b]) for b in range(Bq)]
    assert np.isfinite(got[0]).all() and not np.array_equal(got[0], xa)
    assert_same(got, (np.stack([v[0] for v in want]), [v[1] for v in want], [v[2] for v in want]))
    assert (got[1] == 0).all() and (got[2] == 0).all()


# ---- 7
@pytest.mark.gpu
def test_argument_errors_leave_the_handle_usable():
    c = case(np.float32)
    s, out, xg, xa = c["s"], c["out"], c["xg"], c["xa"]
    el = KNOTS * STEP_US
    with pytest.raises(pyddp.PddpError, match="pddp_simulate_batch"):
        s.simulate_batch(T0_US, el, 40, xg[:, :3], xa, x=out["x"], u=None, KT=out["KT"])
    with pytest.raises(pyddp.PddpError, match="pddp_simulate_batch"):
        s.simulate_batch(T0_US, el, 0, xg[:, :3], xa, **host_plans(out))
    with pytest.raises(pyddp.PddpError, match="pddp_simulate_batch"):
        s.simulate_batch(T0_US, np.where(np.arange(B) == 3, -1.0, el), 40, xg[:, :3], xa, **host_plans(out))
    assert_same(batched(c, "plain40", **host_plans(out)), c["serial"]["plain40"][2:])
