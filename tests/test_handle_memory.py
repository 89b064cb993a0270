"""The blocks of device and pinned memory a handle grows while it is used (csrc/device_mem.hpp, solver_impl.hpp reserve): a block that was too small is replaced, and
what the call then returns is what a handle that started with the large block returns, bit for bit.  The buffer type itself is held on the CPU (test_device_mem.py);
here the handle's own sites run on the GPU, each at the smallest shape where its block regrows: the staging of pddp_store_problems, the helpers' scratch past its
4096-byte floor, the plan buffers of pddp_simulate_batch, and the rows of the two cost tables travelling by runs of consecutive slots.

Pendulum, float64, N = 8, M = 2, A = 4, six problems, loaded and iterated three sweeps; the arm's table on plant 4, float32, N = 16."""
import numpy as np
import pytest

from backends import make_solver
from oracle_binding import example_inputs

pytestmark = pytest.mark.gpu

B = 6
PEND_BUILTIN = np.array([1.0, 0.1, 0.1, 1000.0, 1000.0])          # cost_pend.cuh:19-24 as [q | r | qf]
OUT_KEYS = ("x", "u", "KT", "Jout", "alphaOut", "dmax")


def loaded(plant, dtype, N, sweeps=3, **kw):
    T = np.float32 if dtype == 0 else np.float64
    s = make_solver("hip", plant, dtype=dtype, batch=B, N=N, M=2, A=4, total_time=N / 32.0, max_iter=8, **kw)
    probs = [example_inputs(plant, N, np.float64, noise=np.random.default_rng(40 + b).normal(0, 0.002, (N, s.n))) for b in range(B)]
    x0, u0, xg = (np.concatenate([np.ravel(p[k]) for p in probs]).astype(T) for k in range(3))
    s.load(x0, u0, xg)
    s.iterate(sweeps)
    s.sync()
    return s


def pendulum(**kw):
    return loaded(1, 1, 8, **kw)


def test_store_problems_regrows_its_staging():
    s = pendulum()
    whole = s.store()
    for idx, only in (([4, 1], ("dmax",)), ([4, 1, 5], None), ([0], ("u",))):      # one output's rows, then all six for more slots, then a smaller request again
        got = s.store_problems(idx, only=only)
        assert set(got) == set(only or OUT_KEYS)
        for k in got:
            assert np.array_equal(got[k], whole[k][idx]), (idx, k)
    s.close()


def test_scratch_regrows_past_its_floor():
    rng = np.random.default_rng(7)
    x, u = rng.normal(0, 1, (600, 2)), rng.normal(0, 1, (600, 1))                  # 600 states of two doubles: 9600 bytes, the floor is 4096
    a, b = pendulum(), pendulum()
    one = a.plant_eval(0, x[:1], u[:1])
    many_a = a.plant_eval(0, x, u)
    many_b = b.plant_eval(0, x, u)
    assert many_a.shape == (600, 1) and np.isfinite(many_a).all() and np.ptp(many_a) > 0
    assert np.array_equal(many_a, many_b)
    assert np.array_equal(many_a[0], one[0])
    a.close(); b.close()


def test_simulate_batch_plan_buffers():
    a, b = pendulum(), pendulum()
    N, n, m = 8, a.n, a.m
    rng = np.random.default_rng(11)
    xa = rng.normal(0, 0.1, (B, n))
    t0, el = np.linspace(0.0, 2000.0, B), np.linspace(500.0, 3000.0, B)
    a.simulate_batch(t0, el, substeps=10, xActual=xa)                              # the held solution: no plan buffer yet
    plans = dict(x=rng.normal(0, 0.5, (B, N, n)), u=rng.normal(0, 0.5, (B, N, m)), KT=rng.normal(0, 0.1, (B, N, m, n)))
    got_a = a.simulate_batch(t0, el, substeps=10, xActual=xa, **plans)
    got_b = b.simulate_batch(t0, el, substeps=10, xActual=xa, **plans)
    for va, vb in zip(got_a, got_b):
        assert np.array_equal(va, vb)
    assert np.isfinite(got_a[0]).all() and not np.array_equal(got_a[0], xa)
    a.close(); b.close()


SET_IDX, GET_IDX = [5, 0, 1, 2, 4], [2, 4, 5, 0, 3]


def rows_by_runs(s, setter, getter, records, untouched, T):
    """records[i] set for slot SET_IDX[i]; the getter names four of those slots and slot 3, which keeps `untouched`; every number rounded to the element type once"""
    setter(SET_IDX, records)
    got = getter(GET_IDX)
    by_slot = {q: records[i] for i, q in enumerate(SET_IDX)}
    by_slot[3] = untouched
    want = np.array([by_slot[q] for q in GET_IDX]).astype(T).astype(np.float64)
    assert got.shape == want.shape and np.array_equal(got, want), (got, want)


def test_diagonal_records_travel_by_runs():
    s = pendulum()
    records = PEND_BUILTIN * np.random.default_rng(3).uniform(0.3, 3.0, (5, 5))
    assert len(np.unique(records, axis=0)) == 5
    rows_by_runs(s, s.set_diag_cost_problems, s.get_diag_cost_problems, records, PEND_BUILTIN, np.float64)
    s.close()


def test_arm_records_travel_by_runs():
    s = loaded(4, 0, 16)
    c = s.cfg
    wide = np.array([c.Q1, c.Q2, c.R, c.QF1, c.QF2])
    records = wide * np.random.default_rng(4).uniform(0.3, 3.0, (5, 5))             # (not float32 numbers: the rounding is part of what is held)
    assert len(np.unique(records, axis=0)) == 5 and not np.array_equal(records.astype(np.float32).astype(np.float64), records)
    rows_by_runs(s, s.set_cost_problems, s.get_cost_problems, records, wide, np.float32)
    s.close()
