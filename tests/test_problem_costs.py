"""Per-problem cost weights inside one batch of arm problems: pddp_set_cost_problems / pddp_get_cost_problems / pddp_cost_record_size.

The yardstick of every GPU check is the one tests/test_refill.py uses, never the per-problem path: a SINGLE-PROBLEM handle pinned to the same kernel families, created
with the problem's weights in its pddp_config (the handle-wide record, a kernel argument) and solved sweep by sweep (solve_fresh).  Shapes, pools and pins are those of
tests/test_mixed_states.py (imported, not changed).  All comparisons with the yardstick are bit for bit: the pddp_store outputs, every field of pddp_state, P Pp p pp,
and the arrays H and g right after the load.

Records come from a seeded generator as multiples of the defaults in [0.2, 5] (the end-effector weights whose default is 0 get a small base of their own): any two
problems of a batch differ in every field, within a record no two fields are equal -- a swapped field or a neighbour's row shows -- and slot KEEP of every batch is
never named: it keeps the handle-wide record.

What the bit-for-bit comparison rests on: the batch with a table runs the table instantiations of the kernels (k_fp_tl / k_nis_tl / k_nis `PC`, k_bp_mfma_pc), the
yardstick the ones without -- different machine code over the same source expressions.  The thread-lane headers allow fused multiply-adds, so equality needs the compiler
to contract the same expressions on both sides; every path has a case here (staged and unstaged rollouts, both cost families, both element types).  It has failed once:
with a first form of cost_weights_at (a copy of the record with the row stored over it, looked up inside the rollout step) slot KEEP of the A = 4 case (unstaged
k_fp_tl) differed from its yardstick in the last place of one Jout entry, 1965.1287 against 1965.1288, all of x, u, KT being equal; the field-by-field form, with the
lookup outside the step, has not shown it.

CPU: the surface, the host-only code as a stand-alone program, the slot scheduler against a recording fake solver.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pyddp
from backends import make_solver
from oracle_binding import Oracle, default_cfg
from test_mixed_states import ARM_EE, ARM_FEW, ARM_KW, ARM_TL, EE_KW, pool_of, stack
from test_refill import (ARM_F64, STATE_ALL, UNTOUCHED, FakeSolver, assert_slots_equal_fresh, mixed_batch, pick_mixed_slots, problems_of, run_until_done,
                         snapshot, solve_fresh)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOINT = ("Q1", "Q2", "R", "QF1", "QF2")
EE = ("Q_EE1", "Q_EE2", "QF_EE1", "QF_EE2", "R_EE", "Q_xEE", "QF_xEE", "Q_xdEE", "QF_xdEE")
JOINT_DEFAULT = np.array([0.1, 0.001, 0.0001, 1000.0, 1000.0])
EE_DEFAULT = np.array([0.1, 0.0, 1000.0, 0.0, 0.0001, 0.0, 0.0, 0.1, 1000.0])
EE_BASE = np.array([0.1, 0.013, 1000.0, 170.0, 0.0001, 0.0021, 23.0, 0.07, 810.0])      # what the multiples are taken of (a base of their own where the default is 0)
KEEP = 1                                                                                  # the slot of every batch that is never named


def records(B, ee, seed):
    """[B][5 | 9] records; row KEEP is the handle-wide default.  End-effector batches: row 0 has Q_EE2 = QF_EE2 = 0 (roll / pitch / yaw unweighted) beside rows that weight them,
    so tl_ee_rpy_weighted differs between lanes of one wave."""
    rng = np.random.default_rng(seed)
    base, default = (EE_BASE, EE_DEFAULT) if ee else (JOINT_DEFAULT * np.array([1.0, 1.0, 1.0, 1.0, 0.83]), JOINT_DEFAULT)
    for _ in range(100):
        w = base * np.exp(rng.uniform(np.log(0.2), np.log(5.0), (B, base.size)))
        w[KEEP] = default
        if ee:
            w[0, 1] = w[0, 3] = 0.0
        cols_differ = all(len(set(np.float32(w[:, c]))) == B for c in range(base.size) if not (ee and c in (1, 3)))
        named = [b for b in range(B) if b != KEEP and not (ee and b == 0)]
        rows_differ = all(len(set(np.float32(w[b]))) == base.size for b in named)
        if cols_differ and rows_differ:
            return w
    raise AssertionError("no record set with all fields distinct")


def handle(case, batch, use_graph=1, weights=None, sel=None):
    kw = dict(case["kw"])
    if weights is not None:
        kw.update(dict(zip(EE if kw.get("ee_cost") else JOINT, (float(v) for v in weights))))
    return make_solver("hip", case["plant"], dtype=case["dtype"], batch=batch, use_graph=use_graph, kernels=dict(case["single_sel"] if sel is None else sel), **kw)


def assert_kernels(s, case):
    have = [n for n, _ in s.time_kernels(1)]
    assert all(any(h.startswith(n) for h in have) for n in case["names"]), (case["names"], have)


_YARD = {}


def yardstick(case, prob_key, prob, rec):
    """the single-problem solve of `prob` on a handle whose CONFIGURATION carries `rec`: computed once per (case, problem, record), shared and left unchanged"""
    key = (case["key"], case["dtype"], prob_key, tuple(np.asarray(rec, np.float64)))
    if key not in _YARD:
        s1 = handle(case, 1, weights=rec)
        assert_kernels(s1, case)
        s1.load(prob["x0"], prob["u0"], prob["xg"], clear_vars=1)
        H0, g0 = s1.get("H").copy(), s1.get("g").copy()
        res = solve_fresh(s1, prob)
        res["H0"], res["g0"] = H0, g0
        s1.close()
        _YARD[key] = res
    return _YARD[key]


def reset_like_fresh(s):
    """what solve_fresh does for its single-problem handle, for every slot: the cost-to-go roles and the observables' rows of a fresh handle"""
    B, mi = s.cfg.batch, s.cfg.max_iter
    st = s.get_state()
    for b in range(B):
        st[b].pw = 0
    s.set_state(st)
    s.set("Jout", np.zeros(B * (mi + 2))); s.set("alphaOut", np.zeros(B * (mi + 2), np.int32))


def load_and_compare(s, case, probs, recs, tag, label):
    B = s.cfg.batch
    refs = [yardstick(case, (tag, b), probs[b], recs[b]) for b in range(B)]
    reset_like_fresh(s)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    H, g = s.get("H").reshape(B, -1), s.get("g").reshape(B, -1)
    for b in range(B):
        assert np.array_equal(H[b], refs[b]["H0"].ravel(), equal_nan=True), (label, "H after the load, slot", b)
        assert np.array_equal(g[b], refs[b]["g0"].ravel(), equal_nan=True), (label, "g after the load, slot", b)
    run_until_done(s)
    assert_slots_equal_fresh(s, list(range(B)), refs, label)
    return refs


# ---------------------------------------------------------------------------------------------------------------- CPU 1: the surface
def test_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(pyddp.library_path())
    header = open(os.path.join(ROOT, "include", "pddp.h")).read()
    for sym in ("pddp_cost_record_size", "pddp_set_cost_problems", "pddp_get_cost_problems"):
        assert getattr(lib, sym) is not None
    assert "int pddp_cost_record_size(pddp_handle h);" in header
    assert "int pddp_set_cost_problems(pddp_handle h, int count, const int* idx, const double* w" in header
    assert "int pddp_get_cost_problems(pddp_handle h, int count, const int* idx, double* w" in header
    for name in ("cost_record_size", "set_cost_problems", "get_cost_problems"):
        assert callable(getattr(pyddp.Solver, name))


# ---------------------------------------------------------------------------------------------------------------- CPU 2: the host-only code
def test_host_only_code_as_a_stand_alone_program(tmp_path):
    """tests/native/cost_table_host_check.cpp: cost_weights_at with and without a table (both families, both element types), validation, packing"""
    exe = str(tmp_path / "cost_table_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"), os.path.join(ROOT, "tests", "native", "cost_table_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "cost_table_host_check: ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------- CPU 3: the scheduler
class RecordingSolver(FakeSolver):
    """FakeSolver + the two cost methods; every call in order in `calls`"""
    WIDE = np.array([9.0, 8.0, 7.0, 6.0, 5.0])

    def __init__(self, batch, exit_sweeps):
        super().__init__(batch, exit_sweeps)
        self.calls, self.rows = [], [self.WIDE.copy() for _ in range(batch)]

    def get_cost_problems(self, idx):
        self.calls.append(("get", list(idx)))
        return np.array([self.rows[i] for i in idx])

    def set_cost_problems(self, idx, w):
        w = np.asarray(w, np.float64).reshape(len(idx), -1)
        self.calls.append(("set", [int(i) for i in idx], w.copy()))
        for i, r in zip(idx, w):
            self.rows[int(i)] = r.copy()

    def load(self, x0, u0, xg, clear_vars=1, ignore_first_defect=1):
        self.calls.append(("load", list(range(self.B))))
        super().load(x0, u0, xg, clear_vars, ignore_first_defect)
        self.cost_at_load = {int(x0[s]): self.rows[s].copy() for s in range(self.B)}

    def load_problems(self, idx, x0, u0, xg, ignore_first_defect=1):
        self.calls.append(("load_problems", [int(i) for i in idx]))
        super().load_problems(idx, x0, u0, xg, ignore_first_defect)
        for slot, tag in zip(idx, x0):
            self.cost_at_load[int(tag)] = self.rows[int(slot)].copy()


def test_scheduler_writes_cost_records_immediately_before_the_matching_load():
    rec = lambda p: np.array([p + 0.1, p + 0.2, p + 0.3, p + 0.4, p + 0.5])
    has_rec = lambda p: p % 3 != 2                                                      # problems 2, 5, 8, ... are plain 3-tuples
    count, batch = 11, 3
    fake = RecordingSolver(batch, [2 + (5 * p) % 7 for p in range(count)])
    tag = lambda p: np.array([p])
    problems = ((tag(p), tag(p), tag(p), rec(p)) if has_rec(p) else (tag(p), tag(p), tag(p)) for p in range(count))
    got = list(pyddp.SlotScheduler(fake, problems, batch, sweeps_per_poll=2).run())
    assert sorted(i for i, _ in got) == list(range(count))
    assert sum(1 for c in fake.calls if c[0] == "get") == 1 and fake.calls[0][0] == "get"      # the handle-wide record is read once, before the first write
    loads = [i for i, c in enumerate(fake.calls) if c[0] in ("load", "load_problems")]
    assert len(loads) >= 3
    for i in loads:                                                                     # every load has its set directly in front of it, with the same slots
        assert fake.calls[i - 1][0] == "set" and fake.calls[i - 1][1] == fake.calls[i][1], (fake.calls[i - 1][:2], fake.calls[i])
    assert sum(1 for c in fake.calls if c[0] == "set") == len(loads)
    for p in range(count):                                                              # what was in force when each problem was loaded: its record, or the handle-wide one
        assert np.array_equal(fake.cost_at_load[p], rec(p) if has_rec(p) else RecordingSolver.WIDE), p


def test_scheduler_of_plain_problems_never_touches_the_cost_methods():
    fake = FakeSolver(3, [3, 1, 4, 1, 5, 9, 2])                                         # (has neither set_cost_problems nor get_cost_problems)
    problems = ((np.array([p]), np.array([p]), np.array([p])) for p in range(7))
    got = list(pyddp.SlotScheduler(fake, problems, 3, sweeps_per_poll=2).run())
    assert sorted(i for i, _ in got) == list(range(7))


def test_scheduler_with_a_late_first_record_reads_the_handle_wide_record_then():
    fake = RecordingSolver(2, [1] * 6)
    tag = lambda p: np.array([p])
    problems = [(tag(p), tag(p), tag(p)) for p in range(4)] + [(tag(4), tag(4), tag(4), np.arange(5.0)), (tag(5), tag(5), tag(5))]
    list(pyddp.SlotScheduler(fake, iter(problems), 2, sweeps_per_poll=1).run())
    kinds = [c[0] for c in fake.calls]
    assert kinds.count("get") == 1 and kinds.index("get") == kinds.index("set") - 1 and kinds.index("set") > kinds.index("load")
    assert np.array_equal(fake.cost_at_load[4], np.arange(5.0)) and np.array_equal(fake.cost_at_load[5], RecordingSolver.WIDE)
    for p in range(4):
        assert np.array_equal(fake.cost_at_load[p], RecordingSolver.WIDE)


# ---------------------------------------------------------------------------------------------------------------- GPU 4: batch with a table == single-problem handles
ARM_TL_A4 = dict(ARM_TL, key="arm-thread-lanes-A4", kw=dict(ARM_KW, A=4))
ARM_TL2 = dict(ARM_FEW, key="arm-two-wave-rollouts", single_sel=dict(fp="tl2"), names=("k_bp_mfma", "k_fp_tl2", "k_nis_tl7"))
ARM_LG = dict(ARM_FEW, key="arm-lane-groups", single_sel=dict(bp="lg", fp="lg"), names=("k_bp_lg", "k_fp_lg", "k_nis_lg"))
ARM_LIMITS = dict(ARM_FEW, key="arm-limits", kw=dict(ARM_KW, use_limits=1), names=("k_bp", "k_fp", "k_nis"))
TABLE_CASES = [pytest.param(ARM_TL, id="arm-thread-lanes"), pytest.param(ARM_TL_A4, id="arm-thread-lanes-A4"), pytest.param(ARM_FEW, id="arm-few-problems"),
               pytest.param(ARM_TL2, id="arm-tl2"), pytest.param(ARM_EE, id="arm-end-effector"), pytest.param(ARM_LG, id="arm-lane-groups-f32"),
               pytest.param(ARM_F64, id="arm-float64"), pytest.param(ARM_LIMITS, id="arm-limits")]


def named_slots(B):
    return [b for b in reversed(range(B)) if b != KEEP]                                 # unsorted on purpose


@pytest.mark.gpu
@pytest.mark.parametrize("case", TABLE_CASES)
def test_batch_with_a_table_equals_single_problem_handles(case):
    B, ee = case["B"], bool(case["kw"].get("ee_cost"))
    probs = problems_of(case, B)
    recs = records(B, ee, 41)
    default = EE_DEFAULT if ee else JOINT_DEFAULT
    for use_graph in (1, 0):
        label = "%s use_graph=%d" % (case["key"], use_graph)
        s = handle(case, B, use_graph)
        assert_kernels(s, case)
        named = named_slots(B)
        s.set_cost_problems(named, recs[named])
        refs = load_and_compare(s, case, probs, recs, "first", label)
        s.close()
    # the weights were really used: a non-default slot's costs differ from the same problem's under the default record
    b = named[0]
    plain = yardstick(case, ("first", b), probs[b], default)
    assert not np.array_equal(refs[b]["Jout"], plain["Jout"]), (case["key"], "the records changed nothing")


# ---------------------------------------------------------------------------------------------------------------- GPU 5: rows change without a new graph
@pytest.mark.gpu
def test_rows_change_under_a_captured_graph_and_set_cost_overwrites_them():
    case, B = ARM_TL, ARM_TL["B"]
    probs = problems_of(case, B)
    first, second = records(B, False, 41), records(B, False, 97)
    assert not np.array_equal(first[named_slots(B)], second[named_slots(B)])
    s = handle(case, B, use_graph=1)
    named = named_slots(B)
    s.set_cost_problems(named, first[named])
    load_and_compare(s, case, probs, first, "first", "first records")
    s.set_cost_problems(named, second[named])                                           # the graph of the first solve stays: it holds the pointer, not the numbers
    load_and_compare(s, case, probs, second, "first", "second records")
    wide = JOINT_DEFAULT * np.array([1.7, 0.6, 2.3, 0.45, 1.25])
    s.set_cost(*wide)                                                                   # the handle-wide call afterwards: every row, the last call wins
    load_and_compare(s, case, probs, np.tile(wide, (B, 1)), "first", "after set_cost")
    assert np.array_equal(s.get_cost_problems(list(range(B))), np.tile(np.float32(wide).astype(np.float64), (B, 1)))
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 6: refill with weights
@pytest.mark.gpu
@pytest.mark.parametrize("case", [pytest.param(ARM_TL, id="arm-thread-lanes"), pytest.param(ARM_EE, id="arm-end-effector")])
def test_refill_with_weights(case):
    B, ee = case["B"], bool(case["kw"].get("ee_cost"))
    default = EE_DEFAULT if ee else JOINT_DEFAULT
    first, sweeps, late, _ = mixed_batch(case, 5)
    s = handle(case, B)
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    slots, done = pick_mixed_slots(s, 5, sweeps)
    late = late[: len(slots)]
    recs = records(B, ee, 59)[[b for b in range(B) if b != KEEP][: len(slots)]]
    others = [b for b in range(B) if b not in slots]
    before = snapshot(s)
    s.set_cost_problems(slots, recs)                                                    # (the handle's first per-problem call: the table appears under running problems)
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k])[others], np.asarray(after[k])[others], equal_nan=True), (case["key"], "another slot changed", k)
    assert np.array_equal(s.get_cost_problems(others), np.tile(np.asarray(default, np.float32 if case["dtype"] == 0 else np.float64).astype(np.float64), (len(others), 1)))
    run_until_done(s)
    refs = [yardstick(case, ("late", j), late[j], recs[j]) for j in range(len(slots))]
    assert_slots_equal_fresh(s, slots, refs, case["key"] + " refilled")
    running = [b for b in others if not done[b]]
    assert running, "no running slot among the others"
    assert_slots_equal_fresh(s, running, [yardstick(case, ("first-mixed", b), first[b], default) for b in running], case["key"] + " running others")
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 7: intake chunks
@pytest.mark.gpu
def test_refill_of_300_slots_with_weights_fetches_each_chunks_own_rows():
    """batch 2051, N 32 on the library's own selection (the shape of test_refill's 300-slot test): 300 refilled slots = two chunks of the intake area (256 + 44), slots 0, 1
    and 2050 among them.  Problems with period 11, records with period 7 (coprime): a chunk offset or an index slip in the fetch of the weights pairs a problem with
    another record.  Refilled slots and their +-1 neighbours (handle-wide rows, never named) against single-problem solves."""
    case, B, P, R = ARM_TL, 2051, 11, 7
    probs = problems_of(case, P)
    recs = records(R, False, 71)
    s = handle(case, B, sel={})
    have = [n for n, _ in s.time_kernels(1)]
    assert all(any(h.startswith(n) for h in have) for n in ("k_bp_mfma", "k_fp_tl", "k_nis_tl", "k_ls_many")), have
    reset_like_fresh(s)
    first = [probs[b % P] for b in range(B)]
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    s.iterate(4)
    rng = np.random.default_rng(3)
    slots = [2050, 0, 1] + [int(v) for v in rng.permutation(np.arange(2, 2050))[:297]]
    assert len(set(slots)) == 300
    late = [probs[(b + 5) % P] for b in slots]
    s.set_cost_problems(slots, np.stack([recs[b % R] for b in slots]))
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    run_until_done(s)
    assert len({((b + 5) % P, b % R) for b in slots}) > 60                              # most of the 77 (problem, record) pairs occur
    assert_slots_equal_fresh(s, slots, [yardstick(case, ("period", (b + 5) % P), probs[(b + 5) % P], recs[b % R]) for b in slots], "refilled")
    near = sorted({b + d for b in slots for d in (-1, 1) if 0 <= b + d < B} - set(slots))
    assert_slots_equal_fresh(s, near, [yardstick(case, ("period", b % P), probs[b % P], JOINT_DEFAULT) for b in near], "neighbours")
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 8: MPC
@pytest.mark.gpu
def test_mpc_cycles_with_per_problem_weights_equal_single_problem_handles():
    """end-effector handle, B = 3, per-problem QF_EE1 and Q_xdEE: a solve seeds it, then three pddp_mpc_solve cycles (shift 1, clear_vars 0, 4 iterations, the measured
    state = knot 1 of the previous plan); every cycle's x u KT Jout alphaOut success iters against three single-problem handles driven the same way with pddp_set_cost_ee."""
    B = 3
    probs = problems_of(ARM_EE, B)
    recs = np.tile(EE_DEFAULT, (B, 1))
    recs[0, 2], recs[0, 7] = 2300.0, 0.045
    recs[2, 2], recs[2, 7] = 410.0, 0.31
    keys = ("x", "u", "KT", "Jout", "alphaOut", "success", "iters")

    def drive(s, ps):
        n = len(ps)
        out = [s.solve(stack(ps, "x0"), stack(ps, "u0"), stack(ps, "xg"))]
        for _ in range(3):
            out.append(s.mpc_solve(out[-1]["x"][:, 1].copy(), stack(ps, "xg").reshape(n, -1), 1, clear_vars=0, max_iter=4))
        return out[1:]

    s = make_solver("hip", 4, dtype=0, batch=B, **EE_KW)
    s.set_cost_problems([2, 0], recs[[2, 0]])
    got = drive(s, probs)
    s.close()
    for b in range(B):
        s1 = make_solver("hip", 4, dtype=0, batch=1, **EE_KW)
        s1.set_cost_ee(*recs[b])
        ref = drive(s1, [probs[b]])
        s1.close()
        for cyc in range(3):
            for k in keys:
                assert np.array_equal(np.asarray(got[cyc][k][b]), np.asarray(ref[cyc][k][0]), equal_nan=True), ("cycle", cyc, "problem", b, k)


# ---------------------------------------------------------------------------------------------------------------- GPU 9: the oracle, float64
def oracle_pairs():
    """five (problem, record) pairs of the float64 oracle leg: problems of kinds a, b, c without the indefinite-Huu recipe, five distinct joint-space records"""
    pool = [p for p in pool_of(4, ARM_KW, 1, ARM_TL["recipe"], 4) if p["kind"] in "abc" and not p["c"]]
    return pool[:5], records(5, False, 83)


def oracle_solve(prob, rec):
    o = Oracle(default_cfg(4, cores=1, spawn_threads=0, **dict(ARM_KW, **dict(zip(JOINT, (float(v) for v in rec))))), np.float64)
    with np.errstate(all="ignore"):
        return o.run_ilqr_gpusem(prob["x0"], prob["u0"], prob["xg"])


def test_the_oracle_runs_every_chosen_pair_to_an_exit():
    probs, recs = oracle_pairs()
    assert len({tuple(r) for r in recs}) == 5
    for p, r in zip(probs, recs):
        ref = oracle_solve(p, r)
        assert 1 <= ref["iters"] <= ARM_KW["max_iter"] and np.isfinite(ref["Jout"][: ref["iters"] + 1]).all()


@pytest.mark.gpu
def test_float64_batch_with_a_table_follows_the_oracle():
    """arm bp = mx, fp = tl, float64, B = 5, five distinct records, every problem against Oracle(default_cfg(4, Q1=..., ...)).run_ilqr_gpusem at the bounds of
    test_float64_refilled_problems_follow_the_oracle: identical iter and alphaOut, Jout / x / u within 1e-8 x max|ref|."""
    probs, recs = oracle_pairs()
    refs = [oracle_solve(p, r) for p, r in zip(probs, recs)]
    s = make_solver("hip", 4, dtype=1, batch=5, kernels=dict(bp="mx", fp="tl"), **ARM_KW)
    s.set_cost_problems([4, 3, 2, 0], recs[[4, 3, 2, 0]])                               # (slot KEEP keeps the handle-wide record: recs[KEEP] is the default)
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    run_until_done(s)
    out = s.store()
    st = s.get_state()
    for b, r in enumerate(refs):
        it = r["iters"]
        assert st[b].iter == it, (b, st[b].iter, it)
        assert list(out["alphaOut"][b][: it + 1]) == list(r["alphaOut"][: it + 1]), (b, out["alphaOut"][b], r["alphaOut"])
        for k in ("Jout", "x", "u"):
            ref = r[k][: it + 1] if k == "Jout" else r[k]
            got = out[k][b][: it + 1] if k == "Jout" else out[k][b].ravel()
            assert np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max(), (b, k, float(np.abs(got - ref).max() / np.abs(ref).max()))
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 10: round trip and errors
@pytest.mark.gpu
def test_round_trip_and_argument_errors():
    case, B = ARM_FEW, ARM_FEW["B"]
    probs = problems_of(case, B)
    s = handle(case, B)
    assert s.cost_record_size() == 5
    f32 = lambda w: np.asarray(w, np.float32).astype(np.float64)
    assert np.array_equal(s.get_cost_problems(list(range(B))), np.tile(f32(JOINT_DEFAULT), (B, 1)))      # before any per-problem call
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
    before = snapshot(s)
    lib, EINVAL = s.lib, -1
    lib.pddp_set_cost_problems.argtypes = lib.pddp_get_cost_problems.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    good_idx, w = np.array([3, 0], np.int32), np.arange(1.0, 11.0)
    nan, inf = w.copy(), w.copy()
    nan[7], inf[9] = np.nan, np.inf
    bad = [("count 0", 0, good_idx, w), ("count < 0", -2, good_idx, w), ("idx null", 2, None, w), ("w null", 2, good_idx, None),
           ("index == batch", 2, np.array([0, B], np.int32), w), ("index < 0", 2, np.array([-1, 2], np.int32), w), ("index twice", 2, np.array([2, 2], np.int32), w),
           ("nan", 2, good_idx, nan), ("inf", 2, good_idx, inf)]
    for what, count, idx, ww in bad:
        assert lib.pddp_set_cost_problems(s.h, count, ptr(idx), ptr(ww)) == EINVAL, what
        if what not in ("nan", "inf"):
            out = np.zeros(10)
            assert lib.pddp_get_cost_problems(s.h, count, ptr(idx), None if ww is None else ptr(out)) == EINVAL, what
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), ("a refused call changed", k)
    assert np.array_equal(s.get_cost_problems(list(range(B))), np.tile(f32(JOINT_DEFAULT), (B, 1)))
    run_until_done(s)
    assert_slots_equal_fresh(s, list(range(B)), [yardstick(case, ("first", b), probs[b], JOINT_DEFAULT) for b in range(B)], "after the refused calls")
    # round trip: the float-rounded records for the named slots, the handle-wide record for the others
    recs = records(B, False, 41)
    named = named_slots(B)
    s.set_cost_problems(named, recs[named])
    want = f32(recs); want[KEEP] = f32(JOINT_DEFAULT)
    assert np.array_equal(s.get_cost_problems(list(range(B))), want)
    assert np.array_equal(s.get_cost_problems([B - 1, 0]), want[[B - 1, 0]])
    s.close()
    e = handle(dict(ARM_FEW, kw=EE_KW), 1)
    assert e.cost_record_size() == 9 and np.array_equal(e.get_cost_problems([0])[0], f32(EE_DEFAULT))
    e.close()
    # a plug-in cost (plant 5 of the reference-form two-link build, P::kPluginCost) refuses all three
    from test_ref_plugin import HIPLIB, KW as PLUGIN_KW
    u = pyddp.Solver(pyddp.default_config(5, _lib_path=HIPLIB, dtype=0, batch=2, **PLUGIN_KW), _lib_path=HIPLIB)
    ul = u.lib
    ul.pddp_set_cost_problems.argtypes = ul.pddp_get_cost_problems.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert ul.pddp_cost_record_size(u.h) == EINVAL
    assert ul.pddp_set_cost_problems(u.h, 2, ptr(np.array([0, 1], np.int32)), ptr(w)) == EINVAL
    assert ul.pddp_get_cost_problems(u.h, 2, ptr(np.array([0, 1], np.int32)), ptr(np.zeros(10))) == EINVAL
    u.close()
    c = make_solver("hip", 2, dtype=0, batch=2, N=64, M=4, A=8)                         # a cart-pole handle refuses all three
    lib = c.lib
    lib.pddp_set_cost_problems.argtypes = lib.pddp_get_cost_problems.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    out = np.zeros(10)
    assert lib.pddp_cost_record_size(c.h) == EINVAL
    assert lib.pddp_set_cost_problems(c.h, 2, ptr(np.array([0, 1], np.int32)), ptr(w)) == EINVAL
    assert lib.pddp_get_cost_problems(c.h, 2, ptr(np.array([0, 1], np.int32)), ptr(out)) == EINVAL
    c.close()
