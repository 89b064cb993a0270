"""Refilling and collecting individual slots of a running batch: pddp_load_problems / pddp_store_problems / pyddp.solve_stream.

The yardstick of every GPU check is a single-problem handle pinned to the same kernel families as the batch (solve_fresh: cost-to-go roles and observables as on a fresh
handle, pddp_load with clear_vars = 1, sweeps until the problem exits) -- never the refill path.  Shapes, recipes and kernel pins are those of tests/test_mixed_states.py
(imported, not changed); the problems are its pools without their warm-start arrays (a refill takes none).

CPU: the two entry points exist in the library, the header and the binding; the slot scheduler against a fake solver with scripted exit sweeps.
"""
import ctypes
import itertools
import os

import numpy as np
import pytest

import pyddp
from backends import make_solver
from oracle_binding import Oracle, default_cfg
from test_mixed_states import ARM_EE, ARM_FEW, ARM_TL, CART, CTG, DIMS, ORACLE_LEGS, QUAD, QUAD8_KW, pool_of, stack, typed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_ALL = tuple(name for name, _ in pyddp.binding.PddpState._fields_)
OUT_KEYS = ("x", "u", "KT", "Jout", "alphaOut", "dmax")
EXTRA_SWEEPS = 3


# ---------------------------------------------------------------------------------------------------------------- CPU: the surface
def test_entry_points_are_exported_declared_and_bound():
    lib = ctypes.CDLL(pyddp.library_path())
    header = open(os.path.join(ROOT, "include", "pddp.h")).read()
    for sym in ("pddp_load_problems", "pddp_store_problems"):
        assert getattr(lib, sym) is not None
        assert "int %s(pddp_handle h, int count, const int* idx," % sym in header
    assert callable(pyddp.Solver.load_problems) and callable(pyddp.Solver.store_problems) and callable(pyddp.solve_stream)


# ---------------------------------------------------------------------------------------------------------------- CPU: the scheduler on a fake solver
class FakeSolver:
    """status / iterate / load / load_problems / store_problems of a handle whose problem p exits after exit_sweeps[p] sweeps in its slot.  A problem is (x0, u0, xGoal)
    with x0 = [its index]; everything is logged."""

    def __init__(self, batch, exit_sweeps):
        self.B, self.exit_sweeps = batch, exit_sweeps
        self.slot_problem, self.age = [None] * batch, [0] * batch
        self.loaded, self.stored, self.sweeps = [], [], 0

    def _place(self, slot, tag):
        self.slot_problem[slot], self.age[slot] = int(tag), 0

    def load(self, x0, u0, xg, clear_vars=1, ignore_first_defect=1):
        assert clear_vars == 1 and len(x0) == self.B == len(u0) == len(xg)
        for slot in range(self.B):
            self._place(slot, x0[slot])
            self.loaded.append((int(x0[slot]), slot, "load"))

    def load_problems(self, idx, x0, u0, xg, ignore_first_defect=1):
        assert len(idx) == len(x0) == len(u0) == len(xg) and len(set(idx)) == len(idx)
        for slot, tag in zip(idx, x0):
            assert self.status()[0][slot], "a running slot was overwritten"
            self._place(slot, tag)
            self.loaded.append((int(tag), slot, "refill"))

    def iterate(self, sweeps):
        self.sweeps += sweeps
        for slot in range(self.B):
            self.age[slot] += sweeps

    def status(self):
        done = np.array([int(self.age[s] >= self.exit_sweeps[self.slot_problem[s]]) for s in range(self.B)], np.int32)
        return done, np.array(self.age, np.int32)

    def store_problems(self, idx):
        done = self.status()[0]
        for slot in idx:
            self.stored.append((self.slot_problem[slot], slot, bool(done[slot])))
        return dict(x=np.array([[self.slot_problem[slot]] for slot in idx]), Jout=np.array([[self.age[slot]] for slot in idx]))


@pytest.mark.parametrize("batch,count", [(4, 3), (4, 4), (4, 1), (4, 13), (1, 5), (6, 0)], ids=["shorter", "exactly-batch", "one", "3x+1", "one-slot", "empty"])
def test_scheduler_loads_stores_and_yields_every_problem_once(batch, count):
    rng = np.random.default_rng(batch * 100 + count)
    exit_sweeps = [int(v) for v in rng.integers(1, 23, max(count, 1))]
    fake = FakeSolver(batch, exit_sweeps)
    problems = ((np.array([p]), np.array([p]), np.array([p])) for p in range(count))          # a generator: the scheduler may not look ahead of what it loads
    got = list(pyddp.SlotScheduler(fake, problems, batch, sweeps_per_poll=4).run())
    assert sorted(i for i, _ in got) == list(range(count))                                       # every problem once, padding dropped
    for i, r in got:
        assert int(r["x"][0]) == i and r["done"] == 1                                            # with its own index, after its done
    if count == 0:
        assert not fake.loaded and fake.sweeps == 0
        return
    real = [(p, slot, how) for p, slot, how in fake.loaded if not (how == "load" and slot >= count)]
    assert sorted(p for p, _, _ in real) == list(range(count))                                   # loaded exactly once
    assert [p for p, slot, how in fake.loaded if how == "load" and slot >= count] == [0] * max(0, batch - count)      # the padding: copies of the first problem
    assert sorted(p for p, _, _ in fake.stored) == list(range(count)) and all(d for _, _, d in fake.stored)          # stored exactly once, after done
    assert fake.sweeps <= 4 * (sum(exit_sweeps) // 4 + len(exit_sweeps) + 1)


# ---------------------------------------------------------------------------------------------------------------- GPU: helpers
def problems_of(case, count, skip=0):
    """`count` warm-start-free problems of the case's pool (kinds interleaved a, c, b, d, e: early finishers next to long runners)"""
    pool = pool_of(case["plant"], case["kw"], case["dtype"], case["recipe"], (skip + count + 4) // 5)
    return pool[skip: skip + count]


def handle(case, batch, use_graph=1, sel=None):
    return make_solver("hip", case["plant"], dtype=case["dtype"], batch=batch, use_graph=use_graph, kernels=dict(case["single_sel"] if sel is None else sel), **case["kw"])


def state_rows(s, slots):
    st = s.get_state()
    return {f: np.array([getattr(st[b], f) for b in slots]) for f in STATE_ALL}


def solve_fresh(s1, prob):
    """the yardstick: one problem on a single-problem handle in the state of a fresh one, pddp_load(clear_vars = 1), sweep by sweep until it exits"""
    mi = s1.cfg.max_iter
    st = s1.get_state(); st[0].pw = 0; s1.set_state(st)
    s1.set("Jout", np.zeros(mi + 2)); s1.set("alphaOut", np.zeros(mi + 2, np.int32))
    s1.load(prob["x0"], prob["u0"], prob["xg"], clear_vars=1)
    res = {}
    for sweep in range(1, 4 * mi + 41):
        s1.iterate(1)
        done, _ = s1.status()
        if done[0]:
            break
    assert done[0], "the yardstick problem did not exit"
    res["sweeps"] = sweep
    res.update({k: v[0] for k, v in s1.store().items()})
    res.update({k: v[0] for k, v in state_rows(s1, [0]).items()})
    res.update({k: s1.get(k) for k in CTG})
    return res


_FRESH = {}


def fresh_of(case, probs, tag):
    """single-problem solves of `probs`, computed once per (case, tag), shared and left unchanged"""
    key = (case["key"], case["dtype"], tag)
    if key not in _FRESH:
        s1 = handle(case, 1)
        have = [n for n, _ in s1.time_kernels(1)]
        assert all(any(h.startswith(n) for h in have) for n in case["names"]), (case["names"], have)
        _FRESH[key] = [solve_fresh(s1, p) for p in probs]
        s1.close()
    return _FRESH[key]


def run_until_done(s, extra=EXTRA_SWEEPS):
    for _ in range(200):
        s.iterate(4)
        done, _ = s.status()
        if done.all():
            break
    assert done.all()
    s.iterate(extra); s.sync()


def assert_slots_equal_fresh(s, slots, refs, label):
    """store_problems, the state records and the cost-to-go arrays of `slots` against the single-problem solves refs[i], bit for bit, whole rows"""
    B = s.cfg.batch
    got = s.store_problems(slots)
    got.update(state_rows(s, slots))
    ctg = {k: s.get(k).reshape(B, -1)[slots] for k in CTG}
    for j, (slot, ref) in enumerate(zip(slots, refs)):
        for k in OUT_KEYS + STATE_ALL:
            assert np.array_equal(np.asarray(got[k][j]).ravel(), np.asarray(ref[k]).ravel(), equal_nan=True), (label, "slot", slot, k)
        for k in CTG:
            assert np.array_equal(ctg[k][j], ref[k], equal_nan=True), (label, "slot", slot, k)


CANDIDATES = 24


def mixed_batch(case, refills):
    """(first fill, sweeps before the refill, late problems, their single-problem solves).  The mix comes from the yardstick side: CANDIDATES problems of the pool behind
    the first fill are solved on the single-problem handle; the one that exits first goes to slot 1 and the one that runs longest to slot 2 of the first fill, and the
    refill happens at the sweep at which the former has just exited.  The late problems are the first `refills` candidates."""
    B = case["B"]
    cand = problems_of(case, CANDIDATES, skip=B)
    cref = fresh_of(case, cand, "candidates")
    sweeps = [r["sweeps"] for r in cref]
    early, long = int(np.argmin(sweeps)), int(np.argmax(sweeps))
    assert sweeps[early] < sweeps[long], ("every candidate exits at the same sweep", sweeps)
    first = problems_of(case, B)
    first[1], first[2] = cand[early], cand[long]
    return first, sweeps[early], cand[:refills], cref[:refills]


def pick_mixed_slots(s, want, sweeps):
    """`sweeps` sweeps; then an UNSORTED list of `want` slots: the last slot, slot 1 (done), slot 0, slot 2 (running), then running and done ones in turn"""
    B = s.cfg.batch
    s.iterate(sweeps)
    done = s.status()[0] != 0
    assert done[1] and not done[2], "the batch is not mixed at the sweep the single-problem solves name"
    inner = list(range(3, B - 1))
    fin, run = [b for b in inner if done[b]], [b for b in inner if not done[b]]
    slots = [B - 1, 1, 0, 2]
    rest = [b for pair in itertools.zip_longest(run, fin) for b in pair if b is not None]
    slots += rest[: max(0, want - len(slots))]
    assert slots != sorted(slots)
    return slots, done


def refill_case(case, refills):
    label = case["key"]
    B = case["B"]
    first, sweeps, late, refs = mixed_batch(case, refills)
    for use_graph in (1, 0):
        s = handle(case, B, use_graph)
        s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
        slots, done = pick_mixed_slots(s, refills, sweeps)
        late_n = late[: len(slots)]
        print("%s use_graph=%d: refill of slots %s (done %s)" % (label, use_graph, slots, [int(done[b]) for b in slots]))
        s.load_problems(slots, stack(late_n, "x0"), stack(late_n, "u0"), stack(late_n, "xg"))
        run_until_done(s)
        assert_slots_equal_fresh(s, slots, refs[: len(slots)], "%s use_graph=%d" % (label, use_graph))
        s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 1: refilled slot == fresh handle
ARM_F64 = dict(ARM_FEW, key="arm-float64", dtype=1, names=("k_bp", "k_fp", "k_nis"))
QUAD8 = dict(QUAD, key="quadrotor-N8", kw=QUAD8_KW)
REFILL_CASES = [pytest.param(ARM_TL, 5, id="arm-thread-lanes"), pytest.param(ARM_FEW, 4, id="arm-few-problems"), pytest.param(ARM_EE, 5, id="arm-end-effector"),
                pytest.param(ARM_F64, 4, id="arm-float64"), pytest.param(typed(CART, 0), 9, id="cartpole-f32"), pytest.param(typed(CART, 1), 9, id="cartpole-f64"),
                pytest.param(typed(QUAD, 0), 5, id="quadrotor"), pytest.param(typed(QUAD8, 0), 5, id="quadrotor-N8")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,refills", REFILL_CASES)
def test_refilled_slots_equal_fresh_single_problem_handles(case, refills):
    refill_case(case, refills)


# ---------------------------------------------------------------------------------------------------------------- GPU 2: untouched slots
UNTOUCHED = ("xb", "ucur", "dcur", "P", "Pp", "p", "pp", "AB", "H", "g", "KT", "du", "xGoal", "Jout", "alphaOut")


def snapshot(s):
    B = s.cfg.batch
    snap = {k: s.get(k).reshape(B, -1).copy() for k in UNTOUCHED}
    snap.update(state_rows(s, range(B)))
    return snap


@pytest.mark.gpu
@pytest.mark.parametrize("case", [pytest.param(ARM_TL, id="arm-thread-lanes"), pytest.param(ARM_EE, id="arm-end-effector"), pytest.param(typed(CART, 0), id="cartpole-f32"),
                                  pytest.param(typed(QUAD8, 0), id="quadrotor-N8")])
def test_refill_leaves_every_other_slot_byte_identical(case):
    B = case["B"]
    first, sweeps, late, _ = mixed_batch(case, 5)
    s = handle(case, B)
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    slots, _ = pick_mixed_slots(s, 5, sweeps)
    late = late[: len(slots)]
    refs = []
    for prob in late:                                   # a handle nothing has run on, loaded once: what the setup kernel's init mode alone leaves in [A B], H, g
        s1 = handle(case, 1)
        s1.load(prob["x0"], prob["u0"], prob["xg"], clear_vars=1)
        refs.append({"init_" + k: s1.get(k) for k in ("AB", "H", "g")})
        s1.close()
    before = snapshot(s)
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    after = snapshot(s)
    others = [b for b in range(B) if b not in slots]
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(before[k][others], after[k][others], equal_nan=True), (case["key"], "untouched slots", k)
    for j, slot in enumerate(slots):
        for k in ("AB", "H", "g"):
            assert np.array_equal(after[k][slot], refs[j]["init_" + k], equal_nan=True), (case["key"], "slot", slot, k)
        assert after["iter"][slot] == 1 and after["done"][slot] == 0 and after["pw"][slot] == 0 and after["cur"][slot] == 0
        assert not after["Jout"][slot][1:].any() and not after["alphaOut"][slot][1:].any() and after["alphaOut"][slot][0] == -1
        for k in ("P", "Pp", "p", "pp", "KT", "dcur", "du"):
            assert not after[k][slot].any(), (case["key"], "slot", slot, k)
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 3: the compact layout's edges
@pytest.mark.gpu
def test_refill_of_300_slots_of_2051_on_the_compact_layouts():
    """batch 2051, N 32 on the library's own selection: a 64-knot chunk of the compact [A B] holds two problems, the last chunk is partial; 300 refilled slots = two
    chunks of the intake area (256 + 44), odd and even indices, slot 2050.  The 11 problems of the thread-lane case with period 11 before the refill, shifted by 5 after."""
    case, B, P = ARM_TL, 2051, 11
    probs = problems_of(case, P)
    refs = fresh_of(case, probs, "period")
    s = handle(case, B, sel={})
    have = [n for n, _ in s.time_kernels(1)]
    assert all(any(h.startswith(n) for h in have) for n in ("k_bp_mfma", "k_fp_tl", "k_nis_tl", "k_ls_many")), have
    st = s.get_state()                                  # (the sweep time_kernels ran flipped the cost-to-go roles, which a load keeps: back to those of a fresh handle)
    for b in range(B):
        st[b].pw = 0
    s.set_state(st)
    first = [probs[b % P] for b in range(B)]
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    s.iterate(4)
    rng = np.random.default_rng(3)
    slots = [2050, 0, 1] + [int(v) for v in rng.permutation(np.arange(2, 2050))[:297]]
    assert len(set(slots)) == 300 and sum(b % 2 for b in slots) > 100 and sum(b % 2 == 0 for b in slots) > 100
    late = [probs[(b + 5) % P] for b in slots]
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    run_until_done(s)
    assert_slots_equal_fresh(s, slots, [refs[(b + 5) % P] for b in slots], "compact edge, refilled")
    near = sorted({b + d for b in slots for d in (-1, 1) if 0 <= b + d < B} - set(slots))
    assert_slots_equal_fresh(s, near, [refs[b % P] for b in near], "compact edge, neighbours")
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 4: the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("case", ORACLE_LEGS[:2])
def test_float64_refilled_problems_follow_the_oracle(case):
    """float64 arm (bp = mx, fp = tl) and cart-pole (cf = ts): refilled problems against Oracle.run_ilqr_gpusem at the bounds of test_mixed_states' oracle leg"""
    plant, kw = case["plant"], case["kw"]
    pool = [p for p in pool_of(plant, kw, 1, case["recipe"], 4) if p["kind"] in "abc" and not p["c"]]
    B, late = 5, pool[5:9]
    o = Oracle(default_cfg(plant, cores=1, spawn_threads=0, **kw), np.float64)
    with np.errstate(all="ignore"):
        refs = [o.run_ilqr_gpusem(p["x0"], p["u0"], p["xg"]) for p in late]
    s = make_solver("hip", plant, dtype=1, batch=B, kernels=dict(case["single_sel"]), **kw)
    s.load(stack(pool[:B], "x0"), stack(pool[:B], "u0"), stack(pool[:B], "xg"), clear_vars=1)
    s.iterate(4)
    slots = [4, 0, 2, 3]
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    run_until_done(s)
    out = s.store_problems(slots)
    st = state_rows(s, slots)
    s.close()
    for j, r in enumerate(refs):
        it = r["iters"]
        assert st["iter"][j] == it, (j, st["iter"][j], it)
        assert list(out["alphaOut"][j][: it + 1]) == list(r["alphaOut"][: it + 1]), (j, out["alphaOut"][j], r["alphaOut"])
        for k in ("Jout", "x", "u"):
            ref = r[k][: it + 1] if k == "Jout" else r[k]
            got = out[k][j][: it + 1] if k == "Jout" else out[k][j].ravel()
            assert np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max(), (j, k, float(np.abs(got - ref).max() / np.abs(ref).max()))
        J = r["Jout"]
        if r["alphaOut"][it] >= 0 and (J[it - 1] - J[it]) / J[it - 1] < kw["tol_cost"]:
            assert st["done"][j] == 1, (j, st["done"][j])
        assert st["done"][j] in (1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------- GPU 5: store_problems == rows of store
@pytest.mark.gpu
def test_store_problems_equals_the_rows_of_store_with_null_outputs():
    case, B = ARM_TL, ARM_TL["B"]
    first, sweeps, _, _ = mixed_batch(case, 0)
    s = handle(case, B)
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    slots, done = pick_mixed_slots(s, 6, sweeps)
    assert len({int(done[b]) for b in slots}) >= 2
    whole = s.store()
    assert len(set(state_rows(s, range(B))["cur"])) == 2, "both halves of xb should be current somewhere in the batch"
    rows = s.store_problems(slots)
    for k in OUT_KEYS:
        assert np.array_equal(rows[k], whole[k][slots], equal_nan=True), k
    for drop in itertools.combinations(OUT_KEYS, 2):
        keep = [k for k in OUT_KEYS if k not in drop]
        part = s.store_problems(slots, only=keep)
        assert sorted(part) == sorted(keep)
        for k in keep:
            assert np.array_equal(part[k], whole[k][slots], equal_nan=True), (drop, k)
    every = s.store_problems(list(range(B - 1, -1, -1)))
    for k in OUT_KEYS:
        assert np.array_equal(every[k], whole[k][::-1], equal_nan=True), k
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 6: the stream
@pytest.mark.gpu
def test_solve_stream_equals_single_problem_solves():
    case, B = ARM_TL, ARM_TL["B"]
    probs = problems_of(case, 3 * B)
    refs = fresh_of(case, probs, "stream")
    s = handle(case, B)
    got = dict(pyddp.solve_stream(s, ((p["x0"], p["u0"], p["xg"]) for p in probs), sweeps_per_poll=4))
    s.close()
    assert sorted(got) == list(range(3 * B))
    for i, ref in enumerate(refs):
        for k in OUT_KEYS:
            assert np.array_equal(np.asarray(got[i][k]).ravel(), np.asarray(ref[k]).ravel(), equal_nan=True), (i, k)
        assert got[i]["done"] == ref["done"] and got[i]["iters"] == ref["iter"], (i, got[i]["done"], got[i]["iters"])
    assert len({r["iter"] for r in refs}) >= 3, "the stream's problems should exit at different iterations"


# ---------------------------------------------------------------------------------------------------------------- GPU 7: argument errors
@pytest.mark.gpu
def test_argument_errors_leave_the_handle_unchanged():
    case, B = ARM_TL, ARM_TL["B"]
    first = problems_of(case, B)
    n, m = DIMS[4][1], DIMS[4][2]
    N = case["kw"]["N"]
    x, u, g = np.zeros((2, N, n), np.float32), np.zeros((2, N, m), np.float32), np.zeros((2, n), np.float32)
    s = handle(case, B)
    with pytest.raises(pyddp.PddpError, match="pddp_load_problems.*never been loaded"):
        s.load_problems([0, 1], x, u, g)
    with pytest.raises(pyddp.PddpError, match="pddp_store_problems.*never been loaded"):
        s.store_problems([0])
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    s.iterate(3); s.sync()
    before = snapshot(s)
    lib, einval = s.lib, -1
    lib.pddp_load_problems.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int]
    lib.pddp_store_problems.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 7
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)          # noqa: E731
    ok = np.array([1, 0], np.int32)
    bad = {"count < 1": (0, ok), "negative count": (-2, ok), "index == batch": (2, np.array([0, B], np.int32)), "negative index": (2, np.array([-1, 3], np.int32)),
           "duplicate": (2, np.array([4, 4], np.int32))}
    for what, (count, idx) in bad.items():
        rc = lib.pddp_load_problems(s.h, count, p(idx), p(x), p(u), p(g), 1)
        assert rc != 0 and b"pddp_load_problems" in lib.pddp_last_error(), (what, rc, lib.pddp_last_error())
        einval = rc
        rc = lib.pddp_store_problems(s.h, count, p(idx), p(x), None, None, None, None, None)
        assert rc == einval and b"pddp_store_problems" in lib.pddp_last_error(), (what, rc, lib.pddp_last_error())
    for args in ((None, p(x), p(u), p(g)), (p(ok), None, p(u), p(g)), (p(ok), p(x), None, p(g)), (p(ok), p(x), p(u), None)):
        rc = lib.pddp_load_problems(s.h, 2, *args, 1)
        assert rc == einval and b"pddp_load_problems" in lib.pddp_last_error(), (args, rc)
    assert lib.pddp_store_problems(s.h, 2, None, p(x), None, None, None, None, None) == einval
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(before[k], after[k], equal_nan=True), k
    s.close()
