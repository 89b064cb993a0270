"""Control cycles for named slots of a batch: pddp_mpc_solve_problems / pddp_mpc_load_problems (csrc/mpc_slots.hpp, solver_impl.hpp mpc_problems).

The yardstick everywhere is the WHOLE-HANDLE call on a twin handle -- pddp_mpc_load / pddp_mpc_solve, which tests/test_mpc_load_stage.py, test_mpc_parity.py and
test_mpc_pins.py hold to the reference -- never the new path.  Every comparison is np.array_equal: problems of a batch are independent and each kernel family is
deterministic per problem (tests/test_refill.py relies on the same across batch sizes), so a cycle run for three named slots on the intake area has to leave, bit for
bit, what the cycle of the whole handle leaves in those slots, and nothing anywhere else.

  1 (CPU)  both symbols exported, declared with the documented argument lists, bound in pyddp; tests/native/mpc_slots_host_check.cpp compiles and prints its ok line
  2 (GPU)  the load stage alone, every array set to distinct random values first, state.cur mixed: named rows == the twin's, unnamed rows == what was set
  3 (GPU)  two cycles per slot with per-slot histories, in four calls that cut across the cycles; both success outcomes on the path; graph / no graph / polled loop
  4 (GPU)  a call on two finished slots of a running mixed batch: the slots that are still running end as on a handle that never saw the call
  5 (GPU)  260 of 300 slots in shuffled order: two chunks of the intake area (256 + 4), the compact [A B] with N < 64
  6 (GPU)  every argument error returns PDDP_EINVAL with a message and leaves every array and state as it was
  7 (GPU)  the intake area is shared with pddp_load_problems: a refill that follows cycles of named slots gives fresh slots, by test_refill's own assertions and references
  8 (GPU)  after sweeps with boundary_cost_to_go_only a warm start of named slots is refused, and clearing SOME slots does not lift the refusal for the others
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pyddp
from backends import make_solver
from oracle_binding import example_inputs, PLANT_DIMS
from test_mixed_states import ARM_TL, CART, stack, typed
from test_mpc_load_stage import BYSTANDERS, CASES, SET, fill_inputs
from test_refill import STATE_ALL, assert_slots_equal_fresh, handle, mixed_batch, pick_mixed_slots, problems_of, run_until_done, state_rows
from test_refill import snapshot as refill_snapshot
from test_simulate_batch import SIGMA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every per-problem array pddp_get_array names, [batch][...] rows ("AB" and "H" are the reference-layout views of the compact "ABc" / "Hc" where a handle keeps those)
NAMED = ("xs", "us", "ds", "xb", "ucur", "dcur", "P", "Pp", "p", "pp", "AB", "H", "g", "KT", "du", "ApBK", "Bdu", "J", "dmax", "dJexp", "xGoal", "Jout", "err", "alphaOut",
         "x_old", "u_old", "KT_old", "xTarget", "costk", "tshift", "Jpart", "dpart", "parts_fresh")
FAMILY = ("xw", "segmap")                   # exist on some kernel families only
INPUTS = ("xActual", "shift")               # the cycle's inputs as a whole-handle call leaves them on the device
OUT = ("x", "u", "KT", "Jout", "alphaOut", "success", "iters")
EINVAL = -1


def rows(s, name):
    return s.get(name).reshape(s.cfg.batch, -1).copy()


def snapshot(s, names=NAMED + INPUTS):
    snap = {k: rows(s, k) for k in names}
    for k in FAMILY:
        try:
            snap[k] = rows(s, k)
        except pyddp.PddpError:
            pass
    snap.update(state_rows(s, range(s.cfg.batch)))
    return snap


def assert_rows(got, want, slots, label, want_slots=None):
    """rows `slots` of every array and state field of `got` == rows want_slots (default: the same) of `want`"""
    want_slots = slots if want_slots is None else want_slots
    assert set(got) == set(want), (label, set(got) ^ set(want))
    for k in got:
        assert np.array_equal(got[k][list(slots)], want[k][list(want_slots)], equal_nan=True), (label, k, [b for b, w in zip(slots, want_slots) if not np.array_equal(got[k][b], want[k][w], equal_nan=True)])


# ---------------------------------------------------------------------------------------------------------------- 1: the surface, the host-only code
def test_entry_points_are_exported_declared_and_bound(tmp_path):
    lib = ctypes.CDLL(pyddp.library_path())
    header = " ".join(open(os.path.join(ROOT, "include", "pddp.h")).read().split())
    for sym in ("pddp_mpc_solve_problems", "pddp_mpc_load_problems"):
        assert getattr(lib, sym) is not None
    assert ("int pddp_mpc_solve_problems(pddp_handle h, int count, const int* idx, const void* xActual, const void* xGoal, const int* shift, int clear_vars, "
            "int full_rollout, int ignore_first_defect, int max_iter, double time_budget_ms, int poll_every, void* x, void* u, void* KT, void* Jout, int* alphaOut, "
            "int* success, int* iters);") in header
    assert ("int pddp_mpc_load_problems(pddp_handle h, int count, const int* idx, const void* xActual, const void* xGoal, const int* shift, int clear_vars, "
            "int full_rollout);") in header
    for name in ("mpc_solve_problems", "mpc_load_problems"):
        assert callable(getattr(pyddp.Solver, name))
    assert getattr(lib, "pddp_mpc_slots_profile") is not None and "int pddp_mpc_slots_profile(pddp_handle h, int timing, float* ms3);" in header
    exe = str(tmp_path / "mpc_slots_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "mpc_slots_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "mpc_slots_host_check: ok" in out.stdout, out.stdout + out.stderr


# ---------------------------------------------------------------------------------------------------------------- 2: the load stage
LOAD_CASES = ("arm-f32-pipe-v1", "arm-f32-pipe-m1", "arm-f32-lg", "arm-f64", "cart-f32-rk3", "arm-f32-ee-shift")
LOAD_B, LOAD_IDX, LOAD_SHIFT = 5, [4, 0, 2], [3, 0, 1]          # shift 0 and the last slot are the traps


@pytest.mark.gpu
@pytest.mark.parametrize("case", LOAD_CASES)
def test_load_stage_of_named_slots_equals_the_whole_handle_load_stage(case):
    plant, dt_code, _, kw, sel, _ = CASES[case]
    dtype = np.float64 if dt_code else np.float32
    B, N, M, A = LOAD_B, kw["N"], kw["M"], kw["A"]
    npos, n, m = PLANT_DIMS[plant]
    dims = (B, N, M, N // M, n, m, A)
    twin, subj = [make_solver("hip", plant, dtype=dt_code, batch=B, max_iter=4, kernels=sel, **kw) for _ in range(2)]
    x0, u0, xg = example_inputs(plant, N, dtype)
    for s in (twin, subj):                                          # (a handle has to be loaded before its slots can be named)
        s.load(np.tile(x0, B), np.tile(u0, B), np.tile(xg, B))
    rng = np.random.default_rng([91, LOAD_CASES.index(case)])
    others = [b for b in range(B) if b not in LOAD_IDX]
    call = 0
    for clear in (0, 1):
        for full in (0, 1):
            inp = fill_inputs(rng, plant, dtype, dims)
            inp.update(H=rng.normal(0, 1, (B, N, (n + m) ** 2)).astype(dtype), g=rng.normal(0, 1, (B, N, n + m)).astype(dtype), J=rng.normal(0, 1, (B, A)).astype(dtype),
                       Jout=rng.normal(0, 1, (B, 6)).astype(dtype), alphaOut=rng.integers(1, 1000, (B, 6)).astype(np.int32))
            cur = [(call + i) % 2 for i in range(B)]
            assert 0 in cur and 1 in cur
            for s in (twin, subj):
                for k in SET + BYSTANDERS:
                    s.set(k, inp[k])
                st = s.get_state()
                for i in range(B):
                    st[i].cur = cur[i]
                s.set_state(st)
            shifts = np.zeros(B, np.int32); shifts[LOAD_IDX] = LOAD_SHIFT
            goal = rng.normal(0, 1, (B, n)).astype(dtype)
            xact = np.stack([inp["xb"][i, cur[i], shifts[i]] for i in range(B)]) + rng.normal(0, 0.0005, (B, n)).astype(dtype)
            names = SET + BYSTANDERS + INPUTS
            was = snapshot(subj, names)
            for k in SET + BYSTANDERS:
                if k != "AB":                                       # (a handle on the compact [A B] returns the view of what it kept of an arbitrary array)
                    assert np.array_equal(was[k], np.asarray(inp[k]).reshape(B, -1)), (case, k)
            twin.mpc_load(xact, goal, shifts, clear_vars=clear, full_rollout=full)
            subj.mpc_load_problems(LOAD_IDX, xact[LOAD_IDX], goal[LOAD_IDX], LOAD_SHIFT, clear_vars=clear, full_rollout=full)
            got, want = snapshot(subj, names), snapshot(twin, names)
            label = (case, "clear", clear, "full", full, "cur", cur)
            assert_rows(got, want, LOAD_IDX, label + ("named",))
            assert_rows(got, was, others, label + ("unnamed",))
            assert not np.array_equal(got["xb"][LOAD_IDX], was["xb"][LOAD_IDX])            # (the stage did run)
            call += 1
    twin.close(); subj.close()


# ---------------------------------------------------------------------------------------------------------------- 3: cycles with per-slot histories
CYC_B = 6
ARM_CYC = dict(N=32, M=4, A=8, wafr_urdf=1, mpc_mode=1, tol_cost=1e-5, total_time=0.5, max_iter=10, ignore_max_rho_exit=0)
CYCLE_CASES = {
    "arm-f32": (4, 0, ARM_CYC),                                     # the library's own selection at this batch: the pipeline form
    "arm-f64": (4, 1, ARM_CYC),
    "arm-f32-ee": (4, 0, dict(ARM_CYC, ee_cost=1, ee_cost_shift=1)),     # + two different per-problem cost rows
    "cart-f32-rk3": (2, 0, dict(N=32, M=2, A=8, integrator=3, total_time=2.0, tol_cost=1e-5, max_iter=10)),
}
CYC_SHIFT = np.array([[0, 1, 2, 3, 1, 2], [3, 0, 1, 2, 0, 3]], np.int32)      # [cycle][slot]: different per slot and cycle
CYC_SIGMA = np.concatenate([SIGMA, [0.0]])                                     # test_simulate_batch's start-state noise per problem, and one slot that starts on its plan
CYC_CALLS = [(0, [5, 0, 3]), (0, [1, 2, 4]), (1, [3, 1]), (1, [4, 5, 0, 2])]
EE_ROWS = {1: [0.1, 0.013, 1000.0, 170.0, 0.0001, 0.0021, 23.0, 0.07, 810.0], 4: [0.13, 0.0, 900.0, 0.0, 0.0002, 0.0, 0.0, 0.12, 1100.0]}


def cycle_seed(plant, kw, dtype):
    """(x0, u0, goals of the seeding solve, goals per cycle): six problems towards six different goals"""
    N = kw["N"]
    npos, n, m = PLANT_DIMS[plant]
    step = np.linspace(-0.03, 0.03, CYC_B)
    if kw.get("ee_cost"):
        x0 = np.zeros((CYC_B, N, n), dtype); x0[:, :, 1] = 0.7; x0[:, :, 3] = -0.8; x0[:, :, 5] = 0.75      # the MPC example's start and tool-point goal
        u0 = np.full((CYC_B, N, m), 0.01, dtype)
        xg = np.zeros((CYC_B, n), dtype); xg[:, :3] = np.array([0.45, 0.15, 0.75]) + np.stack([step, -step, 0.5 * step], 1)
        moved = lambda c: np.concatenate([np.full((CYC_B, 3), 0.01 * (c + 1)), np.zeros((CYC_B, n - 3))], 1).astype(dtype)
    else:
        x, u, g = example_inputs(plant, N, dtype)
        x0, u0 = np.tile(x, (CYC_B, 1)), np.tile(u, (CYC_B, 1))
        xg = np.tile(g, (CYC_B, 1)); xg[:, :npos] += step[:, None].astype(dtype)
        moved = lambda c: np.concatenate([np.full((CYC_B, npos), 0.01 * (c + 1)), np.zeros((CYC_B, n - npos))], 1).astype(dtype)
    return x0, u0, xg, [xg + moved(0), xg + moved(1)]


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph,poll_every", [(1, 4), (0, 4), (1, 1)], ids=["graph", "no-graph", "polled"])
@pytest.mark.parametrize("case", list(CYCLE_CASES))
def test_cycles_with_per_slot_histories_equal_whole_handle_cycles(case, use_graph, poll_every):
    plant, dt_code, kw = CYCLE_CASES[case]
    dtype = np.float64 if dt_code else np.float32
    npos, n, m = PLANT_DIMS[plant]
    x0, u0, xg, goals = cycle_seed(plant, kw, dtype)
    twin, subj = [make_solver("hip", plant, dtype=dt_code, batch=CYC_B, use_graph=use_graph, **kw) for _ in range(2)]
    plans = []
    for s in (twin, subj):
        if kw.get("ee_cost"):
            s.set_cost_problems(list(EE_ROWS), list(EE_ROWS.values()))
        plans.append(s.solve(x0, u0, xg))
    assert np.array_equal(plans[0]["x"], plans[1]["x"])
    rng = np.random.default_rng([92, list(CYCLE_CASES).index(case)])
    noise = [np.stack([rng.normal(0, CYC_SIGMA[b], n) for b in range(CYC_B)]).astype(dtype) for _ in range(2)]
    # the twin: cycle 0, then cycle 1, all six slots; a slot's measured state is knot `shift` of the twin's plan after its previous cycle, perturbed
    want, xact, plan = [], [], plans[0]["x"]
    for c in range(2):
        xact.append((plan[np.arange(CYC_B), CYC_SHIFT[c]] + noise[c]).astype(dtype))
        want.append(twin.mpc_solve(xact[c], goals[c], CYC_SHIFT[c], max_iter=4, poll_every=poll_every))
        plan = want[c]["x"]
    success = [int(v) for c in range(2) for v in want[c]["success"]]
    print("%s use_graph %d poll_every %d: success of the twin's 2 x 6 cycles %s" % (case, use_graph, poll_every, success))
    assert 0 in success and 1 in success, success                   # accepted solutions AND the fall-back branch are on the path
    for c, slots in CYC_CALLS:
        was = snapshot(subj)
        r = subj.mpc_solve_problems(slots, xact[c][slots], goals[c][slots], CYC_SHIFT[c][slots], max_iter=4, poll_every=poll_every)
        for k in OUT:
            assert np.array_equal(r[k], want[c][k][slots], equal_nan=True), (case, "cycle", c, "slots", slots, k)
        others = [b for b in range(CYC_B) if b not in slots]
        assert_rows(snapshot(subj), was, others, (case, "cycle", c, "slots", slots, "unnamed"))
    got, ref = snapshot(subj), snapshot(twin)
    assert_rows(got, ref, range(CYC_B), (case, "after the last call"))
    if kw.get("ee_cost"):
        assert np.array_equal(subj.get_cost_problems(range(CYC_B)), twin.get_cost_problems(range(CYC_B)))
    twin.close(); subj.close()


# ---------------------------------------------------------------------------------------------------------------- 4: a running neighbour
@pytest.mark.gpu
def test_a_cycle_on_finished_slots_leaves_running_neighbours_alone():
    case, B = ARM_TL, ARM_TL["B"]
    first, sweeps, _, _ = mixed_batch(case, 4)
    res = {}
    for seen in (False, True):
        s = handle(case, B)
        s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
        _, done = pick_mixed_slots(s, 4, sweeps)
        running = [b for b in range(B) if not done[b]]
        fin = [b for b in range(B) if done[b]][::-1][:2]
        assert len(fin) == 2 and len(running) >= 2, done
        if seen:
            plan = s.store_problems(fin, only=("x",))["x"]
            goal = np.stack([first[b]["xg"] for b in fin])
            r = s.mpc_solve_problems(fin, plan[:, 0], goal, [0, 1], clear_vars=1, max_iter=4)
            assert (r["iters"] >= 1).all()
        run_until_done(s)
        out = s.store_problems(running)
        out.update(state_rows(s, running))
        out.update({k: s.get(k).reshape(B, -1)[running] for k in ("P", "Pp", "p", "pp", "xb", "dcur", "du", "H", "g", "AB")})
        res[seen] = (running, out)
        s.close()
    assert res[False][0] == res[True][0]
    for k in res[False][1]:
        assert np.array_equal(res[True][1][k], res[False][1][k], equal_nan=True), ("running slots", k)


# ---------------------------------------------------------------------------------------------------------------- 5: more than one chunk
@pytest.mark.gpu
@pytest.mark.parametrize("case", [pytest.param(ARM_TL, id="arm-thread-lanes"), pytest.param(typed(CART, 0), id="cartpole-f32")])
def test_260_named_slots_of_300_go_through_two_chunks(case):
    B, P, K = 300, 11, 260
    npos, n, m = PLANT_DIMS[case["plant"]]
    dtype = np.float32
    probs = problems_of(case, P)
    first = [probs[b % P] for b in range(B)]
    rng = np.random.default_rng(93)
    left_out = set(int(v) for v in rng.permutation(np.arange(1, B - 1))[: B - K])      # (the first and the last slot are named)
    slots = [int(v) for v in rng.permutation(B) if int(v) not in left_out]
    assert len(slots) == K and slots != sorted(slots) and B - 1 in slots and 0 in slots
    shift = rng.integers(0, 4, B).astype(np.int32)
    twin, subj = [handle(case, B) for _ in range(2)]
    have = [nm for nm, _ in subj.time_kernels(1)]
    assert all(any(h.startswith(nm) for h in have) for nm in case["names"]), (case["names"], have)
    twin.time_kernels(1)                                             # (both handles the same history)
    plans = [s.solve(stack(first, "x0"), stack(first, "u0"), stack(first, "xg")) for s in (twin, subj)]
    assert np.array_equal(plans[0]["x"], plans[1]["x"])
    xact = (plans[0]["x"][np.arange(B), shift] + rng.normal(0, 0.004, (B, n))).astype(dtype)
    goal = np.stack([p["xg"] for p in first]).astype(dtype)
    want = twin.mpc_solve(xact, goal, shift, max_iter=4)
    was = snapshot(subj)
    r = subj.mpc_solve_problems(slots, xact[slots], goal[slots], shift[slots], max_iter=4)
    for k in OUT:
        assert np.array_equal(r[k], want[k][slots], equal_nan=True), (case["key"], k)
    got, ref = snapshot(subj), snapshot(twin)
    others = [b for b in range(B) if b not in slots]
    assert len(others) == 40
    assert_rows(got, ref, slots, (case["key"], "named"))
    assert_rows(got, was, others, (case["key"], "unnamed"))
    twin.close(); subj.close()


# ---------------------------------------------------------------------------------------------------------------- 6: argument errors
@pytest.mark.gpu
def test_argument_errors_leave_the_handle_unchanged():
    plant, dt_code, kw = CYCLE_CASES["arm-f32"]
    N, n = kw["N"], 14
    x0, u0, xg, goals = cycle_seed(plant, kw, np.float32)
    s = make_solver("hip", plant, dtype=dt_code, batch=CYC_B, **kw)
    lib = s.lib
    lib.pddp_mpc_solve_problems.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 7
    lib.pddp_mpc_load_problems.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.pddp_last_error.restype = ctypes.c_char_p
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    good = dict(count=2, idx=np.array([3, 1], np.int32), xa=np.ascontiguousarray(x0.reshape(CYC_B, N, n)[[3, 1], 0]), xg=np.ascontiguousarray(goals[0][[3, 1]]), shift=np.array([1, 0], np.int32), max_iter=4)

    def both(label, **change):
        a = dict(good, **change)
        for which in ("solve", "load"):
            if which == "load" and "max_iter" in change:
                continue
            if which == "solve":
                rc = lib.pddp_mpc_solve_problems(s.h, a["count"], ptr(a["idx"]), ptr(a["xa"]), ptr(a["xg"]), ptr(a["shift"]), 0, 1, 1, a["max_iter"], 0.0, 4, *([None] * 7))
            else:
                rc = lib.pddp_mpc_load_problems(s.h, a["count"], ptr(a["idx"]), ptr(a["xa"]), ptr(a["xg"]), ptr(a["shift"]), 0, 1)
            assert rc == EINVAL, (label, which, rc)
            assert len(lib.pddp_last_error()) > 10, (label, which)
            print("%-28s %-5s -> %s" % (label, which, lib.pddp_last_error().decode()))

    both("a handle never loaded")
    s.solve(x0, u0, xg)
    was = snapshot(s)
    both("count 0", count=0)
    both("count -1", count=-1)
    for k in ("idx", "xa", "xg", "shift"):
        both("NULL " + k, **{k: None})
    both("index == batch", idx=np.array([3, CYC_B], np.int32))
    both("index -1", idx=np.array([-1, 3], np.int32))
    both("index twice", idx=np.array([3, 3], np.int32))
    both("shift -1", shift=np.array([1, -1], np.int32))
    both("shift N-1", shift=np.array([N - 1, 0], np.int32))
    both("max_iter 0", max_iter=0)
    both("max_iter > config", max_iter=kw["max_iter"] + 1)
    assert_rows(snapshot(s), was, range(CYC_B), "after the refused calls")
    r = s.mpc_solve_problems(good["idx"], good["xa"], good["xg"], good["shift"], max_iter=4)      # ... and the handle is as usable as before
    assert (r["iters"] >= 1).all()
    s.close()


# ---------------------------------------------------------------------------------------------------------------- 7: a refill behind cycles on the shared intake area
@pytest.mark.gpu
@pytest.mark.parametrize("case", [pytest.param(ARM_TL, id="arm-thread-lanes"), pytest.param(typed(CART, 0), id="cartpole-f32")])
def test_refill_after_cycles_of_named_slots_gives_fresh_slots(case):
    """pddp_mpc_solve_problems leaves some robots' solver states (pw flipped by their iterations) and Jout / alphaOut rows in the intake problems; pddp_load_problems on the
    same handle must hand out what it hands out on a handle that never ran a cycle: tests/test_refill.py's assertions on the slot right after the refill, and its
    single-problem fresh-handle references after the solve."""
    B, refills = case["B"], 5
    npos, n, m = PLANT_DIMS[case["plant"]]
    first, sweeps, late, refs = mixed_batch(case, refills)
    s = handle(case, B)
    s.load(stack(first, "x0"), stack(first, "u0"), stack(first, "xg"), clear_vars=1)
    slots, done = pick_mixed_slots(s, refills, sweeps)
    late, refs = late[: len(slots)], refs[: len(slots)]
    # cycles in the intake problems the refill is about to use: more named slots than refilled ones, twice, so that every one of them holds iterated leftovers
    named = slots + [b for b in range(B) if b not in slots][:2]
    goal = np.stack([first[b]["xg"] for b in named])
    for _ in range(2):
        plan = s.store_problems(named, only=("x",))["x"]
        r = s.mpc_solve_problems(named, plan[:, 1], goal, 1, max_iter=4)
        assert (r["iters"] >= 1).all()
    assert np.abs(r["Jout"][:, 1:]).max() > 0                         # (what the intake's rows now hold behind element 0)
    s.load_problems(slots, stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    after = refill_snapshot(s)
    for slot in slots:                                               # tests/test_refill.py test_refill_leaves_every_other_slot_byte_identical, the refilled slots
        assert after["iter"][slot] == 1 and after["done"][slot] == 0 and after["pw"][slot] == 0 and after["cur"][slot] == 0, (case["key"], slot)
        assert not after["Jout"][slot][1:].any() and not after["alphaOut"][slot][1:].any() and after["alphaOut"][slot][0] == -1, (case["key"], slot)
        for k in ("P", "Pp", "p", "pp", "KT", "dcur", "du"):
            assert not after[k][slot].any(), (case["key"], "slot", slot, k)
    run_until_done(s)
    assert_slots_equal_fresh(s, slots, refs, "%s after cycles of named slots" % case["key"])
    s.close()


# ---------------------------------------------------------------------------------------------------------------- 8: the warm-start refusal and partial clears
@pytest.mark.gpu
def test_partial_clear_does_not_lift_the_warm_start_refusal():
    plant, dt_code, kw = CYCLE_CASES["arm-f32"]
    x0, u0, xg, goals = cycle_seed(plant, kw, np.float32)
    s = make_solver("hip", plant, dtype=dt_code, batch=CYC_B, boundary_cost_to_go_only=1, **dict(kw, mpc_mode=0))
    plan = s.solve(x0, u0, xg)["x"]                                  # sweeps that leave the interior cost-to-go slots unwritten
    xa = np.ascontiguousarray(plan[:, 1])
    with pytest.raises(pyddp.PddpError, match="boundary_cost_to_go_only"):
        s.mpc_solve_problems([1], xa[[1]], goals[0][[1]], 1, clear_vars=0, max_iter=4)
    s.mpc_solve_problems([0], xa[[0]], goals[0][[0]], 1, clear_vars=1, max_iter=4)      # clears slot 0 and nothing else
    for call in (s.mpc_solve_problems, s.mpc_load_problems):
        with pytest.raises(pyddp.PddpError, match="named slots"):
            call([1], xa[[1]], goals[0][[1]], 1, clear_vars=0)
    s.mpc_solve(xa, goals[0], 1, clear_vars=1, max_iter=4)           # the whole handle cleared: every slot's cost-to-go is written from here on
    r = s.mpc_solve_problems([1], s.store_problems([1], only=("x",))["x"][:, 1], goals[0][[1]], 1, clear_vars=0, max_iter=4)
    assert (r["iters"] >= 1).all()
    s.close()
