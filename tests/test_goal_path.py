"""Goal paths of the pendulum, cart-pole and quadrotor: pddp_reserve_goal_path / pddp_goal_path_capacity / pddp_set_goal_path_problems /
pddp_set_goal_path_cursor_problems / pddp_get_goal_path_problems (csrc/goal_path_table.hpp, k_goal_window in csrc/kernels.hpp).

A problem with a path keeps path[len][n], a mode and a cursor on the device; its block of the goal trajectory table always holds the window at the cursor, and every call
that shifts the previous solution moves the cursor on by its shift.

The yardstick is the library's own goal trajectory feature (tests/test_goal_trajectory.py): a TWIN handle of the same configuration for which the test writes each cycle's
window -- the NumPy statement window() below -- with pddp_set_goal_trajectory_problems before the cycle.  Everything is compared bit for bit; no tolerance anywhere.
window() itself is held against the output of tests/native/goal_path_host_check.cpp, which runs the C++ index functions the kernel uses.

Shapes: N = 8, M = 2, A = 4, max_iter 4, batch 5, capacity 37; all three plants, both element types, one pinned selection per plant (those tests/test_goal_trajectory.py
pins for its oracle cases; at A = 4 a selection with cf_fp = cf resolves to the thread-serial rollouts) and the library's own choice.  Path rows are seeded random
offsets around the problem's goal and pairwise distinct, so a window that was not advanced, or advanced wrongly, changes bits.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyddp
from backends import make_solver
from test_goal_trajectory import (ARRAYS, BUILTIN, DIMS, STATE_ALL, UNTOUCHED, base_kw, collect, family, np_type, problems, reset_like_fresh, snapshot, stack, state_rows,
                                  trajectory)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, A, MAX_ITER, B, CAP = 8, 2, 4, 4, 5, 37
HOLD, WRAP = 1, 2
EINVAL = -1
SHIFTS = (0, 1, 3, N - 2)
ENTRY_POINTS = ("pddp_reserve_goal_path", "pddp_goal_path_capacity", "pddp_set_goal_path_problems", "pddp_set_goal_path_cursor_problems", "pddp_get_goal_path_problems")
PINNED = {1: "pend-ts", 2: "cart-cf-gl-kb16", 3: "quad-mq-fused-cf-kb16"}
OUT = ("x", "u", "KT", "Jout", "alphaOut", "success", "iters")
CASES = [pytest.param(plant, pinned, dtype, id="%s-%s-%s" % (PINNED[plant].split("-")[0], "pinned" if pinned else "own", "f32" if dtype == 0 else "f64"))
         for plant in (1, 2, 3) for pinned in (True, False) for dtype in (0, 1)]


# ---------------------------------------------------------------------------------------------------------------- the statement
def window(path, ln, mode, cursor, n_knots):
    """the goals of the horizon's knots: row min(cursor + k, len - 1) (hold) or (cursor + k) % len (wrap) of path[:len]"""
    k = cursor + np.arange(n_knots)
    return path[np.minimum(k, ln - 1) if mode == HOLD else k % ln]


def advance(cursor, s, ln, mode):
    return min(cursor + s, ln - 1) if mode == HOLD else (cursor + s) % ln


class Model:
    """what the test expects a handle's paths to be: per problem (rows [len][n], mode, cursor)"""

    def __init__(self):
        self.p = {}

    def set(self, q, rows, mode, cursor=0):
        self.p[q] = [rows, mode, cursor]

    def shift(self, q, s):
        if q in self.p:
            rows, mode, cur = self.p[q]
            self.p[q][2] = advance(cur, s, len(rows), mode)

    def window(self, q):
        rows, mode, cur = self.p[q]
        return window(rows, len(rows), mode, cur, N)


def make(plant, pinned, dtype, batch=B, use_graph=1, **more):
    fam = family(PINNED[plant])
    kw = base_kw(plant, N, M, A, fam["kw"]["integrator"], max_iter=MAX_ITER, tol_cost=0.0, **more)
    if pinned:
        kw["kernels"] = dict(fam["sel"])
    return make_solver("hip", plant, dtype=dtype, batch=batch, use_graph=use_graph, **kw)


def path_rows(plant, dtype, prob, ln, seed):
    """[ln][n] in the element type: the problem's goal plus seeded offsets, pairwise distinct rows"""
    n = DIMS[plant][1]
    rng = np.random.default_rng(77 * plant + 1000 * seed + ln)
    rows = (prob["xg"].astype(np.float64)[None, :] + rng.normal(0, 0.05, (ln, n))).astype(np_type(dtype))
    assert len({r.tobytes() for r in rows}) == ln
    return rows


def set_path(s, model, q, rows, mode, cursor=0):
    s.set_goal_path_problems([q], rows[None], mode, [cursor])
    model.set(q, rows, mode, cursor)


def check_paths(s, model, label):
    """the getters against the model, for every problem of the handle"""
    nb = s.cfg.batch
    ln, mode, cur, rows = s.get_goal_path_problems(list(range(nb)))
    G, has = s.get_goal_trajectory_problems(list(range(nb)))
    assert rows.shape == (nb, CAP, s.n) and rows.dtype == s.dtype
    for q in range(nb):
        if q in model.p:
            want, m, c = model.p[q]
            assert (ln[q], mode[q], cur[q]) == (len(want), m, c), (label, q, ln[q], mode[q], cur[q], len(want), m, c)
            assert np.array_equal(rows[q, :len(want)], want) and not rows[q, len(want):].any(), (label, q, "rows")
            assert has[q] == 1 and np.array_equal(G[q], model.window(q)), (label, q, "window")
        else:
            assert (ln[q], mode[q], cur[q]) == (0, 0, 0) and not rows[q].any(), (label, q)
    return G, has


def arrays_of(s):
    out = {k: s.get(k).copy() for k in ARRAYS}
    out.update(state_rows(s, range(s.cfg.batch)))
    return out


def assert_same(a, b, label):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (label, k)


# ---------------------------------------------------------------------------------------------------------------- CPU 1: the surface
def test_entry_points_are_exported_declared_and_bound():
    lib = C.CDLL(pyddp.library_path())
    header = open(os.path.join(ROOT, "include", "pddp.h")).read()
    for sym in ENTRY_POINTS:
        assert getattr(lib, sym) is not None
    assert "#define PDDP_GOAL_PATH_HOLD 1" in header and "#define PDDP_GOAL_PATH_WRAP 2" in header
    assert "int pddp_reserve_goal_path(pddp_handle h, int capacity);" in header
    assert "int pddp_goal_path_capacity(pddp_handle h);" in header
    assert "int pddp_set_goal_path_problems(pddp_handle h, int count, const int* idx, int len, int mode," in header
    assert "int pddp_set_goal_path_cursor_problems(pddp_handle h, int count, const int* idx, const int* cursor);" in header
    assert "int pddp_get_goal_path_problems(pddp_handle h, int count, const int* idx, int* len, int* mode, int* cursor," in header
    for name in ("reserve_goal_path", "goal_path_capacity", "set_goal_path_problems", "set_goal_path_cursor_problems", "get_goal_path_problems"):
        assert callable(getattr(pyddp.Solver, name))
    assert (pyddp.Solver.GOAL_PATH_HOLD, pyddp.Solver.GOAL_PATH_WRAP) == (HOLD, WRAP)


# ---------------------------------------------------------------------------------------------------------------- CPU 2, 3: the host-only code under the sanitizers
_HOST = {}


def host_check_output(tmp_path_factory):
    if "out" not in _HOST:
        exe = str(tmp_path_factory.mktemp("goal_path") / "goal_path_host_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                               os.path.join(ROOT, "tests", "native", "goal_path_host_check.cpp"), "-o", exe])
        _HOST["out"] = subprocess.run([exe], capture_output=True, text=True)
    return _HOST["out"]


def test_host_only_code_as_a_stand_alone_program(tmp_path_factory):
    """tests/native/goal_path_host_check.cpp (its own main, -fsanitize=address,undefined): every refusal on exactly-sized buffers, goal_path_row / goal_path_advance
    against a brute-force walk for len 1..9, every cursor, k and s in 0..20, both modes, and a kernel-shaped loop that windows with them"""
    out = host_check_output(tmp_path_factory)
    assert out.returncode == 0 and "goal_path_host_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_numpy_statement_of_the_window_is_the_programs(tmp_path_factory):
    """window() / advance() of this file against the rows the stand-alone program's kernel-shaped loop produced with the C++ index functions"""
    out = host_check_output(tmp_path_factory)
    lines = [l for l in out.stdout.splitlines() if l.startswith("window ")]
    assert len(lines) == 2 * 4 * 3 * 4
    seen = set()
    for line in lines:
        head, rows = line.split("|")
        args, cur_after = head.split(":")
        ln, mode, cursor, shift, n_knots = (int(v) for v in args.split()[1:])
        c = advance(cursor, shift, ln, mode)
        assert c == int(cur_after), line
        assert window(np.arange(ln), ln, mode, c, n_knots).tolist() == [int(v) for v in rows.split()], line
        seen.add((ln, mode))
    assert seen == {(ln, mode) for ln in (1, 3, 8, 37) for mode in (HOLD, WRAP)}


# ---------------------------------------------------------------------------------------------------------------- GPU 1: the window is the definition
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("plant", [1, 2, 3], ids=["pend", "cart", "quad"])
def test_the_window_is_the_definition(plant, dtype):
    """problems 2 and 0 carry paths of every shape in turn (len 1, 3 < N, N, capacity; cursors up to len - 1); after the setter, a cursor call, a pddp_mpc_solve and a
    pddp_mpc_load the getters return the model's rows, records and windows.  Problem 3 (a plain trajectory) and problem 4 (none) keep rows, flag and xGoal."""
    probs = problems(plant, N, dtype, B)
    s = make(plant, False, dtype)
    assert s.goal_path_capacity() == 0
    s.reserve_goal_path(CAP)
    assert s.goal_path_capacity() == CAP
    plain = trajectory(plant, N, dtype, probs[3], 3)
    s.set_goal_trajectory_problems([3], plain)
    seed = s.solve(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"))
    xg = stack(probs, "xg").reshape(B, -1)
    model = Model()
    shapes = [(1, HOLD, 0, 0), (1, WRAP, 0, 0), (3, WRAP, 2, 1), (3, HOLD, 1, 0), (N, HOLD, N - 1, 2), (N, WRAP, 0, N - 1), (CAP, HOLD, CAP - 1, CAP - 3), (CAP, WRAP, 30, CAP - 1)]
    saturated = lapped = False
    for j, (ln, mode, c2, c0) in enumerate(shapes):
        label = (plant, dtype, ln, mode)
        rows = np.stack([path_rows(plant, dtype, probs[2], ln, j), path_rows(plant, dtype, probs[0], ln, 50 + j)])
        s.set_goal_path_problems([2, 0], rows, mode, [c2, c0])
        model.set(2, rows[0], mode, c2); model.set(0, rows[1], mode, c0)
        check_paths(s, model, (label, "setter"))
        new = [(c2 + 1) % ln, ln - 1]
        s.set_goal_path_cursor_problems([0, 2], new)
        model.p[0][2], model.p[2][2] = new
        check_paths(s, model, (label, "cursor call"))
        for call, shifts in (("solve", [3, 0, 1, 1, N - 2]), ("load", [N - 2, 1, 3, 0, 0])):
            before = {q: model.p[q][2] for q in model.p}
            if call == "solve":
                s.mpc_solve(seed["x"][:, 1].copy(), xg, shifts, clear_vars=j % 2, max_iter=2)
            else:
                s.mpc_load(seed["x"][:, 2].copy(), xg, shifts, clear_vars=0)
            for q in range(B):
                model.shift(q, shifts[q])
            for q in model.p:
                raw = before[q] + shifts[q]
                saturated |= mode == HOLD and raw > ln - 1 and model.p[q][2] == ln - 1
                lapped |= mode == WRAP and raw >= ln and model.p[q][2] == raw % ln
            G, has = check_paths(s, model, (label, call))
            assert has.tolist() == [1, 0, 1, 1, 0] and np.array_equal(G[3], plain), (label, call, "the plain trajectory")
            assert np.array_equal(G[4], np.tile(xg[4], (N, 1))) and np.array_equal(G[1], np.tile(xg[1], (N, 1))), (label, call)
            assert np.array_equal(s.get("xGoal").reshape(B, -1), xg), (label, call, "xGoal")
    assert saturated and lapped
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 2: cycles equal the caller-written window
def mixed_batch(plant, dtype, probs):
    """problems 0, 1: HOLD paths (1 runs past its end within three cycles), 2: a WRAP path shorter than N, 3: a plain trajectory, 4: none"""
    return {0: (path_rows(plant, dtype, probs[0], 30, 1), HOLD, 4), 1: (path_rows(plant, dtype, probs[1], 5, 2), HOLD, 2), 2: (path_rows(plant, dtype, probs[2], 3, 3), WRAP, 1)}


def path_handle_and_twin(plant, pinned, dtype, probs, layout, plain_slot=3, batch=B, use_graph=1):
    s, twin, model = make(plant, pinned, dtype, batch, use_graph), make(plant, pinned, dtype, batch, use_graph), Model()
    s.reserve_goal_path(CAP)
    for q, (rows, mode, cur) in layout.items():
        set_path(s, model, q, rows, mode, cur)
    plain = trajectory(plant, N, dtype, probs[plain_slot], plain_slot)
    s.set_goal_trajectory_problems([plain_slot], plain)
    twin.set_goal_trajectory_problems([plain_slot], plain)
    write_windows(twin, model)
    return s, twin, model


def write_windows(twin, model, only=None):
    named = sorted(model.p if only is None else [q for q in only if q in model.p], reverse=True)      # (unsorted on purpose)
    if named:
        twin.set_goal_trajectory_problems(named, np.stack([model.window(q) for q in named]))


CYCLES = [([1, 3, N - 2, 0, 1], 0), ([3, N - 2, 1, 1, 0], 1), ([1, 0, 1, N - 2, 3], 0)]      # per-problem shifts, clear_vars


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["solve", "load"])
@pytest.mark.parametrize("plant,pinned,dtype", CASES)
def test_cycles_equal_the_caller_written_window(plant, pinned, dtype, stage):
    """a path handle against its twin over a seed solve and three control cycles (pddp_mpc_solve, or pddp_mpc_load alone): outputs, state records and every array bit for bit"""
    probs = problems(plant, N, dtype, B)
    s, twin, model = path_handle_and_twin(plant, pinned, dtype, probs, mixed_batch(plant, dtype, probs))
    xg = stack(probs, "xg").reshape(B, -1)
    a, b = (h.solve(stack(probs, "x0"), stack(probs, "u0"), xg.ravel()) for h in (s, twin))
    for k in ("x", "u", "Jout", "alphaOut"):
        assert np.array_equal(a[k], b[k], equal_nan=True), ("seed solve", k)
    assert_same(arrays_of(s), arrays_of(twin), "seed solve")
    xa = a["x"][:, 1].copy()
    windows = []
    for c, (shifts, clear_vars) in enumerate(CYCLES):
        for q in range(B):
            model.shift(q, shifts[q])
        write_windows(twin, model)                                   # today's way: the caller uploads the new window
        if stage == "solve":
            a, b = (h.mpc_solve(xa, xg, shifts, clear_vars=clear_vars, max_iter=MAX_ITER) for h in (s, twin))
            for k in OUT:
                assert np.array_equal(a[k], b[k], equal_nan=True), ("cycle", c, k)
            xa = a["x"][:, 1].copy()
        else:
            for h in (s, twin):
                h.mpc_load(xa, xg, shifts, clear_vars=clear_vars)
            xa = s.get("xb").reshape(B, 2, N, -1)[:, 0, 1].copy()
        assert_same(arrays_of(s), arrays_of(twin), ("cycle", c))
        G, has = check_paths(s, model, ("cycle", c))
        Gt, hast = twin.get_goal_trajectory_problems(list(range(B)))
        assert np.array_equal(G, Gt) and has.tolist() == hast.tolist() == [1, 1, 1, 1, 0]
        windows.append(G[:3].copy())
    assert model.p[1][2] == 4 and model.p[0][2] == 4 + sum(sh[0] for sh, _ in CYCLES)      # problem 1 ran past its end and is held there
    assert not np.array_equal(windows[0], windows[1]) and not np.array_equal(windows[1], windows[2])
    s.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 3: named slots
def path_snapshot(s):
    nb = s.cfg.batch
    snap = snapshot(s)
    ln, mode, cur, rows = s.get_goal_path_problems(list(range(nb)))
    G, has = s.get_goal_trajectory_problems(list(range(nb)))
    snap.update(path_len=ln, path_mode=mode, path_cursor=cur, path_rows=rows.reshape(nb, -1), window=G.reshape(nb, -1), has=has, cost_row=s.get_diag_cost_problems(list(range(nb))))
    return snap


@pytest.mark.gpu
@pytest.mark.parametrize("plant,pinned,dtype", CASES)
def test_named_slot_cycles_advance_their_slots_only(plant, pinned, dtype):
    """pddp_mpc_solve_problems / pddp_mpc_load_problems on slots {3, 0} of a path handle against the whole-handle twin's rows of those slots; the other slots' arrays,
    state, cursor, window and cost row unchanged; pddp_load_problems of a slot with a path loads against the window at its cursor and leaves it there"""
    probs = problems(plant, N, dtype, B)
    layout = {0: (path_rows(plant, dtype, probs[0], 30, 1), HOLD, 4), 1: (path_rows(plant, dtype, probs[1], 9, 2), WRAP, 7), 3: (path_rows(plant, dtype, probs[3], 3, 3), WRAP, 1)}
    s, twin, model = path_handle_and_twin(plant, pinned, dtype, probs, layout, plain_slot=2)
    xg = stack(probs, "xg").reshape(B, -1)
    seed = s.solve(stack(probs, "x0"), stack(probs, "u0"), xg.ravel())
    twin.solve(stack(probs, "x0"), stack(probs, "u0"), xg.ravel())
    named, others = [3, 0], [1, 2, 4]
    xa = seed["x"][:, 1].copy()
    for c, (shifts, clear_vars) in enumerate([([N - 2, 3], 0), ([1, 0], 1), ([3, N - 2], 0)]):
        before = path_snapshot(s)
        whole = [0] * B
        for q, sh in zip(named, shifts):
            model.shift(q, sh); whole[q] = sh
        write_windows(twin, model, named)
        got = s.mpc_solve_problems(named, xa[named], xg[named], shifts, clear_vars=clear_vars, max_iter=MAX_ITER)
        ref = twin.mpc_solve(xa, xg, whole, clear_vars=clear_vars, max_iter=MAX_ITER)
        for k in OUT:
            assert np.array_equal(got[k], ref[k][named], equal_nan=True), ("cycle", c, k)
        after = path_snapshot(s)
        for k in before:
            assert np.array_equal(np.asarray(before[k])[others], np.asarray(after[k])[others], equal_nan=True), ("cycle", c, "another slot changed", k)
        check_paths(s, model, ("named cycle", c))
        xa = xa.copy(); xa[named] = got["x"][:, 1]
    # the load stage alone advances too
    before = path_snapshot(s)
    s.mpc_load_problems([0], xa[[0]], xg[[0]], [1])
    model.shift(0, 1)
    check_paths(s, model, "pddp_mpc_load_problems")
    after = path_snapshot(s)
    for k in before:
        assert np.array_equal(np.asarray(before[k])[[1, 2, 3, 4]], np.asarray(after[k])[[1, 2, 3, 4]], equal_nan=True), ("pddp_mpc_load_problems: another slot changed", k)
    # a refill of slot 1: against the window at its cursor, which stays
    write_windows(twin, model, [1])
    late = problems(plant, N, dtype, 1, skip=11)
    for h in (s, twin):
        h.load_problems([1], stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    check_paths(s, model, "pddp_load_problems")
    for k in ("g", "H", "ucur", "Jout", "xGoal"):
        assert np.array_equal(s.get(k).reshape(B, -1)[1], twin.get(k).reshape(B, -1)[1], equal_nan=True), ("refill", k)
    assert np.array_equal(s.get("xb").reshape(B, 2, -1)[1, 0], twin.get("xb").reshape(B, 2, -1)[1, 0]), ("refill", "xb")      # (a refill writes half 0, the fresh state's)
    plainer = make(plant, pinned, dtype)                              # the window matters: the same refill without a trajectory gives another gradient
    plainer.solve(stack(probs, "x0"), stack(probs, "u0"), xg.ravel())
    plainer.load_problems([1], stack(late, "x0"), stack(late, "u0"), stack(late, "xg"))
    assert not np.array_equal(plainer.get("g").reshape(B, -1)[1], s.get("g").reshape(B, -1)[1])
    for h in (s, twin, plainer):
        h.close()


@pytest.mark.gpu
def test_named_slot_cycles_across_the_256_slot_chunks():
    """batch 300 (pendulum, float32), every problem on a path, 260 named slots in shuffled order with per-slot shifts: two chunks of the intake area"""
    plant, dtype, nb, count = 1, 0, 300, 260
    base = problems(plant, N, dtype, 5)
    probs = [base[q % 5] for q in range(nb)]
    rng = np.random.default_rng(9)
    s, twin, model = make(plant, False, dtype, nb), make(plant, False, dtype, nb), Model()
    s.reserve_goal_path(CAP)
    for mode, ln, qs in ((HOLD, CAP, list(range(0, nb, 2))), (WRAP, 5, list(range(1, nb, 2)))):
        rows = (np.stack([probs[q]["xg"] for q in qs])[:, None, :].astype(np.float64) + rng.normal(0, 0.05, (len(qs), ln, 2))).astype(np.float32)
        cur = rng.integers(0, ln, len(qs))
        s.set_goal_path_problems(qs, rows, mode, cur)
        for i, q in enumerate(qs):
            model.set(q, rows[i], mode, int(cur[i]))
    write_windows(twin, model)
    xg = stack(probs, "xg").reshape(nb, -1)
    seed = s.solve(stack(probs, "x0"), stack(probs, "u0"), xg.ravel())
    twin.solve(stack(probs, "x0"), stack(probs, "u0"), xg.ravel())
    named = rng.permutation(nb)[:count].tolist()
    others = sorted(set(range(nb)) - set(named))
    shifts = rng.choice(SHIFTS, count).tolist()
    before = path_snapshot(s)
    whole = [0] * nb
    for q, sh in zip(named, shifts):
        model.shift(q, sh); whole[q] = sh
    write_windows(twin, model, named)
    xa = seed["x"][:, 1].copy()
    got = s.mpc_solve_problems(named, xa[named], xg[named], shifts, max_iter=MAX_ITER)
    ref = twin.mpc_solve(xa, xg, whole, max_iter=MAX_ITER)
    for k in OUT:
        assert np.array_equal(got[k], ref[k][named], equal_nan=True), k
    after = path_snapshot(s)
    for k in before:
        assert np.array_equal(np.asarray(before[k])[others], np.asarray(after[k])[others], equal_nan=True), ("another slot changed", k)
    check_paths(s, model, "260 named slots")
    assert sum(int(before["path_cursor"][q] != after["path_cursor"][q]) for q in named) > 100
    s.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 4: setter semantics and refusals
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_setter_semantics_and_refusals(dtype):
    plant, n = 2, 4
    T = np_type(dtype)
    probs = problems(plant, N, dtype, B)
    xg = stack(probs, "xg").reshape(B, n)
    s = make(plant, True, dtype)
    lib = s.lib
    lib.pddp_reserve_goal_path.argtypes = [C.c_void_p, C.c_int]
    lib.pddp_set_goal_path_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_set_goal_path_cursor_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_get_goal_path_problems.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    idx2, rows2, cur2 = np.array([3, 0], np.int32), np.stack([path_rows(plant, dtype, probs[3], 4, 1), path_rows(plant, dtype, probs[0], 4, 2)]), np.array([3, 0], np.int32)
    three = [np.zeros(2, np.int32) for _ in range(3)]
    # no reserve: refused, and the handle has no table
    assert lib.pddp_set_goal_path_problems(s.h, 2, ptr(idx2), 4, HOLD, ptr(cur2), ptr(rows2)) == EINVAL
    assert lib.pddp_set_goal_path_cursor_problems(s.h, 2, ptr(idx2), ptr(cur2)) == EINVAL
    assert lib.pddp_get_goal_path_problems(s.h, 2, ptr(idx2), *(ptr(a) for a in three), None) == EINVAL
    for cap in (0, -1, 2 ** 31 - N, 2 ** 31 - 1):
        assert lib.pddp_reserve_goal_path(s.h, cap) == EINVAL, cap
    assert s.goal_path_capacity() == 0
    assert np.array_equal(s.get_diag_cost_problems([0]), np.asarray(BUILTIN[plant], T).astype(np.float64)[None])
    s.solve(stack(probs, "x0"), stack(probs, "u0"), xg.ravel())
    assert s.get_goal_trajectory_problems([0, 1])[1].tolist() == [0, 0]
    # reserve twice
    s.reserve_goal_path(CAP); s.reserve_goal_path(CAP)
    assert lib.pddp_reserve_goal_path(s.h, CAP - 1) == EINVAL and lib.pddp_reserve_goal_path(s.h, CAP + 1) == EINVAL and s.goal_path_capacity() == CAP
    model = Model()
    check_paths(s, model, "after the reserve")
    # the setter changes nothing already in a slot
    before = snapshot(s)
    s.set_goal_path_problems(idx2, rows2, HOLD, cur2)
    model.set(3, rows2[0], HOLD, 3); model.set(0, rows2[1], HOLD, 0)
    set_path(s, model, 1, path_rows(plant, dtype, probs[1], CAP, 3), WRAP, CAP - 1)
    plain = trajectory(plant, N, dtype, probs[2], 2)
    s.set_goal_trajectory_problems([2], plain)
    after = snapshot(s)
    for k in UNTOUCHED + STATE_ALL:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), ("the setter changed", k)
    check_paths(s, model, "setters")

    def bad_at(e, v):
        a = rows2.copy().ravel(); a[e] = v
        return a

    too_long = np.zeros((2, CAP + 1, n), T)
    bad_set = [("count 0", 0, idx2, 4, HOLD, cur2, rows2), ("count < 0", -2, idx2, 4, HOLD, cur2, rows2), ("idx null", 2, None, 4, HOLD, cur2, rows2),
               ("path null", 2, idx2, 4, HOLD, cur2, None), ("index == batch", 2, np.array([0, B], np.int32), 4, HOLD, cur2, rows2),
               ("index < 0", 2, np.array([-1, 2], np.int32), 4, HOLD, cur2, rows2), ("index twice", 2, np.array([2, 2], np.int32), 4, HOLD, cur2, rows2),
               ("len 0", 2, idx2, 0, HOLD, None, rows2), ("len < 0", 2, idx2, -4, HOLD, None, rows2), ("len > capacity", 2, idx2, CAP + 1, HOLD, None, too_long),
               ("mode 0", 2, idx2, 4, 0, cur2, rows2), ("mode 3", 2, idx2, 4, 3, cur2, rows2), ("cursor == len", 2, idx2, 4, WRAP, np.array([0, 4], np.int32), rows2),
               ("cursor < 0", 2, idx2, 4, HOLD, np.array([-1, 0], np.int32), rows2), ("nan", 2, idx2, 4, HOLD, cur2, bad_at(4 * n + 1, np.nan)),
               ("inf", 2, idx2, 4, HOLD, cur2, bad_at(8 * n - 1, np.inf)), ("-inf", 2, idx2, 4, HOLD, cur2, bad_at(0, -np.inf))]
    bad_cur = [("count 0", 0, idx2, cur2), ("idx null", 2, None, cur2), ("cursor null", 2, idx2, None), ("index == batch", 2, np.array([0, B], np.int32), cur2),
               ("index twice", 2, np.array([3, 3], np.int32), cur2), ("no path", 2, np.array([3, 4], np.int32), np.zeros(2, np.int32)),
               ("a plain trajectory", 1, np.array([2], np.int32), np.zeros(1, np.int32)), ("cursor == len", 2, idx2, np.array([4, 0], np.int32)),
               ("cursor < 0", 2, idx2, np.array([0, -1], np.int32))]
    before = path_snapshot(s)
    for what, count, idx, ln, mode, cur, rows in bad_set:
        assert lib.pddp_set_goal_path_problems(s.h, count, ptr(idx), ln, mode, ptr(cur), ptr(rows)) == EINVAL, what
    for what, count, idx, cur in bad_cur:
        assert lib.pddp_set_goal_path_cursor_problems(s.h, count, ptr(idx), ptr(cur)) == EINVAL, what
    for what, count, idx in (("count 0", 0, idx2), ("idx null", 2, None), ("index == batch", 2, np.array([0, B], np.int32)), ("index twice", 2, np.array([1, 1], np.int32))):
        assert lib.pddp_get_goal_path_problems(s.h, count, ptr(idx), *(ptr(a) for a in three), None) == EINVAL, what
    # a refused cycle advances nothing
    xa = s.get("xb").reshape(B, 2, N, n)[:, 0, 1].copy()
    with pytest.raises(pyddp.PddpError):
        s.mpc_solve(xa, xg, [1, 1, N - 1, 1, 1])
    with pytest.raises(pyddp.PddpError):
        s.mpc_load(xa, xg, [1, -1, 1, 1, 1])
    with pytest.raises(pyddp.PddpError):
        s.mpc_solve(xa, xg, 1, max_iter=MAX_ITER + 1)
    with pytest.raises(pyddp.PddpError):
        s.mpc_solve_problems([3, 0], xa[[3, 0]], xg[[3, 0]], [1, N - 1])
    with pytest.raises(pyddp.PddpError):
        s.mpc_load_problems([3, 3], xa[[3, 3]], xg[[3, 3]], [1, 1])
    after = path_snapshot(s)
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), ("a refused call changed", k)
    check_paths(s, model, "refused calls")
    # the binding refuses wrong dtypes and shapes before the call
    other = np.float64 if dtype == 0 else np.float32
    for rows in (rows2.astype(other), rows2.tolist(), rows2.reshape(2, -1), rows2[:1], rows2[:, :, :n - 1]):
        with pytest.raises(pyddp.PddpError):
            s.set_goal_path_problems(idx2, rows, HOLD)
    with pytest.raises(pyddp.PddpError):
        s.set_goal_path_problems(idx2, rows2, HOLD, [0])
    with pytest.raises(pyddp.PddpError):
        s.set_goal_path_cursor_problems(idx2, [0, 0, 0])
    check_paths(s, model, "refused by the binding")
    # len, mode, cursor and path may be NULL
    assert lib.pddp_get_goal_path_problems(s.h, 2, ptr(idx2), None, None, ptr(three[2]), None) == 0 and three[2].tolist() == [3, 0]
    # the trajectory setter and the clear call turn a path off; cycles then leave those rows alone
    s.set_goal_trajectory_problems([3], plain)
    s.clear_goal_trajectory_problems([1])
    del model.p[3], model.p[1]
    G, has = check_paths(s, model, "paths turned off")
    assert has.tolist() == [1, 0, 1, 1, 0] and np.array_equal(G[3], plain) and np.array_equal(G[1], np.tile(xg[1], (N, 1)))
    s.mpc_solve(xa, xg, [3, 3, 3, 3, 3], max_iter=2)
    model.shift(0, 3)
    G, has = check_paths(s, model, "a cycle after paths were turned off")
    assert has.tolist() == [1, 0, 1, 1, 0] and np.array_equal(G[3], plain) and np.array_equal(G[2], plain)
    # ... and a path can come back
    set_path(s, model, 1, path_rows(plant, dtype, probs[1], 2, 9), WRAP, 1)
    check_paths(s, model, "a path again")
    s.close()


@pytest.mark.gpu
def test_arm_handles_refuse_all_five():
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    arm = make_solver("hip", 4, dtype=0, batch=2, N=32, M=4, A=8, wafr_urdf=1, total_time=0.5)
    lib = arm.lib
    lib.pddp_reserve_goal_path.argtypes = [C.c_void_p, C.c_int]
    lib.pddp_goal_path_capacity.argtypes = [C.c_void_p]
    lib.pddp_set_goal_path_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_set_goal_path_cursor_problems.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.pddp_get_goal_path_problems.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    idx, cur, rows = np.array([0, 1], np.int32), np.zeros(2, np.int32), np.zeros((2, 4, 14), np.float32)
    out = [np.zeros(2, np.int32) for _ in range(3)]
    assert lib.pddp_reserve_goal_path(arm.h, CAP) == EINVAL
    assert lib.pddp_goal_path_capacity(arm.h) == EINVAL
    assert lib.pddp_set_goal_path_problems(arm.h, 2, ptr(idx), 4, HOLD, ptr(cur), ptr(rows)) == EINVAL
    assert lib.pddp_set_goal_path_cursor_problems(arm.h, 2, ptr(idx), ptr(cur)) == EINVAL
    assert lib.pddp_get_goal_path_problems(arm.h, 2, ptr(idx), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(rows)) == EINVAL
    assert not any(a.any() for a in out) and not rows.any()
    arm.close()


# ---------------------------------------------------------------------------------------------------------------- GPU 5: the captured graph
@pytest.mark.gpu
@pytest.mark.parametrize("plant", [1, 2, 3], ids=[PINNED[p] for p in (1, 2, 3)])
def test_graph_replay_reads_the_rematerialised_window(plant):
    """use_graph = 1 against use_graph = 0: load and iterate (the graph is captured), setter, iterate; cursor call, reload, iterate -- the same bits each time.  The
    window is rewritten in place, behind the pointers the captured graph holds."""
    dtype = 0
    probs = problems(plant, N, dtype, B)
    rows = path_rows(plant, dtype, probs[1], 20, 4)
    outs = []
    for use_graph in (1, 0):
        s = make(plant, True, dtype, use_graph=use_graph)
        s.reserve_goal_path(CAP)
        stages = []
        reset_like_fresh(s)
        s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
        s.iterate(1); s.sync()
        stages.append(collect(s))
        s.set_goal_path_problems([1], rows[None], HOLD, [2])
        s.iterate(2); s.sync()
        stages.append(collect(s))
        for cursor in (2, 11):
            s.set_goal_path_cursor_problems([1], [cursor])
            reset_like_fresh(s)
            s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=1)
            s.iterate(2); s.iterate(1); s.sync()
            stages.append(collect(s))
        outs.append(stages)
        s.close()
    graph, plain = outs
    for i in range(4):
        for k in plain[i]:
            assert np.array_equal(np.asarray(graph[i][k]), np.asarray(plain[i][k]), equal_nan=True), (plant, "stage", i, k)
    assert not np.array_equal(plain[2]["Jout"][1], plain[3]["Jout"][1]), "the window changed nothing"
    assert np.array_equal(plain[2]["Jout"][0], plain[3]["Jout"][0])


# ---------------------------------------------------------------------------------------------------------------- GPU 6: a handle that never reserves
@pytest.mark.gpu
@pytest.mark.parametrize("plant,pinned,dtype", CASES)
def test_a_handle_that_never_reserves_and_one_without_paths(plant, pinned, dtype):
    """without a reserve the getters answer as they always did (no table: xGoal rows, flag 0, the built-in cost record) through a seed solve and two cycles; a handle
    that reserved and set no path runs the same cycles to the same bits"""
    probs = problems(plant, N, dtype, B)
    xg = stack(probs, "xg").reshape(B, -1)
    never, empty = make(plant, pinned, dtype), make(plant, pinned, dtype)
    empty.reserve_goal_path(CAP)
    res = []
    for h in (never, empty):
        out = [h.solve(stack(probs, "x0"), stack(probs, "u0"), xg.ravel())]
        xa = out[0]["x"][:, 1].copy()
        for shifts, clear_vars in CYCLES[:2]:
            out.append(h.mpc_solve(xa, xg, shifts, clear_vars=clear_vars, max_iter=MAX_ITER))
            xa = out[-1]["x"][:, 1].copy()
        res.append((out, arrays_of(h)))
    for a, b in zip(res[0][0], res[1][0]):
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    assert_same(res[0][1], res[1][1], "arrays")
    G, has = never.get_goal_trajectory_problems(list(range(B)))
    assert has.tolist() == [0] * B and np.array_equal(G, np.repeat(xg[:, None, :], N, axis=1))
    assert np.array_equal(never.get_diag_cost_problems(list(range(B))), np.tile(np.asarray(BUILTIN[plant], np_type(dtype)).astype(np.float64), (B, 1)))
    assert never.goal_path_capacity() == 0 and empty.goal_path_capacity() == CAP
    with pytest.raises(pyddp.PddpError):
        never.get_goal_path_problems([0])
    never.close(); empty.close()
