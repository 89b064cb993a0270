"""Packed kernels held to PER-PROBLEM solver state: batches whose neighbouring problems are in different states.

Every problem of a handle has its own SolverState (done, accepted, win_pending, cur, pw, rho, bp_retries, ignore_defect -- solver_state.hpp) and the kernels branch on it per
problem, while the full-device kernels put several problems into one wavefront or one LDS stage (k_ls_many: 64 problems; k_nis_tl / k_fp_tl: 2 at N = 32, M = 4, A = 8;
k_sweep_maps<4>, k_fp_cf / k_sweep_maps_cf: 4 or 8; k_bp_ts / k_nis_ts / k_fp_ts: 64 / M, 64 / N, 64 / A; k_bp_cl, k_bp_gl<32>, k_nis_kb<16>: 2).  The other whole-solve batch
tests run benign problems with tol_cost = 0 to max_iter: every problem of a wave takes the same branch in every sweep.  Here the neighbours differ.

The scenario (build_scenario) interleaves five kinds of problems so that consecutive indices differ in kind:
  (a) exits by tolerance after few iterations             (an easy goal)
  (b) runs to max_iter
  (c) the line search rejects every candidate at least once (alphaOut == -1, rho raised)
  (d) warm start with a NEGATIVE DEFINITE cost-to-go P0 on the block-boundary slots (the slots a backward pass reads from the previous iteration, M > 1): Huu = R + B' P B + rho
      is not positive until rho has been raised a few times -- the backward pass fails (accepted == -1, bp_retries counts) and the sweep is repeated
  (e) the same with a P0 no rho below the maximum repairs: done == 3 (ignore_max_rho_exit = 0)
The arm's 7 x 7 inversion never reports a failure (the reference's generic invHuu, utils/cudaUtils.h:291; bp_mfma.hpp, bp_lg.hpp), so on the arm a (d) problem shows as
line searches that reject everything until rho is large enough (accepted == 0, bp_retries stays 0) and (e) reaches the maximum rho through rejections; the cart-pole (1 x 1)
and the quadrotor (4 x 4 adjugate, det > 0 test) report the failure and show bp_retries >= 2.  The magnitudes were chosen on the host emulation and the float64 oracle.

What is asserted:
  * THE MIX, from the reference side only (the single-problem solves, traced sweep by sweep with iterate(1); sync(); get_state()): for at least one sweep index every packing
    group of the case with two or more problems holds a problem with accepted == 1, one with accepted == 0 or -1 and one with done != 0; over the run every kind occurs
    (mix_report).  (A group of one problem -- the ragged tail of a launch -- cannot hold two states; it is compared like every other problem.)
  * BATCH == SINGLE-PROBLEM HANDLES ON THE SAME KERNELS, BIT FOR BIT (kernels= pins the selection of both, the names of time_kernels(1) are asserted): the batch runs
    (largest sweep count of any single problem) + 3 sweeps -- a finished problem stays frozen while its wave-mates go on and the graph keeps replaying -- once with
    use_graph = 1 and once with 0; x, u, KT, Jout, alphaOut (the untouched tail included: both sides fill it with a sentinel before the load), dmax, iters, done, rho, drho,
    bp_retries, cur, pw, ignore_defect, accepted and both halves of the cost-to-go double buffer.
  * FLOAT64 AGAINST THE ORACLE (so that batch and single cannot be wrong together): the warm-start-free part of the scenario in one handle, every problem against
    Oracle.run_ilqr_gpusem: identical iters, identical alphaOut up to iters (the -1 entries included), Jout / x / u to 1e-8 of the largest magnitude, exit kind 1 where the
    oracle left by tolerance (DESIGN section 2's bar for whole float64 solves).
"""
import numpy as np
import pytest

from backends import BACKENDS, make_solver
from oracle_binding import Oracle, default_cfg, example_inputs
from test_quad_bench_geometry import PINNED

SENTINEL_J, SENTINEL_A = -7.5, -99          # the untouched tail of Jout / alphaOut
EXTRA_SWEEPS = 3                            # sweeps of the batch after its last problem has exited
DIMS = {2: (2, 4, 1), 3: (6, 12, 4), 4: (7, 14, 7)}      # npos, n, m


# ---------------------------------------------------------------------------------------------------------------- the scenario
def boundary_slots(N, M):
    NB = N // M
    return [k for k in range(N - 1) if (k + 1) % NB == 0]


def make_problem(plant, kw, dtype, kind, noise, goal, c, seed):
    """One problem of the scenario.  noise: scale of the start trajectory's velocity noise; goal: where the goal lies between the start (0) and the example's goal (1; > 1:
    beyond it); c: P0 = -c I on the block-boundary slots (0: no warm start -- zero arrays, the same as a cold start)."""
    N, M = kw["N"], kw["M"]
    npos, n, m = DIMS[plant]
    rng = np.random.default_rng(seed)
    if kw.get("ee_cost"):
        x0 = np.zeros((N, n)); x0[:, 1] = 0.7; x0[:, 3] = -0.8; x0[:, 5] = 0.75          # the MPC example's start (tests/test_ee_thread_lanes.py start())
        x0[:, npos:] = rng.normal(0, noise, (N, npos))
        u0 = np.full((N, m), 0.01)
        tool0, tool1 = np.array([0.0, 0.0, 1.0]), np.array([0.45, 0.15, 0.75])
        xg = np.zeros(n); xg[:3] = tool1 + (goal - 1.0) * (tool1 - tool0)
        x0, u0 = x0.ravel(), u0.ravel()
    else:
        x0, u0, xg = example_inputs(plant, N, np.float64, noise=rng.normal(0, noise, (N, n)))
        start = x0.reshape(N, n)[0, :npos]
        xg = xg.copy(); xg[:npos] = start + goal * (xg[:npos] - start)
    P0 = np.zeros((N, n, n))
    if c:
        P0[boundary_slots(N, M)] = -c * np.eye(n)
    T = np.float32 if dtype == 0 else np.float64
    return dict(kind=kind, c=c, x0=x0.astype(T), u0=u0.astype(T), xg=xg.astype(T), P0=P0.astype(T).ravel(), p0=np.zeros(N * n, T), KT0=np.zeros(N * n * m, T), d0=np.zeros(N * n, T))


def build_scenario(plant, kw, dtype, layout, recipe):
    """layout: one letter per problem (its kind); recipe[kind] = [(noise, goal, c), ...] taken in turn -- the j-th problem of a kind gets the j-th entry (wrapping around
    with the magnitudes moved by a few per cent, so that no two problems are the same)."""
    seen, probs = {}, []
    for i, kind in enumerate(layout):
        j = seen.get(kind, 0); seen[kind] = j + 1
        noise, goal, c = recipe[kind][j % len(recipe[kind])]
        wrap = 1.0 + 0.03 * (j // len(recipe[kind]))
        probs.append(make_problem(plant, kw, dtype, kind, noise * wrap, goal, c * wrap, 1000 * plant + i))
    return probs


def stack(probs, key):
    return np.concatenate([p[key].ravel() for p in probs])


def load(s, probs):
    """the call sequence of both sides: sentinel into the observables' rows, the cost-to-go double buffer's roles as on a fresh handle (a load keeps state.pw for warm starts
    from the handle's own previous solve, bodies.hpp init_cost_body; the single-problem handle is loaded again for every problem), then load with every warm-start array"""
    B, mi = s.cfg.batch, s.cfg.max_iter
    st = s.get_state()
    for b in range(B):
        st[b].pw = 0
    s.set_state(st)
    s.set("Jout", np.full(B * (mi + 2), SENTINEL_J)); s.set("alphaOut", np.full(B * (mi + 2), SENTINEL_A, np.int32))
    s.load(stack(probs, "x0"), stack(probs, "u0"), stack(probs, "xg"), clear_vars=0, P0=stack(probs, "P0"), p0=stack(probs, "p0"), KT0=stack(probs, "KT0"), d0=stack(probs, "d0"))


STATE_FIELDS = ("rho", "drho", "bp_retries", "cur", "pw", "ignore_defect", "accepted", "done", "iter")
CTG = ("P", "Pp", "p", "pp")


def collect(s):
    """everything that is compared, [B][...]"""
    B = s.cfg.batch
    out = s.store()
    st = s.get_state()
    for f in STATE_FIELDS:
        out[f] = np.array([getattr(st[b], f) for b in range(B)])
    for name in CTG:
        out[name] = s.get(name).reshape(B, -1)
    return out


def solve_single(s1, prob):
    """reference side: one problem on a one-problem handle, traced sweep by sweep until it exits"""
    load(s1, [prob])
    trace, cap = [], 4 * s1.cfg.max_iter + 40
    for _ in range(cap):
        s1.iterate(1); s1.sync()
        st = s1.get_state()[0]
        trace.append((st.accepted, st.done, st.bp_retries))
        if st.done:
            break
    assert trace[-1][1], "the problem did not exit within %d sweeps" % cap
    res = {k: v[0] for k, v in collect(s1).items()}
    res["trace"] = trace
    return res


def kinds_reached(probs, singles):
    """kind -> indices of the problems that show it, from the single-problem solves"""
    got = {k: [] for k in "abcde"}
    for i, (p, r) in enumerate(zip(probs, singles)):
        tr = r["trace"]
        if r["done"] == 1:
            got["a"].append(i)
        if r["done"] == 2:
            got["b"].append(i)
        if any(a == 0 for a, d, _ in tr) and (r["alphaOut"] == -1).sum() >= 2:          # (alphaOut[0] is -1 for every problem)
            got["c"].append(i)
        if p["c"] and r["done"] != 3 and any(a == 1 for a, _, _ in tr) and (tr[-1][2] >= 2 or [a for a, _, _ in tr[:2]] == [0, 0]):
            got["d"].append(i)                                                           # failed (or, on the arm, rejected) at least twice, then recovered
        if r["done"] == 3:
            got["e"].append(i)
    return got


def mix_report(singles, group_sizes, label):
    """The condition of the module docstring on the single-problem traces: per packing-group size, for every group of >= 2 consecutive problems the sweep indices at which
    it holds all three states.  Returns {group size: the smallest number of such sweeps over its groups}."""
    K = max(len(r["trace"]) for r in singles)
    tr = [r["trace"] + [r["trace"][-1]] * (K - len(r["trace"])) for r in singles]         # an exited problem keeps its state
    B, ok = len(singles), {}
    for g in group_sizes:
        chunks = [range(lo, min(lo + g, B)) for lo in range(0, B, g)]
        chunks = [ch for ch in chunks if len(ch) >= 2]
        counts = []
        for ch in chunks:
            good = []
            for t in range(K):
                acc = [tr[b][t][0] for b in ch]; done = [tr[b][t][1] for b in ch]
                if 1 in acc and (0 in acc or -1 in acc) and any(done):
                    good.append(t)
            counts.append(len(good))
            if len(chunks) <= 8:
                print("%s: group of %d, problems %d..%d: accepted / rejected-or-failed / done side by side at sweeps %s" % (label, g, ch[0], ch[-1], good))
        ok[g] = min(counts)
        print("%s: groups of %d problems: %d groups, sweeps with all three states per group: min %d, median %d" % (label, g, len(chunks), min(counts), int(np.median(counts))))
    return ok


def describe(probs, singles, label):
    sym = {1: "A", 0: "r", -1: "F"}
    for i, (p, r) in enumerate(zip(probs, singles)):
        print("%s: problem %2d kind %s (aimed at %s, c %-7g) %-28s done %d iters %2d bp_retries %2d rho %.3g" % (label, i, primary_kind(p, r), p["kind"], p["c"], "".join(sym[a] for a, _, _ in r["trace"]), r["done"], r["iter"], r["bp_retries"], r["rho"]))


def assert_mix(probs, singles, group_sizes, label, need, quiet=False):
    if not quiet:
        describe(probs, singles, label)
    got = kinds_reached(probs, singles[: len(probs)])
    print("%s: kinds reached %s" % (label, {k: len(v) for k, v in got.items()}))
    for kind, count in need.items():
        assert len(got[kind]) >= count, (label, "kind", kind, got)
    ok = mix_report(singles, group_sizes, label)
    assert all(v >= 1 for v in ok.values()), (label, ok)
    return got


def assert_equal_bits(batch, singles, label, index=None):
    keys = ("x", "u", "KT", "Jout", "alphaOut", "dmax") + STATE_FIELDS + CTG
    for b in range(len(batch["done"])):
        ref = singles[b if index is None else index[b]]
        for k in keys:
            assert np.array_equal(np.asarray(batch[k][b]), np.asarray(ref[k]), equal_nan=True), (label, "problem", b, k)


def run_batch(backend, plant, dtype, kw, sel, probs, sweeps, use_graph, names=()):
    s = make_solver(backend, plant, dtype=dtype, batch=len(probs), use_graph=use_graph, kernels=dict(sel), **kw)
    if backend == "hip":
        have = [n for n, _ in s.time_kernels(1)]
        assert all(any(h == n or h.startswith(n) for h in have) for n in names), (names, have)
    load(s, probs)
    s.iterate(sweeps); s.sync()
    out = collect(s)
    s.close()
    return out


_SINGLES = {}


def singles_of(backend, plant, dtype, kw, sel, probs, key, names=()):
    """the single-problem solves of a scenario on a selection: computed once, shared by the tests that need them, never changed"""
    key = (backend, key)
    if key not in _SINGLES:
        s1 = make_solver(backend, plant, dtype=dtype, batch=1, use_graph=1, kernels=dict(sel), **kw)
        if backend == "hip":
            have = [n for n, _ in s1.time_kernels(1)]
            assert all(any(h == n or h.startswith(n) for h in have) for n in names), (names, have)
        _SINGLES[key] = [solve_single(s1, p) for p in probs]
        s1.close()
    return _SINGLES[key]


# ---------------------------------------------------------------------------------------------------------------- the cases
# ---------------------------------------------------------------------------------------------------------------- from a pool of candidates to a batch
# Whether a float32 solve of these short, coarse horizons accepts or rejects at a given sweep depends on the kernels' summation order (the host emulation, the lane-group and
# the matrix-core backward pass decide differently from the second or third iteration on), so no fixed list of magnitudes yields the same kinds on every selection.  Each case
# therefore solves a POOL of candidates (a recipe per kind, about three candidates per place in the batch) on its single-problem handle -- the reference side -- and builds the
# batch from what those solves showed: an early finisher next to a problem that is still accepting and rejecting, kinds rotating.  The batch under test has no part in it.
def primary_kind(p, r):
    tr = r["trace"]
    if r["done"] == 3:
        return "e"
    if p["c"] and any(a == 1 for a, _, _ in tr) and (tr[-1][2] >= 2 or [a for a, _, _ in tr[:2]] == [0, 0]):
        return "d"
    if r["done"] == 1:
        return "a"
    return "c" if any(a == 0 for a, _, _ in tr) else "b"


def pair_mixed(ri, rj):
    K = max(len(ri["trace"]), len(rj["trace"]))
    ti, tj = (r["trace"] + [r["trace"][-1]] * (K - len(r["trace"])) for r in (ri, rj))
    return any(1 in (a[0], b[0]) and (a[0] != 1 or b[0] != 1) and (a[1] or b[1]) for a, b in zip(ti, tj))


def assemble(probs, res, B, pairs=True):
    """indices into the pool, in batch order.  pairs: (early finisher, problem that goes on) x B // 2 with every pair holding the three states at some sweep, then one
    problem on its own (packing groups of two); otherwise the kinds in rotation (wider packing groups)."""
    n = len(probs)
    kind = [primary_kind(p, r) for p, r in zip(probs, res)]
    used, order = set(), []
    if not pairs:
        by_kind = {k: [i for i in range(n) if kind[i] == k] for k in "acbdaeca"}
        for k in "acbdaeca" * B:
            if len(order) == B:
                break
            left = [i for i in by_kind[k] if i not in used]
            if left:
                used.add(left[0]); order.append(left[0])
        assert len(order) == B, ("the pool is too small", {k: len(v) for k, v in by_kind.items()})
        return order
    early = sorted((i for i in range(n) if res[i]["done"] in (1, 3)), key=lambda i: len(res[i]["trace"]))
    rot = "cdeb"
    for pair in range(B // 2):
        first = next((i for i in early if i not in used and (not order or kind[i] != kind[order[-1]])), None)
        assert first is not None, ("no early finisher left in the pool", kind)
        used.add(first)
        want = rot[pair % len(rot)]
        cands = [j for j in range(n) if j not in used and kind[j] == want and kind[j] != kind[first]] + [j for j in range(n) if j not in used and kind[j] != kind[first]]
        second = next((j for j in cands if pair_mixed(res[first], res[j])), None)
        assert second is not None, ("no partner that holds the three states with problem", first, kind)
        used.add(second); order += [first, second]
    if B % 2:
        left = [j for j in range(n) if j not in used and kind[j] != kind[order[-1]]]
        have = {kind[i] for i in order}
        want = next((k for k in "ebdc" if k not in have), "b")                     # a kind the pairs left out, else a plain run to max_iter
        order.append(next((j for j in left if kind[j] == want), left[0]))
    return order


def pool_of(plant, kw, dtype, recipe, per_kind):
    layout = "".join(k * 1 for _ in range(per_kind) for k in "acbde")
    return build_scenario(plant, kw, dtype, layout, recipe)


_CASES = {}


def scenario_of(backend, case):
    """(problems, their single-problem solves) of a case: the pool solved once on the case's single-problem selection, the batch assembled from it; shared and left unchanged"""
    key = (backend, case["key"])
    if key not in _CASES:
        pool = pool_of(case["plant"], case["kw"], case["dtype"], case["recipe"], case["per_kind"])
        res = singles_of(backend, case["plant"], case["dtype"], case["kw"], case["single_sel"], pool, case["key"], case["names"] if backend == "hip" else ())
        kinds = [primary_kind(p, r) for p, r in zip(pool, res)]
        print("%s[%s]: pool of %d candidates, kinds shown by their single-problem solves %s" % (case["key"], backend, len(pool), {k: kinds.count(k) for k in "abcde"}))
        order = assemble(pool, res, case["B"], pairs=case["groups"][0] == 2)
        _CASES[key] = ([pool[i] for i in order], [res[i] for i in order])
    return _CASES[key]


def run_case(backend, case, sel=None, names=None, batch=None, groups=None, graphs=(1, 0)):
    """sel / names / batch / groups: the batch handle's selection and expected kernels, number of problems (the scenario repeated) and packing groups when they differ from the
    case's own (the full-device arm case runs the thread-lane case's scenario on the library's own selection)."""
    probs, singles = scenario_of(backend, case)
    label = "%s[%s]" % (case["key"], backend)
    B = batch or case["B"]
    index = np.arange(B) % case["B"]
    assert_mix([probs[i] for i in index] if B <= 128 else probs, [singles[i] for i in index], groups or case["groups"], label, case["need"], quiet=B > 128)
    sweeps = max(len(r["trace"]) for r in singles) + EXTRA_SWEEPS
    for use_graph in (graphs if backend == "hip" else (0,)):
        out = run_batch(backend, case["plant"], case["dtype"], case["kw"], case["single_sel"] if sel is None else sel, [probs[i] for i in index], sweeps, use_graph,
                        case["names"] if names is None else names)
        assert_equal_bits(out, singles, "%s B=%d use_graph=%d" % (label, B, use_graph), index)
        del out
    return probs, singles


# ---------------------------------------------------------------------------------------------------------------- the cases
# recipe[kind] = [(noise, goal, c), ...]: what each entry AIMS at (found on the host emulation); the kind a problem counts as is what its single-problem solve shows
ARM_KW = dict(N=32, M=4, A=8, wafr_urdf=1, total_time=0.5, tol_cost=5e-3, max_iter=12, ignore_max_rho_exit=0)
ARM_RECIPE = {"a": [(0.001, 0.02, 0), (0.02, 0.02, 0), (0.02, 0.05, 0), (0.001, 0.05, 0), (0.02, 0.1, 0), (0.001, 0.1, 0), (0.05, 0.05, 0)],
              "b": [(0.001, 1.0, 0), (0.05, 1.0, 0), (0.05, 1.5, 0), (0.25, 2.0, 0), (0.25, 0.3, 0)],
              "c": [(0.3, 1.0, 0), (0.3, 0.3, 0), (0.05, 0.1, 0), (0.3, 2.5, 0), (0.001, 1.5, 0), (0.3, 0.1, 0)],
              # the window of c in which Huu of the boundary knots is indefinite: below it R + rho dominates, above it the Schur complement is that of a hard constraint again
              "d": [(0.001, 2.0, 2e3), (0.001, 0.3, 2e3), (0.001, 0.3, 5e3), (0.001, 2.0, 3e3), (0.001, 1.0, 5e3), (0.001, 1.0, 1e3), (0.001, 1.0, 2e3), (0.001, 1.0, 3e3), (0.001, 1.0, 4e3), (0.001, 1.0, 5e3), (0.001, 1.0, 6e3), (0.001, 1.0, 8e3), (0.001, 1.0, 1e4),
                    (0.02, 1.0, 2.2e3), (0.02, 1.0, 2.8e3), (0.02, 1.0, 3.5e3)],
              "e": [(0.001, 1.0, 1.5e3), (0.001, 1.0, 2.5e3), (0.001, 1.0, 2.8e3), (0.25, 2.5, 0), (0.35, 0.3, 0), (0.35, 2.0, 0), (0.05, 0.02, 0)]}
ARM_TL = dict(key="arm-thread-lanes", plant=4, dtype=0, kw=ARM_KW, B=11, recipe=ARM_RECIPE, per_kind=11, single_sel=dict(bp="mx", fp="tl", ls="many"),
              names=("k_bp_mfma", "k_fp_tl", "k_nis_tl", "k_ls_many"), groups=(2, 11), need=dict(a=2, b=1, c=2, d=1, e=1))
ARM_FEW = dict(ARM_TL, key="arm-few-problems", B=5, single_sel={}, names=("k_bp_mfma", "k_fp_tl4", "k_nis_tl7"), groups=(2, 5), need=dict(a=1, b=1, c=1, d=1, e=1))
EE_KW = dict(ARM_KW, mpc_mode=1, ee_cost=1)
EE_RECIPE = {"a": [(0.001, 0.05, 0), (0.001, 0.1, 0), (0.01, 0.05, 0), (0.001, 0.02, 0), (0.01, 0.2, 0)],
             "b": [(0.05, 1.0, 0), (0.001, 2.0, 0), (0.02, 1.0, 0), (0.001, 1.0, 1e5)],
             "c": [(0.05, 0.05, 0), (0.001, 0.3, 0), (0.05, 0.3, 0), (0.3, 1.0, 0), (0.3, 2.0, 0)],
             "d": [(0.001, 1.0, 100), (0.001, 1.0, 300), (0.001, 1.0, 1e3), (0.001, 1.0, 1e4), (0.001, 1.0, 3e4)],
             "e": [(0.001, 1.0, 3e3), (0.001, 1.0, 5e3), (0.001, 1.0, 2e3), (1.0, 0.05, 0), (0.3, 0.3, 0)]}
ARM_EE = dict(ARM_TL, key="arm-end-effector", kw=EE_KW, B=7, recipe=EE_RECIPE, per_kind=6, groups=(2, 7), need=dict(a=1, b=1, c=1, d=1, e=1))
CART_KW = dict(N=64, M=4, A=8, integrator=3, total_time=2.0, tol_cost=5e-2, max_iter=12, ignore_max_rho_exit=0)
CART_RECIPE = {"a": [(0.001, 0.03, 0), (0.1, 0.1, 0), (0.001, 0.3, 0), (0.1, 1.0, 0), (0.001, 1.3, 0), (0.5, 1.3, 0), (0.1, 0.03, 0)],
               "b": [(0.001, 0.6, 0), (0.1, 0.6, 0), (0.1, 0.003, 0), (0.5, 1.0, 0), (0.001, 1.0, 0)],
               "c": [(0.5, 0.1, 0), (0.5, 0.3, 0), (0.5, 0.6, 0), (1.0, 1.0, 0), (1.0, 0.1, 0)],
               "d": [(0.001, 1.0, 10), (0.001, 1.0, 30), (0.001, 1.0, 100), (0.001, 1.0, 300), (0.001, 0.1, 10), (0.001, 0.1, 30), (0.001, 0.1, 100), (0.001, 0.1, 1e3)],
               "e": [(0.001, 1.0, 1e4), (0.001, 1.0, 1e5), (0.001, 1.0, 1e6), (0.001, 0.1, 1e5), (0.001, 0.1, 1e6), (0.001, 0.003, 0)]}
CART = dict(key="cart-pole", plant=2, kw=CART_KW, B=70, recipe=CART_RECIPE, per_kind=30, single_sel=dict(cf="ts", cf_fp="cf", ls="many"),
            names=("k_bp_ts", "k_fp_cf", "k_nis_ts", "k_ls_many"), groups=(8, 16, 64), need=dict(a=4, b=4, c=4, d=4, e=4))
QUAD_KW = dict(N=16, M=2, A=16, integrator=3, total_time=1.0, tol_cost=1e-3, max_iter=12, ignore_max_rho_exit=0)
QUAD_RECIPE = {"a": [(0.001, 0.02, 0), (0.001, 0.01, 0), (0.003, 0.02, 0), (0.001, 0.03, 0), (0.03, 0.1, 3e6), (0.001, 0.3, 0), (0.03, 0.3, 0)],
               "b": [(0.001, 1.0, 0), (0.03, 1.0, 0), (0.1, 1.0, 0), (0.1, 0.3, 0)],
               "c": [(0.03, 0.1, 0), (0.1, 0.1, 0), (0.3, 0.1, 0), (0.03, 0.02, 0), (0.3, 1.0, 0), (0.3, 0.3, 0)],
               "d": [(0.03, 0.1, 10), (0.03, 0.1, 30), (0.03, 0.1, 300), (0.03, 0.1, 1e3), (0.03, 0.1, 3e3), (0.03, 0.1, 3e4), (0.03, 0.1, 1e6), (0.03, 0.1, 1e7)],
               "e": [(3.0, 0.3, 0), (0.03, 0.1, 1e12), (0.03, 0.1, 1e4), (2.0, 0.3, 0), (0.03, 0.02, 1e4), (3.0, 0.1, 0), (0.03, 0.1, 3e7), (0.03, 0.1, 1e8), (1.0, 0.3, 0), (0.3, 0.02, 0), (0.1, 0.1, 0), (1.0, 0.1, 0), (0.3, 0.1, 0), (1.0, 1.0, 0), (0.03, 0.1, 3e8)]}
QUAD = dict(key="quadrotor", plant=3, kw=QUAD_KW, B=9, recipe=QUAD_RECIPE, per_kind=10, single_sel=PINNED, names=("k_bp_mq", "k_sweep_maps", "k_fp_cf", "k_ls_many", "k_nis_kb"),
            groups=(2, 4, 9), need=dict(a=1, b=1, c=1, d=1, e=1))
QUAD8_KW = dict(QUAD_KW, N=8, total_time=0.5)
BACKENDS_HIP = [pytest.param("hip", id="hip", marks=pytest.mark.gpu)]


def typed(case, dtype):
    return dict(case, dtype=dtype, key="%s-%s" % (case["key"], "f32" if dtype == 0 else "f64"))


@pytest.mark.parametrize("backend", BACKENDS)
def test_arm_thread_lanes_mixed_batch_equals_single_problem_solves(backend):
    """Arm, joint cost, N 32, M 4, A 8, 11 problems on bp=mx, fp=tl, ls=many: two problems per k_nis_tl wave (64 knots; one 64-knot chunk of the compact [A B]) and per
    k_fp_tl wave (64 / A (problem, segment) pairs), all 11 in one k_ls_many wave.  (hostsim: the same scenario on the emulation's own bodies.)"""
    run_case(backend, ARM_TL)


@pytest.mark.gpu
def test_arm_full_device_mixed_batch_equals_the_thread_lane_originals():
    """2051 problems = the 11-problem scenario of the thread-lane case repeated with period 11 (coprime to 4 and 64: every wave is mixed, every alignment occurs) on the
    library's OWN selection, which from 2048 problems takes k_sweep_maps<T, 4> (four problems per wave) and k_ls_many; every replica equals its original's single-problem
    solve bit for bit, the last problem (a ragged last wave) included."""
    run_case("hip", ARM_TL, sel={}, names=("k_bp_mfma", "k_sweep_maps", "k_fp_tl", "k_ls_many", "k_nis_tl"), batch=2051, groups=(4, 64))


@pytest.mark.parametrize("backend", BACKENDS)
def test_arm_end_effector_mixed_batch_equals_single_problem_solves(backend):
    """The same packing with ee_cost = 1, mpc_mode = 1 (7 problems): the Hc path (compact position block of the Gauss-Newton Hessian, setup -> backward pass) and the in-sim cost."""
    run_case(backend, ARM_EE)


@pytest.mark.gpu
def test_arm_few_problem_kernels_mixed_batch_equals_single_problem_solves():
    """5 problems on the library's own selection for few problems (k_fp_tl4 with the line search inside the rollouts, k_nis_tl7): workgroup tails."""
    run_case("hip", ARM_FEW)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [0, 1], ids=["float32", "float64"])
def test_cartpole_mixed_batch_equals_single_problem_solves(backend, dtype):
    """Cart-pole N 64, M 4, A 8, RK3, 70 problems on cf=ts, cf_fp=cf, ls=many (cf_nis as the library chooses: k_nis_ts): 16 problems per k_bp_ts wave, 8 per k_fp_cf wave
    (one LDS operand stage), one knot per k_nis_ts lane, 64 per k_ls_many wave; the 1 x 1 Huu reports its failures (kinds d, e through bp_retries)."""
    probs, singles = run_case(backend, typed(CART, dtype))
    got = kinds_reached(probs, singles)
    assert sum(singles[i]["bp_retries"] >= 2 for i in got["d"]) >= 4, got


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", [0, 1], ids=["float32", "float64"])
def test_quadrotor_mixed_batch_equals_single_problem_solves(backend, dtype):
    """Quadrotor N 16, M 2, A 16, RK3, 9 problems on PINNED of test_quad_bench_geometry.py: four problems per k_fp_cf / k_sweep_maps_cf wave, k_bp_mq with the sweep maps
    fused, one problem per k_nis_kb<16> wave (N = 16), all in one k_ls_many wave."""
    probs, singles = run_case(backend, typed(QUAD, dtype))
    got = kinds_reached(probs, singles)
    assert any(singles[i]["bp_retries"] >= 2 for i in got["d"]), got


@pytest.mark.gpu
@pytest.mark.parametrize("cf_bp,kernel", [("cl", "k_bp_cl"), ("gl32", "k_bp_gl")])
def test_quadrotor_column_lane_backward_passes_mixed_batch(cf_bp, kernel):
    """cf_bp = cl (16 lanes per block of knots: four blocks = two problems per wave) and gl32 (two blocks per wave).  Second yardstick: the cooperative kernels (cf = coop) on a
    single-problem handle, which tests/test_closed_form_serial.py holds as bit-identical to these."""
    case = dict(QUAD, key="quadrotor-" + cf_bp, dtype=0, single_sel=dict(PINNED, cf_bp=cf_bp), names=(kernel, "k_fp_cf", "k_ls_many", "k_nis_kb"))
    probs, singles = run_case("hip", case)
    coop = singles_of("hip", 3, 0, case["kw"], dict(cf="coop"), probs, case["key"] + "-coop")
    for b, (r, c) in enumerate(zip(singles, coop)):
        for k in ("x", "u", "KT", "Jout", "alphaOut", "dmax") + STATE_FIELDS + CTG:
            assert np.array_equal(np.asarray(r[k]), np.asarray(c[k]), equal_nan=True), (cf_bp, "cooperative single-problem handle", b, k)


@pytest.mark.gpu
def test_quadrotor_knot_batched_setup_two_problems_per_wave():
    """N = 8: k_nis_kb<16> takes 16 knots per wave = two problems (PINNED, 9 problems)."""
    run_case("hip", dict(QUAD, key="quadrotor-N8", dtype=0, kw=QUAD8_KW))


# ---------------------------------------------------------------------------------------------------------------- float64 against the oracle
ORACLE_LEGS = [pytest.param(dict(ARM_TL, dtype=1, single_sel=dict(bp="mx", fp="tl")), id="arm-mx-tl"),
               pytest.param(dict(CART, dtype=1, single_sel=dict(cf="ts")), id="cartpole-ts"),
               pytest.param(dict(QUAD, dtype=1), id="quadrotor-pinned")]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", ORACLE_LEGS)
def test_float64_mixed_batch_follows_the_oracle(backend, case):
    """The warm-start-free part of the scenario (the recipes of kinds a, b, c; the oracle's run_ilqr_gpusem takes no P0), the whole mixed batch in ONE float64 handle, every
    problem against the oracle: identical iters and alphaOut up to iters (the -1 entries included), Jout / x / u to 1e-8 of the largest magnitude, done == 1 where the oracle
    left by tolerance."""
    plant, kw = case["plant"], case["kw"]
    pool = [p for p in pool_of(plant, kw, 1, case["recipe"], 4) if p["kind"] in "abc" and not p["c"]]
    B = len(pool)
    o = Oracle(default_cfg(plant, cores=1, spawn_threads=0, **kw), np.float64)
    with np.errstate(all="ignore"):
        refs = [o.run_ilqr_gpusem(p["x0"], p["u0"], p["xg"]) for p in pool]
    s = make_solver(backend, plant, dtype=1, batch=B, kernels=dict(case["single_sel"]), **kw)
    load(s, pool)
    s.iterate(4 * kw["max_iter"] + 40); s.sync()
    out = collect(s)
    s.close()
    exits = {1: 0, 2: 0, 3: 0}
    for b, r in enumerate(refs):
        it = r["iters"]
        assert out["iter"][b] == it, (b, out["iter"][b], it)
        assert list(out["alphaOut"][b][: it + 1]) == list(r["alphaOut"][: it + 1]), (b, out["alphaOut"][b], r["alphaOut"])
        for k in ("Jout", "x", "u"):
            ref = r[k][: it + 1] if k == "Jout" else r[k]
            got = out[k][b][: it + 1] if k == "Jout" else out[k][b].ravel()
            assert np.abs(got - ref).max() <= 1e-8 * np.abs(ref).max(), (b, k, float(np.abs(got - ref).max() / np.abs(ref).max()))
        J = r["Jout"]
        by_tolerance = r["alphaOut"][it] >= 0 and (J[it - 1] - J[it]) / J[it - 1] < kw["tol_cost"]
        if by_tolerance:
            assert out["done"][b] == 1, (b, out["done"][b])
        assert out["done"][b] in (1, 2, 3)
        exits[int(out["done"][b])] += 1
    print("float64 %s[%s]: %d problems, exits by tolerance / max_iter / max rho: %s, rejected line searches: %d" % (case["key"], backend, B, exits, sum(int((r["alphaOut"][1: r["iters"] + 1] == -1).sum()) for r in refs)))
    assert exits[1] >= 2 and exits[2] >= 2 and sum((r["alphaOut"][1: r["iters"] + 1] == -1).any() for r in refs) >= 2, exits
