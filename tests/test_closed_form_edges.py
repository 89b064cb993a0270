"""The kernel families of the pendulum, cart-pole and quadrotor at the edges of the accepted N, M, A domain (config_complaint, csrc/handle_setup.hpp: N a power of two in
[4, 1024], M <= 16 with M | N and N / M >= 2, A in [1, 64]): two-knot segments, M = 8 / 16, N = 4 / 8 (a wavefront of k_nis_kb spans several problems), odd A and
A = 64, N = kTsMaxN and the horizon behind it, where the plan steps aside to k_fp.

SHAPES is closed; every shape runs every ROW (a selection pinned through pddp_config.kernels), and EXPECT states BY HAND which kernels each (shape, row) resolves to --
the fallbacks included -- as  backward pass / linear sweep / rollouts / setup.  A row that resolves to the kernels of an earlier row at a shape is not run twice there.

Inputs (fixed): problem b of a shape is the example's inputs with velocity noise normal(0, 0.002 (b + 1)) from default_rng(1000 plant + 100 b + N + M); beyond b = 4
the noise scale is that of problem b mod 5 and the seed keeps its own b.  tol_cost = 0, max_iter = 6, total_time = N / 32.

Comparisons:
  1  float64, every row, B = 1 and B2, per problem against the oracle's GPU-semantics driver: iters and alphaOut identical, Jout rtol 1e-8, x and u 1e-8 of the largest
     reference element, KT 1e-7 of max(largest reference element, 1) -- the bounds of tests/test_quad_matrix_core.py / tests/test_solver_parity.py;
  2  every row without a matrix-core kernel, float32 and float64, bit for bit the cf=coop handle on the same inputs: x, u, KT, Jout, alphaOut, dmax and the cost-to-go P;
  3  float32 rows with k_bp_mq: alphaOut equal to the float64 oracle's over the L leading entries on which {oracle32 strict, oracle32 fma, oracle64} agree for that
     problem, and at EACH of those entries |J / J64 - 1| <= max(1e-5, 4 x the larger of the two float32 oracles' deviations at that entry);
  4  comparison 1 at B2 on a GoalTab handle for POLICY_CASES: odd problems with a goal trajectory and a diagonal record of their own against the shim-oracle, even
     ones as before against the plain oracle;
  5  (CPU) the host emulation's cooperative bodies at every shape but Q9 with the bounds of 1, and the conditions the inputs must meet, on the oracles alone: every
     problem accepts an iteration in float64, and L >= 3.

B2 has a partial last wave for the row's kernels (batch2): k_fp_cf<16> B2 % 4 != 0, k_fp_cf<8> B2 % 8 != 0, k_nis_kb<KB> (B2 N) % KB != 0 where a batch can achieve it,
k_fp_ts with N <= 32: B2 A > 64 and (B2 A) % 64 != 0; shapes with N >= 256 keep B2 <= 5.  profiles/closed_form_edges.md records the batches, the measured float32
ratios and the added GPU time.
"""
import numpy as np
import pytest

from backends import make_solver
from oracle_binding import Oracle, default_cfg, example_inputs
from test_goal_trajectory import BUILTIN, DIMS, set_trajectories, shim_oracle, trajectory

# id: plant, N, M, A, integrator
SHAPES = {
    "P1": (1, 4, 2, 1, 1),       # smallest horizon, 2-knot segments, one candidate
    "P2": (1, 8, 4, 3, 2),       # 2-knot segments, odd A, midpoint
    "P3": (1, 32, 16, 5, 3),     # M = 16, 2-knot segments
    "P4": (1, 256, 1, 64, 1),    # N = kTsMaxN, A = 64, single shooting
    "P5": (1, 512, 4, 4, 1),     # beyond kTsMaxN
    "C1": (2, 4, 1, 8, 3),       # N < KB, k_fp_cf<8>
    "C2": (2, 8, 4, 8, 3),       # 2-knot segments through k_sweep_cf + k_fp_cf<8>, N < KB
    "C3": (2, 32, 16, 16, 3),    # M = 16, k_fp_cf<16>
    "C4": (2, 16, 2, 7, 2),      # A = 7 (no staged kernel), M = 2
    "C5": (2, 64, 8, 64, 1),     # A = 64, M = 8
    "C6": (2, 256, 2, 8, 3),     # N = 256 on the staged kernel
    "Q1": (3, 4, 1, 1, 3),       # smallest horizon, one candidate
    "Q2": (3, 4, 2, 16, 3),      # N = 4 with the fused matrix-core pass, one map
    "Q3": (3, 8, 4, 16, 3),      # 2-knot segments, three maps, N < KB
    "Q4": (3, 32, 16, 16, 3),    # fifteen maps, 2-knot segments
    "Q5": (3, 16, 2, 16, 3),     # M = 2
    "Q6": (3, 16, 8, 5, 3),      # matrix-core pass without fusion + k_fp_ts, odd A
    "Q7": (3, 8, 2, 8, 2),       # A = 8 cannot stage 12 states; midpoint -> k_nis_gl
    "Q8": (3, 256, 16, 16, 3),   # longest staged horizon with M = 16
    "Q9": (3, 512, 4, 16, 3),    # beyond kTsMaxN: k_bp_mq + k_nis_kb pinned, rollouts fall back
    "Q10": (3, 8, 1, 1, 1),      # Euler, one candidate
}
ROWS = {
    "coop": dict(cf="coop"),
    "ts": dict(cf="ts"),
    "gl32-ts-gl8": dict(cf_bp="gl32", cf_fp="ts", cf_nis="gl8"),
    "gl-cf-kb16": dict(cf_bp="gl", cf_fp="cf", cf_nis="kb16"),
    # the quadrotor's own
    "mq-cf-kb16": dict(cf_bp="mq", cf_fp="cf", cf_nis="kb16"),
    "mq-st-cf-kb16": dict(cf_bp="mq", cf_fp="cf", cf_nis="kb16", sweep="st"),
    "cl-cf-kb20": dict(cf_bp="cl", cf_fp="cf", cf_nis="kb20"),
    "mq-ts-kb32": dict(cf_bp="mq", cf_fp="ts", cf_nis="kb32"),
    "mq-cf-kb64": dict(cf_bp="mq", cf_fp="cf", cf_nis="kb64"),      # k_nis_kb<64> exists in float32 only: a double handle runs k_nis_kb<32> (solver_impl.hpp launch_nis)
}
COMMON_ROWS = ("coop", "ts", "gl32-ts-gl8", "gl-cf-kb16")
# What every (shape, row) resolves to, written out by hand in the order of ROWS:  backward pass / linear sweep / rollouts / setup.
#   co k_bp | k_fp | k_nis     wide k_bp_wide     ts k_bp_ts | k_fp_ts | k_nis_ts     gl16 gl32 k_bp_gl<16 | 32>     gl8 k_nis_gl<8>     cl k_bp_cl     mq k_bp_mq     mqF k_bp_mq<FUSE>
#   sweep: - none, cf k_sweep_cf, maps k_sweep_maps (k_sweep_maps_cf)     cf8 cf16 k_fp_cf<8 | 16>     kbNN k_nis_kb<NN>
EXPECT = {
    "P1": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/co",
    "P2": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/co",
    "P3": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/kb16",
    "P4": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/co",
    "P5": "co/-/co/co    co/-/co/co  gl32/-/co/gl8  gl16/-/co/co",                 # ts_fits is false: kernels.cf = ts and cf_fp = ts | cf resolve to k_fp
    "C1": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/cf8/kb16",
    "C2": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/cf/cf8/kb16",
    "C3": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/cf/cf16/kb16",
    "C4": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/co",
    "C5": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/co",
    "C6": "co/-/co/co    ts/-/ts/ts  gl32/-/ts/gl8  gl16/cf/cf8/kb16",
    "Q1": "wide/-/co/co  ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/kb16     mq/-/ts/kb16       mq/-/ts/kb16     cl/-/ts/kb20     mq/-/ts/kb32  mq/-/ts/kb64",
    "Q2": "wide/-/co/co  ts/-/ts/ts  gl32/-/ts/gl8  gl16/cf/cf16/kb16  mqF/maps/cf16/kb16 mq/cf/cf16/kb16  cl/cf/cf16/kb20  mq/-/ts/kb32  mqF/maps/cf16/kb64",
    "Q3": "wide/-/co/co  ts/-/ts/ts  gl32/-/ts/gl8  gl16/cf/cf16/kb16  mqF/maps/cf16/kb16 mq/cf/cf16/kb16  cl/cf/cf16/kb20  mq/-/ts/kb32  mqF/maps/cf16/kb64",
    "Q4": "wide/-/co/co  ts/-/ts/ts  gl32/-/ts/gl8  gl16/cf/cf16/kb16  mqF/maps/cf16/kb16 mq/cf/cf16/kb16  cl/cf/cf16/kb20  mq/-/ts/kb32  mqF/maps/cf16/kb64",
    "Q5": "wide/-/co/co  ts/-/ts/ts  gl32/-/ts/gl8  gl16/cf/cf16/kb16  mqF/maps/cf16/kb16 mq/cf/cf16/kb16  cl/cf/cf16/kb20  mq/-/ts/kb32  mqF/maps/cf16/kb64",
    "Q6": "wide/-/co/co  ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/kb16     mq/-/ts/kb16       mq/-/ts/kb16     cl/-/ts/kb20     mq/-/ts/kb32  mq/-/ts/kb64",
    "Q7": "wide/-/co/co  ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/co       mq/-/ts/co         mq/-/ts/co       cl/-/ts/co       mq/-/ts/co    mq/-/ts/co",      # midpoint: no k_nis_kb
    "Q8": "wide/-/co/co  ts/-/ts/ts  gl32/-/ts/gl8  gl16/cf/cf16/kb16  mqF/maps/cf16/kb16 mq/cf/cf16/kb16  cl/cf/cf16/kb20  mq/-/ts/kb32  mqF/maps/cf16/kb64",
    "Q9": "wide/-/co/co  wide/-/co/co gl32/-/co/gl8 gl16/-/co/kb16     mq/-/co/kb16       mq/-/co/kb16     cl/-/co/kb20     mq/-/co/kb32  mq/-/co/kb64",     # ts_fits is false: k_fp, no records, no fusion
    "Q10": "wide/-/co/co ts/-/ts/ts  gl32/-/ts/gl8  gl16/-/ts/co       mq/-/ts/co         mq/-/ts/co       cl/-/ts/co       mq/-/ts/co    mq/-/ts/co",      # Euler: no k_nis_kb
}
BP_NAME = dict(co="k_bp", wide="k_bp_wide", ts="k_bp_ts", gl16="k_bp_gl", gl32="k_bp_gl", cl="k_bp_cl", mq="k_bp_mq", mqF="k_bp_mq")
SWEEP_NAME = {"-": None, "cf": "k_sweep_cf", "maps": "k_sweep_maps"}
FP_NAME = dict(co="k_fp", ts="k_fp_ts", cf8="k_fp_cf", cf16="k_fp_cf")
NIS_NAME = dict(co="k_nis", ts="k_nis_ts", gl8="k_nis_gl", gl16="k_nis_gl", kb16="k_nis_kb", kb20="k_nis_kb", kb32="k_nis_kb", kb64="k_nis_kb")
POLICY_CASES = [("P3", "ts"), ("P4", "ts"), ("C2", "gl-cf-kb16"), ("C3", "gl-cf-kb16"), ("C6", "gl-cf-kb16"), ("Q2", "mq-cf-kb16"), ("Q3", "mq-cf-kb16"),
                ("Q4", "mq-cf-kb16"), ("Q8", "mq-cf-kb16"), ("Q6", "mq-ts-kb32"), ("Q7", "gl32-ts-gl8")]
SHAPE_PARAMS = list(SHAPES)
QUAD_SHAPES = [k for k in SHAPES if SHAPES[k][0] == 3]
J_FLOOR, J_FACTOR = 1e-5, 4.0       # comparison 3: about 100 float32 epsilons; a third summation order is one more draw from a heavy-tailed error whose yardstick is two samples


def shape_kw(shape):
    plant, N, M, A, integ = SHAPES[shape]
    return dict(N=N, M=M, A=A, integrator=integ, total_time=N / 32.0, tol_cost=0.0, max_iter=6)


def shape_rows(shape):
    return list(ROWS) if SHAPES[shape][0] == 3 else list(COMMON_ROWS)


def resolved(shape, row, dtype):
    """(bp, sweep, fp, nis) of EXPECT for the handle's element type: a double handle asked for kb64 runs k_nis_kb<32>"""
    rows = shape_rows(shape)
    cells = EXPECT[shape].split()
    assert len(cells) == len(rows), (shape, cells)
    bp, sw, fp, nis = cells[rows.index(row)].split("/")
    if dtype == 1 and nis == "kb64":
        nis = "kb32"
    return bp, sw, fp, nis


def expected_names(shape, row, dtype):
    bp, sw, fp, nis = resolved(shape, row, dtype)
    return [n for n in (BP_NAME[bp], SWEEP_NAME[sw], FP_NAME[fp], "k_ls", NIS_NAME[nis]) if n]


def rows_to_run(shape, dtype):
    """the rows of a shape without those that resolve to the kernels of an earlier row"""
    seen, out = set(), []
    for row in shape_rows(shape):
        r = resolved(shape, row, dtype)
        if r not in seen:
            seen.add(r); out.append(row)
    return out


def has_matrix_cores(shape, row, dtype):
    return resolved(shape, row, dtype)[0] in ("mq", "mqF")


def batch2(shape, row, dtype):
    """the batch with a partial last wave for every kernel of the row that packs problems into wavefronts"""
    plant, N, M, A, integ = SHAPES[shape]
    bp, sw, fp, nis = resolved(shape, row, dtype)
    conds = []
    if fp == "cf16":
        conds.append(lambda B: B % 4 != 0)              # (also k_sweep_maps_cf: four problems per wavefront)
    if fp == "cf8":
        conds.append(lambda B: B % 8 != 0 and (B > 8 or N >= 256))      # (a full wavefront in front of the partial one where the cap allows it)
    if nis.startswith("kb"):
        KB = int(nis[2:])
        if any((B * N) % KB for B in range(1, KB + 1)):     # (N a multiple of KB: every batch fills its waves)
            conds.append(lambda B: (B * N) % KB != 0)
    if fp == "ts" and N <= 32:
        conds.append(lambda B: B * A > 64 and (B * A) % 64 != 0)
    cap = 5 if N >= 256 else 67
    for B in [5, 9, 3, 7, 6, 2, 4, 8] + list(range(10, 68)):
        if B <= cap and all(c(B) for c in conds):
            return B
    raise AssertionError(("no batch with a partial last wave", shape, row))


def problems_needed(shape):
    return max(batch2(shape, row, dtype) for dtype in (0, 1) for row in rows_to_run(shape, dtype))


_PROB, _ORA, _RUN = {}, {}, {}


def problem(shape, b):
    """float64 x0, u0, xg of problem b"""
    if (shape, b) not in _PROB:
        plant, N, M, A, integ = SHAPES[shape]
        n = DIMS[plant][1]
        rng = np.random.default_rng(1000 * plant + 100 * b + N + M)
        x0, u0, xg = example_inputs(plant, N, np.float64, noise=rng.normal(0, 0.002 * (b % 5 + 1), (N, n)))
        _PROB[(shape, b)] = dict(x0=x0, u0=u0, xg=xg)
    return _PROB[(shape, b)]


def typed(p, dtype):
    T = np.float32 if dtype == 0 else np.float64
    return {k: v.astype(T) for k, v in p.items()}


def stacked(shape, B, dtype):
    probs = [typed(problem(shape, b), dtype) for b in range(B)]
    return tuple(np.concatenate([p[k].ravel() for p in probs]) for k in ("x0", "u0", "xg"))


def oracle64(shape, b):
    key = (shape, b, "f64")
    if key not in _ORA:
        p = problem(shape, b)
        _ORA[key] = Oracle(default_cfg(SHAPES[shape][0], cores=1, spawn_threads=0, **shape_kw(shape)), np.float64).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
    return _ORA[key]


def oracle32(shape, b, variant):
    key = (shape, b, variant)
    if key not in _ORA:
        p = typed(problem(shape, b), 0)
        _ORA[key] = Oracle(default_cfg(SHAPES[shape][0], cores=1, spawn_threads=0, **shape_kw(shape)), np.float32, variant=variant).run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
    return _ORA[key]


def leading(shape, b):
    """L: the leading entries of alphaOut on which the two float32 oracles and the float64 oracle agree"""
    r64, rs, rf = oracle64(shape, b), oracle32(shape, b, "strict"), oracle32(shape, b, "fma")
    top = r64["iters"] + 1
    return next((i for i in range(top) if not (rs["alphaOut"][i] == rf["alphaOut"][i] == r64["alphaOut"][i])), top)


def check_against_oracle(out, j, ref, label):
    """comparison 1 for problem j of a batch"""
    it = ref["iters"]
    assert int(out["iters"][j]) == it, (label, "iters", int(out["iters"][j]), it)
    assert list(out["alphaOut"][j][: it + 1]) == list(ref["alphaOut"][: it + 1]), (label, list(out["alphaOut"][j]), list(ref["alphaOut"]))
    np.testing.assert_allclose(out["Jout"][j][: it + 1], ref["Jout"][: it + 1], rtol=1e-8, atol=0, err_msg=str(label))
    for k in ("x", "u"):
        np.testing.assert_allclose(out[k][j].ravel(), ref[k], rtol=0, atol=1e-8 * np.abs(ref[k]).max(), err_msg=str((label, k)))
    np.testing.assert_allclose(out["KT"][j].ravel(), ref["KT"], rtol=0, atol=1e-7 * max(np.abs(ref["KT"]).max(), 1.0), err_msg=str((label, "KT")))


def handle(shape, row, dtype, B):
    """a handle pinned to the row; the kernels it reports are the ones written out in EXPECT"""
    s = make_solver("hip", SHAPES[shape][0], dtype=dtype, batch=B, kernels=dict(ROWS[row]), **shape_kw(shape))
    names = [n for n, _ in s.time_kernels(1)]
    assert names == expected_names(shape, row, dtype), (shape, row, dtype, names, expected_names(shape, row, dtype))
    return s


def run(shape, row, dtype, B):
    """the whole solve of problems 0 .. B - 1 on the row's kernels, once per session"""
    key = (shape, row, dtype, B)
    if key not in _RUN:
        s = handle(shape, row, dtype, B)
        out = s.solve(*stacked(shape, B, dtype))
        assert out["done"].all(), key
        out["P"] = s.get_cost_to_go()[0]
        s.close()
        _RUN[key] = out
    return _RUN[key]


def batches(shape, row, dtype):
    return (1, batch2(shape, row, dtype))


# ---------------------------------------------------------------------------------------------------------------- CPU: the inputs, on the oracles alone
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_every_problem_accepts_an_iteration_and_the_oracles_agree_on_three_entries(shape):
    """Problems 0 .. 4 -- part of every batch of five or more -- each accept an iteration; so does every problem behind them but problems 13 and 44 of Q1 (one
    candidate, four knots: the full step or nothing), which reject all six steps in the oracle and are compared decision for decision all the same.  L >= 3 holds
    for every problem."""
    worst_L, worst_dev, rejecting = 99, 0.0, []
    for b in range(max(problems_needed(shape), 5)):
        r64 = oracle64(shape, b)
        if sum(a >= 0 for a in r64["alphaOut"][1: r64["iters"] + 1]) < 1:
            rejecting.append(b)
        L = leading(shape, b)
        assert L >= 3, (shape, b, L, list(oracle32(shape, b, "strict")["alphaOut"]), list(oracle32(shape, b, "fma")["alphaOut"]), list(r64["alphaOut"]))
        dev = max(abs(float(oracle32(shape, b, v)["Jout"][i]) / r64["Jout"][i] - 1.0) for v in ("strict", "fma") for i in range(L))
        worst_L, worst_dev = min(worst_L, L), max(worst_dev, dev)
    assert rejecting == ([13, 44] if shape == "Q1" else []), (shape, "problems without an accepted iteration", rejecting)
    print("%s: %d problems, worst L %d, worst float32-oracle deviation of J over the leading entries %.2e" % (shape, problems_needed(shape), worst_L, worst_dev))


def test_the_table_names_every_row_of_every_shape_and_drops_only_repeats():
    for shape in SHAPES:
        for dtype in (0, 1):
            run_rows = rows_to_run(shape, dtype)
            assert run_rows[0] == "coop" and len({resolved(shape, r, dtype) for r in run_rows}) == len(run_rows)
            for row in shape_rows(shape):
                expected_names(shape, row, dtype)
    # the horizons behind kTsMaxN: every request for thread-serial or staged rollouts resolves to k_fp
    for shape in ("P5", "Q9"):
        assert all(resolved(shape, row, 0)[2] == "co" for row in shape_rows(shape))
    # two-knot segments, M = 8 / 16, N = 4 / 8, odd A, A = 64 are all there
    assert {SHAPES[s][1] // SHAPES[s][2] for s in SHAPES} >= {2} and {SHAPES[s][2] for s in SHAPES} >= {8, 16} and {SHAPES[s][1] for s in SHAPES} >= {4, 8, 256, 512}
    assert {SHAPES[s][3] for s in SHAPES} >= {1, 3, 5, 7, 64}


@pytest.mark.parametrize("shape", [s for s in SHAPE_PARAMS if s != "Q9"])
def test_host_emulation_of_the_cooperative_bodies_follows_the_oracle(shape):
    B = 5
    s = make_solver("hostsim", SHAPES[shape][0], dtype=1, batch=B, kernels=dict(cf="coop"), **shape_kw(shape))
    out = s.solve(*stacked(shape, B, 1))
    assert out["done"].all()
    for b in range(B):
        check_against_oracle(out, b, oracle64(shape, b), (shape, "hostsim", b))
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU: the kernels behind every row
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_rows_resolve_to_the_kernels_written_out_by_hand(shape):
    """every row, the dropped repeats included, float32 and float64; at P5 and Q9 the requests for k_fp_ts / k_fp_cf come out as k_fp"""
    for dtype in (0, 1):
        for row in shape_rows(shape):
            s = handle(shape, row, dtype, 1)
            if shape in ("P5", "Q9"):
                assert "k_fp" in [n for n, _ in s.time_kernels(1)], (shape, row)
            s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_float64_rows_follow_the_oracle(shape):
    for row in rows_to_run(shape, 1):
        for B in batches(shape, row, 1):
            out = run(shape, row, 1, B)
            for b in range(B):
                check_against_oracle(out, b, oracle64(shape, b), (shape, row, "B", B, "problem", b))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_rows_without_matrix_cores_equal_the_cooperative_kernels_bit_for_bit(shape, dtype):
    compared = 0
    for row in rows_to_run(shape, dtype):
        if row == "coop" or has_matrix_cores(shape, row, dtype):
            continue
        for B in batches(shape, row, dtype):
            a, c = run(shape, row, dtype, B), run(shape, "coop", dtype, B)
            assert np.array_equal(a["iters"], c["iters"]), (shape, row, B, "iters")
            for k in ("x", "u", "KT", "Jout", "alphaOut", "dmax", "P"):
                assert np.array_equal(a[k], c[k], equal_nan=True), (shape, row, "B", B, k)
            compared += 1
    assert compared >= 4, (shape, compared)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", QUAD_SHAPES)
def test_float32_matrix_core_rows_follow_the_oracles_over_the_leading_entries(shape):
    worst = (0.0, "", 0, 0, 0, 0.0, 0.0)
    rows = [r for r in rows_to_run(shape, 0) if has_matrix_cores(shape, r, 0)]
    assert rows, shape
    for row in rows:
        for B in batches(shape, row, 0):
            out = run(shape, row, 0, B)
            for b in range(B):
                r64, L = oracle64(shape, b), leading(shape, b)
                assert list(out["alphaOut"][b][:L]) == list(r64["alphaOut"][:L]), (shape, row, B, b, list(out["alphaOut"][b]), list(r64["alphaOut"]))
                for i in range(L):
                    ek = abs(float(out["Jout"][b][i]) / r64["Jout"][i] - 1.0)
                    eo = max(abs(float(oracle32(shape, b, v)["Jout"][i]) / r64["Jout"][i] - 1.0) for v in ("strict", "fma"))
                    worst = max(worst, (ek / max(eo, J_FLOOR / J_FACTOR), row, B, b, i, ek, eo))
                    assert ek <= max(J_FLOOR, J_FACTOR * eo), (shape, row, "B", B, "problem", b, "entry", i, ek, eo)
    print("%s: float32 matrix-core rows, worst |J / J64 - 1| over max(the larger float32 oracle's, %.1e): %.2f (bound %.0f) at row %s B %d problem %d entry %d: %.2e against %.2e"
          % ((shape, J_FLOOR / J_FACTOR, worst[0], J_FACTOR) + worst[1:]))


def other_record(plant, b):
    """a diagonal record that differs from the built-in one in every entry"""
    rng = np.random.default_rng(7000 + 100 * plant + b)
    return BUILTIN[plant] * rng.uniform(0.5, 2.0, BUILTIN[plant].size)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,row", POLICY_CASES, ids=["%s-%s" % c for c in POLICY_CASES])
def test_float64_goal_trajectory_handles_follow_the_shim_oracle(shape, row):
    plant, N = SHAPES[shape][0], SHAPES[shape][1]
    kw, B = shape_kw(shape), batch2(shape, row, 1)
    probs = [problem(shape, b) for b in range(B)]
    odd = [b for b in range(B) if b % 2 == 1]
    trajs = [trajectory(plant, N, 1, probs[b], b) if b % 2 == 1 else None for b in range(B)]
    recs = {b: other_record(plant, b) for b in odd}
    s = handle(shape, row, 1, B)
    set_trajectories(s, trajs)
    s.set_diag_cost_problems(odd, np.stack([recs[b] for b in odd]))
    assert [n for n, _ in s.time_kernels(1)] == expected_names(shape, row, 1), "the tables changed the family"
    out = s.solve(*stacked(shape, B, 1))
    s.close()
    plain = run(shape, row, 1, B)
    for b in range(B):
        if b % 2 == 1:
            ref = shim_oracle(plant, kw, trajs[b], rec=recs[b]).run_ilqr_gpusem(probs[b]["x0"], probs[b]["u0"], probs[b]["xg"])
            assert not np.array_equal(ref["Jout"], oracle64(shape, b)["Jout"]), "the trajectory and the record changed nothing"
        else:
            ref = oracle64(shape, b)
            assert np.array_equal(out["Jout"][b], plain["Jout"][b]) and np.array_equal(out["x"][b], plain["x"][b]), (shape, row, b, "a problem without a trajectory differs from the plain handle's")
        check_against_oracle(out, b, ref, (shape, row, "GoalTab", "problem", b))
