"""The arm's kernel families at the edges of the accepted N, M, A domain (config_complaint, csrc/handle_setup.hpp: N a power of two in [4, 1024], M <= 16 with M | N and
N / M >= 2, A in [1, 64]): N = 4 (sixteen problems share a 64-knot chunk of the compact [A B] and a wavefront of k_nis_tl), two-knot segments (every knot a block's first
and last), M = 16 (fifteen segment maps), M = 2 / 8 (the branch of pddp_mx.hip that M = 4 does not take), one candidate, odd A (a wavefront of k_fp_tl4 straddles problems
and k_ls returns), A = 64, M A > 64, M A > 128 (k_fp_lg divides the candidates over workgroups: kernel_plan.hpp fp_lg_chunks), N / M > 96 (k_sweep_wg hands over to
k_sweep_st), N = 512 and N = 1024.  The arm integrates with Euler steps only (pddp_plant_arm.hip), so every shape does; there is no midpoint / RK3 shape to add.

SHAPES is closed; every shape runs every ROW (a selection pinned through pddp_config.kernels), and EXPECT states BY HAND which kernels each (shape, row) resolves to on a
float handle -- fallbacks included -- as  backward pass / linear sweep / rollouts / line search / setup;  F64_ROW_IS and F64_SWEEP state what differs on a double handle.
A row that resolves to the kernels of an earlier row at a shape is not run twice there.  The GPU test asserts the table through pddp_time_kernels (and the compact [A B]
through the handle's arrays), the CPU suite through make_kernel_plan (tests/native/kernel_plan_host_check.cpp).

Inputs (fixed): problem b of a shape is the example's inputs with velocity noise normal(0, 0.002 (b mod 5 + 1)) from default_rng(4000 + 100 b + N + M + A); the shape
with the end-effector cost starts from the posture of tests/test_ee_thread_lanes.py with the same noise and a goal point moved by b.  tol_cost = 0, max_iter = 8 (4 from N = 512 on),
total_time per shape (TOTAL_TIME).

Comparisons:
  1  float64, every row, B = 1 and B2, per problem against the oracle's GPU-semantics driver: iters and alphaOut identical, J, x, u within 1e-7 and KT within 1e-6 of the
     largest reference element (the arm's float64 bounds, tests/test_f64_benched_family.py); the rows off the matrix cores and thread lanes (coop, lg, wide) within the
     tighter bounds of test_closed_form_edges.check_against_oracle;
  2  the rows without a matrix-core or thread-lane kernel whose sweep is the per-candidate one (coop-lg, lg-alpha, wide; on a double handle and with one segment also
     lg), float32 and float64, bit for bit the coop handle on the same inputs (the coop-lg handle on a double handle with M = 16, where pddp_create refuses k_fp's
     sixteen scratch areas; A14, M = 8 with twenty candidates, is the shape at which a k_fp_lg divided over two workgroups meets k_fp itself in float64):
     x, u, KT, Jout, alphaOut, dmax and the cost-to-go P, p;
  3  float32 rows with k_bp_mfma / k_fp_tl* / k_sweep_st / k_sweep_wg (the two-sequence sweeps round differently from the per-candidate sweep: bitwise()): alphaOut equal to the float64 oracle's over the L leading entries on which {oracle32 strict, oracle32 fma, oracle64} agree
     for that problem, and at EACH of those entries |J / J64 - 1| <= max(the shape's floor, 4 x the larger of the two float32 oracles' deviations at that
     entry); the floor is max(1e-5, 4 x J_ORACLE_DEV[shape]), the oracles' worst deviation over the shape's problems;
  4  every problem of B2 on the mx-tl and mx-tl4 rows at N = 4 and N = 8, float32, bit for bit the same problem alone in a B = 1 handle pinned to the same row;
  5  (CPU) the host emulation's arm bodies (fp = coop and fp = lg) at every shape in float64 with the bounds of 1, and the conditions the inputs must meet, on the oracles
     alone: every problem accepts an iteration in float64, and L >= 3.

B2 has a partial last wave for the row's kernels that pack problems into wavefronts (batch2, each rule from the kernel's launcher): k_fp_tl (B2 M A) % 256 != 0,
k_fp_tl4 (B2 M A) % 64 != 0, k_bp_lg (B2 M) % 8 != 0, k_sweep_st (2 B2) % 8 != 0, and for k_nis_tl / k_nis_tl7 and the chunks of the compact [A B], where N < 64 lets a
batch achieve it, (B2 N) % 64 != 0 behind at least one full wave / chunk.  B2 <= 3 for N >= 512, <= 5 for N = 256, <= 67 otherwise.  profiles/arm_edges.md records the batches, the
oracles' L and deviations, the measured float32 ratios and the added GPU time.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pyddp
from backends import make_solver
from oracle_binding import Oracle, default_cfg, example_inputs
from test_closed_form_edges import check_against_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# id: N, M, A, integrator, end-effector cost
SHAPES = {
    "A1": (4, 1, 8, 1, 0),        # smallest horizon, single shooting: 16 problems per wavefront of k_nis_tl and per chunk of the compact [A B]
    "A2": (4, 2, 1, 1, 0),        # smallest horizon, 2-knot segments, one candidate on the thread lanes
    "A3": (8, 4, 3, 1, 0),        # 2-knot segments: every knot a block's first and last; odd A, M A = 12 does not divide 64
    "A4": (32, 16, 5, 1, 0),      # M = 16, 2-knot segments, fifteen maps; odd A; M A = 80
    "A5": (32, 16, 12, 1, 0),     # M A = 192 lane groups: k_fp_lg in two workgroups of 6 candidates
    "A6": (16, 2, 7, 1, 0),       # M = 2, A = 7
    "A7": (64, 8, 16, 1, 0),      # M = 8, M A = 128 > 64: a problem spans two wavefronts of k_fp_tl4
    "A8": (16, 1, 64, 1, 0),      # A = 64: a problem spans a whole wavefront of k_fp_tl4, eight workgroups of k_fp_lg
    "A9": (128, 1, 4, 1, 0),      # N / M = 128 > 96 with one segment: sweep_kind steps aside to k_sweep_st, and no sweep runs
    "A10": (256, 16, 4, 1, 0),    # N = 256 with M = 16; M A = 64: k_fp_tl4 begins with the sweep over fifteen maps
    "A11": (512, 4, 4, 1, 0),     # N = 512; N / M = 128 > 96: a request for k_sweep_wg comes out as k_sweep_st
    "A12": (1024, 8, 8, 1, 0),    # the longest horizon
    "A13": (16, 4, 4, 1, 1),      # end-effector cost (ee_cost = 1, mpc_mode = 1, ignore_max_rho_exit = 0); M A = 16: k_fp_tl4 begins with the sweep
    "A14": (16, 8, 20, 1, 0),     # M A = 160 lane groups with M = 8: k_fp_lg in two workgroups of 10 candidates on a double handle that still takes the coop row (A5's does not)
}
ROWS = {
    "coop": dict(bp="coop", fp="coop"),
    "coop-lg": dict(bp="coop", fp="lg", sweep="alpha"),    # the cooperative backward pass in front of the lane groups: comparison 2's reference where create refuses the coop row
    "lg": dict(bp="lg", fp="lg"),
    "lg-alpha": dict(bp="lg", fp="lg", sweep="alpha"),
    "lg-st": dict(bp="lg", fp="lg", sweep="st"),
    "lg-wg": dict(bp="lg", fp="lg", sweep="wg"),
    "wide": dict(bp="wide", fp="lg", sweep="alpha"),   # (bp = wide alone leaves a float handle's rollouts on the thread lanes: the row pins them, and the sweep, for comparison 2)
    "mx-lg": dict(bp="mx", fp="lg"),
    "mx-tl": dict(bp="mx", fp="tl"),
    "mx-tl-full": dict(bp="mx", fp="tl", ab="full"),
    "mx-tl4": dict(bp="mx", fp="tl4"),
    "mx-tl4-maps": dict(bp="mx", fp="tl4", sweep="maps"),
    "mx-tl4-lswg": dict(bp="mx", fp="tl4", ls="wg"),
    "mx-tl2": dict(bp="mx", fp="tl2"),                 # float, joint-space cost; otherwise the row below
    "mx-tl-many": dict(bp="mx", fp="tl", ls="many"),
}
# What every (shape, row) resolves to on a FLOAT handle, written out by hand in the order of ROWS:  backward pass / linear sweep / rollouts / line search / setup.
#   bp: co k_bp, wide k_bp_wide, lg k_bp_lg, mx k_bp_mfma on the reference-layout [A B], mxc k_bp_mfma on the compact [A B] (the handle has the array ABc)
#   sweep: - none (one segment, or k_fp / k_fp_tl4 sweeps itself), al k_sweep_lg, st k_sweep_st, wg k_sweep_wg, maps k_sweep_maps
#   rollouts: co k_fp, lg k_fp_lg, tl k_fp_tl, tl2 k_fp_tl2, tl4 k_fp_tl4     line search: - (k_fp_tl4 ends with it), wg k_ls, many k_ls_many
#   setup: co k_nis, lg k_nis_lg, tl k_nis_tl, tl7 k_nis_tl7
_ONE_SEGMENT = ("co/-/co/wg/co  co/-/lg/wg/lg  lg/-/lg/wg/lg  lg/-/lg/wg/lg  lg/-/lg/wg/lg  lg/-/lg/wg/lg  wide/-/lg/wg/lg  mx/-/lg/wg/lg  mxc/-/tl/wg/tl  mx/-/tl/wg/tl  "
                "mx/-/tl4/-/tl7  mx/-/tl4/-/tl7  mx/-/tl4/wg/tl7  mx/-/tl2/wg/tl7  mxc/-/tl/many/tl")            # M A divides 64: k_fp_tl4 ends with the line search
_STRADDLING = ("co/-/co/wg/co  co/al/lg/wg/lg  lg/wg/lg/wg/lg  lg/al/lg/wg/lg  lg/st/lg/wg/lg  lg/wg/lg/wg/lg  wide/al/lg/wg/lg  mx/maps/lg/wg/lg  mxc/maps/tl/wg/tl  mx/maps/tl/wg/tl  "
               "mx/maps/tl4/wg/tl7  mx/maps/tl4/wg/tl7  mx/maps/tl4/wg/tl7  mx/maps/tl2/wg/tl7  mxc/maps/tl/many/tl")  # M A does not divide 64: k_ls returns
EXPECT = {
    "A1": _ONE_SEGMENT,
    # M A = 2 divides 64 but is below 16: k_fp_tl4 ends with the line search and leaves the sweep to k_sweep_maps
    "A2": "co/-/co/wg/co  co/al/lg/wg/lg  lg/wg/lg/wg/lg  lg/al/lg/wg/lg  lg/st/lg/wg/lg  lg/wg/lg/wg/lg  wide/al/lg/wg/lg  mx/maps/lg/wg/lg  mxc/maps/tl/wg/tl  mx/maps/tl/wg/tl  "
          "mx/maps/tl4/-/tl7  mx/maps/tl4/-/tl7  mx/maps/tl4/wg/tl7  mx/maps/tl2/wg/tl7  mxc/maps/tl/many/tl",
    "A3": _STRADDLING,
    "A4": _STRADDLING,
    "A5": _STRADDLING,
    "A6": _STRADDLING,
    "A7": _STRADDLING,
    "A8": _ONE_SEGMENT,
    "A9": _ONE_SEGMENT,
    # M A = 64: k_fp_tl4 begins with the sweep and ends with the line search; sweep = maps keeps k_sweep_maps, ls = wg keeps k_ls
    "A10": "co/-/co/wg/co  co/al/lg/wg/lg  lg/wg/lg/wg/lg  lg/al/lg/wg/lg  lg/st/lg/wg/lg  lg/wg/lg/wg/lg  wide/al/lg/wg/lg  mx/maps/lg/wg/lg  mxc/maps/tl/wg/tl  mx/maps/tl/wg/tl  "
           "mx/-/tl4/-/tl7  mx/maps/tl4/-/tl7  mx/-/tl4/wg/tl7  mx/maps/tl2/wg/tl7  mxc/maps/tl/many/tl",
    # N / M = 128 knots do not fit the 96-knot staging area of k_sweep_wg: the default and the request for it come out as k_sweep_st
    "A11": "co/-/co/wg/co  co/al/lg/wg/lg  lg/st/lg/wg/lg  lg/al/lg/wg/lg  lg/st/lg/wg/lg  lg/st/lg/wg/lg  wide/al/lg/wg/lg  mx/maps/lg/wg/lg  mxc/maps/tl/wg/tl  mx/maps/tl/wg/tl  "
           "mx/-/tl4/-/tl7  mx/maps/tl4/-/tl7  mx/-/tl4/wg/tl7  mx/maps/tl2/wg/tl7  mxc/maps/tl/many/tl",
    "A12": "co/-/co/wg/co  co/al/lg/wg/lg  lg/st/lg/wg/lg  lg/al/lg/wg/lg  lg/st/lg/wg/lg  lg/st/lg/wg/lg  wide/al/lg/wg/lg  mx/maps/lg/wg/lg  mxc/maps/tl/wg/tl  mx/maps/tl/wg/tl  "
           "mx/-/tl4/-/tl7  mx/maps/tl4/-/tl7  mx/-/tl4/wg/tl7  mx/maps/tl2/wg/tl7  mxc/maps/tl/many/tl",
    # end-effector cost: k_fp_tl2 carries the joint-space cost only, the request comes out as k_fp_tl4
    "A13": "co/-/co/wg/co  co/al/lg/wg/lg  lg/wg/lg/wg/lg  lg/al/lg/wg/lg  lg/st/lg/wg/lg  lg/wg/lg/wg/lg  wide/al/lg/wg/lg  mx/maps/lg/wg/lg  mxc/maps/tl/wg/tl  mx/maps/tl/wg/tl  "
           "mx/-/tl4/-/tl7  mx/maps/tl4/-/tl7  mx/-/tl4/wg/tl7  mx/-/tl4/-/tl7  mxc/maps/tl/many/tl",
    "A14": _STRADDLING,
}
# A DOUBLE handle: k_sweep_st, k_sweep_wg and k_fp_tl2 exist in float only.  Every sweep off the maps is k_sweep_lg, so the three sweep rows are the lg row; a request
# for k_fp_tl2 leaves the rollouts and the setup on lane groups, which is the mx-lg row.
F64_ROW_IS = {"lg-alpha": "lg", "lg-st": "lg", "lg-wg": "lg", "mx-tl2": "mx-lg"}
F64_SWEEP = {"st": "al", "wg": "al"}
# ... and k_fp keeps one scratch area per segment in LDS: sixteen of them in double are 295 KiB, and pddp_create refuses the coop row ("reduce M")
def refused(shape, row, dtype):
    return dtype == 1 and row == "coop" and SHAPES[shape][1] == 16



BP_NAME = dict(co="k_bp", wide="k_bp_wide", lg="k_bp_lg", mx="k_bp_mfma", mxc="k_bp_mfma")
SWEEP_NAME = {"-": None, "al": "k_sweep_lg", "st": "k_sweep_st", "wg": "k_sweep_wg", "maps": "k_sweep_maps"}
FP_NAME = dict(co="k_fp", lg="k_fp_lg", tl="k_fp_tl", tl2="k_fp_tl2", tl4="k_fp_tl4")
LS_NAME = {"-": None, "wg": "k_ls", "many": "k_ls_many"}
NIS_NAME = dict(co="k_nis", lg="k_nis_lg", tl="k_nis_tl", tl7="k_nis_tl7")
SHAPE_PARAMS = list(SHAPES)
ALONE_ROWS = ("mx-tl", "mx-tl4")                                   # comparison 4 ...
ALONE_SHAPES = [s for s in SHAPES if SHAPES[s][0] <= 8]            # ... where chunks and wavefronts are shared by the most problems
# comparison 3.  The closed-form file's floor of 1e-5 is 4 x 2.5e-6, the deviation its float32 oracles stay under.  The arm's two float32 oracles deviate from the
# float64 oracle by more than that at several shapes: J_ORACLE_DEV is the worst |J32 / J64 - 1| over the leading entries of all the problems the shape uses, either
# oracle, measured on the CPU and rounded up (the input-conditions test asserts and prints it; profiles/arm_edges.md).  A kernel with a third summation order is one more
# draw from that error, so the floor of a shape is 4 x its figure -- the oracles' own, never the kernel's.
J_FACTOR = 4.0
J_ORACLE_DEV = {"A1": 1.5e-3, "A2": 2.4e-3, "A3": 7e-6, "A4": 2.5e-6, "A5": 1.7e-4, "A6": 2.5e-6, "A7": 3.1e-5, "A8": 1.3e-3, "A9": 7e-6, "A10": 2.5e-6, "A11": 5e-6,
                "A12": 2.5e-6, "A13": 1.1e-5, "A14": 2.8e-4}


def j_floor(shape):
    return max(1e-5, J_FACTOR * J_ORACLE_DEV[shape])


# total_time per shape, chosen on the oracles alone (profiles/arm_edges.md): every problem accepts an iteration and the three oracles agree on three entries or more
TOTAL_TIME = {"A1": 0.03125, "A2": 0.25, "A3": 0.03125, "A4": 0.03125, "A5": 0.125, "A6": 0.03125, "A7": 0.03125, "A8": 0.25, "A9": 0.03125, "A10": 0.03125, "A11": 0.25, "A12": 0.5, "A13": 0.0625, "A14": 0.03125}

# max_iter: 4 where a float64 oracle solve takes most of a second (N >= 512), and at A8, whose float32 oracles spread to 1.5e-3 of J by the seventh entry
MAX_ITER = {"A8": 4, "A11": 4, "A12": 4}


def shape_kw(shape):
    N, M, A, integ, ee = SHAPES[shape]
    kw = dict(N=N, M=M, A=A, integrator=integ, wafr_urdf=1, total_time=TOTAL_TIME.get(shape, 0.5), tol_cost=0.0, max_iter=MAX_ITER.get(shape, 8))
    if ee:
        kw.update(ee_cost=1, mpc_mode=1, ignore_max_rho_exit=0)
    return kw


def resolved(shape, row, dtype):
    """(bp, sweep, fp, ls, nis) of EXPECT for the handle's element type"""
    if dtype == 1:
        row = F64_ROW_IS.get(row, row)
    cells = EXPECT[shape].split()
    assert len(cells) == len(ROWS), (shape, cells)
    bp, sw, fp, ls, nis = cells[list(ROWS).index(row)].split("/")
    if dtype == 1:
        sw = F64_SWEEP.get(sw, sw)
    return bp, sw, fp, ls, nis


def expected_names(shape, row, dtype):
    bp, sw, fp, ls, nis = resolved(shape, row, dtype)
    return [n for n in (BP_NAME[bp], SWEEP_NAME[sw], FP_NAME[fp], LS_NAME[ls], NIS_NAME[nis]) if n]


def rows_to_run(shape, dtype):
    """the rows of a shape without those that resolve to the kernels of an earlier row"""
    seen, out = set(), []
    for row in ROWS:
        r = resolved(shape, row, dtype)
        if r not in seen and not refused(shape, row, dtype):
            seen.add(r); out.append(row)
    return out


def on_matrix_cores_or_thread_lanes(shape, row, dtype):
    bp, sw, fp, ls, nis = resolved(shape, row, dtype)
    return bp in ("mx", "mxc") or fp in ("tl", "tl2", "tl4")


def bitwise(shape, row, dtype):
    """comparison 2 applies: no matrix-core or thread-lane kernel, and the sweep is the per-candidate one.  k_sweep_st / k_sweep_wg walk TWO sequences per problem and form
    every candidate's states as t_k - alpha s_k ("k_sweep_st"): another rounding than the per-candidate sweep's, so those float rows are held as in comparison 3"""
    return not on_matrix_cores_or_thread_lanes(shape, row, dtype) and resolved(shape, row, dtype)[1] in ("-", "al")


def batch2(shape, row, dtype):
    """the batch with a partial last wave for every kernel of the row that packs problems into wavefronts"""
    N, M, A, integ, ee = SHAPES[shape]
    bp, sw, fp, ls, nis = resolved(shape, row, dtype)
    conds = []
    if fp == "tl":
        conds.append(lambda B: (B * M * A) % 256 != 0)
    if fp == "tl4":
        conds.append(lambda B: (B * M * A) % 64 != 0)
    if bp == "lg":
        conds.append(lambda B: (B * M) % 8 != 0)
    if sw == "st":
        conds.append(lambda B: (2 * B) % 8 != 0)
    if (nis in ("tl", "tl7") or bp == "mxc") and N < 64:            # (N a multiple of 64: every batch fills its waves and chunks)
        conds.append(lambda B: (B * N) % 64 != 0 and B * N > 64)
    cap = 3 if N >= 512 else 5 if N >= 256 else 67                          # (a float64 oracle solve of N = 1024 takes most of a second)
    conds = [c for c in conds if any(c(B) for B in range(1, cap + 1))]      # (M = 8 / 16 fill every wave of k_bp_lg, M A a multiple of 64 every wave of k_fp_tl4)
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
        N, M, A, integ, ee = SHAPES[shape]
        rng = np.random.default_rng(4000 + 100 * b + N + M + A)
        x0, u0, xg = example_inputs(4, N, np.float64, noise=rng.normal(0, 0.002 * (b % 5 + 1), (N, 14)))
        if ee:                                                       # the posture and the goal point of tests/test_ee_thread_lanes.py
            x0 = x0.reshape(N, 14).copy(); x0[:, :7] = 0.0; x0[:, 1] = 0.7; x0[:, 3] = -0.8; x0[:, 5] = 0.75; x0 = x0.ravel()
            u0 = np.full(N * 7, 0.01)
            xg = np.zeros(14); xg[:3] = [0.45, 0.15 + 0.01 * (b % 7), 0.75]
        _PROB[(shape, b)] = dict(x0=x0, u0=u0, xg=xg)
    return _PROB[(shape, b)]


def typed(p, dtype):
    T = np.float32 if dtype == 0 else np.float64
    return {k: v.astype(T) for k, v in p.items()}


def stacked(shape, problems, dtype):
    probs = [typed(problem(shape, b), dtype) for b in problems]
    return tuple(np.concatenate([p[k].ravel() for p in probs]) for k in ("x0", "u0", "xg"))


def oracle(shape, b, which):
    """which: "f64", or the float32 oracle's variant, "strict" | "fma" """
    key = (shape, b, which)
    if key not in _ORA:
        T = np.float64 if which == "f64" else np.float32
        p = typed(problem(shape, b), 1 if which == "f64" else 0)
        o = Oracle(default_cfg(4, cores=1, spawn_threads=0, **shape_kw(shape)), T, **({} if which == "f64" else dict(variant=which)))
        with np.errstate(all="ignore"):
            _ORA[key] = o.run_ilqr_gpusem(p["x0"], p["u0"], p["xg"])
    return _ORA[key]


def leading(shape, b):
    """L: the leading entries of alphaOut on which the two float32 oracles and the float64 oracle agree"""
    r64, rs, rf = oracle(shape, b, "f64"), oracle(shape, b, "strict"), oracle(shape, b, "fma")
    top = r64["iters"] + 1
    return next((i for i in range(top) if not (rs["alphaOut"][i] == rf["alphaOut"][i] == r64["alphaOut"][i])), top)


def oracle_deviation(shape, b, i):
    """the larger of the two float32 oracles' |J / J64 - 1| at entry i"""
    return max(abs(float(oracle(shape, b, v)["Jout"][i]) / oracle(shape, b, "f64")["Jout"][i] - 1.0) for v in ("strict", "fma"))


def check_against_oracle_arm(out, j, ref, label):
    """comparison 1 for problem j of a batch on a row with matrix cores or thread lanes: the arm's float64 bounds (tests/test_f64_benched_family.py)"""
    it = ref["iters"]
    assert np.isfinite(ref["Jout"][: it + 1]).all() and np.isfinite(ref["x"]).all() and np.isfinite(ref["KT"]).all(), (label, "a non-finite reference")
    assert int(out["iters"][j]) == it, (label, "iters", int(out["iters"][j]), it)
    assert list(out["alphaOut"][j][: it + 1]) == list(ref["alphaOut"][: it + 1]), (label, list(out["alphaOut"][j]), list(ref["alphaOut"]))
    np.testing.assert_allclose(out["Jout"][j][: it + 1], ref["Jout"][: it + 1], rtol=1e-7, atol=0, err_msg=str(label))
    for k in ("x", "u"):
        np.testing.assert_allclose(out[k][j].ravel(), ref[k], rtol=0, atol=1e-7 * np.abs(ref[k]).max(), err_msg=str((label, k)))
    np.testing.assert_allclose(out["KT"][j].ravel(), ref["KT"], rtol=0, atol=1e-6 * np.abs(ref["KT"]).max(), err_msg=str((label, "KT")))


def has_array(s, name):
    nb = ctypes.c_size_t(0)
    return s.lib.pddp_array_bytes(s.h, name.encode(), ctypes.byref(nb)) == 0 and nb.value != 0


def handle(shape, row, dtype, B):
    """a handle pinned to the row; the kernels it reports are the ones written out in EXPECT"""
    if refused(shape, row, dtype):
        with pytest.raises(pyddp.PddpError, match="LDS footprint exceeds 160 KiB: reduce M"):
            make_solver("hip", 4, dtype=dtype, batch=B, kernels=dict(ROWS[row]), **shape_kw(shape))
        return None
    s = make_solver("hip", 4, dtype=dtype, batch=B, kernels=dict(ROWS[row]), **shape_kw(shape))
    names = [n for n, _ in s.time_kernels(1) if n]
    assert names == expected_names(shape, row, dtype), (shape, row, dtype, names, expected_names(shape, row, dtype))
    assert has_array(s, "ABc") == (resolved(shape, row, dtype)[0] == "mxc"), (shape, row, dtype, "ABc")
    return s


def run(shape, row, dtype, problems):
    """the whole solve of the named problems on the row's kernels, once per session"""
    key = (shape, row, dtype, tuple(problems))
    if key not in _RUN:
        s = handle(shape, row, dtype, len(problems))
        out = s.solve(*stacked(shape, problems, dtype))
        assert out["done"].all(), key
        out["P"], out["p"] = s.get_cost_to_go()[:2]
        s.close()
        _RUN[key] = out
    return _RUN[key]


def batches(shape, row, dtype):
    return (1, batch2(shape, row, dtype))


# ---------------------------------------------------------------------------------------------------------------- CPU: the inputs, the table, the host emulation
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_every_problem_accepts_an_iteration_and_the_oracles_agree_on_three_entries(shape):
    """Every problem any batch of the shape uses accepts an iteration in the float64 oracle, has a finite reference, and L >= 3; the float32 oracles' deviation of J over
    the leading entries stays under the shape's J_ORACLE_DEV, the figure the floor of comparison 3 is made of."""
    worst_L, worst_dev, rejecting = 99, 0.0, []
    for b in range(problems_needed(shape)):
        r64 = oracle(shape, b, "f64")
        it = r64["iters"]
        assert np.isfinite(r64["Jout"][: it + 1]).all() and np.isfinite(r64["x"]).all() and np.isfinite(r64["u"]).all() and np.isfinite(r64["KT"]).all(), (shape, b)
        if sum(a >= 0 for a in r64["alphaOut"][1: it + 1]) < 1:
            rejecting.append(b)
        L = leading(shape, b)
        assert L >= 3, (shape, b, L, list(oracle(shape, b, "strict")["alphaOut"]), list(oracle(shape, b, "fma")["alphaOut"]), list(r64["alphaOut"]))
        worst_L, worst_dev = min(worst_L, L), max(worst_dev, max(oracle_deviation(shape, b, i) for i in range(L)))
        # no accepted step among the leading entries may leave J where it was at float32 resolution: a converged solve accepts whichever candidate rounds lowest
        stalled = [i for i in range(1, L) if r64["alphaOut"][i] >= 0 and abs(r64["Jout"][i] / r64["Jout"][i - 1] - 1.0) < 1e-6]
        assert not stalled, (shape, b, "accepted steps that change J by less than 1e-6 of it", stalled)
    assert rejecting == [], (shape, "problems without an accepted iteration", rejecting)
    print("%s: %d problems, worst L %d, worst float32-oracle deviation of J over the leading entries %.2e" % (shape, problems_needed(shape), worst_L, worst_dev))
    assert worst_dev <= J_ORACLE_DEV[shape], (shape, worst_dev)


def test_the_table_names_every_row_of_every_shape_and_drops_only_repeats():
    assert list(EXPECT) == list(SHAPES)
    for shape in SHAPES:
        for dtype in (0, 1):
            run_rows = rows_to_run(shape, dtype)
            assert run_rows[0] == ("coop-lg" if refused(shape, "coop", dtype) else "coop") and len({resolved(shape, r, dtype) for r in run_rows}) == len(run_rows)
            for row in ROWS:
                expected_names(shape, row, dtype)
            assert {"coop-lg", "lg", "wide", "mx-lg", "mx-tl", "mx-tl-full", "mx-tl4", "mx-tl-many"} <= set(run_rows), (shape, dtype, run_rows)
    dims = [SHAPES[s][:3] for s in SHAPES]
    assert {(4, 1), (4, 2), (8, 4), (32, 16), (256, 16)} <= {(N, M) for N, M, A in dims} and {2, 8} <= {M for N, M, A in dims} and {512, 1024} <= {N for N, M, A in dims}
    assert {1, 3, 5, 7, 64} <= {A for N, M, A in dims} and (32, 16, 12) in dims and (64, 8, 16) in dims and any(M == 1 and N > 96 for N, M, A in dims)
    assert any(M > 1 and N // M > 96 for N, M, A in dims) and sum(SHAPES[s][4] for s in SHAPES) == 1
    # the hand-over: wherever a segment is longer than the staging area of k_sweep_wg, no row resolves to it
    for shape in SHAPES:
        if SHAPES[shape][0] // SHAPES[shape][1] > 96:
            assert all(resolved(shape, row, 0)[1] != "wg" for row in ROWS), shape


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("arm_edges") / "kernel_plan_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "kernel_plan_host_check.cpp"), "-o", exe])
    return exe


def test_the_table_is_what_make_kernel_plan_resolves(host_check):
    """every (shape, row, element type, batch) of the GPU tests through make_kernel_plan + plan_kernel_names: the same names, and the compact [A B] where the table says mxc"""
    cases, text = [], ""
    for shape in SHAPES:
        N, M, A, integ, ee = SHAPES[shape]
        for dtype in (0, 1):
            for row in ROWS:
                for B in () if refused(shape, row, dtype) else batches(shape, row, dtype):
                    k = pyddp.set_kernels(pyddp.PddpConfig(), **ROWS[row]).kernels
                    fields = [4, dtype, N, M, A, integ, B, ee, 0, ee, 0] + [getattr(k, f) for f, _ in pyddp.PddpKernelSelection._fields_]
                    cases.append((shape, row, dtype, B)); text += " ".join(str(v) for v in fields) + "\n"
    out = subprocess.run([host_check, "rows"], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    wrong = []
    for (shape, row, dtype, B), line in zip(cases, lines):
        names, arrays = line.split("|")
        if names.split() != expected_names(shape, row, dtype) or bool(int(arrays.split()[2])) != (resolved(shape, row, dtype)[0] == "mxc"):
            wrong.append((shape, row, dtype, B, line, expected_names(shape, row, dtype)))
    assert not wrong, wrong[:5]


@pytest.mark.parametrize("fp", ["coop", "lg"])
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_host_emulation_of_the_arm_bodies_follows_the_oracle(shape, fp):
    B = 2 if SHAPES[shape][0] >= 256 else 5
    s = make_solver("hostsim", 4, dtype=1, batch=B, kernels=dict(bp=fp, fp=fp), **shape_kw(shape))
    out = s.solve(*stacked(shape, range(B), 1))
    assert out["done"].all()
    for b in range(B):
        check_against_oracle(out, b, oracle(shape, b, "f64"), (shape, "hostsim", fp, b))
    s.close()


# ---------------------------------------------------------------------------------------------------------------- GPU: the kernels behind every row
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_rows_resolve_to_the_kernels_written_out_by_hand(shape):
    """every row, the dropped repeats included, float32 and float64"""
    for dtype in (0, 1):
        for row in ROWS:
            s = handle(shape, row, dtype, 1)
            assert (s is None) == refused(shape, row, dtype)
            if s is not None:
                s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_float64_rows_follow_the_oracle(shape):
    for row in rows_to_run(shape, 1):
        check = check_against_oracle_arm if on_matrix_cores_or_thread_lanes(shape, row, 1) else check_against_oracle
        for B in batches(shape, row, 1):
            out = run(shape, row, 1, range(B))
            for b in range(B):
                check(out, b, oracle(shape, b, "f64"), (shape, row, "B", B, "problem", b))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_rows_off_matrix_cores_and_thread_lanes_equal_the_cooperative_kernels_bit_for_bit(shape, dtype):
    compared = 0
    for row in rows_to_run(shape, dtype):
        reference = "coop-lg" if refused(shape, "coop", dtype) else "coop"
        if not bitwise(shape, row, dtype) or row == reference:
            continue
        for B in batches(shape, row, dtype):
            a, c = run(shape, row, dtype, range(B)), run(shape, reference, dtype, range(B))
            assert np.array_equal(a["iters"], c["iters"]), (shape, row, B, "iters")
            for k in ("x", "u", "KT", "Jout", "alphaOut", "dmax", "P", "p"):
                assert np.array_equal(a[k], c[k], equal_nan=True), (shape, row, "B", B, k)
            compared += 1
    assert compared >= (4 if reference == "coop" else 2), (shape, compared)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_float32_rows_that_round_differently_follow_the_oracles_over_the_leading_entries(shape):
    worst = (0.0, "", 0, 0, 0, 0.0, 0.0)
    rows = [r for r in rows_to_run(shape, 0) if not bitwise(shape, r, 0)]
    assert len(rows) >= 5, (shape, rows)
    for row in rows:
        for B in batches(shape, row, 0):
            out = run(shape, row, 0, range(B))
            for b in range(B):
                r64, L = oracle(shape, b, "f64"), leading(shape, b)
                assert list(out["alphaOut"][b][:L]) == list(r64["alphaOut"][:L]), (shape, row, B, b, list(out["alphaOut"][b]), list(r64["alphaOut"]))
                for i in range(L):
                    ek, eo = abs(float(out["Jout"][b][i]) / r64["Jout"][i] - 1.0), oracle_deviation(shape, b, i)
                    worst = max(worst, (ek / max(eo, j_floor(shape) / J_FACTOR), row, B, b, i, ek, eo))
                    assert ek <= max(j_floor(shape), J_FACTOR * eo), (shape, row, "B", B, "problem", b, "entry", i, ek, eo)
    print("%s: float32 rows off comparison 2, worst |J / J64 - 1| over max(the larger float32 oracle's, %.1e): %.2f (bound %.0f) at row %s B %d problem %d entry %d: %.2e against %.2e"
          % ((shape, j_floor(shape) / J_FACTOR, worst[0], J_FACTOR) + worst[1:]))


@pytest.mark.gpu
@pytest.mark.parametrize("row", ALONE_ROWS)
@pytest.mark.parametrize("shape", ALONE_SHAPES)
def test_every_problem_of_a_packed_batch_equals_the_same_problem_alone(shape, row):
    """float32, B2 problems in shared chunks of the compact [A B] and shared wavefronts of k_fp_tl / k_fp_tl4 / k_nis_tl / k_nis_tl7: each bit for bit what a one-problem
    handle pinned to the same row gives for it"""
    B = batch2(shape, row, 0)
    assert B * SHAPES[shape][0] > 64
    batch = run(shape, row, 0, range(B))
    for b in range(B):
        alone = run(shape, row, 0, (b,))
        assert np.any(alone["KT"] != 0) and np.isfinite(alone["KT"]).all(), (shape, row, b, "the backward pass of the problem must run and stay finite")
        bad = [k for k in ("iters", "x", "u", "KT", "Jout", "alphaOut", "P", "p") if not np.array_equal(batch[k][b], alone[k][0], equal_nan=batch[k].dtype.kind == "f")]
        assert not bad, (shape, row, "problem", b, "of", B, "differs from the same problem alone in", bad)
