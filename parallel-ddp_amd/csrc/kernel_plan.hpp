// Which kernel family runs each phase of a handle's sweep: ONE pure function of the configuration, a few compile-time facts of the plant and whether the robot tables are
// a built-in model's.  The Solver (solver_impl.hpp) holds the result as `plan`, its intake area copies it, pddp_time_kernels reports the names resolved here, and its
// launch functions are switches over the plan's kernel enums: launch_bp and launch_nis directly, launch_fp over what plan_fp_launch makes of them for the way the forward
// pass is asked for (FpMode: production, one kernel alone, the initial rollout, the phase hooks).  State that changes while a handle runs (MPC use, an overridden H, a
// dropped compact layout, the line search's mode) is not plan and stays in the Solver.
// Host code only, no HIP header, no environment (tests/native/kernel_plan_host_check.cpp holds it to the recorded selection table without a GPU).
#pragma once
#include <cstddef>

#include "../../include/pddp.h"

namespace pddp {

// pddp_config.kernels by name: the numbers documented in include/pddp.h (pyddp.KERNEL_NAMES lists them in the same order).  0, and any value outside a field's range:
// the library's choice.
enum BpSel { kBpSelAuto = 0, kBpSelMx = 1, kBpSelLg = 2, kBpSelCoop = 3, kBpSelWide = 4 };
enum FpSel { kFpSelAuto = 0, kFpSelTl = 1, kFpSelLg = 2, kFpSelCoop = 3, kFpSelTl2 = 4, kFpSelTl4 = 5 };
enum SweepSel { kSweepSelAuto = 0, kSweepSelAlpha = 1, kSweepSelSt = 2, kSweepSelWg = 3, kSweepSelMaps = 4 };
enum LsSel { kLsSelAuto = 0, kLsSelMany = 1, kLsSelWg = 2 };
enum AbSel { kAbSelAuto = 0, kAbSelFull = 1 };
enum CfSel { kCfSelAuto = 0, kCfSelTs = 1, kCfSelCoop = 2 };
enum CfBpSel { kCfBpSelAuto = 0, kCfBpSelTs = 1, kCfBpSelCoop = 2, kCfBpSelGl = 3, kCfBpSelGl32 = 4, kCfBpSelCl = 5, kCfBpSelMq = 6 };
enum CfFpSel { kCfFpSelAuto = 0, kCfFpSelTs = 1, kCfFpSelCoop = 2, kCfFpSelCf = 3 };
enum CfNisSel { kCfNisSelAuto = 0, kCfNisSelTs = 1, kCfNisSelCoop = 2, kCfNisSelGl = 3, kCfNisSelGl8 = 4, kCfNisSelKb16 = 5, kCfNisSelKb32 = 6, kCfNisSelKb64 = 7, kCfNisSelKb20 = 8 };
template <typename E> constexpr E kernel_sel(int v, E last) { return (v > 0 && v <= (int)last) ? (E)v : (E)0; }
inline BpSel sel_bp(const pddp_config& c) { return kernel_sel(c.kernels.bp, kBpSelWide); }
inline FpSel sel_fp(const pddp_config& c) { return kernel_sel(c.kernels.fp, kFpSelTl4); }
inline SweepSel sel_sweep(const pddp_config& c) { return kernel_sel(c.kernels.sweep, kSweepSelMaps); }
inline LsSel sel_ls(const pddp_config& c) { return kernel_sel(c.kernels.ls, kLsSelWg); }
inline AbSel sel_ab(const pddp_config& c) { return kernel_sel(c.kernels.ab, kAbSelFull); }
inline CfSel sel_cf(const pddp_config& c) { return kernel_sel(c.kernels.cf, kCfSelCoop); }
inline CfBpSel sel_cf_bp(const pddp_config& c) { return kernel_sel(c.kernels.cf_bp, kCfBpSelMq); }
inline CfFpSel sel_cf_fp(const pddp_config& c) { return kernel_sel(c.kernels.cf_fp, kCfFpSelCf); }
inline CfNisSel sel_cf_nis(const pddp_config& c) { return kernel_sel(c.kernels.cf_nis, kCfNisSelKb20); }

// The kernel of every slot of pddp_time_kernels that has one (slot 4, the former winner re-roll, has none); the numbers index kKernelNames.
enum BpKernel { kBpCoop = 0, kBpWide, kBpLg, kBpMfma, kBpTs, kBpGl, kBpCl, kBpMq };
enum SweepKernel { kSweepNone = 8, kSweepLg, kSweepSt, kSweepWg, kSweepMaps, kSweepCf, kSweepMapsCf };      // none: the rollout kernel sweeps itself
enum FpKernel { kFpKernNone = -1, kFpKernCoop = 15, kFpKernLg, kFpKernTl, kFpKernTl2, kFpKernTl4, kFpKernTs, kFpKernCf };        // none: a call for the sweep alone (FpLaunch), never a plan's
enum LsKernel { kLsNone = 22, kLsWg, kLsMany };                                                              // none: the rollout kernel ends with the line search
enum NisKernel { kNisCoop = 25, kNisLg, kNisTl, kNisTl7, kNisTs, kNisGl, kNisKb };
inline const char* kernel_name(int k) {
    static const char* const kKernelNames[32] = {"k_bp", "k_bp_wide", "k_bp_lg", "k_bp_mfma", "k_bp_ts", "k_bp_gl", "k_bp_cl", "k_bp_mq",
                                                 "", "k_sweep_lg", "k_sweep_st", "k_sweep_wg", "k_sweep_maps", "k_sweep_cf", "k_sweep_maps",
                                                 "k_fp", "k_fp_lg", "k_fp_tl", "k_fp_tl2", "k_fp_tl4", "k_fp_ts", "k_fp_cf",
                                                 "", "k_ls", "k_ls_many",
                                                 "k_nis", "k_nis_lg", "k_nis_tl", "k_nis_tl7", "k_nis_ts", "k_nis_gl", "k_nis_kb"};
    return (k >= 0 && k < 32) ? kKernelNames[k] : "";
}

constexpr int kTsMaxN = 256, kTsMaxM = 16;        // longest horizon / most segments the thread-serial forward pass keeps per-knot costs / hand-off states for

// Measured crossovers on MI355X.  "blocks" / "units" are (problem, segment) pairs, batch * M.
// (problem, block) pairs from which the matrix-core backward pass is the default for float handles of the arm (profiles/r02_path_sweep_mx.txt)
constexpr size_t kBpMfmaMinBlocks = 1;
// backward pass of the arm off the matrix cores (Kuka N=128): wide <= 256 problems < cooperative < 1024 <= lane groups.  The lane-group kernel carries 8 (problem, block)
// pairs per wave and wins once the GPU is full; the wave-cooperative kernel has the shorter critical path for a handful of problems; a whole workgroup per block of knots
// (k_bp_wide) for few problems in flight of the plants with 12 states or more
constexpr size_t kBpLgMinBlocks = 4096, kBpWideMaxBlocks = 1024;
constexpr int kNisTl7MaxBatch = 511;              // a split-rollout handle's setup runs on k_nis_tl7 up to here: measured crossover against k_nis_lg (profiles/)
constexpr int kLsManyMinBatch = 2048;             // line search one thread per problem (k_ls_many): from 2048 problems in flight
// closed-form plants (and user plants): one wave per unit while a handful of problems is in flight (the shorter critical path), one thread per unit once the batch fills
// the device (64 units per wave instead of 1); the horizon has to fit the per-thread cost table of k_fp_ts
constexpr size_t kCfSerialMinUnits = 256;
// ... the backward pass thread-serially (small plants) or on lane groups / the matrix cores (12 states) only with the device full
constexpr size_t kCfBpMinUnits = 8192;
// float handles of the arm: the staged workgroup sweep up to 512 problems (profiles/r02b_sweep_wg.txt); a segment has to fit the 96-knot staging area of k_sweep_wg
constexpr int kSweepWgMaxBatch = 512, kSweepWgMaxKnots = 96;

// Which implementation of the arm's forward pass / next-iteration setup a handle uses.  kernels.fp = coop | lg | tl overrides (comparison tests).
//   coop: one wave per unit (fp.hpp, nis.hpp)   lg: 8-lane groups (fp_lg.hpp, nis_lg.hpp)   tl: one thread per instance (fp_tl.hpp)
// Default: tl for float handles of >= 512 problems with an iiwa-structured model (joint-space and end-effector cost); lg otherwise (float64 handles keep
// the reference's operation order, which the 1e-9 parity tests rely on; the initial rollout exists on lane
// groups only; below ~512 problems a thread per knot leaves most of the GPU idle and the lane groups' shorter critical path wins:
// profiles/r02_path_sweep.txt -- one problem: setup 33 us on lane groups, 145 us on thread lanes; 1024 problems: 0.37 ms vs 0.24 ms).
enum FpPath { kFpCoop = 0, kFpLg = 1, kFpTl = 2 };
constexpr int kFpTlMinBatch = 512;
inline FpPath select_fp_path(FpSel sel, bool is_float, bool tl_model_ok, int batch) {
    if (sel == kFpSelCoop) return kFpCoop;
    if (sel == kFpSelLg) return kFpLg;
    if (sel == kFpSelTl2 || sel == kFpSelTl4) return kFpLg;      // the split rollout kernels of a few-problem handle (a lane-group handle otherwise; tl4 also selects them on a double handle)
    if (sel == kFpSelTl && tl_model_ok) return kFpTl;
    return (is_float && tl_model_ok && batch >= kFpTlMinBatch) ? kFpTl : kFpLg;
}
// The same choice for a caller that names the family as pyddp.KERNEL_NAMES["fp"] does (nullptr: the library's choice) and passes the cost family, which the choice
// does not depend on: the host emulation (tests/hostsim), which has no plan.
inline FpPath select_fp_path(const char* name, bool is_float, bool /*ee_cost*/, bool tl_model_ok, int batch) {
    FpSel sel = kFpSelAuto;
    if (name && name[0] == 'c') sel = kFpSelCoop;
    else if (name && name[0] == 'l') sel = kFpSelLg;
    else if (name && name[0] == 't' && name[1] == 'l') sel = name[2] == '2' ? kFpSelTl2 : name[2] == '4' ? kFpSelTl4 : kFpSelTl;
    return select_fp_path(sel, is_float, tl_model_ok, batch);
}

struct PlantTraits { int plant, NX, NU; bool scalar_plugin, plugin_cost; };      // P::PLANT, P::NX, P::NU, P::kScalarPlugin, P::kPluginCost

struct KernelPlan {
    // backward pass
    bool bp_mfma = false;          // matrix-core backward pass, one wavefront per block of knots (bp_mfma.hpp): float handles of the arm; kernels.bp = mx
    bool bp_lane_groups = false;   // the arm on 8-lane groups (k_bp_lg); kernels.bp = lg | coop
    bool bp_wide = false;          // cooperative backward pass with a whole workgroup per block of knots (few problems in flight); kernels.bp = wide
    bool cf_serial = false;        // closed-form plants with many problems in flight: thread-serial kernels (k_bp_ts / k_fp_ts / k_nis_ts); kernels.cf = coop | ts overrides
    bool cf_bp = false, cf_fp = false, cf_nis = false;   // ... per phase
    bool gl_bp = false, gl_nis = false;                  // 16 lanes per unit (k_bp_gl / k_nis_gl): the 12-state plants with the device full; kernels.cf_bp / cf_nis = gl
    bool gl_bp32 = false, gl_nis8 = false;               // 32 lanes per block of knots (k_bp_gl<32>) / 8 lanes per knot (k_nis_gl<8>)
    bool cl_bp = false;            // 12 states + 4 controls: 16 lanes per block of knots, lane = column (k_bp_cl, bp_cl.hpp) instead of k_bp_gl; kernels.cf_bp = cl | gl | gl32
    bool mq_bp = false;            // 12 states + 4 controls on the matrix cores (k_bp_mq, bp_mq.hpp): where k_bp_cl was the choice, for the plant's own diagonal cost Hessian; kernels.cf_bp = mq | cl
    bool mq_fused = false;         // k_bp_mq composes the segments' forward-sweep maps itself (bp_mq.hpp FUSE) and k_sweep_maps_cf finishes: no A - B K / B du traffic, no per-knot sweep; kernels.sweep = st: k_sweep_cf
    // linear sweep
    bool sweep_fused = false;      // production sweeps of the arm: forward-sweep maps composed inside k_bp_mfma + k_sweep_maps (no A - B K / B du traffic)
    int sweep_kind = 0;            // the arm's own linear sweep (also the phase hook's): 0 one lane group per candidate (k_sweep_lg), 1 two sequences on lane groups (k_sweep_st), 2 two sequences, workgroup per problem (k_sweep_wg); kernels.sweep = alpha | st | wg
    // rollouts and setup
    FpPath fp_path = kFpLg;        // the arm's forward pass / next-iteration setup (select_fp_path)
    bool fp_coop = false;          // kernels.fp = coop; the arm with USE_LIMITS_FLAG / USE_SMOOTH_ABS off the thread lanes
    bool fp_split = false;         // rollouts of a lane-group handle on the split thread-lane kernels (k_fp_tl4 / k_fp_tl2)
    bool fp_two_wave = false;
    bool nis_tl7_batch = false;    // batch <= kNisTl7MaxBatch: a split-rollout handle's setup runs on k_nis_tl7
    bool cf_fp_staged = false;     // thread-serial rollouts with the knot's operands staged through LDS once per wavefront (k_fp_cf: 8 / 16 step sizes); kernels.cf_fp = cf | ts
    int kb_nis = 0;                // knots per wavefront of the knot-batched setup kernel (k_nis_kb: scalar plug-ins, RK3); 0 = k_nis_gl.  kernels.cf_nis = kb16 | kb20 | kb32 | kb64
    bool ls_many = false;          // line search one thread per problem (k_ls_many)
    // few problems in flight on the four-wave rollout pipeline, every problem's M x A rollouts inside one wavefront: the rollout kernel ends with the line search (k_fp_tl4)
    bool ls_in_rollouts = false;
    // ... and BEGINS with the linear forward sweep: the segment maps the backward pass composed are applied in the rollout kernel's prologue (a problem's M x A lanes sit in
    // one wavefront, 14 of them walk the maps) instead of by a k_sweep_maps launch in front of it -- one more kernel boundary of the ~115 us iteration gone.
    // kernels.sweep = maps keeps the separate kernel (A/B, tests); so do the phase hooks and the per-phase / per-kernel timing, which launch the sweep on its own.
    bool maps_in_rollouts = false;
    bool cf_records = false;       // production rollouts = k_sweep_cf + k_fp_cf (records in xw)
    bool mpc_split_roll = false;   // the MPC load stage as the 512-thread pipeline (warm-start rollout split over two waves): float Euler arm with a built-in robot model, not kernels.fp = lg | coop
    // the arrays that exist only on some kernel families, and the one launch attribute that does
    int xw_rec = 0;                // numbers per record of "xw" (0: no such array): staged closed-form rollouts NX + NU, thread-lane arm 22
    bool segmap = false;           // the composed forward-sweep maps
    bool ab_compact = false;       // "ABc": [A B] of the arm in the compact layout
    bool h_compact = false;        // "Hc": the end-effector cost's 7 x 7 position block
    bool fp_coop_lds = false;      // k_fp's dynamic LDS attribute has to cover the handle's segments
    // what pddp_time_kernels reports and launch_bp / launch_fp / launch_nis switch over (the forward pass through plan_fp_launch below)
    BpKernel bp = kBpCoop; SweepKernel sweep = kSweepNone; FpKernel fp = kFpKernCoop; LsKernel ls = kLsWg; NisKernel nis = kNisCoop;
};

// tl_variant: which built-in robot model the arm's tables equal (-1: neither; any other plant: -1)
inline KernelPlan make_kernel_plan(const pddp_config& c, const PlantTraits& t, bool is_float, int tl_variant) {
    KernelPlan p;
    const bool arm = t.plant == 4, nm16 = t.NX + t.NU <= 16, quad_shape = t.NX == 12 && t.NU == 4;
    const size_t units = (size_t)c.batch * c.M;
    const bool ts_fits = c.N <= kTsMaxN && c.M <= kTsMaxM;
    const BpSel bp = sel_bp(c); const FpSel fp = sel_fp(c); const SweepSel sweep = sel_sweep(c); const LsSel ls = sel_ls(c);
    const CfSel cf = sel_cf(c); const CfBpSel cf_bp = sel_cf_bp(c); const CfFpSel cf_fp = sel_cf_fp(c); const CfNisSel cf_nis = sel_cf_nis(c);
    p.nis_tl7_batch = c.batch <= kNisTl7MaxBatch;
    p.bp_lane_groups = units >= kBpLgMinBlocks;
    p.bp_wide = units <= kBpWideMaxBlocks && t.NX >= 12;
    p.fp_coop = fp == kFpSelCoop;                      // (the arm refines this below)
    p.ls_many = ls != kLsSelAuto ? ls == kLsSelMany : c.batch >= kLsManyMinBatch;
    p.cf_serial = !arm && (cf != kCfSelAuto ? cf == kCfSelTs : units >= kCfSerialMinUnits) && ts_fits;
    // measured on MI355X (tools/cf_variants.py; profiles/r03_closed_form_variants.txt): the rollouts always win thread-serially once the device is full (cart-pole, 16384
    // problems: 0.74 against 15.7 ms; quadrotor, 4096: 3.0 against 57.9 ms); the derivative kernel too for the small plants (0.16 against 2.1 ms) but not for the
    // quadrotor's 12 states, whose per-thread stage scratch spills to memory (6.2 against 5.4 ms); the backward pass thread-serially only for the small plants with the
    // device full (0.42 against 0.65 ms; quadrotor: its 64-knot serial chain on private memory takes 15 ms against 1.9 ms for a wave per block)
    p.cf_fp = p.cf_serial;
    p.cf_nis = p.cf_serial && t.NX < 12;
    p.cf_bp = p.cf_serial && t.NX < 12 && units >= kCfBpMinUnits;
    if (cf != kCfSelAuto) p.cf_bp = p.cf_nis = p.cf_fp;         // the override forces every phase
    // per-phase overrides (measurement): kernels.cf_bp / cf_fp / cf_nis = coop | ts
    if (cf_bp != kCfBpSelAuto) p.cf_bp = !arm && cf_bp == kCfBpSelTs;
    if (cf_fp != kCfFpSelAuto) p.cf_fp = !arm && cf_fp == kCfFpSelTs && ts_fits;
    if (cf_nis != kCfNisSelAuto) p.cf_nis = !arm && cf_nis == kCfNisSelTs;
    p.gl_nis = p.cf_serial && !p.cf_nis && nm16 && cf == kCfSelAuto;
    p.gl_bp = p.cf_serial && !p.cf_bp && nm16 && units >= kCfBpMinUnits && cf == kCfSelAuto;
    p.gl_bp32 = true;                                           // 32 lanes per block of knots: 1.92 -> 1.72 ms (quadrotor, 4096 problems); 16 lanes: 2.5 ms
    if (cf_nis != kCfNisSelAuto) { p.gl_nis = !arm && (cf_nis == kCfNisSelGl || cf_nis == kCfNisSelGl8) && nm16; p.gl_nis8 = cf_nis == kCfNisSelGl8; }
    p.cl_bp = p.gl_bp && quad_shape;
    p.mq_bp = p.cl_bp;                                          // round 5: 4.1 -> ... ms at 16384 quadrotor problems (profiles/r05_quad_mfma.md)
    const bool cf_fits = (c.A == 16 && (64 / 16) * t.NX <= 64) || (c.A == 8 && (64 / 8) * t.NX <= 64);      // whole problems per wavefront, one state fetch per lane
    p.cf_fp_staged = p.cf_fp && cf_fits && cf == kCfSelAuto;    // (cart-pole, 16384 problems: 0.73 -> 0.69 ms; quadrotor: 8.6 -> 5.1 ms)
    if (cf_fp == kCfFpSelCf) { p.cf_fp = !arm && ts_fits; p.cf_fp_staged = p.cf_fp && cf_fits; }
    else if (cf_fp != kCfFpSelAuto) p.cf_fp_staged = false;
    p.kb_nis = (p.gl_nis && c.integrator == 3) ? 16 : 0;        // 16 knots per wavefront: 2.15 ms (32: 2.6, 64: 3.6; the 16-lane-group kernel 5.7-7.1) at 16384 quadrotor problems -- LDS per block sets the occupancy
    if (cf_nis != kCfNisSelAuto) {
        const int kb = cf_nis == kCfNisSelKb16 ? 16 : cf_nis == kCfNisSelKb20 ? 20 : cf_nis == kCfNisSelKb32 ? 32 : cf_nis == kCfNisSelKb64 ? 64 : 0;
        p.kb_nis = (!arm && nm16 && c.integrator == 3) ? kb : 0;
        if (p.kb_nis) { p.gl_nis = true; p.cf_nis = false; }
    }
    if (cf_bp != kCfBpSelAuto) {
        const bool col = (cf_bp == kCfBpSelCl || cf_bp == kCfBpSelMq) && quad_shape;
        p.gl_bp = !arm && (cf_bp == kCfBpSelGl || cf_bp == kCfBpSelGl32 || col) && nm16;
        p.gl_bp32 = cf_bp == kCfBpSelGl32; p.cl_bp = p.gl_bp && col; p.mq_bp = p.cl_bp && cf_bp == kCfBpSelMq;
    }
    const bool maps_allowed = sweep == kSweepSelAuto || sweep == kSweepSelMaps;
    // the matrix-core backward pass of the 12-state plants with the record rollouts behind it: fused sweep maps by default (round 6: profiles/r06_quad.md)
    p.mq_fused = !arm && quad_shape && t.scalar_plugin && p.gl_bp && p.cl_bp && p.mq_bp && !p.cf_bp && p.cf_fp && p.cf_fp_staged && c.M > 1 && maps_allowed;
    if (arm && is_float) {
        p.sweep_kind = (c.batch <= kSweepWgMaxBatch && c.N / c.M <= kSweepWgMaxKnots) ? 2 : 1;
        if (sweep == kSweepSelAlpha) p.sweep_kind = 0; else if (sweep == kSweepSelSt) p.sweep_kind = 1; else if (sweep == kSweepSelWg) p.sweep_kind = 2;
        if (p.sweep_kind == 2 && c.N / c.M > kSweepWgMaxKnots) p.sweep_kind = 1;
        // default with the matrix-core backward pass: that pass composes the segments' sweep maps itself (bp_mfma.hpp kMxFuseSweep) and k_sweep_maps finishes;
        // sweep_kind stays the kernel of the phase hook, whose teacher-forced A - B K / B du must be what the sweep reads.  kernels.sweep = alpha | st | wg: no fusion.
    }
    p.bp_mfma = arm && is_float && units >= kBpMfmaMinBlocks;
    // kernels.bp = mx on a double handle: the same tile algebra on v_mfma_f64_16x16x4_f64 (a test selection: float64 handles default to the lane-group family,
    // whose operation order is the reference's)
    if (bp != kBpSelAuto) { p.bp_lane_groups = bp == kBpSelLg; p.bp_wide = bp == kBpSelWide; p.bp_mfma = arm && bp == kBpSelMx; }
    p.sweep_fused = p.bp_mfma && c.M > 1 && maps_allowed;
    if (arm) {
        // USE_FINITE_DIFF: the setup runs on the wave-cooperative kernel (k_nis: any plant's `dynamics`), which adopts the winner from the candidate-major
        // xs / us / ds -- so the rollouts stay on lane groups (they write those), not on the thread-lane kernels
        const bool tl_ok = tl_variant >= 0 && !c.use_finite_diff;
        p.fp_path = select_fp_path(fp, is_float, tl_ok, c.batch);
        if ((c.use_limits || c.use_smooth_abs) && p.fp_path == kFpLg) p.fp_path = kFpCoop;      // USE_LIMITS_FLAG / USE_SMOOTH_ABS: the lane-group family does not carry the variants
        p.fp_coop = p.fp_path == kFpCoop;
        // few problems in flight, float, built-in robot model: the rollouts run on the split thread-lane kernels; sweep, line search and setup stay on the lane-group
        // kernels.  kernels.fp = lg keeps the lane-group rollouts (bit-identity tests)
        p.fp_split = is_float && p.fp_path == kFpLg && tl_ok && fp != kFpSelLg;
        // kernels.fp = tl4 on a DOUBLE handle: the same few-problem selection (k_fp_tl4 pipeline + k_nis_tl7) in its parity instantiation (tests/test_f64_benched_family.py)
        if (!is_float && fp == kFpSelTl4 && p.fp_path == kFpLg && tl_ok && !c.use_limits && !c.use_smooth_abs) p.fp_split = true;
        // the split's current form is the four-wave pipeline (k_fp_tl4, fp_pipe.hpp; also the end-effector cost family); kernels.fp = tl2 keeps the two-wave kernel (joint-space cost only)
        p.fp_two_wave = p.fp_split && !c.ee_cost && fp == kFpSelTl2;
        p.mpc_split_roll = is_float && c.integrator == 1 && tl_variant >= 0 && fp != kFpSelLg && fp != kFpSelCoop;
    }
    const bool one_wave = 64 % (c.M * c.A) == 0;               // a problem's M x A rollouts inside one wavefront
    p.ls_in_rollouts = arm && p.fp_split && !p.fp_two_wave && !p.ls_many && ls == kLsSelAuto && one_wave;
    p.maps_in_rollouts = arm && p.sweep_fused && sweep == kSweepSelAuto && p.fp_split && !p.fp_two_wave && one_wave && c.M * c.A >= 16;
    p.cf_records = !arm && p.cf_fp && p.cf_fp_staged;
    // optional arrays: records of the staged closed-form rollouts (k_fp_cf) / knot-major candidate states of the thread-lane arm (fp_tl.hpp); the composed maps; the
    // compact [A B] -- not with kernels.ab = full (comparison runs), nor with the end-effector cost under USE_LIMITS_FLAG (the whole diagonal of H moves with the
    // trajectory -> reference-layout H and [A B]) -- and with the end-effector cost the Gauss-Newton Hessian's only dense part, the 7 x 7 position block (bp_mfma.hpp HQQ)
    p.xw_rec = arm ? (p.fp_path == kFpTl ? 22 : 0) : (p.cf_fp_staged ? t.NX + t.NU : 0);
    p.segmap = (arm && p.sweep_fused) || p.mq_fused;
    p.ab_compact = arm && p.bp_mfma && p.fp_path == kFpTl && sel_ab(c) != kAbSelFull && !(c.ee_cost && c.use_limits);
    p.h_compact = p.ab_compact && c.ee_cost;
    p.fp_coop_lds = !arm || p.fp_coop || c.use_limits || c.use_smooth_abs;      // the arm's forward pass runs on lane groups (no per-segment LDS scratch) unless it is on k_fp
    // the kernels by slot, in the priority order of the launch functions
    p.bp = p.bp_mfma ? kBpMfma : (arm && p.bp_lane_groups) ? kBpLg : p.cf_bp ? kBpTs : (p.gl_bp && p.cl_bp && p.mq_bp) ? kBpMq : (p.gl_bp && p.cl_bp) ? kBpCl : p.gl_bp ? kBpGl
         : p.bp_wide ? kBpWide : kBpCoop;
    const bool lg = arm && !p.fp_coop;
    p.sweep = lg ? (p.maps_in_rollouts ? kSweepNone : p.sweep_fused ? kSweepMaps : p.sweep_kind == 2 ? kSweepWg : p.sweep_kind == 1 ? kSweepSt : kSweepLg)
            : p.cf_records ? (p.mq_fused ? kSweepMapsCf : kSweepCf) : kSweepNone;
    p.fp = (lg && p.fp_path == kFpTl) ? kFpKernTl : (lg && p.fp_split) ? (p.fp_two_wave ? kFpKernTl2 : kFpKernTl4) : lg ? kFpKernLg
         : (p.cf_fp && p.cf_fp_staged) ? kFpKernCf : p.cf_fp ? kFpKernTs : kFpKernCoop;
    p.ls = p.ls_in_rollouts ? kLsNone : p.ls_many ? kLsMany : kLsWg;
    // (USE_FINITE_DIFF on the arm: the wave-cooperative setup, see above)
    p.nis = (arm && p.fp_path == kFpTl) ? kNisTl : (lg && !c.use_finite_diff) ? ((p.fp_split && p.nis_tl7_batch) ? kNisTl7 : kNisLg)
          : p.cf_nis ? kNisTs : (p.gl_nis && p.kb_nis && t.scalar_plugin) ? kNisKb : p.gl_nis ? kNisGl : kNisCoop;
    return p;
}

// The kernels of one sweep in launch order, by name: slots 0 backward pass, 1 linear sweep, 2 rollouts, 3 line search, 4 (none), 5 next-iteration setup; "" where the
// path has no separate kernel for a slot
inline void plan_kernel_names(const KernelPlan& p, const pddp_config& c, const char* out[6]) {
    out[0] = kernel_name(p.bp); out[1] = kernel_name(c.M > 1 ? p.sweep : kSweepNone); out[2] = kernel_name(p.fp); out[3] = kernel_name(p.ls); out[4] = ""; out[5] = kernel_name(p.nis);
}

// The ways the forward pass (linear sweep + rollouts) is asked for.
enum FpMode {
    kFpProduction,        // a sweep of pddp_iterate / a captured graph; the timing slot of a rollout kernel that sweeps itself
    kFpSweepOnly,         // the linear sweep's own kernel alone (slot 1 of pddp_time_kernels, row 4 of the traced iteration)
    kFpRolloutsOnly,      // the rollout kernel alone (slot 2; a kernel that sweeps itself still does)
    kFpInitial,           // the optional rollout of a load: one candidate, every segment from the loaded state
    kFpHook,              // pddp_run_phase(PDDP_PHASE_FP): teacher-forced sweep + rollouts, every candidate's x, u, d stored in the reference's arrays
    kFpHookFusedSweep,    // pddp_run_phase(PDDP_PHASE_SWEEP_FUSED): the production sweep from the composed maps, alone (run_phase refuses a handle without one)
    kFpHookRollouts       // pddp_run_phase(PDDP_PHASE_ROLLOUT): the hook's rollouts without any sweep, from the start states in xs
};
// What one call launches: launch_fp_sweep / launch_fp_rollouts (solver_impl.hpp) switch over `sweep` and `fp` and pass the rest on.
struct FpLaunch {
    SweepKernel sweep = kSweepNone;      // none: no sweep launch
    FpKernel fp = kFpKernNone;           // none: no rollout launch
    int seed = 0;                        // where the rollouts start: 0 the sweep's states, 1 the loaded trajectory, 2 the start states in xs (k_fp's argument; no_sweep of k_fp_ts)
    bool store_candidates = false;       // k_fp_tl writes every candidate's x, u, d
    bool maps_prologue = false;          // k_fp_tl4 begins with the sweep
    bool ls_tail = false;                // k_fp_tl4 ends with the line search
    bool cand_to_xw = false;             // k_cand_to_xw follows: the candidate-major arrays into the records
    bool cand_stale = false;             // the call leaves the candidate-major arrays behind the records
};
// In production: plan.sweep (with M > 1) and plan.fp, the kernels pddp_time_kernels names.  Every other mode is that with the deviations stated below.
inline FpLaunch plan_fp_launch(const KernelPlan& p, const pddp_config& c, FpMode mode) {
    FpLaunch L;
    const bool lg = c.plant == 4 && !p.fp_coop, records = p.cf_records;
    const bool hook = mode == kFpHook || mode == kFpHookFusedSweep || mode == kFpHookRollouts;
    const SweepKernel prod = c.M > 1 ? p.sweep : kSweepNone;
    const SweepKernel alone = p.maps_in_rollouts ? kSweepMaps : prod;      // asked for alone, the sweep of a rollout kernel that begins with it is the kernel that prologue replaces
    if (mode == kFpProduction) L.sweep = prod;
    if (mode == kFpSweepOnly) L.sweep = alone;
    if (mode == kFpHookFusedSweep && (alone == kSweepMaps || alone == kSweepMapsCf)) L.sweep = alone;       // the production sweep where that applies composed maps
    if (mode != kFpSweepOnly && mode != kFpHookFusedSweep) L.fp = p.fp;
    L.seed = mode == kFpInitial ? 1 : mode == kFpHookRollouts ? 2 : 0;
    L.store_candidates = hook;
    L.maps_prologue = p.maps_in_rollouts && mode == kFpProduction;
    L.ls_tail = p.ls_in_rollouts && (mode == kFpProduction || mode == kFpRolloutsOnly);
    L.cand_stale = records && !hook && mode != kFpInitial;
    // the hook's sweep must read the teacher-forced A - B K / B du, so it is sweep_kind's kernel and never the maps (the other families sweep inside their hook rollouts)
    if (mode == kFpHook && lg && c.M > 1) L.sweep = p.sweep_kind == 2 ? kSweepWg : p.sweep_kind == 1 ? kSweepSt : kSweepLg;
    // the hook wants the reference's candidate-major arrays: k_fp_ts, then k_cand_to_xw, instead of the record rollouts
    if (records && (mode == kFpHook || mode == kFpHookRollouts)) { L.fp = kFpKernTs; L.cand_to_xw = true; }
    // the initial rollout exists on lane groups, or on k_fp: for the arm with USE_LIMITS_FLAG / USE_SMOOTH_ABS, and for every other plant
    if (mode == kFpInitial) L.fp = (lg && !c.use_limits && !c.use_smooth_abs) ? kFpKernLg : kFpKernCoop;
    return L;
}

}  // namespace pddp
