// Stand-alone host program over the kernel selection (csrc/kernel_plan.hpp).  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc kernel_plan_host_check.cpp -o kernel_plan_host_check
//   ./kernel_plan_host_check            the choices that kernel names do not show, and what every mode of the forward pass launches on eight handles, asserted by hand; prints its ok line
//   ./kernel_plan_host_check sel        the pddp_config.kernels enums as "field name=value ..." lines (tests/test_kernel_plan.py: include/pddp.h, pyddp.KERNEL_NAMES)
//   ./kernel_plan_host_check rows       stdin: one configuration per line -- plant dtype N M A integrator batch ee_cost use_limits mpc_mode tl_variant and the nine
//                                       kernels fields in the order of include/pddp.h; stdout: the names of its sweep's kernels in launch order | xw_rec segmap ABc Hc
//   ./kernel_plan_host_check fp         stdin: the same rows; stdout: plan_fp_launch of the seven modes in the order of FpMode, " | " between them, each as
//                                       sweep,rollouts,seed,flags ("-": no launch; flags: store_candidates maps_prologue ls_tail cand_to_xw cand_stale)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>

#include "kernel_plan.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// the numbers of include/pddp.h
static_assert(kBpSelMx == 1 && kBpSelLg == 2 && kBpSelCoop == 3 && kBpSelWide == 4, "kernels.bp");
static_assert(kFpSelTl == 1 && kFpSelLg == 2 && kFpSelCoop == 3 && kFpSelTl2 == 4 && kFpSelTl4 == 5, "kernels.fp");
static_assert(kSweepSelAlpha == 1 && kSweepSelSt == 2 && kSweepSelWg == 3 && kSweepSelMaps == 4, "kernels.sweep");
static_assert(kLsSelMany == 1 && kLsSelWg == 2 && kAbSelFull == 1 && kCfSelTs == 1 && kCfSelCoop == 2, "kernels.ls / ab / cf");
static_assert(kCfBpSelTs == 1 && kCfBpSelCoop == 2 && kCfBpSelGl == 3 && kCfBpSelGl32 == 4 && kCfBpSelCl == 5 && kCfBpSelMq == 6, "kernels.cf_bp");
static_assert(kCfFpSelTs == 1 && kCfFpSelCoop == 2 && kCfFpSelCf == 3, "kernels.cf_fp");
static_assert(kCfNisSelTs == 1 && kCfNisSelCoop == 2 && kCfNisSelGl == 3 && kCfNisSelGl8 == 4 && kCfNisSelKb16 == 5 && kCfNisSelKb32 == 6 && kCfNisSelKb64 == 7 && kCfNisSelKb20 == 8, "kernels.cf_nis");

static PlantTraits traits_of(int plant) {            // the built-in plants (csrc/plants.hpp)
    static const PlantTraits t[4] = {{1, 2, 1, true, false}, {2, 4, 1, true, false}, {3, 12, 4, true, false}, {4, 14, 7, false, false}};
    CHECK(plant >= 1 && plant <= 4);
    return t[plant - 1];
}
static pddp_config config_of(int plant, int dtype, int N, int M, int A, int integrator, int batch) {
    pddp_config c;
    std::memset(&c, 0, sizeof(c));
    c.plant = plant; c.dtype = dtype; c.N = N; c.M = M; c.A = A; c.integrator = integrator; c.batch = batch;
    return c;
}
static KernelPlan plan_of(const pddp_config& c, int tl_variant = -1) { return make_kernel_plan(c, traits_of(c.plant), c.dtype == 0, c.plant == 4 ? tl_variant : -1); }
static auto fields(const KernelPlan& p) {
    return std::make_tuple(p.bp_mfma, p.bp_lane_groups, p.bp_wide, p.cf_serial, p.cf_bp, p.cf_fp, p.cf_nis, p.gl_bp, p.gl_nis, p.gl_bp32, p.gl_nis8, p.cl_bp, p.mq_bp, p.mq_fused,
                           p.sweep_fused, p.sweep_kind, (int)p.fp_path, p.fp_coop, p.fp_split, p.fp_two_wave, p.nis_tl7_batch, p.cf_fp_staged, p.kb_nis, p.ls_many,
                           p.ls_in_rollouts, p.maps_in_rollouts, p.cf_records, p.mpc_split_roll, p.xw_rec, p.segmap, p.ab_compact, p.h_compact, p.fp_coop_lds,
                           (int)p.bp, (int)p.sweep, (int)p.fp, (int)p.ls, (int)p.nis);
}

static void check_by_hand() {
    // 32 lanes per block of knots in k_bp_gl by default; kernels.cf_bp = gl asks for 16, gl32 for 32
    pddp_config quad = config_of(3, 0, 64, 4, 8, 3, 2048);
    CHECK(plan_of(quad).gl_bp32);
    quad.kernels.cf_bp = kCfBpSelGl; CHECK(plan_of(quad).gl_bp && !plan_of(quad).gl_bp32 && plan_of(quad).bp == kBpGl);
    quad.kernels.cf_bp = kCfBpSelGl32; CHECK(plan_of(quad).gl_bp && plan_of(quad).gl_bp32 && plan_of(quad).bp == kBpGl);
    quad.kernels.cf_bp = 0;
    // knots per wavefront of the knot-batched setup: 16 by default with RK3, none with Euler; 16 / 20 / 32 / 64 by override
    CHECK(plan_of(quad).kb_nis == 16 && plan_of(quad).nis == kNisKb);
    quad.integrator = 1; CHECK(plan_of(quad).kb_nis == 0 && plan_of(quad).nis == kNisGl);
    quad.integrator = 3;
    const int kb[4][2] = {{kCfNisSelKb16, 16}, {kCfNisSelKb20, 20}, {kCfNisSelKb32, 32}, {kCfNisSelKb64, 64}};
    for (const auto& v : kb) {
        for (int batch : {3, 2048}) {
            quad.batch = batch; quad.kernels.cf_nis = v[0];
            CHECK(plan_of(quad).kb_nis == v[1] && plan_of(quad).gl_nis && !plan_of(quad).cf_nis && plan_of(quad).nis == kNisKb);
        }
    }
    // 8 lanes per knot of k_nis_gl only on request
    quad.kernels.cf_nis = kCfNisSelGl8; CHECK(plan_of(quad).gl_nis && plan_of(quad).gl_nis8 && plan_of(quad).kb_nis == 0 && plan_of(quad).nis == kNisGl);
    quad.kernels.cf_nis = kCfNisSelGl; CHECK(plan_of(quad).gl_nis && !plan_of(quad).gl_nis8 && plan_of(quad).nis == kNisGl);
    quad.kernels.cf_nis = 0; CHECK(!plan_of(quad).gl_nis8);
    // the 512-thread MPC load stage: float Euler arm with a built-in robot model, not with kernels.fp = lg | coop
    pddp_config arm = config_of(4, 0, 64, 4, 8, 1, 1);
    for (int batch : {1, 4096}) {
        arm.batch = batch;
        for (int fp = 0; fp <= 5; fp++) {
            arm.kernels.fp = fp;
            CHECK(plan_of(arm, 0).mpc_split_roll == (fp != kFpSelLg && fp != kFpSelCoop));
            CHECK(plan_of(arm, 1).mpc_split_roll == (fp != kFpSelLg && fp != kFpSelCoop));
            CHECK(!plan_of(arm, -1).mpc_split_roll);
            arm.dtype = 1; CHECK(!plan_of(arm, 0).mpc_split_roll); arm.dtype = 0;
        }
        arm.kernels.fp = 0;
    }
    CHECK(!plan_of(quad).mpc_split_roll);
    // USE_FINITE_DIFF on the arm: the wave-cooperative setup behind lane-group rollouts
    arm.batch = 1; arm.use_finite_diff = 1;
    CHECK(plan_of(arm, 0).nis == kNisCoop && plan_of(arm, 0).fp == kFpKernLg && !plan_of(arm, 0).fp_split);
    arm.use_finite_diff = 0;
    CHECK(plan_of(arm, 0).nis == kNisTl7 && plan_of(arm, 0).fp == kFpKernTl4);
    // the by-name form of select_fp_path (the host emulation's) is the enum's
    const char* const fp_names[6] = {nullptr, "tl", "lg", "coop", "tl2", "tl4"};
    for (int fp = 0; fp <= 5; fp++)
        for (int is_float = 0; is_float < 2; is_float++)
            for (int ok = 0; ok < 2; ok++)
                for (int batch : {1, 511, 512, 4096})
                    CHECK(select_fp_path(fp_names[fp], is_float != 0, false, ok != 0, batch) == select_fp_path((FpSel)fp, is_float != 0, ok != 0, batch));
    // a value outside a field's range is the library's choice
    for (int plant = 1; plant <= 4; plant++) {
        for (int dtype = 0; dtype < 2; dtype++) {
            for (int batch : {1, 64, 512, 2048, 4096}) {
                for (int A : {8, 16}) {
                    pddp_config c = config_of(plant, dtype, 64, 4, A, plant == 4 ? 1 : 3, batch);
                    const auto want = fields(plan_of(c, 0));
                    const int last[9] = {kBpSelWide, kFpSelTl4, kSweepSelMaps, kLsSelWg, kAbSelFull, kCfSelCoop, kCfBpSelMq, kCfFpSelCf, kCfNisSelKb20};
                    int* f[9] = {&c.kernels.bp, &c.kernels.fp, &c.kernels.sweep, &c.kernels.ls, &c.kernels.ab, &c.kernels.cf, &c.kernels.cf_bp, &c.kernels.cf_fp, &c.kernels.cf_nis};
                    for (int i = 0; i < 9; i++) {
                        for (int v : {-1, last[i] + 1, 99, -2147483647 - 1, 2147483647}) { *f[i] = v; CHECK(fields(plan_of(c, 0)) == want); }
                        *f[i] = 0;
                    }
                }
            }
        }
    }
}

// What the forward pass launches, mode by mode (plan_fp_launch), on eight handles: N = 64, M = 4; the arm with Euler steps and a built-in model, cart-pole and quadrotor
// with RK3.  Read from the launch code of the commit before plan_fp_launch existed, whose nested conditions these records replace.
struct Want { SweepKernel sweep; FpKernel fp; int seed; bool store, maps, ls, xw, stale; };
static void check_modes(const pddp_config& c, const Want (&want)[7]) {
    const KernelPlan p = plan_of(c, 0);
    for (int m = kFpProduction; m <= kFpHookRollouts; m++) {
        const FpLaunch L = plan_fp_launch(p, c, (FpMode)m);
        const Want& w = want[m];
        if (L.sweep != w.sweep || L.fp != w.fp || L.seed != w.seed || L.store_candidates != w.store || L.maps_prologue != w.maps || L.ls_tail != w.ls || L.cand_to_xw != w.xw || L.cand_stale != w.stale) {
            std::printf("FAILED: plant %d dtype %d batch %d A %d use_limits %d, mode %d: %s %s seed %d flags %d%d%d%d%d\n", c.plant, c.dtype, c.batch, c.A, c.use_limits, m, kernel_name(L.sweep), kernel_name(L.fp),
                        L.seed, (int)L.store_candidates, (int)L.maps_prologue, (int)L.ls_tail, (int)L.cand_to_xw, (int)L.cand_stale);
            std::exit(1);
        }
    }
}
static void check_fp_modes() {
    const SweepKernel S0 = kSweepNone; const FpKernel F0 = kFpKernNone;
    // the order of FpMode: production, sweep only, rollouts only, initial rollout, hook, hook's fused sweep, hook's rollouts from xs
    // one problem of the float arm: k_fp_tl4 begins with the sweep and ends with the line search -- in production; alone it is neither's place, and the sweep alone is k_sweep_maps
    const pddp_config arm1 = config_of(4, 0, 64, 4, 8, 1, 1);
    check_modes(arm1, {{S0, kFpKernTl4, 0, 0, 1, 1, 0, 0}, {kSweepMaps, F0, 0, 0, 0, 0, 0, 0}, {S0, kFpKernTl4, 0, 0, 0, 1, 0, 0}, {S0, kFpKernLg, 1, 0, 0, 0, 0, 0},
                       {kSweepWg, kFpKernTl4, 0, 1, 0, 0, 0, 0}, {kSweepMaps, F0, 0, 1, 0, 0, 0, 0}, {S0, kFpKernTl4, 2, 1, 0, 0, 0, 0}});
    const pddp_config arm512 = config_of(4, 0, 64, 4, 8, 1, 512);
    check_modes(arm512, {{kSweepMaps, kFpKernTl, 0, 0, 0, 0, 0, 0}, {kSweepMaps, F0, 0, 0, 0, 0, 0, 0}, {S0, kFpKernTl, 0, 0, 0, 0, 0, 0}, {S0, kFpKernLg, 1, 0, 0, 0, 0, 0},
                         {kSweepWg, kFpKernTl, 0, 1, 0, 0, 0, 0}, {kSweepMaps, F0, 0, 1, 0, 0, 0, 0}, {S0, kFpKernTl, 2, 1, 0, 0, 0, 0}});
    // a double handle has no fused sweep: pddp_run_phase refuses the mode, and there is nothing to launch
    const pddp_config arm64 = config_of(4, 1, 64, 4, 8, 1, 2);
    check_modes(arm64, {{kSweepLg, kFpKernLg, 0, 0, 0, 0, 0, 0}, {kSweepLg, F0, 0, 0, 0, 0, 0, 0}, {S0, kFpKernLg, 0, 0, 0, 0, 0, 0}, {S0, kFpKernLg, 1, 0, 0, 0, 0, 0},
                        {kSweepLg, kFpKernLg, 0, 1, 0, 0, 0, 0}, {S0, F0, 0, 1, 0, 0, 0, 0}, {S0, kFpKernLg, 2, 1, 0, 0, 0, 0}});
    // USE_LIMITS_FLAG off the thread lanes: k_fp, which sweeps itself, in every mode (its backward pass composes maps, so the hook's fused sweep is accepted and launches nothing)
    pddp_config armlim = config_of(4, 0, 64, 4, 8, 1, 1); armlim.use_limits = 1;
    const Want coop[7] = {{S0, kFpKernCoop, 0, 0, 0, 0, 0, 0}, {S0, F0, 0, 0, 0, 0, 0, 0}, {S0, kFpKernCoop, 0, 0, 0, 0, 0, 0}, {S0, kFpKernCoop, 1, 0, 0, 0, 0, 0},
                          {S0, kFpKernCoop, 0, 1, 0, 0, 0, 0}, {S0, F0, 0, 1, 0, 0, 0, 0}, {S0, kFpKernCoop, 2, 1, 0, 0, 0, 0}};
    CHECK(plan_of(armlim, 0).sweep_fused);
    check_modes(armlim, coop);
    // the record rollouts of the closed-form plants leave the candidate-major arrays behind; the hook fills those (k_fp_ts) and converts
    const pddp_config cart8 = config_of(2, 0, 64, 4, 8, 3, 4096);
    check_modes(cart8, {{kSweepCf, kFpKernCf, 0, 0, 0, 0, 0, 1}, {kSweepCf, F0, 0, 0, 0, 0, 0, 1}, {S0, kFpKernCf, 0, 0, 0, 0, 0, 1}, {S0, kFpKernCoop, 1, 0, 0, 0, 0, 0},
                        {S0, kFpKernTs, 0, 1, 0, 0, 1, 0}, {S0, F0, 0, 1, 0, 0, 0, 0}, {S0, kFpKernTs, 2, 1, 0, 0, 1, 0}});
    const pddp_config cart4 = config_of(2, 0, 64, 4, 4, 3, 4096);      // four step sizes: no records
    check_modes(cart4, {{S0, kFpKernTs, 0, 0, 0, 0, 0, 0}, {S0, F0, 0, 0, 0, 0, 0, 0}, {S0, kFpKernTs, 0, 0, 0, 0, 0, 0}, {S0, kFpKernCoop, 1, 0, 0, 0, 0, 0},
                        {S0, kFpKernTs, 0, 1, 0, 0, 0, 0}, {S0, F0, 0, 1, 0, 0, 0, 0}, {S0, kFpKernTs, 2, 1, 0, 0, 0, 0}});
    check_modes(config_of(2, 0, 64, 4, 8, 3, 2), coop);
    const pddp_config quad16 = config_of(3, 0, 64, 4, 16, 3, 2048);    // the matrix-core backward pass composes the maps: k_sweep_maps_cf (reported as k_sweep_maps)
    check_modes(quad16, {{kSweepMapsCf, kFpKernCf, 0, 0, 0, 0, 0, 1}, {kSweepMapsCf, F0, 0, 0, 0, 0, 0, 1}, {S0, kFpKernCf, 0, 0, 0, 0, 0, 1}, {S0, kFpKernCoop, 1, 0, 0, 0, 0, 0},
                         {S0, kFpKernTs, 0, 1, 0, 0, 1, 0}, {kSweepMapsCf, F0, 0, 1, 0, 0, 0, 0}, {S0, kFpKernTs, 2, 1, 0, 0, 1, 0}});
    // production has none of the other modes' deviations: it is plan.sweep + plan.fp ...
    for (const pddp_config& c : {arm1, arm512, arm64, armlim, cart8, cart4, quad16}) {
        const KernelPlan p = plan_of(c, 0);
        const FpLaunch L = plan_fp_launch(p, c, kFpProduction);
        CHECK(L.sweep == p.sweep && L.fp == p.fp && L.seed == 0 && !L.store_candidates && !L.cand_to_xw);
    }
    // ... the record rollouts, not the hook's k_fp_ts + k_cand_to_xw
    CHECK(plan_fp_launch(plan_of(cart8), cart8, kFpProduction).fp == kFpKernCf && plan_fp_launch(plan_of(cart8), cart8, kFpHook).fp == kFpKernTs);
    // ... the composed maps, not the hook's sweep over the teacher-forced A - B K
    CHECK(plan_fp_launch(plan_of(arm512, 0), arm512, kFpProduction).sweep == kSweepMaps && plan_fp_launch(plan_of(arm512, 0), arm512, kFpHook).sweep == kSweepWg);
    // ... the handle's own rollout kernel, not the initial rollout's lane groups / k_fp
    CHECK(plan_fp_launch(plan_of(arm512, 0), arm512, kFpProduction).fp == kFpKernTl && plan_fp_launch(plan_of(cart8), cart8, kFpProduction).fp != kFpKernCoop);
    pddp_config tl_lim = arm512; tl_lim.use_limits = 1;                 // (a thread-lane handle with USE_LIMITS_FLAG: only its initial rollout is k_fp's)
    CHECK(plan_fp_launch(plan_of(tl_lim, 0), tl_lim, kFpProduction).fp == kFpKernTl && plan_fp_launch(plan_of(tl_lim, 0), tl_lim, kFpInitial).fp == kFpKernCoop);
    // one segment: no sweep in any mode
    pddp_config m1 = config_of(4, 0, 64, 1, 8, 1, 512);
    for (int m = kFpProduction; m <= kFpHookRollouts; m++) CHECK(plan_fp_launch(plan_of(m1, 0), m1, (FpMode)m).sweep == kSweepNone);
    m1 = config_of(2, 0, 64, 1, 8, 3, 4096);
    for (int m = kFpProduction; m <= kFpHookRollouts; m++) CHECK(plan_fp_launch(plan_of(m1), m1, (FpMode)m).sweep == kSweepNone);
}

static void print_sel() {
    std::printf("bp mx=%d lg=%d coop=%d wide=%d\n", kBpSelMx, kBpSelLg, kBpSelCoop, kBpSelWide);
    std::printf("fp tl=%d lg=%d coop=%d tl2=%d tl4=%d\n", kFpSelTl, kFpSelLg, kFpSelCoop, kFpSelTl2, kFpSelTl4);
    std::printf("sweep alpha=%d st=%d wg=%d maps=%d\n", kSweepSelAlpha, kSweepSelSt, kSweepSelWg, kSweepSelMaps);
    std::printf("ls many=%d wg=%d\n", kLsSelMany, kLsSelWg);
    std::printf("ab full=%d\n", kAbSelFull);
    std::printf("cf ts=%d coop=%d\n", kCfSelTs, kCfSelCoop);
    std::printf("cf_bp ts=%d coop=%d gl=%d gl32=%d cl=%d mq=%d\n", kCfBpSelTs, kCfBpSelCoop, kCfBpSelGl, kCfBpSelGl32, kCfBpSelCl, kCfBpSelMq);
    std::printf("cf_fp ts=%d coop=%d cf=%d\n", kCfFpSelTs, kCfFpSelCoop, kCfFpSelCf);
    std::printf("cf_nis ts=%d coop=%d gl=%d gl8=%d kb16=%d kb32=%d kb64=%d kb20=%d\n", kCfNisSelTs, kCfNisSelCoop, kCfNisSelGl, kCfNisSelGl8, kCfNisSelKb16, kCfNisSelKb32, kCfNisSelKb64, kCfNisSelKb20);
}

static int print_rows(bool modes) {
    int v[20];
    for (;;) {
        int got = 0;
        for (; got < 20; got++) if (std::scanf("%d", &v[got]) != 1) break;
        if (got == 0) return 0;
        if (got != 20) { std::printf("FAILED: a row of %d numbers\n", got); return 1; }
        pddp_config c = config_of(v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
        c.ee_cost = v[7]; c.use_limits = v[8]; c.mpc_mode = v[9];
        c.kernels.bp = v[11]; c.kernels.fp = v[12]; c.kernels.sweep = v[13]; c.kernels.ls = v[14]; c.kernels.ab = v[15];
        c.kernels.cf = v[16]; c.kernels.cf_bp = v[17]; c.kernels.cf_fp = v[18]; c.kernels.cf_nis = v[19];
        const KernelPlan p = plan_of(c, v[10]);
        if (modes) {
            for (int m = kFpProduction; m <= kFpHookRollouts; m++) {
                const FpLaunch L = plan_fp_launch(p, c, (FpMode)m);
                std::printf("%s%s,%s,%d,%d%d%d%d%d", m ? " | " : "", L.sweep == kSweepNone ? "-" : kernel_name(L.sweep), L.fp == kFpKernNone ? "-" : kernel_name(L.fp), L.seed,
                            (int)L.store_candidates, (int)L.maps_prologue, (int)L.ls_tail, (int)L.cand_to_xw, (int)L.cand_stale);
            }
            std::printf("\n");
            continue;
        }
        const char* nm[6];
        plan_kernel_names(p, c, nm);
        for (int k = 0; k < 6; k++) if (nm[k][0]) std::printf("%s ", nm[k]);
        std::printf("| %d %d %d %d\n", p.xw_rec, (int)p.segmap, (int)p.ab_compact, (int)p.h_compact);
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "sel") == 0) { print_sel(); return 0; }
    if (argc > 1 && std::strcmp(argv[1], "rows") == 0) return print_rows(false);
    if (argc > 1 && std::strcmp(argv[1], "fp") == 0) return print_rows(true);
    check_by_hand();
    check_fp_modes();
    std::printf("kernel_plan_host_check: ok\n");
    return 0;
}
