// From a pddp_config to what the kernel bodies consume: defaults, the ABI's rules, plant constants, parameters, cost weights, the array table, the public view of the solver
// state.  Host code only, written ONCE for the three programs that set a handle up: the library (pddp_api.hip, solver_impl.hpp), tests/hostsim and cpu_twin.cpp.
#pragma once
#include <cmath>
#include <cstring>
#include <map>
#include <string>

#include "../../include/pddp.h"
#include "iiwa14_model_data.h"
#include "plants.hpp"
#include "solver_state.hpp"

namespace pddp {

template <typename T> struct MpcBuffers;      // mpc.hpp

// STATE_SIZE / CONTROL_SIZE of the built-in plants (-1: not one of them)
inline int builtin_state_size(int plant) { return plant == 1 ? 2 : plant == 2 ? 4 : plant == 3 ? 12 : plant == 4 ? 14 : -1; }
inline int builtin_control_size(int plant) { return plant == 1 ? 1 : plant == 2 ? 1 : plant == 3 ? 4 : plant == 4 ? 7 : -1; }

// Reference defaults: config.cuh:24-61 per plant, :78-136 algorithm, plants/cost_arm.cuh:97-103 weights.
inline void default_config(pddp_config* c, int plant) {
    std::memset(c, 0, sizeof(*c));                               // (kernels all zero: the library's own kernel selection)
    c->plant = plant; c->dtype = 0;
    c->N = plant == 4 ? 64 : 128; c->M = 4;                      // plant 5 (a user plant) starts from the pendulum's defaults
    c->A = (plant == 3 || plant == 4) ? 16 : 32;
    c->integrator = plant == 4 ? 1 : 3;
    c->batch = 1; c->max_iter = 100; c->ignore_max_rho_exit = 1;
    c->total_time = plant == 4 ? 0.5 : 4.0;
    c->alpha_base = (plant == 3 || plant == 4) ? 0.5 : 0.75;
    c->rho_init = plant == 4 ? 12.5 : (plant == 3 ? 1.0 : 10.0);
    c->max_defect = plant == 2 ? 0.75 : 1.0;
    c->tol_cost = 0.0001; c->exp_red_min = 0.05; c->exp_red_max = 1.25;
    c->Q1 = 0.1; c->Q2 = 0.001; c->R = 0.0001; c->QF1 = 1000.0; c->QF2 = 1000.0;
    c->Q_EE1 = 0.1; c->Q_EE2 = 0.0; c->QF_EE1 = 1000.0; c->QF_EE2 = 0.0; c->R_EE = 0.0001; c->Q_xEE = 0.0; c->QF_xEE = 0.0; c->Q_xdEE = 0.1; c->QF_xdEE = 1000.0;
    c->ee_on_link_z = 0.0635;   // plants/cost_arm.cuh:104-115, dynamics_arm.cuh:57-58 (EE_TYPE 1)
    c->use_finite_diff = 0; c->finite_diff_epsilon = 0.00001;   // config.cuh:68-71
    c->use_limits = 0; c->use_smooth_abs = 0; c->smooth_abs_alpha = 0.2;   // config.cuh:171-176, cost_arm.cuh:116-118
    c->ee_type = 1;                                             // dynamics_arm.cuh:50-52
}

// The rules of the ABI a configuration has to meet whatever runs it: "" or the complaint (pddp_create answers PDDP_EINVAL with it).
inline const char* config_complaint(const pddp_config& c, int max_plant) {
    if (c.plant < 1 || c.plant > max_plant) return "plant must be 1..4 (5: the user plant of a `make user PLANT_POLICY=...` build)";
    if (c.N < 4 || (c.N & (c.N - 1)) || c.N > 1024) return "N must be a power of two in [4,1024] (the reference's tree reductions assume it)";
    if (c.M < 1 || c.N % c.M || c.N / c.M < 2 || c.M > 16) return "M must divide N, N/M >= 2, M <= 16";
    if (c.A < 1 || c.A > 64 || c.batch < 1 || c.max_iter < 1) return "A in [1,64], batch >= 1, max_iter >= 1";
    if (c.ee_cost && c.plant != 4) return "ee_cost: the end-effector cost family belongs to the KUKA arm (plant 4)";
    if (c.ee_type < 0 || c.ee_type > 2) return "ee_type: EE_TYPE is 0 (no end effector), 1 (flange) or 2 (flange + peg) (dynamics_arm.cuh:50-65)";
    if (c.use_limits && c.plant != 4) return "use_limits: USE_LIMITS_FLAG belongs to the KUKA arm's cost files (plant 4)";
    if (c.use_smooth_abs && !(c.plant == 4 && c.ee_cost && c.smooth_abs_alpha > 0.0)) return "use_smooth_abs: USE_SMOOTH_ABS belongs to the end-effector cost (plant 4, ee_cost = 1, smooth_abs_alpha > 0)";
    if (c.use_finite_diff && (c.integrator != 1 || c.ee_cost || !(c.finite_diff_epsilon > 0.0)))
        return "use_finite_diff: the finite-difference [A B] is the Euler rule's (finiteDiffInner, nisInitHelpers.cuh:138-166), with the joint-space cost and a positive finite_diff_epsilon";
    return "";
}

// plant constants (P::Model) of a configuration, in the element type of the model
template <typename T> void fill_model(ArmModel<T>& m, const pddp_config& c) {
    const int v = c.wafr_urdf ? 1 : 0;
    for (int b = 0; b < 7; b++) {
        for (int i = 0; i < 36; i++) m.I[36 * b + i] = (T)IIWA14_SPATIAL_INERTIA[v][b][i];
        for (int i = 0; i < 16; i++) m.F[16 * b + i] = (T)IIWA14_JOINT_FRAME[v][b][i];
    }
    m.grav = (T)(c.mpc_mode ? 0.0 : 9.81);   // plants/dynamics_arm.cuh:42-46
    arm_model_apply_ee_type(m, c.wafr_urdf, c.ee_type);
}
inline void fill_model(EmptyModel& m, const pddp_config&) { m.unused = 0; }

inline SolverParams solver_params_of(const pddp_config& c) {
    SolverParams sp{};
    sp.max_iter = c.max_iter; sp.out_stride = c.max_iter + 2; sp.ignore_max_rho_exit = c.ignore_max_rho_exit; sp.tol_cost = c.tol_cost;
    sp.exp_red_min = c.exp_red_min; sp.exp_red_max = c.exp_red_max; sp.max_defect = c.max_defect; sp.rho_init = c.rho_init; sp.ee_initial_cost_fix = c.ee_initial_cost_fix;
    return sp;
}
template <typename T, int PLANT> CostWeights<T> cost_weights_of(const pddp_config& c) {
    CostWeights<T> cw{};
    cw.Q1 = (T)c.Q1; cw.Q2 = (T)c.Q2; cw.R = (T)c.R; cw.QF1 = (T)c.QF1; cw.QF2 = (T)c.QF2;
    cw.ee = c.ee_cost; cw.Q_EE1 = (T)c.Q_EE1; cw.Q_EE2 = (T)c.Q_EE2; cw.QF_EE1 = (T)c.QF_EE1; cw.QF_EE2 = (T)c.QF_EE2; cw.R_EE = (T)c.R_EE;
    cw.Q_xEE = (T)c.Q_xEE; cw.QF_xEE = (T)c.QF_xEE; cw.Q_xdEE = (T)c.Q_xdEE; cw.QF_xdEE = (T)c.QF_xdEE; cw.ee_z = (T)c.ee_on_link_z;
    cw.fd_eps = c.use_finite_diff ? c.finite_diff_epsilon : 0.0;
    cw.limits = (PLANT == 4) ? c.use_limits : 0;
    cw.smooth_abs = (PLANT == 4 && c.ee_cost) ? c.use_smooth_abs : 0; cw.sa = (T)c.smooth_abs_alpha; cw.sa2 = (T)(c.smooth_abs_alpha * c.smooth_abs_alpha);
    return cw;
}
template <typename T> T time_step(const pddp_config& c) { return (T)(c.total_time / (c.N - 1)); }      // TIME_STEP, config.cuh:136
inline double step_us(double total_time, int N) { return total_time / (N - 1) * 1000.0 * 1000.0; }     // the same in microseconds (the plant simulator's clock) ...
inline double step_us(const pddp_config& c) { return step_us(c.total_time, c.N); }                       // ... of the handle, and of a slot with its own horizon time (pddp_simulate_problems)
template <typename T> void alpha_table(const pddp_config& c, T* out) { for (int i = 0; i < c.A; i++) out[i] = (T)std::pow(c.alpha_base, (double)i); }   // nisInitHelpers.cuh:829

// The arrays every implementation of a handle registers under a name: visit(name, pointer slot in b / mb, element count) allocates `count` zeroed elements, points the
// slot at them, enters {pointer, bytes} into `arrays` and returns 0 (or its error, which ends the walk).  P / p are double buffers: their second halves become Pp / pp.
template <int NX, int NU, typename T, typename Visit>
int for_each_array(const pddp_config& c, Buffers<T>& b, MpcBuffers<T>& mb, std::map<std::string, std::pair<void*, size_t>>& arrays, Visit&& visit) {
    constexpr size_t NM = NX + NU;
    const size_t B = c.batch, N = c.N, A = c.A, M = c.M, out = c.max_iter + 2;
    int rc = 0;
#define PDDP_ARRAY(owner, name, count) if ((rc = visit(#name, &owner.name, (count)))) return rc
    PDDP_ARRAY(b, xs, B * A * N * NX); PDDP_ARRAY(b, us, B * A * N * NU); PDDP_ARRAY(b, ds, B * A * N * NX);
    PDDP_ARRAY(b, xb, B * 2 * N * NX); PDDP_ARRAY(b, ucur, B * N * NU); PDDP_ARRAY(b, dcur, B * N * NX);
    PDDP_ARRAY(b, P, 2 * B * N * NX * NX); PDDP_ARRAY(b, p, 2 * B * N * NX);
    PDDP_ARRAY(b, AB, B * N * NX * NM); PDDP_ARRAY(b, H, B * N * NM * NM); PDDP_ARRAY(b, g, B * N * NM);
    PDDP_ARRAY(b, KT, B * N * NX * NU); PDDP_ARRAY(b, du, B * N * NU); PDDP_ARRAY(b, ApBK, B * N * NX * NX); PDDP_ARRAY(b, Bdu, B * N * NX);
    PDDP_ARRAY(b, J, B * A); PDDP_ARRAY(b, dmax, B * A); PDDP_ARRAY(b, dJexp, B * 2 * M); PDDP_ARRAY(b, alpha, A); PDDP_ARRAY(b, xGoal, B * NX);
    PDDP_ARRAY(b, Jout, B * out); PDDP_ARRAY(b, err, B * M); PDDP_ARRAY(b, alphaOut, B * out); PDDP_ARRAY(b, state, B);
    b.Pp = b.P + B * N * NX * NX; b.pp = b.p + B * N * NX;
    arrays["P"].second /= 2; arrays["p"].second /= 2;
    arrays["Pp"] = {b.Pp, arrays["P"].second}; arrays["pp"] = {b.pp, arrays["p"].second};
    PDDP_ARRAY(mb, x_old, B * N * NX); PDDP_ARRAY(mb, u_old, B * N * NU); PDDP_ARRAY(mb, KT_old, B * N * NX * NU);
    PDDP_ARRAY(b, xTarget, B * NX); PDDP_ARRAY(b, costk, B * N); PDDP_ARRAY(b, tshift, B);
    PDDP_ARRAY(b, Jpart, B * A * M); PDDP_ARRAY(b, dpart, B * A * M); PDDP_ARRAY(b, parts_fresh, B);
#undef PDDP_ARRAY
    return 0;
}

// pddp_state <-> SolverState<T>: the public record carries every field but the two a sweep derives for itself
template <typename T> void to_public(const SolverState<T>& s, pddp_state& o) {
    o.rho = s.rho; o.drho = s.drho; o.prevJ = s.prevJ; o.dJ = s.dJ; o.z = s.z; o.iter = s.iter; o.alphaIndex = s.alphaIndex;
    o.ignore_defect = s.ignore_defect; o.accepted = s.accepted; o.done = s.done; o.cur = s.cur; o.cur2 = s.cur2; o.bp_retries = s.bp_retries; o.pw = s.pw;
}
template <typename T> void from_public(const pddp_state& o, SolverState<T>& s) {
    s.rho = (T)o.rho; s.drho = (T)o.drho; s.prevJ = (T)o.prevJ; s.dJ = (T)o.dJ; s.z = (T)o.z; s.iter = o.iter; s.alphaIndex = o.alphaIndex;
    s.ignore_defect = o.ignore_defect; s.accepted = o.accepted; s.done = o.done; s.cur = o.cur; s.cur2 = o.cur2; s.bp_retries = o.bp_retries; s.pw = o.pw;
    s.took_step = 0; s.win_pending = (o.accepted == 1) ? 1 : 0;
}

}  // namespace pddp
