// libpddp.so: host side of the C ABI declared in include/pddp.h.  gfx950 only; no CPU fallback.
#include "solver_base.hpp"
#include "handle_setup.hpp"
#include "slots.hpp"
#include "cost_table.hpp"

static thread_local std::string g_err;
extern "C" const char* pddp_last_error(void) { return g_err.c_str(); }
int pddp_internal_fail(int code, const std::string& msg) { g_err = msg; return code; }      // every translation unit of the library reports through this (solver_base.hpp)
#ifdef PDDP_HAS_USER_PLANT
static constexpr int kMaxPlant = 5;
static int user_nx() { return pddp_user_plant_state_size(); }
static int user_nu() { return pddp_user_plant_control_size(); }
#else
static constexpr int kMaxPlant = 4;
static int user_nx() { return -1; }
static int user_nu() { return -1; }
#endif
extern "C" int pddp_state_size(int plant) { return plant == 5 ? user_nx() : pddp::builtin_state_size(plant); }
extern "C" int pddp_control_size(int plant) { return plant == 5 ? user_nu() : pddp::builtin_control_size(plant); }

extern "C" int pddp_default_config(pddp_config* c, int plant) {
    if (!c || plant < 1 || plant > kMaxPlant) return fail(PDDP_EINVAL, "plant must be 1..4 (5: the user plant of a `make user PLANT_POLICY=...` build)");
    pddp::default_config(c, plant);
    return 0;
}

static SolverBase* make_solver(const pddp_config& c) {
    switch (c.plant) {
    case 1: return pddp_make_solver_pend(c);
    case 2: return pddp_make_solver_cart(c);
    case 3: return pddp_make_solver_quad(c);
    case 4: return pddp_make_solver_arm(c);      // the arm is Euler-only, as config.cuh:58
#ifdef PDDP_HAS_USER_PLANT
    case 5: return pddp_make_solver_user(c);
#endif
    }
    return nullptr;
}

// HBM counter calibration (profiling tool): streams `count` floats from src to dst with the access shape the sweep kernels use (one dword per lane, consecutive lanes on
// consecutive addresses).  Its byte count is known exactly, which calibrates rocprofv3's FETCH_SIZE / WRITE_SIZE for this access width (MI355X_MICROARCH.md, "HBM").
__global__ __launch_bounds__(256) void k_hbm_calib_dword(const float* __restrict__ src, float* __restrict__ dst, size_t count) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

extern "C" int pddp_create(const pddp_config* cfg, pddp_handle* out) {
    if (!cfg || !out) return fail(PDDP_EINVAL, "null argument");
    const pddp_config& c = *cfg;
    if (const char* complaint = pddp::config_complaint(c, kMaxPlant); complaint[0]) return fail(PDDP_EINVAL, complaint);
    // the arm's lane-group kernels: 128 rollouts per workgroup, 32-bit element offsets
    if (c.plant == 4 && ((c.A > 8 && c.A % 8 == 0) ? 8 : c.A) * c.M > 128)
        return fail(PDDP_EINVAL, "KUKA arm: (candidates per workgroup) * M must not exceed 128 -- a workgroup rolls out 8 candidates when A is a multiple of 8, otherwise all A");
    if (c.plant == 4 && (double)c.batch * c.N * (c.A * 14 > 441 ? c.A * 14 : 441) >= 4294967296.0)
        return fail(PDDP_EINVAL, "KUKA arm: batch * N too large for the 32-bit element offsets of the lane-group kernels (split the batch over several handles)");
    SolverBase* s = make_solver(c);
    if (!s) return fail(PDDP_EINVAL, "unsupported plant / integrator / dtype combination (the arm supports Euler only)");
    s->cfg = c;
    int rc = s->init();
    if (rc) { delete s; return rc; }
    *out = new pddp_solver{s};
    return 0;
}
extern "C" int pddp_destroy(pddp_handle h) { if (h) { delete h->impl; delete h; } return 0; }
#define IMPL(h) if (!(h)) return fail(PDDP_EINVAL, "null handle"); SolverBase* s = (h)->impl
extern "C" int pddp_load(pddp_handle h, const void* x0, const void* u0, const void* xg, int clear, int ifd) { IMPL(h); return s->load(x0, u0, xg, nullptr, nullptr, nullptr, nullptr, 0, clear, ifd); }
extern "C" int pddp_load_ex(pddp_handle h, const void* x0, const void* u0, const void* xg, const void* KT0, const void* P0, const void* p0, const void* d0,
                            int rollout, int clear, int ifd) {
    IMPL(h);
    if (!x0 || !u0 || !xg) return fail(PDDP_EINVAL, "pddp_load: null trajectory or goal");
    return s->load(x0, u0, xg, KT0, P0, p0, d0, rollout, clear, ifd);
}
// individual slots of a loaded handle (slots.hpp): the arguments are checked here, before anything is enqueued
static int slots_check(SolverBase* s, const char* who, int count, const int* idx) {
    if (!s->loaded) return fail(PDDP_EINVAL, std::string(who) + ": the handle has never been loaded (the first fill is pddp_load / pddp_solve; an unloaded slot has no state to idle in)");
    const std::string complaint = pddp::slots_complaint(count, idx, s->cfg.batch);
    if (!complaint.empty()) return fail(PDDP_EINVAL, std::string(who) + ": " + complaint);
    return 0;
}
extern "C" int pddp_load_problems(pddp_handle h, int count, const int* idx, const void* x0, const void* u0, const void* xg, int ifd) {
    IMPL(h);
    if (!idx || !x0 || !u0 || !xg) return fail(PDDP_EINVAL, "pddp_load_problems: null idx, trajectory or goal");
    if (int rc = slots_check(s, "pddp_load_problems", count, idx)) return rc;
    return s->load_problems(count, idx, x0, u0, xg, ifd);
}
extern "C" int pddp_store_problems(pddp_handle h, int count, const int* idx, void* x, void* u, void* KT, void* Jout, int* alphaOut, void* dmax) {
    IMPL(h);
    if (!idx) return fail(PDDP_EINVAL, "pddp_store_problems: null idx");
    if (int rc = slots_check(s, "pddp_store_problems", count, idx)) return rc;
    return s->store_problems(count, idx, x, u, KT, Jout, alphaOut, dmax);
}
extern "C" int pddp_iterate(pddp_handle h, int sweeps) { IMPL(h); return s->iterate(sweeps); }
extern "C" int pddp_sync(pddp_handle h) { IMPL(h); return s->sync(); }
extern "C" int pddp_status(pddp_handle h, int* done, int* iters) { IMPL(h); return s->status(done, iters); }
extern "C" int pddp_store(pddp_handle h, void* x, void* u, void* KT, void* Jout, int* alphaOut, void* dmax) { IMPL(h); return s->store(x, u, KT, Jout, alphaOut, dmax); }
extern "C" int pddp_time_sweeps(pddp_handle h, int sweeps, float* ms_total, float* ms_phase) { IMPL(h); return s->time_sweeps(sweeps, ms_total, ms_phase); }
extern "C" int pddp_time_kernels(pddp_handle h, int sweeps, float* ms6, char* names, int name_stride) {
    IMPL(h); if (sweeps < 1 || !ms6 || (names && name_stride < 8)) return fail(PDDP_EINVAL, "pddp_time_kernels: bad arguments");
    return s->time_kernels(sweeps, ms6, names, name_stride);
}
extern "C" int pddp_set_cost(pddp_handle h, double Q1, double Q2, double R, double QF1, double QF2) { IMPL(h); return s->set_cost(Q1, Q2, R, QF1, QF2); }
// per-problem cost weights (cost_table.hpp): every argument is checked here, before the handle is touched
static int cost_problems_check(SolverBase* s, const char* who, int count, const int* idx, const double* w, bool check_w) {
    const int rec = s->cost_record_size();
    if (!rec) return fail(PDDP_EINVAL, std::string(who) + ": per-problem cost weights belong to the KUKA arm's own cost families (plant 4); the other plants' weights are constants");
    const std::string complaint = pddp::cost_records_complaint(count, idx, w, s->cfg.batch, rec, check_w);
    if (!complaint.empty()) return fail(PDDP_EINVAL, std::string(who) + ": " + complaint);
    return 0;
}
extern "C" int pddp_cost_record_size(pddp_handle h) {
    IMPL(h);
    const int rec = s->cost_record_size();
    return rec ? rec : fail(PDDP_EINVAL, "pddp_cost_record_size: per-problem cost weights belong to the KUKA arm's own cost families (plant 4)");
}
extern "C" int pddp_set_cost_problems(pddp_handle h, int count, const int* idx, const double* w) {
    IMPL(h);
    if (int rc = cost_problems_check(s, "pddp_set_cost_problems", count, idx, w, true)) return rc;
    return s->set_cost_problems(count, idx, w);
}
extern "C" int pddp_get_cost_problems(pddp_handle h, int count, const int* idx, double* w) {
    IMPL(h);
    if (int rc = cost_problems_check(s, "pddp_get_cost_problems", count, idx, w, false)) return rc;
    return s->get_cost_problems(count, idx, w);
}
// run-time diagonal cost weights of the pendulum, cart-pole and quadrotor (diag_cost_table.hpp): the handle checks every argument in its element type before it is touched
extern "C" int pddp_diag_cost_size(pddp_handle h) {
    IMPL(h);
    const int rec = s->diag_cost_size();
    return rec ? rec : fail(PDDP_EINVAL, "pddp_diag_cost_size: diagonal cost records belong to the pendulum, cart-pole and quadrotor (plants 1-3)");
}
extern "C" int pddp_set_diag_cost(pddp_handle h, const double* w) { IMPL(h); return s->set_diag_cost(w); }
extern "C" int pddp_set_diag_cost_problems(pddp_handle h, int count, const int* idx, const double* w) { IMPL(h); return s->set_diag_cost_problems(count, idx, w); }
extern "C" int pddp_get_diag_cost_problems(pddp_handle h, int count, const int* idx, double* w) { IMPL(h); return s->get_diag_cost_problems(count, idx, w); }
// per-knot goal trajectories of the same plants (goal_traj_table.hpp)
extern "C" int pddp_goal_trajectory_size(pddp_handle h) {
    IMPL(h);
    const int len = s->goal_trajectory_size();
    return len ? len : fail(PDDP_EINVAL, "pddp_goal_trajectory_size: goal trajectories belong to the pendulum, cart-pole and quadrotor (plants 1-3)");
}
extern "C" int pddp_set_goal_trajectory_problems(pddp_handle h, int count, const int* idx, const void* G) { IMPL(h); return s->set_goal_trajectory_problems(count, idx, G); }
extern "C" int pddp_get_goal_trajectory_problems(pddp_handle h, int count, const int* idx, void* G, int* has) { IMPL(h); return s->get_goal_trajectory_problems(count, idx, G, has); }
extern "C" int pddp_clear_goal_trajectory_problems(pddp_handle h, int count, const int* idx) { IMPL(h); return s->clear_goal_trajectory_problems(count, idx); }
// per-problem horizon times of the same plants (horizon_time_table.hpp): the handle checks every argument before it is touched
extern "C" int pddp_set_horizon_time_problems(pddp_handle h, int count, const int* idx, const double* total_time) { IMPL(h); return s->set_horizon_time_problems(count, idx, total_time); }
extern "C" int pddp_get_horizon_time_problems(pddp_handle h, int count, const int* idx, double* total_time, double* time_step) {
    IMPL(h); return s->get_horizon_time_problems(count, idx, total_time, time_step);
}
// control references of the same plants (control_ref_table.hpp): the handle checks every argument before it is touched
extern "C" int pddp_control_reference_size(pddp_handle h) {
    IMPL(h);
    const int len = s->control_reference_size();
    return len ? len : fail(PDDP_EINVAL, "pddp_control_reference_size: control references belong to the pendulum, cart-pole and quadrotor (plants 1-3)");
}
extern "C" int pddp_set_control_reference_problems(pddp_handle h, int count, const int* idx, const void* U) { IMPL(h); return s->set_control_reference_problems(count, idx, U); }
extern "C" int pddp_get_control_reference_problems(pddp_handle h, int count, const int* idx, void* U, int* has) { IMPL(h); return s->get_control_reference_problems(count, idx, U, has); }
extern "C" int pddp_clear_control_reference_problems(pddp_handle h, int count, const int* idx) { IMPL(h); return s->clear_control_reference_problems(count, idx); }
// goal paths of the same plants (goal_path_table.hpp): the handle checks every argument before it is touched
extern "C" int pddp_reserve_goal_path(pddp_handle h, int capacity) { IMPL(h); return s->reserve_goal_path(capacity); }
extern "C" int pddp_goal_path_capacity(pddp_handle h) { IMPL(h); return s->goal_path_capacity(); }
extern "C" int pddp_set_goal_path_problems(pddp_handle h, int count, const int* idx, int len, int mode, const int* cursor, const void* path) {
    IMPL(h); return s->set_goal_path_problems(count, idx, len, mode, cursor, path);
}
extern "C" int pddp_set_goal_path_cursor_problems(pddp_handle h, int count, const int* idx, const int* cursor) { IMPL(h); return s->set_goal_path_cursor_problems(count, idx, cursor); }
extern "C" int pddp_get_goal_path_problems(pddp_handle h, int count, const int* idx, int* len, int* mode, int* cursor, void* path) {
    IMPL(h); return s->get_goal_path_problems(count, idx, len, mode, cursor, path);
}
extern "C" int pddp_goal_path_profile(pddp_handle h, int timing, float* ms) { IMPL(h); return s->goal_path_profile(timing, ms); }
extern "C" int pddp_simulate(pddp_handle h, const void* x, const void* u, const void* KT, double t0_us, double elapsed_us, int substeps, const void* goal_xyz,
                             void* xActual_inout, double* avg_err, int* failed) {
    IMPL(h); if (!x || !u || !KT || !xActual_inout) return fail(PDDP_EINVAL, "null argument");
    return s->simulate(x, u, KT, t0_us, elapsed_us, substeps, goal_xyz, xActual_inout, avg_err, failed);
}
extern "C" int pddp_simulate_batch(pddp_handle h, const void* x, const void* u, const void* KT, const double* t0_us, const double* elapsed_us, int substeps,
                                   const void* goal_xyz, void* xActual_inout, double* avg_err, int* failed) {
    IMPL(h); if (!t0_us || !elapsed_us || !xActual_inout) return fail(PDDP_EINVAL, "pddp_simulate_batch: null t0_us, elapsed_us or xActual_inout");
    return s->simulate_batch(x, u, KT, t0_us, elapsed_us, substeps, goal_xyz, xActual_inout, avg_err, failed);
}
// the simulated robots of named slots (sim_slots.hpp): the handle checks every argument before anything is enqueued
extern "C" int pddp_simulate_problems(pddp_handle h, int count, const int* idx, const void* x, const void* u, const void* KT, const double* t0_us, const double* elapsed_us,
                                      const int* substeps, const void* goal_xyz, void* xActual_inout, double* avg_err, int* failed, int family) {
    IMPL(h); return s->simulate_problems(count, idx, x, u, KT, t0_us, elapsed_us, substeps, goal_xyz, xActual_inout, avg_err, failed, family);
}
extern "C" int pddp_ee_pos(pddp_handle h, int count, const void* x, void* eePos) { IMPL(h); if (!x || !eePos) return fail(PDDP_EINVAL, "null argument"); return s->ee_pos(count, x, eePos); }
extern "C" int pddp_set_ee_cost_shift(pddp_handle h, int on) { IMPL(h); s->cfg.ee_cost_shift = on ? 1 : 0; return 0; }
extern "C" int pddp_set_cost_ee(pddp_handle h, double Q_EE1, double Q_EE2, double QF_EE1, double QF_EE2, double R_EE, double Q_xEE, double QF_xEE,
                                double Q_xdEE, double QF_xdEE) {
    IMPL(h); const double v[9] = {Q_EE1, Q_EE2, QF_EE1, QF_EE2, R_EE, Q_xEE, QF_xEE, Q_xdEE, QF_xdEE}; return s->set_cost_ee(v);
}
extern "C" int pddp_set_benchmark_mode(pddp_handle h, int on) { IMPL(h); s->bench_mode = on ? 1 : 0; return 0; }
extern "C" int pddp_array_bytes(pddp_handle h, const char* name, size_t* bytes) { IMPL(h); void* p; return s->array(name, &p, bytes); }
extern "C" int pddp_refresh_reference_views(pddp_handle h) { IMPL(h); return s->reference_views(3); }
extern "C" int pddp_array_ptr(pddp_handle h, const char* name, void** ptr, size_t* bytes) { IMPL(h); if (!ptr || !bytes) return fail(PDDP_EINVAL, "null argument"); return s->array(name, ptr, bytes); }
extern "C" int pddp_set_array(pddp_handle h, const char* name, const void* host, size_t bytes) {
    IMPL(h); void* p; size_t cap; int rc = s->array(name, &p, &cap); if (rc) return rc;
    if (bytes > cap) return fail(PDDP_EINVAL, "set_array: too many bytes");
    HIPCHK(hipStreamSynchronize(s->stream));
    if (std::strcmp(name, "AB") == 0 && bytes < cap && (rc = s->ab_view(0))) return rc;      // a partial write lands on the current values
    // the first write into "H" of a handle that keeps the compact end-effector position block: bring the reference-layout array up to date FIRST (a partial write
    // then lands on the current values, and the caller's data is not overwritten by the expansion afterwards)
    if (std::strcmp(name, "H") == 0 && !s->h_overridden && (rc = s->h_view())) return rc;
    // A - B K / B du of a handle whose production sweeps compose maps instead of writing them: materialise both from the last sweep FIRST (the one that is not being
    // written must not stay stale, and the phase hook's rollouts must not rebuild over the caller's data afterwards)
    if ((std::strcmp(name, "ApBK") == 0 || std::strcmp(name, "Bdu") == 0) && s->fs_vars_stale && (rc = s->reference_views(1))) return rc;
    const bool cand = std::strcmp(name, "xs") == 0 || std::strcmp(name, "us") == 0;
    if (cand && s->cand_stale && (rc = s->cand_view(0))) return rc;                          // (the other of the two arrays must hold the records' values before both go back)
    HIPCHK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    if (cand) return s->cand_view(1);                                                         // handles whose setup adopts from the knot-major records: keep them in step
    if (std::strncmp(name, "model_", 6) == 0) return s->model_changed();
    if (std::strcmp(name, "AB") == 0) return s->ab_view(1);
    if (std::strcmp(name, "H") == 0 && !s->h_overridden) { s->h_overridden = true; s->drop_graph(); return s->ab_keep_reference_layout(); }
    return 0;
}
extern "C" int pddp_get_array(pddp_handle h, const char* name, void* host, size_t bytes) {
    IMPL(h); void* p; size_t cap; int rc = s->array(name, &p, &cap); if (rc) return rc;
    if (bytes > cap) return fail(PDDP_EINVAL, "get_array: too many bytes");
    HIPCHK(hipStreamSynchronize(s->stream));
    if (std::strcmp(name, "AB") == 0 && (rc = s->ab_view(0))) return rc;
    if (std::strcmp(name, "H") == 0 && (rc = s->h_view())) return rc;
    if ((std::strcmp(name, "ApBK") == 0 || std::strcmp(name, "Bdu") == 0) && s->fs_vars_stale && (rc = s->reference_views(1))) return rc;
    if ((std::strcmp(name, "xs") == 0 || std::strcmp(name, "us") == 0) && s->cand_stale && (rc = s->cand_view(0))) return rc;      // (handles whose rollouts keep records)
    HIPCHK(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost)); return 0;
}
extern "C" int pddp_get_state(pddp_handle h, pddp_state* out) { IMPL(h); return s->get_state(out); }
extern "C" int pddp_set_state(pddp_handle h, const pddp_state* in) { IMPL(h); return s->set_state(in); }
extern "C" int pddp_run_phase(pddp_handle h, int phase) { IMPL(h); return s->run_phase(phase); }
extern "C" int pddp_plant_eval(pddp_handle h, int what, int count, const void* x, const void* u, void* out) { IMPL(h); return s->plant_eval(what, count, x, u, out); }

extern "C" int pddp_hbm_calibration(int device, size_t bytes, int reps) {
    if (bytes < 4096 || reps < 1) return fail(PDDP_EINVAL, "hbm_calibration: bad arguments");
    HIPCHK(hipSetDevice(device));
    DeviceBuf a, b2;                 // (released on every return)
    if (!a.reserve(bytes) || !b2.reserve(bytes)) return fail(PDDP_ENODEVICE, "hbm_calibration: hipMalloc failed");
    HIPCHK(hipMemset(a.ptr, 1, bytes)); HIPCHK(hipMemset(b2.ptr, 0, bytes));
    for (int i = 0; i < reps; i++) hipLaunchKernelGGL(k_hbm_calib_dword, dim3(256 * 16), dim3(256), 0, 0, a.as<float>(), b2.as<float>(), bytes / sizeof(float));
    HIPCHK(hipGetLastError()); HIPCHK(hipDeviceSynchronize());
    return 0;
}

extern "C" int pddp_mpc_solve(pddp_handle h, const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout, int ifd,
                              int max_iter, double time_budget_ms, int poll_every, void* x, void* u, void* KT, void* Jout, int* alphaOut, int* success, int* iters) {
    IMPL(h);
    if (!xActual || !xGoal || !shift) return fail(PDDP_EINVAL, "pddp_mpc_solve: null argument");
    return s->mpc_solve(xActual, xGoal, shift, clear_vars, full_rollout, ifd, max_iter, time_budget_ms, poll_every, x, u, KT, Jout, alphaOut, success, iters);
}
extern "C" int pddp_mpc_load(pddp_handle h, const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout) {
    IMPL(h);
    if (!xActual || !xGoal || !shift) return fail(PDDP_EINVAL, "pddp_mpc_load: null argument");
    return s->mpc_load(xActual, xGoal, shift, clear_vars, full_rollout);
}
// control cycles of named slots: every argument is checked here, before the handle is touched
static int mpc_problems_check(SolverBase* s, const char* who, int count, const int* idx, const void* xActual, const void* xGoal, const int* shift) {
    if (count >= 1 && (!idx || !xActual || !xGoal || !shift)) return fail(PDDP_EINVAL, std::string(who) + ": null idx, xActual, xGoal or shift");
    if (int rc = slots_check(s, who, count, idx)) return rc;
    for (int i = 0; i < count; i++)
        if (shift[i] < 0 || shift[i] >= s->cfg.N - 1) return fail(PDDP_EINVAL, std::string(who) + ": shift[" + std::to_string(i) + "] = " + std::to_string(shift[i]) + " must be in [0, N-2]");
    return 0;
}
extern "C" int pddp_mpc_solve_problems(pddp_handle h, int count, const int* idx, const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout,
                                       int ifd, int max_iter, double time_budget_ms, int poll_every, void* x, void* u, void* KT, void* Jout, int* alphaOut, int* success,
                                       int* iters) {
    IMPL(h);
    if (int rc = mpc_problems_check(s, "pddp_mpc_solve_problems", count, idx, xActual, xGoal, shift)) return rc;
    if (max_iter < 1 || max_iter > s->cfg.max_iter) return fail(PDDP_EINVAL, "pddp_mpc_solve_problems: max_iter must be in [1, config.max_iter]");
    return s->mpc_solve_problems(count, idx, xActual, xGoal, shift, clear_vars, full_rollout, ifd, max_iter, time_budget_ms, poll_every, x, u, KT, Jout, alphaOut, success, iters);
}
extern "C" int pddp_mpc_load_problems(pddp_handle h, int count, const int* idx, const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout) {
    IMPL(h);
    if (int rc = mpc_problems_check(s, "pddp_mpc_load_problems", count, idx, xActual, xGoal, shift)) return rc;
    return s->mpc_load_problems(count, idx, xActual, xGoal, shift, clear_vars, full_rollout);
}
extern "C" int pddp_mpc_slots_profile(pddp_handle h, int timing, float* ms3) { IMPL(h); return s->mpc_slots_profile(timing, ms3); }
extern "C" int pddp_get_config(pddp_handle h, pddp_config* out) { IMPL(h); if (!out) return fail(PDDP_EINVAL, "null argument"); *out = s->cfg; return 0; }
extern "C" int pddp_stream(pddp_handle h, void** hip_stream) { IMPL(h); if (!hip_stream) return fail(PDDP_EINVAL, "null argument"); *hip_stream = (void*)s->stream; return 0; }

// runiLQR_GPU (DDPWrappers.cuh:10-138) for the batch.
extern "C" int pddp_solve_ex(pddp_handle h, void* x0, void* u0, const void* xGoal, const void* KT0, const void* P0, const void* p0, const void* d0,
                             void* Jout, int* alphaOut, int rollout, int clear, int ifd, int poll_every, double* times_ms, double* phase_ms,
                             int* sweeps_out) {
    IMPL(h);
    if (!x0 || !u0 || !xGoal) return fail(PDDP_EINVAL, "pddp_solve: null trajectory or goal");
    const double t0 = now_ms();
    int rc = s->load(x0, u0, xGoal, KT0, P0, p0, d0, rollout, clear, ifd);
    if (rc) return rc;
    double t_init = now_ms() - t0;
    std::vector<int> done(s->cfg.batch);
    const int chunk = poll_every > 0 ? poll_every : 8;         // sweeps enqueued between two polls of the exit flags
    const int stride = s->cfg.max_iter + 2;
    int sweeps = 0;
    for (int guard = 0; guard < 1000000; guard++) {
        if ((rc = phase_ms ? s->iterate_traced(chunk, phase_ms, sweeps, stride) : s->iterate(chunk))) return rc;
        sweeps += chunk;
        if ((rc = s->status(done.data(), nullptr))) return rc;
        bool all = true;
        for (int d : done) all &= (d != 0);
        if (all) break;
    }
    const double t1 = now_ms();
    if ((rc = s->store(x0, u0, nullptr, Jout, alphaOut, nullptr))) return rc;
    const double t2 = now_ms();
    if (times_ms) { times_ms[0] = t2 - t0; times_ms[1] = t_init + (t2 - t1); }
    if (sweeps_out) *sweeps_out = sweeps;
    return 0;
}
extern "C" int pddp_solve(pddp_handle h, void* x0, void* u0, const void* xGoal, void* Jout, int* alphaOut, int clear, int ifd, double* times_ms) {
    return pddp_solve_ex(h, x0, u0, xGoal, nullptr, nullptr, nullptr, nullptr, Jout, alphaOut, 0, clear, ifd, 8, times_ms, nullptr, nullptr);
}
