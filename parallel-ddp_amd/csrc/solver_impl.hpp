// Solver<Plant, Integrator, T>: buffers, kernel selection and launches of one handle (the host side of allocateMemory_GPU / runiLQR_GPU for a batch).  Included by the
// per-plant translation units only (pddp_plant_*.hip); the C ABI sees SolverBase (solver_base.hpp).
#pragma once
#include "solver_base.hpp"
#include "kernels.hpp"
#include "handle_setup.hpp"
#include "slots.hpp"
#include "cost_table.hpp"
#include "diag_cost_table.hpp"
#include "goal_traj_table.hpp"
#include "goal_path_table.hpp"
#include "horizon_time_table.hpp"
#include "control_ref_table.hpp"
#include "sim_slots.hpp"
#include "mpc_slots.hpp"
#include "mpc_record.hpp"
#include "tl_launch.hpp"
#include "mx_launch.hpp"

using namespace pddp;

template <typename P, int INTEG, typename T>
struct Solver : SolverBase {
    static constexpr int NX = P::NX, NU = P::NU, NM = NX + NU, NP = P::NPOS;
    Buffers<T> b{};
    MpcBuffers<T> mb{};
    T* d_xActual = nullptr; T* d_goal_in = nullptr; int* d_shift = nullptr;
    unsigned char* d_mpc_out = nullptr;      // MPC outputs of a control cycle packed per problem by k_mpc_store (one transfer)
    PinnedBuf h_state;                       // pinned copy target of the solver states (status polls)
    PinnedBuf h_stage;                       // pinned host staging of the MPC call (inputs, then outputs): its transfers are asynchronous, one sync per control cycle
    Dims dm{};
    SolverParams sp{};
    CostWeights<T> cw{};
    T dt{};
    std::map<std::string, std::pair<void*, size_t>> arrays;
    std::vector<DeviceBuf> allocs;           // the blocks behind `arrays`, the robot model and mpc_out
    // A handle's device and pinned memory are MemBufs (device_mem.hpp): members, or elements of `allocs`.  This is the one place that grows one: the stream is waited for
    // before a block that may still be in use is released, and a failed allocation returns the error code of its kind of memory (PDDP_ENOMEM device, PDDP_ENODEVICE pinned) with the message `what`.
    // (The wait costs the MPC call's h_stage nothing: its size is a function of cap_batch, N and max_iter, which are fixed per handle, so it never regrows.)
    template <typename Mem> int reserve(MemBuf<Mem>& buf, size_t bytes, const char* what, size_t min_cap = 0) {
        if (buf.holds(bytes)) return 0;
        if (buf.ptr) HIPCHK(hipStreamSynchronize(stream));
        return buf.reserve(bytes, min_cap) ? 0 : fail(Mem::kFailCode, what);
    }
    KernelPlan plan;               // which kernel family runs each phase and which optional arrays they need (kernel_plan.hpp); an intake area holds its handle's
    void resolve_plan() { plan = make_kernel_plan(cfg, PlantTraits{P::PLANT, NX, NU, P::kScalarPlugin, P::kPluginCost}, sizeof(T) == 4, tl_variant); }
    int tl_variant = -1;           // which built-in robot model the handle's tables equal (the thread-lane kernels fold it into literals); -1: neither
    T tl_grav = T(0);
    void derive_tl_model(const ArmModel<T>& hm) {
        ArmTlModel<T> m;
        tl_variant = -1;
        if (arm_tl_model_from_tables(m, hm))
            for (int v = 0; v < 2; v++) if (arm_tl_models_equal(m, arm_tl_builtin<T>(v))) tl_variant = v;
        tl_grav = hm.grav;
    }
    void derive_tl_model(const EmptyModel&) {}
    // pddp_set_array("model_I" / "model_F"): re-derive what the kernels take from the model tables as launch arguments
    void drop_graph() override {
        for (hipGraphExec_t* g : {&graph, &graph_lean, &graph_n, &graph_n_lean}) if (*g) { hipGraphExecDestroy(*g); *g = nullptr; }
        graph_mode = -1;
    }
    int ab_view(int to_compact) override {
        if constexpr (P::PLANT == 4) {
            if (b.ABc) { launch_abc_convert<T>(stream, b, (int)(cfg.batch * cfg.N), cfg.N, dt, to_compact); HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(stream)); }
        }
        return 0;
    }
    int ab_keep_reference_layout() override {
        if (!b.ABc) return 0;
        int rc = ab_view(0);       // (the caller refreshed the reference-layout H from the compact position block BEFORE it wrote into it: pddp_set_array)
        b.ABc = nullptr; b.Hc = nullptr; drop_graph();
        return rc;
    }
    // end-effector handles with the compact position block: refresh the reference-layout array "H" of the running knots from it (API view)
    int h_view() override {
        if constexpr (P::PLANT == 4) {
            if (b.Hc) {
                hipLaunchKernelGGL((k_hc_expand<T>), dim3((cfg.batch * cfg.N + 63) / 64), dim3(64), 0, stream, b, (int)(cfg.batch * cfg.N), cfg.N, hw[1], hw[2]);      // (with per-problem weights: every problem's own, from the table)
                HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(stream));
            }
        }
        return 0;
    }
    int cand_view(int to_records) override {
        if constexpr (P::PLANT != 4) {
            if (b.xw && plan.cf_fp_staged) {
                const dim3 g((unsigned)(((size_t)cfg.batch * cfg.N * cfg.A + 255) / 256));
                if (to_records) hipLaunchKernelGGL((k_cand_to_xw<P, T>), g, dim3(256), 0, stream, b, dm, (int)cfg.batch);
                else hipLaunchKernelGGL((k_xw_to_cand<P, T>), g, dim3(256), 0, stream, b, dm, (int)cfg.batch);
                HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(stream));
            }
        }
        cand_stale = false;
        return 0;
    }
    int reference_views(int what) override {
        if ((what & 1) && cfg.M > 1) { int rc = ab_view(0); if (rc) return rc; }           // (the reference-layout [A B] from the compact one)
        hipLaunchKernelGGL((k_reference_views<P, T>), dim3(cfg.N, cfg.batch), dim3(64), 0, stream, b, dm, what);
        HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(stream));
        if (what & 1) fs_vars_stale = false;
        if (what & 2) cand_stale = false;                // (xs / us now hold the winner in every slot: the records must not be expanded over them by the next pddp_get_array)
        return 0;
    }
    int model_changed() override {
        typename P::Model hm;
        HIPCHK(hipMemcpy(&hm, b.model, sizeof(hm), hipMemcpyDeviceToHost));
        derive_tl_model(hm);
        resolve_plan();
        drop_graph();
        return 0;
    }
    bool mpc_used = false;         // pddp_mpc_solve ran on this handle: its warm start shifts every cost-to-go slot, so the backward pass keeps writing all of them
    bool lean_ctg_ran = false;     // sweeps ran that left the interior cost-to-go slots unwritten (config.boundary_cost_to_go_only): a warm-started MPC call would shift stale slots
    // every knot's P, p written (the reference's d_P / d_p) unless the caller opted out; MPC handles always keep them (MPCHelpers.cuh:602-655 shifts the whole arrays)
    bool keep_all_ctg() const { return !cfg.boundary_cost_to_go_only || cfg.mpc_mode || mpc_used; }
    // The interior slots can only be looked at between two calls that enqueue sweeps, and what is there to see are the two halves of the double buffer: the interiors
    // of every problem's last two passes.  So the last kKeepSweeps sweeps of a call write them and the sweeps in front are lean for every problem that provably runs on
    // for two more sweeps (mx_launch.hpp; the pass checks max_iter and the maximum rho per problem).  The exit by tolerance cannot be foreseen, so it has to be
    // impossible: tol_cost <= 0 and a cost that is never negative (no negative weight; a table of per-problem weights is not looked through) -- a relative decrease
    // dJ / prevJ of an accepted step is then never below the tolerance.  Matrix-core backward pass of a handle that keeps every slot; everything else runs one kind of sweep.
    static constexpr int kKeepSweeps = 2;
    bool split_sweeps() const {
        const T w[] = {cw.Q1, cw.Q2, cw.R, cw.QF1, cw.QF2, cw.Q_EE1, cw.Q_EE2, cw.QF_EE1, cw.QF_EE2, cw.R_EE, cw.Q_xEE, cw.QF_xEE, cw.Q_xdEE, cw.QF_xdEE};
        for (T v : w) if (!(v >= T(0))) return false;
        return plan.bp_mfma && keep_all_ctg() && !(sp.tol_cost > 0.0) && !b.cwt;
    }
    hipGraphExec_t graph = nullptr, graph_lean = nullptr;      // one keeping sweep | one lean sweep (split_sweeps() only)
    int graph_mode = -1;
    size_t fp_lds = 0;

    // what is not memory.  The member buffers are released after this body, when the stream is gone: releasing device or pinned memory needs no stream.
    ~Solver() override {
        drop_graph();
        for (hipEvent_t e : trace_ev) hipEventDestroy(e);
        for (hipEvent_t e : slots_ev) if (e) hipEventDestroy(e);
        for (hipEvent_t e : gp_ev) if (e) hipEventDestroy(e);
        delete intake;                                              // (before the stream it runs on)
        if (stream && !intake_of) hipStreamDestroy(stream);        // (an intake area runs on its handle's stream)
    }
    void register_model(void* dmodel, const ArmModel<T>&) {
        arrays["model_I"] = {dmodel, sizeof(T) * kArmNB * 36};
        arrays["model_F"] = {(char*)dmodel + offsetof(ArmModel<T>, F), sizeof(T) * kArmNB * 16};
    }
    void register_model(void*, const EmptyModel&) {}
    template <typename U> int alloc(const char* name, U** out, size_t count) {
        DeviceBuf blk;
        if (!blk.reserve(count * sizeof(U))) return fail(PDDP_ENOMEM, std::string("hipMalloc failed for ") + name);
        if (hipMemset(blk.ptr, 0, count * sizeof(U)) != hipSuccess) return fail(PDDP_ENODEVICE, "hipMemset failed");
        arrays[name] = {blk.ptr, count * sizeof(U)}; *out = blk.template as<U>();
        allocs.push_back(std::move(blk));
        return 0;
    }
    int init() override {
        const pddp_config& c = cfg;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= c.device)
            return fail(PDDP_ENODEVICE, "no HIP device available: libpddp has no CPU fallback");
        HIPCHK(hipSetDevice(c.device));
#ifdef PDDP_REF_PLANT_FILE
        if constexpr (P::PLANT == 5) { const std::string complaint = ref_plugin_setup<T>(c.N); if (!complaint.empty()) return fail(PDDP_EINVAL, complaint); }
#endif
        if constexpr (P::PLANT == 5) {
            if (!scalar_plugin_qdd_is_dynamics<P, T>())
                return fail(PDDP_EINVAL, "plant 5: the plug-in's gradient routine returns a qdd that differs from its dynamics routine at the same state; the kernel families build the "
                                         "integrators' stage states from either one, so the two have to be the same numbers (call the dynamics routine inside the gradient routine)");
        }
        if (intake_of) stream = intake_of->stream;
        else HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        dm.N = c.N; dm.M = c.M; dm.A = c.A; dm.NB = c.N / c.M;
        cap_batch = c.batch;
        sp = solver_params_of(c); cw = cost_weights_of<T, P::PLANT>(c); dt = time_step<T>(c);
        const size_t B = c.batch, N = c.N, A = c.A, M = c.M;
        int rc = for_each_array<NX, NU>(c, b, mb, arrays, [this](const char* name, auto** out, size_t count) { return alloc(name, out, count); });
        if (rc) return rc;
        // MPC inputs of a control cycle in ONE device run (one transfer): measured states | goals | shifts
        const MpcInputRun in = mpc_input_run(sizeof(T), NX, B);
        if ((rc = alloc("mpc_in", &d_xActual, in.elems))) return rc;
        d_goal_in = mpc_at<T>(d_xActual, in.goal); d_shift = mpc_at<int>(d_xActual, in.shift);
        arrays["xActual"] = {d_xActual, in.x_bytes}; arrays["shift"] = {d_shift, in.shift_bytes};     // the views the facade's GPUVars name (MPCHelpers.hpp)
        std::vector<T> al(A);
        alpha_table(c, al.data());
        HIPCHK(hipMemcpy(b.alpha, al.data(), A * sizeof(T), hipMemcpyHostToDevice));
        typename P::Model hm; fill_model(hm, c);
        allocs.emplace_back();
        if (!allocs.back().reserve(sizeof(hm))) return fail(PDDP_ENODEVICE, "hipMalloc failed for the robot model");
        void* dmodel = allocs.back().ptr;
        HIPCHK(hipMemcpy(dmodel, &hm, sizeof(hm), hipMemcpyHostToDevice));
        b.model = dmodel;
        register_model(dmodel, hm);
        derive_tl_model(hm);
        if (intake_of) adopt_selection(*intake_of); else resolve_plan();      // before the arrays below that exist only on some kernel families
        if (plan.xw_rec) { b.xw_rec = plan.xw_rec; if ((rc = alloc("xw", &b.xw, B * N * A * b.xw_rec))) return rc; }   // candidate records: staged closed-form rollouts (k_fp_cf), knot-major states of the thread-lane arm (fp_tl.hpp)
        if (plan.segmap) { if ((rc = alloc("segmap", &b.segmap, B * M * 256))) return rc; }
        if (plan.ab_compact) { if ((rc = alloc("ABc", &b.ABc, abc_floats(B * N)))) return rc; }
        if (plan.h_compact) { if ((rc = alloc("Hc", &b.Hc, B * N * 49 + 16))) return rc; }
        // device tables of per-alpha pointers, the reference's d_x / d_u / d_d (nisInitHelpers.cuh:777-789,808-813)
        void** tab[3]; const char* tn[3] = {"xs_ptrs", "us_ptrs", "ds_ptrs"};
        T* base[3] = {b.xs, b.us, b.ds}; const size_t per[3] = {N * NX, N * NU, N * NX};
        for (int t = 0; t < 3; t++) {
            if ((rc = alloc(tn[t], &tab[t], B * A))) return rc;
            std::vector<void*> hp(B * A);
            for (size_t i = 0; i < B * A; i++) hp[i] = base[t] + i * per[t];
            HIPCHK(hipMemcpy(tab[t], hp.data(), B * A * sizeof(void*), hipMemcpyHostToDevice));
        }
        fp_lds = FpLds<P, T>::bytes(c.M, c.N);
        if constexpr (P::PLANT == 4) {                                 // lane-group forward pass: A * (N + M) elements of dynamic LDS per workgroup
            const size_t a_wg = (c.A > 8 && c.A % 8 == 0) ? 8 : c.A;       // candidates per workgroup (launch_fp_rollouts)
            const size_t lds = a_wg * (c.N + c.M) * sizeof(T);
            if (lds > 160 * 1024) return fail(PDDP_EINVAL, "forward-pass LDS footprint (candidates per workgroup * (N + M) elements) exceeds 160 KiB: reduce A or N");
            if (lds > 48 * 1024) {
                for (int k = 0; k < 6; k++) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(fp_lg_kernel(k % 3, k >= 3)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            }
        }
        if (plan.fp_coop_lds) {
            if (fp_lds > 160 * 1024) return fail(PDDP_EINVAL, "forward-pass LDS footprint exceeds 160 KiB: reduce M");
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fp<P, INTEG, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fp_lds));
        }
        HIPCHK(hipDeviceSynchronize());
        return 0;
    }
    int load(const void* x0, const void* u0, const void* xg, const void* KT0, const void* P0, const void* p0, const void* d0, int rollout, int clear,
             int ignore_first_defect) override {
        if (int rc = enqueue_load(x0, u0, xg, KT0, P0, p0, d0, rollout, clear, ignore_first_defect)) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        loaded = true;
        return 0;
    }
    // the whole load on the stream, without the wait (pddp_load_problems enqueues the scatter of the loaded problems behind it)
    int enqueue_load(const void* x0, const void* u0, const void* xg, const void* KT0, const void* P0, const void* p0, const void* d0, int rollout, int clear,
                     int ignore_first_defect) {
        const size_t B = cfg.batch, N = cfg.N;
        // current trajectory goes to half 0 of xb (state.cur = 0 after init): one strided copy for the whole batch
        HIPCHK(hipMemcpy2DAsync(b.xb, 2 * N * NX * sizeof(T), x0, N * NX * sizeof(T), N * NX * sizeof(T), B, hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(b.ucur, u0, B * N * NU * sizeof(T), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(b.xGoal, xg, B * NX * sizeof(T), hipMemcpyHostToDevice, stream));
        if (clear) {                                                 // clearVarsFlag, nisInitHelpers.cuh:612-619
            HIPCHK(hipMemsetAsync(b.P, 0, B * N * NX * NX * sizeof(T), stream)); HIPCHK(hipMemsetAsync(b.Pp, 0, B * N * NX * NX * sizeof(T), stream));
            HIPCHK(hipMemsetAsync(b.p, 0, B * N * NX * sizeof(T), stream)); HIPCHK(hipMemsetAsync(b.pp, 0, B * N * NX * sizeof(T), stream));
            HIPCHK(hipMemsetAsync(b.KT, 0, B * N * NX * NU * sizeof(T), stream)); HIPCHK(hipMemsetAsync(b.dcur, 0, B * N * NX * sizeof(T), stream));
        } else {                                                     // warm start (:621-628); a NULL array keeps the device values
            if (P0) { HIPCHK(hipMemcpyAsync(b.P, P0, B * N * NX * NX * sizeof(T), hipMemcpyHostToDevice, stream)); HIPCHK(hipMemcpyAsync(b.Pp, P0, B * N * NX * NX * sizeof(T), hipMemcpyHostToDevice, stream)); }
            if (p0) { HIPCHK(hipMemcpyAsync(b.p, p0, B * N * NX * sizeof(T), hipMemcpyHostToDevice, stream)); HIPCHK(hipMemcpyAsync(b.pp, p0, B * N * NX * sizeof(T), hipMemcpyHostToDevice, stream)); }
            if (KT0) HIPCHK(hipMemcpyAsync(b.KT, KT0, B * N * NX * NU * sizeof(T), hipMemcpyHostToDevice, stream));
            if (d0) HIPCHK(hipMemcpyAsync(b.dcur, d0, B * N * NX * sizeof(T), hipMemcpyHostToDevice, stream));
        }
        HIPCHK(hipMemsetAsync(b.du, 0, B * N * NU * sizeof(T), stream));   // always (:630-632)
        HIPCHK(hipMemsetAsync(b.err, 0, B * cfg.M * sizeof(int), stream));
        HIPCHK(hipMemsetAsync(b.dmax, 0, B * cfg.A * sizeof(T), stream));
        const int ee = cfg.ee_cost ? 1 : 0;                          // end-effector cost: the initial cost comes out of the setup kernel (stage 2)
        HIPCHK(hipMemsetAsync(b.tshift, 0, B * sizeof(int), stream));
        if (rollout) {                                               // forwardRolloutFlag (:642-648)
            launch_init_cost(stream, ignore_first_defect, 1, ee, 0);   // state.cur = 0
            launch_fp(stream, kFpInitial);
            hipLaunchKernelGGL((k_adopt_slot0<P, T>), dim3(N, B), dim3(64), 0, stream, b, dm);
        }
        launch_init_cost_and_setup(stream, ignore_first_defect, rollout, 0);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // what starts a solve from the loaded trajectory: initial cost, setup kernel in init mode and, for the end-effector cost, the cost's second pass (its initial cost comes
    // out of the setup kernel).  keep_alpha: the MPC call keeps alphaIndex (runiLQR_MPC_GPU does not reset it)
    void launch_init_cost(hipStream_t s, int ignore_first_defect, int rollout, int stage, int keep_alpha) {
        with_ref_cost_plant([&](auto pl) {
            using Q = decltype(pl);
            hipLaunchKernelGGL((k_init_cost<Q, T>), dim3(cfg.batch), dim3(64), (size_t)cfg.N * sizeof(T), s, b, dm, cw, sp, ignore_first_defect, rollout, stage, keep_alpha);
        });
    }
    void launch_init_cost_and_setup(hipStream_t s, int ignore_first_defect, int rollout, int keep_alpha) {
        const int ee = cfg.ee_cost ? 1 : 0;
        launch_init_cost(s, ignore_first_defect, rollout, ee, keep_alpha);
        launch_nis(s, 1);
        if (ee) launch_init_cost(s, ignore_first_defect, rollout, 2, keep_alpha);
    }
    // forward pass: plan_fp_launch (kernel_plan.hpp) resolves what `mode` launches -- in production plan.sweep and plan.fp, the kernels pddp_time_kernels names --, the
    // two switches below launch it.  What is not plan is applied here: the line search's mode, the robot model's variant, the arrays this handle has.
    void launch_fp(hipStream_t s, FpMode mode) {
        const FpLaunch L = plan_fp_launch(plan, cfg, mode);
        if (L.cand_stale) cand_stale = true;
        launch_fp_sweep(s, L);
        launch_fp_rollouts(s, L);
    }
    // the record kernels of the closed-form plants (kernels.hpp fp_cf_body): whole problems per wavefront, the step-size count a template argument
    template <int AA> void launch_cf(hipStream_t s, bool rollouts) {
        if constexpr (P::PLANT != 4 && P::kScalarPlugin && (64 / AA) * P::NX <= 64) {
            const unsigned B = cfg.batch;
            const dim3 grid((B + 64 / AA - 1) / (64 / AA));
            if (rollouts) with_ref_plant([&](auto pl) { using Q = decltype(pl); hipLaunchKernelGGL((k_fp_cf<Q, INTEG, T, AA>), grid, dim3(64), 0, s, b, dm, cw, dt, (int)B); });
            else hipLaunchKernelGGL((k_sweep_cf<P, INTEG, T, AA>), grid, dim3(64), 0, s, b, dm, cw, dt, (int)B);
        }
    }
    // k_fp_lg by workgroup size (0: up to 256 threads, 1: 512, 2: 1024) and cost family
    using FpLgKernel = void (*)(Buffers<T>, Dims, CostWeights<T>, T, int);
    static FpLgKernel fp_lg_kernel(int size, bool ee) {
        static constexpr FpLgKernel k[2][3] = {{&k_fp_lg<T, 256, false>, &k_fp_lg<T, 512, false>, &k_fp_lg<T, 1024, false>}, {&k_fp_lg<T, 256, true>, &k_fp_lg<T, 512, true>, &k_fp_lg<T, 1024, true>}};
        return k[ee][size];
    }
    void launch_fp_sweep(hipStream_t s, const FpLaunch& L) {
        const unsigned B = cfg.batch;
        switch (L.sweep) {
        case kSweepNone: break;
        case kSweepLg:
            if constexpr (P::PLANT == 4) hipLaunchKernelGGL((k_sweep_lg<T>), dim3((cfg.A + kLgPerWave - 1) / kLgPerWave, B), dim3(64), 0, s, b, dm, dt);
            break;
        case kSweepSt: if constexpr (P::PLANT == 4 && sizeof(T) == 4) launch_sweep_st(s, b, dm, (int)B); break;
        case kSweepWg: if constexpr (P::PLANT == 4 && sizeof(T) == 4) launch_sweep_wg(s, b, dm, (int)B); break;
        case kSweepMaps: if constexpr (P::PLANT == 4) launch_sweep_maps<T>(s, b, dm, (int)B); break;
        case kSweepCf: if (cfg.A == 16) launch_cf<16>(s, false); else if (cfg.A == 8) launch_cf<8>(s, false); break;      // segment start states -> the candidates' records
        case kSweepMapsCf:        // the same from the maps the fused matrix-core backward pass left
            if constexpr (P::PLANT != 4 && P::NX == 12 && P::NU == 4) hipLaunchKernelGGL((k_sweep_maps_cf<P, T>), dim3((B + 3) / 4), dim3(64), 0, s, b, dm, (int)B);
            break;
        }
    }
    void launch_fp_rollouts(hipStream_t s, const FpLaunch& L) {
        const unsigned B = cfg.batch;
        const int A_all = L.seed == 1 ? 1 : cfg.A;                  // the initial rollout: one candidate
        switch (L.fp) {
        case kFpKernNone: break;
        case kFpKernTl:           // one thread per (candidate, segment) rollout
            if constexpr (P::PLANT == 4) launch_fp_tl<T>(s, tl_variant, b, dm, cw, dt, tl_grav, (int)B, L.store_candidates ? 1 : 0);
            break;
        case kFpKernTl2: if constexpr (P::PLANT == 4 && sizeof(T) == 4) launch_fp_tl2(s, tl_variant, b, dm, cw, dt, tl_grav, (int)B); break;
        case kFpKernTl4:
            if constexpr (P::PLANT == 4) launch_fp_tl4<T>(s, tl_variant, b, dm, cw, dt, tl_grav, (int)B, sp, L.ls_tail ? bench_mode : -1, L.maps_prologue);
            break;
        case kFpKernLg:
            if constexpr (P::PLANT == 4) {
                const unsigned chunks = (A_all > 8 && A_all % 8 == 0) ? A_all / 8 : 1;      // one workgroup per 8 candidates when they tile exactly (see k_fp_lg)
                const int A_eff = A_all / chunks;
                const unsigned waves = (A_eff * cfg.M + kLgPerWave - 1) / kLgPerWave;
                hipLaunchKernelGGL(fp_lg_kernel(waves <= 4 ? 0 : waves <= 8 ? 1 : 2, cfg.ee_cost != 0), dim3(B, chunks), dim3(64 * waves), (size_t)A_eff * (cfg.N + cfg.M) * sizeof(T), s,
                                   b, dm, cw, dt, L.seed == 1 ? 1 : 0);
            }
            break;
        case kFpKernCf: if (cfg.A == 16) launch_cf<16>(s, true); else if (cfg.A == 8) launch_cf<8>(s, true); break;
        case kFpKernTs:           // (the arm has its own families: no thread-serial instantiation of its cooperative bodies)
            if constexpr (P::PLANT != 4) with_ref_plant([&](auto pl) { using Q = decltype(pl); hipLaunchKernelGGL((k_fp_ts<Q, INTEG, T>), dim3((B * cfg.A + 63) / 64), dim3(64), 0, s, b, dm, cw, dt, (int)B, L.seed == 2 ? 1 : 0); });
            break;
        case kFpKernCoop:
            with_ref_plant([&](auto pl) { using Q = decltype(pl); hipLaunchKernelGGL((k_fp<Q, INTEG, T>), dim3(A_all, B), dim3(64 * cfg.M), fp_lds, s, b, dm, cw, dt, L.seed); });
            break;
        }
        if constexpr (P::PLANT != 4) { if (L.cand_to_xw && b.xw) hipLaunchKernelGGL((k_cand_to_xw<P, T>), dim3((unsigned)(((size_t)B * cfg.N * cfg.A + 255) / 256)), dim3(256), 0, s, b, dm, (int)B); }
    }
    // part: -1 everything; 0 nothing (slot of a former separate winner kernel in the per-kernel timing); 1 only the setup kernel
    // The running knots' cost Hessian the matrix-core backward pass does not read (diag_h) is the one the LAST setup kernel wrote -- the reference's d_H holds exactly
    // that (costGradientHessianKern runs inside the setup, nisInitHelpers.cuh:46-93).  The weights are therefore remembered at every setup launch: a pddp_set_cost /
    // pddp_set_cost_ee between a setup and the next backward pass (phase hook, re-captured graph) must not mix new weights into a Hessian whose gradient and compact
    // position block still carry the old ones.
    T hw[3] = {T(0), T(0), T(0)};
    void note_setup_weights() { const bool ee = cfg.ee_cost != 0; hw[0] = ee ? cw.Q_xEE : cw.Q1; hw[1] = ee ? cw.Q_xdEE : cw.Q2; hw[2] = ee ? cw.R_EE : cw.R; }
    void launch_nis(hipStream_t s, int mode, int part = -1) {
        const unsigned B = cfg.batch;
        if (part == 0) return;
        note_setup_weights();
        switch (plan.nis) {
        case kNisTl:                  // mode 0: adopts the accepted candidate first (arm_tl_adopt_knot)
            if constexpr (P::PLANT == 4) launch_nis_tl<T>(s, tl_variant, b, dm, cw, dt, tl_grav, mode, (int)B);
            break;
        case kNisTl7:
            if constexpr (P::PLANT == 4) launch_nis_tl7<T>(s, tl_variant, b, dm, cw, dt, tl_grav, mode, (int)B);
            break;
        case kNisLg:
            if constexpr (P::PLANT == 4) {
                if (cfg.ee_cost) hipLaunchKernelGGL((k_nis_lg<T, true>), dim3((cfg.N + 31) / 32, B), dim3(256), 0, s, b, dm, cw, dt, mode);
                else hipLaunchKernelGGL((k_nis_lg<T>), dim3((cfg.N + 31) / 32, B), dim3(256), 0, s, b, dm, cw, dt, mode);
            }
            break;
        case kNisTs:
            if constexpr (P::PLANT != 4) with_ref_plant([&](auto pl) { using Q = decltype(pl); hipLaunchKernelGGL((k_nis_ts<Q, INTEG, T>), dim3((B * cfg.N + 63) / 64), dim3(64), 0, s, b, dm, cw, dt, mode, (int)B); });
            break;
        case kNisKb:
            if constexpr (P::PLANT != 4 && P::NX + P::NU <= 16 && INTEG == 3 && P::kScalarPlugin) {
                const int units = (int)(B * cfg.N);
                with_ref_plant([&](auto pl) {
                    using Q = decltype(pl);
                    if (plan.kb_nis == 16) hipLaunchKernelGGL((k_nis_kb<Q, T, 16>), dim3((units + 15) / 16), dim3(64), 0, s, b, dm, cw, dt, mode, (int)B);
                    else if (plan.kb_nis == 20) hipLaunchKernelGGL((k_nis_kb<Q, T, 20>), dim3((units + 19) / 20), dim3(64), 0, s, b, dm, cw, dt, mode, (int)B);
                    else if (plan.kb_nis == 64 && sizeof(T) == 4) hipLaunchKernelGGL((k_nis_kb<Q, T, sizeof(T) == 4 ? 64 : 16>), dim3((units + 63) / 64), dim3(64), 0, s, b, dm, cw, dt, mode, (int)B);
                    else hipLaunchKernelGGL((k_nis_kb<Q, T, 32>), dim3((units + 31) / 32), dim3(64), 0, s, b, dm, cw, dt, mode, (int)B);
                });
            }
            break;
        case kNisGl:
            if constexpr (P::PLANT != 4 && P::NX + P::NU <= 16) {
                with_ref_plant([&](auto pl) {
                    using Q = decltype(pl);
                    if (plan.gl_nis8) hipLaunchKernelGGL((k_nis_gl<Q, INTEG, T, 8>), dim3((B * cfg.N + 7) / 8), dim3(64), 0, s, b, dm, cw, dt, mode, (int)B);
                    else hipLaunchKernelGGL((k_nis_gl<Q, INTEG, T, 16>), dim3((B * cfg.N + 3) / 4), dim3(64), 0, s, b, dm, cw, dt, mode, (int)B);
                });
            }
            break;
        case kNisCoop:
            if constexpr (P::PLANT == 4) { if (b.cwt) { hipLaunchKernelGGL((k_nis<P, INTEG, T, true>), dim3(cfg.N, B), dim3(64), 0, s, b, dm, cw, dt, mode); break; } }
            with_ref_plant([&](auto pl) { using Q = decltype(pl); hipLaunchKernelGGL((k_nis<Q, INTEG, T>), dim3(cfg.N, B), dim3(64), 0, s, b, dm, cw, dt, mode); });
            break;
        }
    }
    // fused_hook: pddp_run_phase(PDDP_PHASE_BP_FUSED), the hook's backward pass composing the sweep maps as production's does
    // lean: a sweep of split_sweeps() in front of its call's last kKeepSweeps -- interior cost-to-go slots unwritten for the problems that run on
    void launch_bp(hipStream_t s, int store_candidates, bool fused_hook = false, bool lean = false) {
        const unsigned B = cfg.batch;
        switch (plan.bp) {
        case kBpMfma:
            if constexpr (P::PLANT == 4) {
                // the running knots' cost Hessian is known without reading it: the joint-space cost's diagonal, or (end-effector cost on the compact path) the diagonal of
                // the nominal-state / control weights + the compact position block b.Hc
                const bool ee = cfg.ee_cost != 0;
                const bool diag_h = !h_overridden && (!ee || b.Hc != nullptr);
                launch_bp_mfma<T>(s, b, dm, (int)B, diag_h, hw[0], hw[1], hw[2], dt, (keep_all_ctg() && !lean) || store_candidates,
                                  plan.sweep_fused && (!store_candidates || fused_hook), ee ? 1 : 0, lean ? &sp : nullptr);      // (per-problem weights: the diagonal comes from the table, not from hw)
            }
            break;
        case kBpLg:
            if constexpr (P::PLANT == 4) hipLaunchKernelGGL((k_bp_lg<T>), dim3((B * cfg.M + kLgPerWave - 1) / kLgPerWave), dim3(64), 0, s, b, dm, (int)B);
            break;
        case kBpTs:
            if constexpr (P::PLANT != 4) hipLaunchKernelGGL((k_bp_ts<P, T>), dim3((B * cfg.M + 63) / 64), dim3(64), 0, s, b, dm, (int)B);
            break;
        case kBpMq:
            if constexpr (P::PLANT != 4 && P::NX == 12 && P::NU == 4) {
                const bool fu = plan.mq_fused && (!store_candidates || fused_hook);      // (the phase hook's backward pass writes A - B K / B du: its sweep is teacher-forced from them)
                const bool dh = !P::kPluginCost && !h_overridden;   // the plant's own diagonal cost Hessian: not read
                // (only the instantiations that take the running knots' Hessian from the weights differ with a table of diagonal records: the others read H)
                if (dh && fu) with_weight_plant([&](auto pl) { using Q = decltype(pl); hipLaunchKernelGGL((k_bp_mq<Q, T, true, true>), dim3(B * cfg.M), dim3(64), 0, s, b, dm, cw, (int)B); });
                else if (dh) with_weight_plant([&](auto pl) { using Q = decltype(pl); hipLaunchKernelGGL((k_bp_mq<Q, T, true>), dim3(B * cfg.M), dim3(64), 0, s, b, dm, cw, (int)B); });
                else if (fu) hipLaunchKernelGGL((k_bp_mq<P, T, false, true>), dim3(B * cfg.M), dim3(64), 0, s, b, dm, cw, (int)B);
                else hipLaunchKernelGGL((k_bp_mq<P, T, false>), dim3(B * cfg.M), dim3(64), 0, s, b, dm, cw, (int)B);
            }
            break;
        case kBpCl:
            if constexpr (P::PLANT != 4 && P::NX == 12 && P::NU == 4)
                with_weight_plant([&](auto pl) { using Q = decltype(pl); hipLaunchKernelGGL((k_bp_cl<Q, T>), dim3((B * cfg.M + 3) / 4), dim3(64), 0, s, b, dm, cw, (int)B, (!P::kPluginCost && !h_overridden) ? 1 : 0); });
            break;
        case kBpGl:
            if constexpr (P::PLANT != 4 && P::NX + P::NU <= 16) {
                if (plan.gl_bp32) hipLaunchKernelGGL((k_bp_gl<P, T, 32>), dim3((B * cfg.M + 1) / 2), dim3(64), 0, s, b, dm, (int)B);
                else hipLaunchKernelGGL((k_bp_gl<P, T, 16>), dim3((B * cfg.M + 3) / 4), dim3(64), 0, s, b, dm, (int)B);
            }
            break;
        case kBpWide: hipLaunchKernelGGL((k_bp_wide<P, T>), dim3(cfg.M, B), dim3(256), 0, s, b, dm); break;
        case kBpCoop: hipLaunchKernelGGL((k_bp<P, T>), dim3(cfg.M, B), dim3(64), 0, s, b, dm); break;
        }
    }
    // one sweep, or its phase `only`.  store_candidates: the phase hook; part 0 / 1: the forward pass's sweep / rollout kernel alone (per-kernel timing); lean: launch_bp
    void launch_sweep(hipStream_t s, int only = -1, int store_candidates = 0, int part = -1, bool lean = false) {
        const unsigned B = cfg.batch;
        if (only < 0 || only == PDDP_PHASE_BP) launch_bp(s, store_candidates, false, lean);
        if (only < 0 || only == PDDP_PHASE_FP) launch_fp(s, store_candidates ? kFpHook : part == 0 ? kFpSweepOnly : part == 1 ? kFpRolloutsOnly : kFpProduction);
        if ((only < 0 || only == PDDP_PHASE_LS) && !(plan.ls_in_rollouts && !store_candidates)) {      // (k_fp_tl4 ended with the line search of its problems)
            if (plan.ls_many) hipLaunchKernelGGL((k_ls_many<T>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, b, dm, sp, bench_mode, (int)B);
            else hipLaunchKernelGGL((k_ls<T>), dim3(B), dim3(64), 0, s, b, dm, sp, bench_mode);
        }
        if (only < 0 || only == PDDP_PHASE_NIS) launch_nis(s, 0, part);
    }
    // The kernels of one sweep in launch order, by name, and their average duration over `sweeps` sweeps (an event after every launch, one pass).
    // Slots: 0 backward pass, 1 linear sweep, 2 rollouts, 3 line search, 4 winner re-roll, 5 next-iteration setup; a path without a separate kernel
    // for a slot leaves its name empty and its time 0 (kernel_plan.hpp plan_kernel_names: the names of the enums launch_bp / launch_fp / launch_nis switch over).
    int time_kernels(int sweeps, float* ms, char* names, int name_stride) override {
        const char* nm[6];
        plan_kernel_names(plan, cfg, nm);
        static const int phase_of[6] = {PDDP_PHASE_BP, PDDP_PHASE_FP, PDDP_PHASE_FP, PDDP_PHASE_LS, PDDP_PHASE_NIS, PDDP_PHASE_NIS};
        const int part_of[6] = {-1, 0, plan.maps_in_rollouts ? -1 : 1, -1, 0, 1};      // (a rollout kernel that begins with the sweep is timed as it runs in production)
        HIPCHK(hipStreamSynchronize(stream));
        note_sweeps_enqueued();
        if (int erc = need_events(7 * (size_t)sweeps)) return erc;
        for (int i = 0; i < sweeps; i++) {
            const bool lean = split_sweeps() && i + kKeepSweeps < sweeps;                         // (pddp_iterate's schedule)
            HIPCHK(hipEventRecord(trace_ev[7 * i], stream));
            for (int k = 0; k < 6; k++) { if (nm[k][0]) launch_sweep(stream, phase_of[k], 0, part_of[k], lean); HIPCHK(hipEventRecord(trace_ev[7 * i + k + 1], stream)); }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        for (int k = 0; k < 6; k++) {
            double sum = 0;
            for (int i = 0; i < sweeps; i++) { float t = 0; HIPCHK(hipEventElapsedTime(&t, trace_ev[7 * i + k], trace_ev[7 * i + k + 1])); sum += t; }
            ms[k] = nm[k][0] ? (float)(sum / sweeps) : 0.f;
            if (names) { std::strncpy(names + (size_t)k * name_stride, nm[k], name_stride - 1); names[(size_t)k * name_stride + name_stride - 1] = 0; }
        }
        return 0;
    }
    // One sweep is one graph; a second executable holds kGraphUnroll sweeps back to back: between the kernels INSIDE a graph there is no gap, between two graph
    // launches ~9 us (measured, rocprofv3 kernel trace) -- 5 % of a single problem's 175 us iteration, nothing at large batch.
    // With split_sweeps() each exists twice: graph / graph_n end a call (graph: one keeping sweep; graph_n: kGraphUnroll - kKeepSweeps lean sweeps and the
    // kKeepSweeps keeping ones), graph_lean / graph_n_lean hold lean sweeps only.
    static constexpr int kGraphUnroll = 4;
    hipGraphExec_t graph_n = nullptr, graph_n_lean = nullptr;
    // `count` sweeps, the first `lean` of them lean
    int capture_sweeps(int count, int lean, hipGraphExec_t* out) {
        hipGraph_t gr;
        HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < count; i++) launch_sweep(stream, -1, 0, -1, i < lean);
        {   // a failed launch inside the capture must not leave the stream capturing
            const hipError_t le = hipGetLastError(), ce = hipStreamEndCapture(stream, &gr);
            if (le != hipSuccess || ce != hipSuccess) {
                if (ce == hipSuccess && gr) hipGraphDestroy(gr);
                return fail(PDDP_ENODEVICE, std::string("sweep capture failed: ") + hipGetErrorString(le != hipSuccess ? le : ce));
            }
        }
        HIPCHK(hipGraphInstantiate(out, gr, nullptr, nullptr, 0));
        HIPCHK(hipGraphDestroy(gr));
        return 0;
    }
    // production sweeps leave the reference-layout views behind (marked here, not only in launch_fp: a hipGraph REPLAY does not pass through the launch functions)
    void note_sweeps_enqueued() {
        if (plan.sweep_fused || plan.mq_fused) fs_vars_stale = true;
        if (plan.cf_fp && plan.cf_fp_staged) cand_stale = true;
    }
    int iterate(int sweeps) override {
        if (plan.bp_mfma && !keep_all_ctg()) lean_ctg_ran = true;
        if (sweeps > 0) note_sweeps_enqueued();
        const bool split = split_sweeps();                                             // every sweep but the last kKeepSweeps is lean
        if (sweeps > 0 && cfg.use_graph) {
            const int key = bench_mode + 2 * sp.max_iter + (split ? 1 << 30 : 0);      // (the iteration limit is part of a lean pass's arguments; graph_n holds lean sweeps only with the split)
            if (!graph || graph_mode != key) {
                drop_graph();
                int rc = capture_sweeps(1, 0, &graph);
                if (rc) return rc;
                graph_mode = key;
            }
            // executables captured on first use; without the split the keeping ones stand for both kinds
            auto need = [&](hipGraphExec_t* g, int count, int lean) { return *g ? 0 : capture_sweeps(count, lean, g); };
            const bool unroll = sweeps >= kGraphUnroll && (size_t)cfg.batch * cfg.N <= 65536;      // only where a launch gap is a visible share of a sweep
            const int tail = unroll ? kGraphUnroll : sweeps < kKeepSweeps ? sweeps : kKeepSweeps;      // sweeps of the executable(s) that end the call
            int front = sweeps - tail;
            if (split && front > 0) { if (int rc = need(&graph_lean, 1, 1)) return rc; }
            hipGraphExec_t one = split ? graph_lean : graph;
            if (unroll) {
                if (int rc = need(&graph_n, kGraphUnroll, split ? kGraphUnroll - kKeepSweeps : 0)) return rc;
                if (split && front >= kGraphUnroll) { if (int rc = need(&graph_n_lean, kGraphUnroll, kGraphUnroll)) return rc; }
                hipGraphExec_t four = split ? graph_n_lean : graph_n;
                for (; front >= kGraphUnroll; front -= kGraphUnroll) HIPCHK(hipGraphLaunch(four, stream));
            }
            for (; front > 0; front--) HIPCHK(hipGraphLaunch(one, stream));
            if (unroll) HIPCHK(hipGraphLaunch(graph_n, stream));
            else for (int i = 0; i < tail; i++) HIPCHK(hipGraphLaunch(graph, stream));
        } else {
            for (int i = 0; i < sweeps; i++) launch_sweep(stream, -1, 0, -1, split && i + kKeepSweeps < sweeps);
        }
        HIPCHK(hipGetLastError());
        return 0;
    }
    // `sweeps` sweeps, kernel by kernel, an event after every launch; phase_ms[ph*stride + first_sweep + i] = duration of phase ph of sweep i, FIVE rows:
    // 0 backward pass, 1 forward pass (linear sweep + rollouts), 2 line search, 3 next-iteration setup, 4 the linear forward sweep's own kernel alone (a part of row 1:
    // the reference's sweepTime[], DDPWrappers.cuh:77; 0 on paths whose rollout kernel sweeps itself)
    std::vector<hipEvent_t> trace_ev;             // grow-only, released with the handle
    int need_events(size_t n) { while (trace_ev.size() < n) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); trace_ev.push_back(e); } return 0; }
    int iterate_traced(int sweeps, double* phase_ms, int first_sweep, int stride) override {
        if (sweeps > 0) note_sweeps_enqueued();
        if (int erc = need_events(6 * (size_t)sweeps)) return erc;
        static const int phase_of[5] = {PDDP_PHASE_BP, PDDP_PHASE_FP, PDDP_PHASE_FP, PDDP_PHASE_LS, PDDP_PHASE_NIS};
        const bool own_sweep = !plan.maps_in_rollouts;                                  // (otherwise the rollout kernel begins with it: row 4 stays 0)
        const int part_of[5] = {-1, 0, own_sweep ? 1 : -1, -1, -1};
        for (int i = 0; i < sweeps; i++) {
            const bool lean = split_sweeps() && i + kKeepSweeps < sweeps;                   // (pddp_iterate's schedule)
            HIPCHK(hipEventRecord(trace_ev[6 * i], stream));
            for (int k = 0; k < 5; k++) { if (k != 1 || own_sweep) launch_sweep(stream, phase_of[k], 0, part_of[k], lean); HIPCHK(hipEventRecord(trace_ev[6 * i + k + 1], stream)); }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        for (int i = 0; i < sweeps; i++) {
            if (first_sweep + i >= stride) continue;
            float ms[5];
            for (int k = 0; k < 5; k++) HIPCHK(hipEventElapsedTime(&ms[k], trace_ev[6 * i + k], trace_ev[6 * i + k + 1]));
            if (!own_sweep) ms[1] = 0.f;
            const size_t o = (size_t)first_sweep + i;
            phase_ms[0 * (size_t)stride + o] = ms[0]; phase_ms[1 * (size_t)stride + o] = (double)ms[1] + ms[2]; phase_ms[2 * (size_t)stride + o] = ms[3];
            phase_ms[3 * (size_t)stride + o] = ms[4]; phase_ms[4 * (size_t)stride + o] = ms[1];
        }
        return 0;
    }
    int sync() override { HIPCHK(hipStreamSynchronize(stream)); return 0; }
    // runiLQR_MPC_GPU (MPCHelpers.cuh:864-1045) for the batch
    int set_cost(double Q1, double Q2, double R, double QF1, double QF2) override {
        HIPCHK(hipStreamSynchronize(stream));
        cfg.Q1 = Q1; cfg.Q2 = Q2; cfg.R = R; cfg.QF1 = QF1; cfg.QF2 = QF2;
        cw = cost_weights_of<T, P::PLANT>(cfg);
        drop_graph();                                                // the weights are kernel arguments baked into the captured sweep
        return fill_cost_table();
    }
    int set_cost_ee(const double* v) override {
        if (!cfg.ee_cost) return fail(PDDP_EINVAL, "pddp_set_cost_ee: the handle was not created with ee_cost = 1");
        HIPCHK(hipStreamSynchronize(stream));
        cfg.Q_EE1 = v[0]; cfg.Q_EE2 = v[1]; cfg.QF_EE1 = v[2]; cfg.QF_EE2 = v[3]; cfg.R_EE = v[4]; cfg.Q_xEE = v[5]; cfg.QF_xEE = v[6]; cfg.Q_xdEE = v[7]; cfg.QF_xdEE = v[8];
        cw = cost_weights_of<T, P::PLANT>(cfg);
        drop_graph();
        return fill_cost_table();
    }
    // ---- per-problem cost weights (cost_table.hpp, plants.hpp cost_weights_at): pddp_set_cost_problems / pddp_get_cost_problems
    // The table exists from the first pddp_set_cost_problems on; until then b.cwt is null and every kernel takes the handle-wide record from its arguments, as it always did.
    // Its creation changes which kernels a sweep launches (the matrix-core backward pass and the thread-lane kernels have instantiations of their own) and a kernel
    // argument, so the captured graph goes ONCE; afterwards the graph holds the pointer and a call only writes rows, on the stream, behind what is enqueued there.
    DeviceBuf d_cwt;
    T* cwt_rows() const { return d_cwt.template as<T>(); }
    std::vector<T> cwt_stage;                      // host rows of the call in flight (the call waits for the stream before it returns)
    int cost_record_size() const override { return P::PLANT == 4 && !P::kPluginCost ? cost_record_len(cfg.ee_cost) : 0; }
    // The three ways rows of `rec` numbers travel between cwt_stage and the table; each waits for the stream before it returns.
    // rows i of cwt_stage -> rows idx[i] of the table (to_device) or the reverse: contiguous runs of slots in one transfer each; rows that are not named keep their values
    int cwt_move_rows(int count, const int* idx, int rec, bool to_device) {
        hipError_t e = hipSuccess;
        for_each_slot_run(count, idx, [&](int first, int len) {
            T* h = cwt_stage.data() + (size_t)first * rec; T* d = cwt_rows() + (size_t)idx[first] * rec;
            if (e == hipSuccess) e = to_device ? hipMemcpyAsync(d, h, (size_t)len * rec * sizeof(T), hipMemcpyHostToDevice, stream) : hipMemcpyAsync(h, d, (size_t)len * rec * sizeof(T), hipMemcpyDeviceToHost, stream);
        });
        if (e != hipSuccess) return fail(PDDP_ENODEVICE, std::string("cost table: transfer of rows failed: ") + hipGetErrorString(e));
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    int cwt_upload_rows(int count, const int* idx, int rec) { return cwt_move_rows(count, idx, rec, true); }
    int cwt_download_rows(int count, const int* idx, int rec) { return cwt_move_rows(count, idx, rec, false); }
    // every one of the table's `rows` rows <- `record` (not a part of cwt_stage)
    int cwt_fill_rows(int rows, int rec, const T* record) {
        cwt_stage.resize((size_t)rows * rec);
        for (int i = 0; i < rows; i++) std::memcpy(cwt_stage.data() + (size_t)i * rec, record, rec * sizeof(T));
        HIPCHK(hipMemcpyAsync(cwt_rows(), cwt_stage.data(), cwt_stage.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    // every row <- the handle-wide record (a table that exists: pddp_set_cost / pddp_set_cost_ee after per-problem weights; the last call wins)
    int fill_cost_table() {
        if (!d_cwt.ptr || kDiagCost) return 0;                      // (plants 1-3: the table holds diagonal records, which pddp_set_cost has no part in -- the call is as inert there as it always was)
        T row[kCostRecEe];                                          // (the longer of the two records)
        cost_record_of<T>(cw, row);
        return cwt_fill_rows(cfg.batch, cost_record_len(cfg.ee_cost), row);
    }
    // numbers per row of the table: the arm's record of its cost family, or the diagonal record of the pendulum, cart-pole and quadrotor
    int table_record_len() const { return kDiagCost ? kDiagRec : cost_record_len(cfg.ee_cost); }
    int ensure_cost_table(int rows) { return reserve(d_cwt, (size_t)rows * table_record_len() * sizeof(T), "hipMalloc failed for the per-problem cost weights"); }
    int set_cost_problems(int count, const int* idx, const double* w) override {
        const int rec = cost_record_len(cfg.ee_cost);
        if (!d_cwt.ptr) {
            if (int rc = ensure_cost_table(cfg.batch)) return rc;
            if (int rc = fill_cost_table()) return rc;                 // (waits for the stream: nothing in flight reads the old argument set)
            b.cwt = cwt_rows();
            drop_graph();
        }
        cwt_stage.resize((size_t)count * rec);
        cost_records_pack<T>(count, rec, w, cwt_stage.data());
        return cwt_upload_rows(count, idx, rec);
    }
    int get_cost_problems(int count, const int* idx, double* w) override {
        const int rec = cost_record_len(cfg.ee_cost);
        cwt_stage.resize((size_t)count * rec);
        if (d_cwt.ptr) { if (int rc = cwt_download_rows(count, idx, rec)) return rc; }
        else for (int i = 0; i < count; i++) cost_record_of<T>(cw, cwt_stage.data() + (size_t)i * rec);
        for (size_t e = 0; e < (size_t)count * rec; e++) w[e] = (double)cwt_stage[e];
        return 0;
    }
    // ---- run-time diagonal cost weights of the pendulum, cart-pole and quadrotor (diag_cost_table.hpp, plants.hpp DiagTab): pddp_set_diag_cost* / pddp_get_diag_cost_problems
    // The same table machinery (d_cwt, b.cwt, the intake fetch) with rows of 2 NX + NU numbers.  Without a table every launch below is the one it always was; with one,
    // every kernel that reads a weight runs in its DiagTab instantiation (with_cost_plant), which takes problem pb's weights from row pb.
    static constexpr bool kDiagCost = P::PLANT >= 1 && P::PLANT <= 3;
    static constexpr int kDiagRec = 2 * NX + NU;
    int diag_cost_size() const override { return kDiagCost ? kDiagRec : 0; }
    // f(plant policy): DiagTab<P, T> for a handle with a table of diagonal records, P otherwise (the arm's per-problem weights are a run-time branch inside its kernels)
    // and GoalTab<P, T> for one that also has a table of goal trajectories (the kernels that evaluate the cost or its gradient: they read the goal)
    template <typename F> void with_cost_plant(F&& f) {
        if constexpr (kDiagCost) {
            if (b.gtab) { f(GoalTab<P, T>{}); return; }
            if (b.cwt) { f(DiagTab<P, T>{}); return; }
        }
        f(P{});
    }
    // the same for the kernels that only take the running knots' Hessian from the weights (k_bp_mq, k_bp_cl): they read no goal, so a goal table changes nothing for them
    template <typename F> void with_weight_plant(F&& f) {
        if constexpr (kDiagCost) { if (b.cwt) { f(DiagTab<P, T>{}); return; } }
        f(P{});
    }
    // the kernels that integrate (rollouts, setup, warm start): StepTab<P, T> for a handle with a table of per-problem time steps (it always has the other two tables),
    // with_cost_plant's choice otherwise -- a handle without the table launches the instantiations it always launched
    template <typename F> void with_step_plant(F&& f) {
        if constexpr (kDiagCost) { if (b.dtab) { f(StepTab<P, T>{}); return; } }
        with_cost_plant(f);
    }
    // the kernels that form the control term of the cost (rollouts, setup): RefTab<P, T> for a handle with a table of control references (it always has the other
    // three tables), with_step_plant's choice otherwise; with_ref_cost_plant: the same for the initial cost, which integrates nothing and falls through to with_cost_plant
    template <typename F> void with_ref_plant(F&& f) {
        if constexpr (kDiagCost) { if (b.utab) { f(RefTab<P, T>{}); return; } }
        with_step_plant(f);
    }
    template <typename F> void with_ref_cost_plant(F&& f) {
        if constexpr (kDiagCost) { if (b.utab) { f(RefTab<P, T>{}); return; } }
        with_cost_plant(f);
    }
    int diag_refuse(const char* who) { return fail(PDDP_EINVAL, std::string(who) + ": diagonal cost records belong to the pendulum, cart-pole and quadrotor (plants 1-3); the arm has pddp_set_cost_problems, a plug-in plant its own cost file"); }
    // first setter call: the table, every row the built-in record; b.cwt; the captured graph goes once (other kernels, another argument)
    int ensure_diag_table() {
        if (b.cwt) return 0;                                        // (keyed on what the kernels see: a first call that failed half way is done again in full)
        if constexpr (kDiagCost) {
            T row[kDiagRec];
            if (!diag_record_builtin<P, T>(cfg.N, row)) return fail(PDDP_EINVAL, "diagonal cost records: the plant's QR(NX + j, N) differs from its Rw(N), so its control weight is not one number");
            if (int rc = ensure_cost_table(cfg.batch)) return rc;
            if (int rc = cwt_fill_rows(cfg.batch, kDiagRec, row)) return rc;      // (waits for the stream: nothing in flight reads the old argument set)
            if (fp_lds > 48 * 1024) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fp<DiagTab<P, T>, INTEG, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fp_lds));
            b.cwt = cwt_rows();
            drop_graph();
        }
        return 0;
    }
    int set_diag_cost_problems(int count, const int* idx, const double* w) override {
        if (!kDiagCost) return diag_refuse("pddp_set_diag_cost_problems");
        const std::string complaint = diag_records_complaint<T>(count, idx, w, cfg.batch, NX, NU);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_set_diag_cost_problems: " + complaint);
        if (int rc = ensure_diag_table()) return rc;
        cwt_stage.resize((size_t)count * kDiagRec);
        cost_records_pack<T>(count, kDiagRec, w, cwt_stage.data());
        return cwt_upload_rows(count, idx, kDiagRec);
    }
    int set_diag_cost(const double* w) override {
        if (!kDiagCost) return diag_refuse("pddp_set_diag_cost");
        const int zero = 0;
        const std::string complaint = diag_records_complaint<T>(1, &zero, w, cfg.batch, NX, NU);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_set_diag_cost: " + complaint);
        if (int rc = ensure_diag_table()) return rc;
        T row[kDiagRec];
        cost_records_pack<T>(1, kDiagRec, w, row);
        return cwt_fill_rows(cfg.batch, kDiagRec, row);
    }
    int get_diag_cost_problems(int count, const int* idx, double* w) override {
        if (!kDiagCost) return diag_refuse("pddp_get_diag_cost_problems");
        const std::string complaint = diag_records_complaint<T>(count, idx, w, cfg.batch, NX, NU, false);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_get_diag_cost_problems: " + complaint);
        cwt_stage.resize((size_t)count * kDiagRec);
        if (d_cwt.ptr) { if (int rc = cwt_download_rows(count, idx, kDiagRec)) return rc; }
        else if constexpr (kDiagCost) {
            for (int i = 0; i < count; i++) diag_record_builtin<P, T>(cfg.N, cwt_stage.data() + (size_t)i * kDiagRec);
        }
        for (size_t e = 0; e < (size_t)count * kDiagRec; e++) w[e] = (double)cwt_stage[e];
        return 0;
    }
    // ---- per-knot goal trajectories of the same plants (goal_traj_table.hpp, plants.hpp GoalTab): pddp_set_goal_trajectory_problems / pddp_get_... / pddp_clear_...
    // A table [batch][N][NX] and a flag per problem, from the first setter call on; b.gtab / b.gflag are what the kernels see.  With them every kernel that evaluates the
    // cost or its gradient runs in its GoalTab instantiation (with_cost_plant); a flagged problem's knot k reads row k of its block, an unflagged one xGoal.  A handle with
    // goal trajectories always has the table of diagonal records too (GoalTab is layered on DiagTab), created through ensure_diag_table with the built-in rows.
    DeviceBuf d_gtab, d_gflag;
    T* gtab_rows() const { return d_gtab.template as<T>(); }
    int* gflag_rows() const { return d_gflag.template as<int>(); }
    std::vector<T> gt_stage;                       // host rows of the getter call in flight
    std::vector<int> gf_stage;                     // host flags of the call in flight
    size_t goal_len() const { return (size_t)cfg.N * NX; }
    int goal_trajectory_size() const override { return kDiagCost ? (int)goal_len() : 0; }
    int goal_refuse(const char* who) { return fail(PDDP_EINVAL, std::string(who) + ": goal trajectories belong to the pendulum, cart-pole and quadrotor (plants 1-3)"); }
    // room for `rows` problems, flags cleared; the kernels do not see it yet
    int reserve_goal_table(int rows) {
        if (int rc = reserve(d_gtab, (size_t)rows * goal_len() * sizeof(T), "hipMalloc failed for the goal trajectories")) return rc;
        if (int rc = reserve(d_gflag, (size_t)rows * sizeof(int), "hipMalloc failed for the goal trajectories' flags")) return rc;
        HIPCHK(hipMemsetAsync(d_gtab.ptr, 0, (size_t)rows * goal_len() * sizeof(T), stream));
        HIPCHK(hipMemsetAsync(d_gflag.ptr, 0, (size_t)rows * sizeof(int), stream));
        return 0;
    }
    // first setter call: the cost table if there is none, the goal table, no problem flagged; b.gtab / b.gflag; the captured graph goes once (other kernels, other arguments)
    int ensure_goal_table() {
        if (b.gtab) return 0;
        if constexpr (kDiagCost) {
            if (int rc = ensure_diag_table()) return rc;
            if (int rc = reserve_goal_table(cfg.batch)) return rc;
            HIPCHK(hipStreamSynchronize(stream));                   // (nothing in flight reads the old argument set)
            if (fp_lds > 48 * 1024) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fp<GoalTab<P, T>, INTEG, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fp_lds));
            b.gtab = gtab_rows(); b.gflag = gflag_rows();
            drop_graph();
        }
        return 0;
    }
    // flag `on` for the named problems, on the stream (gf_stage stays alive until the caller has waited for it)
    int goal_flags_upload(int count, const int* idx, int on) {
        gf_stage.assign((size_t)count, on);
        hipError_t e = hipSuccess;
        for_each_slot_run(count, idx, [&](int first, int len) {
            if (e == hipSuccess) e = hipMemcpyAsync(gflag_rows() + idx[first], gf_stage.data() + first, (size_t)len * sizeof(int), hipMemcpyHostToDevice, stream);
        });
        return e == hipSuccess ? 0 : fail(PDDP_ENODEVICE, std::string("goal trajectories: transfer of flags failed: ") + hipGetErrorString(e));
    }
    int set_goal_trajectory_problems(int count, const int* idx, const void* Gv) override {
        if (!kDiagCost) return goal_refuse("pddp_set_goal_trajectory_problems");
        const T* G = static_cast<const T*>(Gv);
        const std::string complaint = goal_rows_complaint<T>(count, idx, G, cfg.batch, cfg.N, NX);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_set_goal_trajectory_problems: " + complaint);
        if (int rc = ensure_goal_table()) return rc;
        if (int rc = goal_path_drop(count, idx)) return rc;         // (a named problem with a goal path becomes one with a plain trajectory)
        const size_t len = goal_len();
        hipError_t e = hipSuccess;
        for_each_slot_run(count, idx, [&](int first, int run) {     // contiguous runs of slots in one transfer each; problems that are not named keep theirs
            if (e == hipSuccess) e = hipMemcpyAsync(gtab_rows() + (size_t)idx[first] * len, G + (size_t)first * len, (size_t)run * len * sizeof(T), hipMemcpyHostToDevice, stream);
        });
        if (e != hipSuccess) { hipStreamSynchronize(stream); return fail(PDDP_ENODEVICE, std::string("pddp_set_goal_trajectory_problems: transfer of rows failed: ") + hipGetErrorString(e)); }
        const int rc = goal_flags_upload(count, idx, 1);
        HIPCHK(hipStreamSynchronize(stream));
        return rc;
    }
    int clear_goal_trajectory_problems(int count, const int* idx) override {
        if (!kDiagCost) return goal_refuse("pddp_clear_goal_trajectory_problems");
        const std::string complaint = goal_rows_complaint<T>(count, idx, nullptr, cfg.batch, cfg.N, NX, false);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_clear_goal_trajectory_problems: " + complaint);
        if (!b.gtab) return 0;                                      // never had a trajectory: every problem reads xGoal already
        if (int rc = goal_path_drop(count, idx)) return rc;         // (a goal path goes with its window)
        const int rc = goal_flags_upload(count, idx, 0);
        HIPCHK(hipStreamSynchronize(stream));
        return rc;
    }
    int get_goal_trajectory_problems(int count, const int* idx, void* Gv, int* has) override {
        if (!kDiagCost) return goal_refuse("pddp_get_goal_trajectory_problems");
        T* G = static_cast<T*>(Gv);
        const std::string complaint = goal_rows_complaint<T>(count, idx, G, cfg.batch, cfg.N, NX, true, false);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_get_goal_trajectory_problems: " + complaint);
        const size_t len = goal_len();
        gt_stage.resize((size_t)count * NX);                        // the named problems' xGoal
        gf_stage.assign((size_t)count, 0);
        hipError_t e = hipSuccess;
        for_each_slot_run(count, idx, [&](int first, int run) {
            if (e == hipSuccess) e = hipMemcpyAsync(gt_stage.data() + (size_t)first * NX, b.xGoal + (size_t)idx[first] * NX, (size_t)run * NX * sizeof(T), hipMemcpyDeviceToHost, stream);
            if (b.gtab) {
                if (e == hipSuccess) e = hipMemcpyAsync(G + (size_t)first * len, gtab_rows() + (size_t)idx[first] * len, (size_t)run * len * sizeof(T), hipMemcpyDeviceToHost, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(gf_stage.data() + first, gflag_rows() + idx[first], (size_t)run * sizeof(int), hipMemcpyDeviceToHost, stream);
            }
        });
        const hipError_t es = hipStreamSynchronize(stream);
        if (e != hipSuccess || es != hipSuccess) return fail(PDDP_ENODEVICE, std::string("pddp_get_goal_trajectory_problems: transfer failed: ") + hipGetErrorString(e != hipSuccess ? e : es));
        for (int i = 0; i < count; i++) {
            if (!gf_stage[i]) goal_rows_from_xgoal<T>(gt_stage.data() + (size_t)i * NX, cfg.N, NX, G + (size_t)i * len);      // no trajectory: what the cost reads, xGoal at every knot
            if (has) has[i] = gf_stage[i] ? 1 : 0;
        }
        return 0;
    }
    // ---- per-problem horizon times of the same plants (horizon_time_table.hpp, plants.hpp StepTab): pddp_set_horizon_time_problems / pddp_get_horizon_time_problems
    // A table [batch] of time steps from the first setter call on; b.dtab is what the kernels see.  With it every kernel that integrates runs in its StepTab instantiation
    // (with_step_plant) and takes problem pb's step from entry pb; `dt`, the handle-wide step, stays the argument of every launch (and the step of pddp_plant_eval and
    // pddp_simulate, which have no problem index).  A handle with a step table always has the goal table and the table of diagonal records too (StepTab is layered on
    // GoalTab), created through ensure_goal_table: no problem flagged, the built-in rows.  The host keeps the times as they were given (ht_host).
    DeviceBuf d_dtab;
    T* dtab_rows() const { return d_dtab.template as<T>(); }
    std::vector<double> ht_host;                   // [batch] horizon times in seconds as given; cfg.total_time for a problem no call has named
    std::vector<T> ht_stage;                       // host steps of the call in flight (the call waits for the stream before it returns)
    int horizon_refuse(const char* who) { return fail(PDDP_EINVAL, std::string(who) + ": per-problem horizon times belong to the pendulum, cart-pole and quadrotor (plants 1-3)"); }
    // first setter call: the goal table and the cost table if there are none, the step table with the handle-wide step in every entry; b.dtab; the captured graph goes
    // once (other kernels).  Everything of the step table is released again if a step fails.  What ensure_goal_table() created before that step stays: a failed
    // allocation or transfer here (PDDP_ENOMEM / PDDP_ENODEVICE, never PDDP_EINVAL -- the arguments were checked before) leaves the handle with the goal table and the
    // cost table of a first pddp_set_goal_trajectory_problems call (no problem flagged, built-in rows, the graph dropped), which compute what it computed without them
    // (tests/test_goal_trajectory.py, tests/test_diag_costs.py), and with no step table; the call can be repeated.
    int ensure_step_table() {
        if (b.dtab) return 0;
        if constexpr (kDiagCost) {
            if (int rc = ensure_goal_table()) return rc;
            if (int rc = reserve(d_dtab, (size_t)cfg.batch * sizeof(T), "hipMalloc failed for the per-problem time steps")) return rc;
            ht_stage.assign((size_t)cfg.batch, time_step<T>(cfg));
            hipError_t e = hipMemcpyAsync(d_dtab.ptr, ht_stage.data(), (size_t)cfg.batch * sizeof(T), hipMemcpyHostToDevice, stream);
            const hipError_t es = hipStreamSynchronize(stream);     // (nothing in flight reads the old argument set)
            if (e == hipSuccess) e = es;
            if (e == hipSuccess && fp_lds > 48 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fp<StepTab<P, T>, INTEG, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fp_lds);
            if (e != hipSuccess) { d_dtab.release(); return fail(PDDP_ENODEVICE, std::string("per-problem time steps: creating the table failed: ") + hipGetErrorString(e)); }
            ht_host.assign((size_t)cfg.batch, cfg.total_time);
            b.dtab = dtab_rows();
            drop_graph();
        }
        return 0;
    }
    int set_horizon_time_problems(int count, const int* idx, const double* total_time) override {
        if (!kDiagCost) return horizon_refuse("pddp_set_horizon_time_problems");
        const std::string complaint = horizon_times_complaint<T>(count, idx, total_time, cfg.batch, cfg.N);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_set_horizon_time_problems: " + complaint);
        if (int rc = ensure_step_table()) return rc;
        ht_stage.resize((size_t)count);
        for (int i = 0; i < count; i++) ht_stage[i] = horizon_time_step<T>(total_time[i], cfg.N);
        hipError_t e = hipSuccess;
        for_each_slot_run(count, idx, [&](int first, int run) {     // contiguous runs of slots in one transfer each; problems that are not named keep theirs
            if (e == hipSuccess) e = hipMemcpyAsync(dtab_rows() + idx[first], ht_stage.data() + first, (size_t)run * sizeof(T), hipMemcpyHostToDevice, stream);
        });
        const hipError_t es = hipStreamSynchronize(stream);
        if (e != hipSuccess || es != hipSuccess) return fail(PDDP_ENODEVICE, std::string("pddp_set_horizon_time_problems: transfer of entries failed: ") + hipGetErrorString(e != hipSuccess ? e : es));
        for (int i = 0; i < count; i++) ht_host[idx[i]] = total_time[i];
        return 0;
    }
    int get_horizon_time_problems(int count, const int* idx, double* total_time, double* step) override {
        if (!kDiagCost) return horizon_refuse("pddp_get_horizon_time_problems");
        const std::string complaint = horizon_times_complaint<T>(count, idx, nullptr, cfg.batch, cfg.N, false);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_get_horizon_time_problems: " + complaint);
        if (total_time) for (int i = 0; i < count; i++) total_time[i] = b.dtab ? ht_host[idx[i]] : cfg.total_time;
        if (!step) return 0;
        ht_stage.assign((size_t)count, time_step<T>(cfg));          // (no table: the handle-wide step)
        if (b.dtab) {
            hipError_t e = hipSuccess;
            for_each_slot_run(count, idx, [&](int first, int run) {
                if (e == hipSuccess) e = hipMemcpyAsync(ht_stage.data() + first, dtab_rows() + idx[first], (size_t)run * sizeof(T), hipMemcpyDeviceToHost, stream);
            });
            const hipError_t es = hipStreamSynchronize(stream);
            if (e != hipSuccess || es != hipSuccess) return fail(PDDP_ENODEVICE, std::string("pddp_get_horizon_time_problems: transfer failed: ") + hipGetErrorString(e != hipSuccess ? e : es));
        }
        for (int i = 0; i < count; i++) step[i] = (double)ht_stage[i];
        return 0;
    }
    // ---- control references of the same plants (control_ref_table.hpp, plants.hpp RefTab): pddp_set_control_reference_problems / pddp_get_... / pddp_clear_...
    // A table [batch][N][NU] behind its zero row and a flag per problem, from the first setter call on; b.utab / b.uflag are what the kernels see.  With them every kernel
    // that forms the control term of the cost or of its gradient runs in its RefTab instantiation (with_ref_plant, with_ref_cost_plant); a flagged problem's running knot k
    // reads row k of its block, an unflagged one the zero row.  A handle with a reference table always has the step, goal and cost tables too (RefTab is layered on
    // StepTab), created through ensure_step_table: default entries, no problem flagged, the built-in rows.
    DeviceBuf d_utab, d_uflag;
    T* utab_rows() const { return d_utab.template as<T>() + control_ref_pad<T>(NU); }      // (behind the zero row)
    int* uflag_rows() const { return d_uflag.template as<int>(); }
    std::vector<int> uf_stage;                     // host flags of the call in flight
    size_t ref_len() const { return (size_t)cfg.N * NU; }
    int control_reference_size() const override { return kDiagCost ? (int)ref_len() : 0; }
    int ref_refuse(const char* who) { return fail(PDDP_EINVAL, std::string(who) + ": control references belong to the pendulum, cart-pole and quadrotor (plants 1-3)"); }
    // room for `rows` problems: the zero row, the blocks and the flags all cleared; the kernels do not see it yet
    int reserve_ref_table(int rows) {
        const size_t bytes = control_ref_table_elems<T>(rows, cfg.N, NU) * sizeof(T);
        if (int rc = reserve(d_utab, bytes, "hipMalloc failed for the control references")) return rc;
        if (int rc = reserve(d_uflag, (size_t)rows * sizeof(int), "hipMalloc failed for the control references' flags")) return rc;
        hipError_t e = hipMemsetAsync(d_utab.ptr, 0, bytes, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_uflag.ptr, 0, (size_t)rows * sizeof(int), stream);
        return e == hipSuccess ? 0 : fail(PDDP_ENODEVICE, std::string("control references: clearing the table failed: ") + hipGetErrorString(e));
    }
    // first setter call: the step, goal and cost tables if there are none, the reference table, no problem flagged; b.utab / b.uflag; the captured graph goes once (other
    // kernels).  Everything of the reference table is released again if a step fails; what ensure_step_table() created before that step stays, by the rule written there: a
    // failed allocation or transfer here (PDDP_ENOMEM / PDDP_ENODEVICE) leaves the handle with the tables of a first pddp_set_horizon_time_problems call at their defaults,
    // which compute what it computed without them, and with no reference table; the call can be repeated.
    int ensure_ref_table() {
        if (b.utab) return 0;
        if constexpr (kDiagCost) {
            if (int rc = ensure_step_table()) return rc;
            if (int rc = reserve_ref_table(cfg.batch)) { d_utab.release(); d_uflag.release(); return rc; }
            hipError_t e = hipStreamSynchronize(stream);            // (nothing in flight reads the old argument set)
            if (e == hipSuccess && fp_lds > 48 * 1024) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fp<RefTab<P, T>, INTEG, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fp_lds);
            if (e != hipSuccess) { d_utab.release(); d_uflag.release(); return fail(PDDP_ENODEVICE, std::string("control references: creating the table failed: ") + hipGetErrorString(e)); }
            b.utab = utab_rows(); b.uflag = uflag_rows();
            drop_graph();
        }
        return 0;
    }
    // flag `on` for the named problems, on the stream (uf_stage stays alive until the caller has waited for it)
    int ref_flags_upload(int count, const int* idx, int on) {
        uf_stage.assign((size_t)count, on);
        hipError_t e = hipSuccess;
        for_each_slot_run(count, idx, [&](int first, int len) {
            if (e == hipSuccess) e = hipMemcpyAsync(uflag_rows() + idx[first], uf_stage.data() + first, (size_t)len * sizeof(int), hipMemcpyHostToDevice, stream);
        });
        return e == hipSuccess ? 0 : fail(PDDP_ENODEVICE, std::string("control references: transfer of flags failed: ") + hipGetErrorString(e));
    }
    int set_control_reference_problems(int count, const int* idx, const void* Uv) override {
        if (!kDiagCost) return ref_refuse("pddp_set_control_reference_problems");
        const T* U = static_cast<const T*>(Uv);
        const std::string complaint = control_rows_complaint<T>(count, idx, U, cfg.batch, cfg.N, NU);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_set_control_reference_problems: " + complaint);
        if (int rc = ensure_ref_table()) return rc;
        const size_t len = ref_len();
        hipError_t e = hipSuccess;
        for_each_slot_run(count, idx, [&](int first, int run) {     // contiguous runs of slots in one transfer each; problems that are not named keep theirs
            if (e == hipSuccess) e = hipMemcpyAsync(utab_rows() + (size_t)idx[first] * len, U + (size_t)first * len, (size_t)run * len * sizeof(T), hipMemcpyHostToDevice, stream);
        });
        if (e != hipSuccess) { hipStreamSynchronize(stream); return fail(PDDP_ENODEVICE, std::string("pddp_set_control_reference_problems: transfer of rows failed: ") + hipGetErrorString(e)); }
        const int rc = ref_flags_upload(count, idx, 1);
        HIPCHK(hipStreamSynchronize(stream));
        return rc;
    }
    int clear_control_reference_problems(int count, const int* idx) override {
        if (!kDiagCost) return ref_refuse("pddp_clear_control_reference_problems");
        const std::string complaint = control_rows_complaint<T>(count, idx, nullptr, cfg.batch, cfg.N, NU, false);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_clear_control_reference_problems: " + complaint);
        if (!b.utab) return 0;                                      // never had a reference: every control term is taken on u already
        const int rc = ref_flags_upload(count, idx, 0);
        HIPCHK(hipStreamSynchronize(stream));
        return rc;
    }
    int get_control_reference_problems(int count, const int* idx, void* Uv, int* has) override {
        if (!kDiagCost) return ref_refuse("pddp_get_control_reference_problems");
        T* U = static_cast<T*>(Uv);
        const std::string complaint = control_rows_complaint<T>(count, idx, U, cfg.batch, cfg.N, NU, true, false);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_get_control_reference_problems: " + complaint);
        const size_t len = ref_len();
        uf_stage.assign((size_t)count, 0);
        if (b.utab) {
            hipError_t e = hipSuccess;
            for_each_slot_run(count, idx, [&](int first, int run) {
                if (e == hipSuccess) e = hipMemcpyAsync(U + (size_t)first * len, utab_rows() + (size_t)idx[first] * len, (size_t)run * len * sizeof(T), hipMemcpyDeviceToHost, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(uf_stage.data() + first, uflag_rows() + idx[first], (size_t)run * sizeof(int), hipMemcpyDeviceToHost, stream);
            });
            const hipError_t es = hipStreamSynchronize(stream);
            if (e != hipSuccess || es != hipSuccess) return fail(PDDP_ENODEVICE, std::string("pddp_get_control_reference_problems: transfer failed: ") + hipGetErrorString(e != hipSuccess ? e : es));
        }
        for (int i = 0; i < count; i++) {
            if (!uf_stage[i]) for (size_t e = 0; e < len; e++) U[(size_t)i * len + e] = T(0);      // no reference: what the control term subtracts, zero at every knot
            if (has) has[i] = uf_stage[i] ? 1 : 0;
        }
        return 0;
    }
    // ---- goal paths of the same plants (goal_path_table.hpp, k_goal_window in kernels.hpp): pddp_reserve_goal_path / pddp_set_goal_path_problems / ..._cursor_problems / pddp_get_...
    // path[batch][capacity][NX] and a record {len, mode, cursor} per problem on the device, from the reserve on.  The invariant: the block of the goal table of a
    // problem with a path holds the window at its cursor, so nothing that reads a goal knows about paths.  k_goal_window restores it wherever a cursor moves: in the
    // setter and the cursor call, and in front of every load stage of a control cycle (mpc_launch_load for the whole handle, mpc_problems for named slots), by the
    // call's shifts.  The host keeps len and mode of every problem (gp_host; the cursor lives on the device alone) and the number of problems with a path: no launch
    // and no transfer is added to a call of a handle where that number is zero.
    DeviceBuf d_gpath, d_gpmeta, d_gp_idx, d_gp_shift;
    int gp_capacity = 0;                           // rows per problem; 0: no reserve
    int gp_count = 0;                              // problems with a path
    std::vector<GoalPathRec> gp_host;              // [batch] len and mode as last written (cursor unused)
    std::vector<GoalPathRec> gp_stage;             // host records of the call in flight
    T* gpath_rows() const { return d_gpath.template as<T>(); }
    GoalPathRec* gpmeta_rows() const { return d_gpmeta.template as<GoalPathRec>(); }
    int reserve_goal_path(int capacity) override {
        if (!kDiagCost) return goal_refuse("pddp_reserve_goal_path");
        const std::string complaint = goal_path_reserve_complaint(capacity, cfg.N, gp_capacity);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_reserve_goal_path: " + complaint);
        if (gp_capacity) return 0;                                  // the same capacity again
        const size_t B = cfg.batch, per = (size_t)NX * sizeof(T);
        if ((size_t)capacity > ((size_t)-1) / (B * per)) return fail(PDDP_ENOMEM, "pddp_reserve_goal_path: batch * capacity * n elements do not fit the address space");
        const size_t bytes = B * (size_t)capacity * per;
        int rc = reserve(d_gpath, bytes, "hipMalloc failed for the goal paths");
        if (!rc) rc = reserve(d_gpmeta, B * sizeof(GoalPathRec), "hipMalloc failed for the goal paths' records");
        if (!rc) rc = reserve(d_gp_idx, B * sizeof(int), "hipMalloc failed for the goal paths' index list");
        if (!rc) rc = reserve(d_gp_shift, kSlotIntakeMax * sizeof(int), "hipMalloc failed for the goal paths' chunk shifts");
        if (!rc && (hipMemsetAsync(d_gpath.ptr, 0, bytes, stream) != hipSuccess || hipMemsetAsync(d_gpmeta.ptr, 0, B * sizeof(GoalPathRec), stream) != hipSuccess))
            rc = fail(PDDP_ENODEVICE, "pddp_reserve_goal_path: clearing the goal paths failed");
        if (!rc) rc = ensure_goal_table();                          // (the goal table and the cost table as by the first trajectory setter call: waits for the stream, drops the graph once)
        if (rc) { hipStreamSynchronize(stream); d_gpath.release(); d_gpmeta.release(); d_gp_idx.release(); d_gp_shift.release(); return rc; }
        HIPCHK(hipStreamSynchronize(stream));
        gp_host.assign(B, GoalPathRec{0, 0, 0});
        gp_count = 0; gp_capacity = capacity;
        return 0;
    }
    int goal_path_capacity() override { return kDiagCost ? gp_capacity : goal_refuse("pddp_goal_path_capacity"); }
    // gp_stage[first .. first + run) -> the records of slots idx[first] ..., one transfer per run of ascending slots
    hipError_t goal_path_records_upload(int count, const int* idx) {
        hipError_t e = hipSuccess;
        for_each_slot_run(count, idx, [&](int first, int run) {
            if (e == hipSuccess) e = hipMemcpyAsync(gpmeta_rows() + idx[first], gp_stage.data() + first, (size_t)run * sizeof(GoalPathRec), hipMemcpyHostToDevice, stream);
        });
        return e;
    }
    // the windows of the named problems at their cursors, enqueued (setter and cursor call: no shift)
    hipError_t goal_path_window_named(int count, const int* idx) {
        const hipError_t e = hipMemcpyAsync(d_gp_idx.ptr, idx, (size_t)count * sizeof(int), hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_goal_window<T>), dim3(count), dim3(256), 0, stream, (const T*)gpath_rows(), gpmeta_rows(), gtab_rows(), (const int*)d_gp_idx.template as<int>(),
                           (const int*)nullptr, count, (int)cfg.batch, (int)cfg.N, (int)NX, gp_capacity);
        return hipGetLastError();
    }
    // the windows of entries [0, n) moved on by their shifts, in front of a load stage: d_idx null: problem i, else slot d_idx[i]; d_sh: the shifts on the device
    void goal_path_advance_enqueue(int n, const int* d_idx, const int* d_sh) {
        if (gp_timing) hipEventRecord(gp_ev[0], stream);
        hipLaunchKernelGGL((k_goal_window<T>), dim3(n), dim3(256), 0, stream, (const T*)gpath_rows(), gpmeta_rows(), gtab_rows(), d_idx, d_sh, n, (int)cfg.batch, (int)cfg.N, (int)NX,
                           gp_capacity);
        if (gp_timing) { hipEventRecord(gp_ev[1], stream); gp_timed = true; }
    }
    // pddp_goal_path_profile (measurement): HIP events around the k_goal_window launch in front of a control cycle; ms: the last timed launch's stream time
    bool gp_timing = false, gp_timed = false;
    hipEvent_t gp_ev[2] = {nullptr, nullptr};
    int goal_path_profile(int on, float* ms) override {
        if (on >= 0) {
            if (on && !gp_ev[0]) for (hipEvent_t& e : gp_ev) HIPCHK(hipEventCreate(&e));
            gp_timing = on != 0;
        }
        if (ms) {
            *ms = 0.f;
            if (gp_timed) { HIPCHK(hipEventSynchronize(gp_ev[1])); HIPCHK(hipEventElapsedTime(ms, gp_ev[0], gp_ev[1])); }
        }
        return 0;
    }
    // the named problems that have a path lose it (their block of the goal table stays what it is): enqueued; nothing at all on a handle without paths
    int goal_path_drop(int count, const int* idx) {
        if (!gp_count) return 0;
        bool any = false;
        for (int i = 0; i < count; i++) any |= gp_host[idx[i]].len != 0;
        if (!any) return 0;
        gp_stage.assign((size_t)count, GoalPathRec{0, 0, 0});
        hipError_t e = hipSuccess;
        for (int i = 0; i < count && e == hipSuccess; i++)          // (only the records of problems that had a path are written)
            if (gp_host[idx[i]].len) e = hipMemcpyAsync(gpmeta_rows() + idx[i], gp_stage.data() + i, sizeof(GoalPathRec), hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) { hipStreamSynchronize(stream); return fail(PDDP_ENODEVICE, std::string("goal paths: transfer of records failed: ") + hipGetErrorString(e)); }
        for (int i = 0; i < count; i++) if (gp_host[idx[i]].len) { gp_host[idx[i]] = GoalPathRec{0, 0, 0}; gp_count--; }
        return 0;
    }
    int set_goal_path_problems(int count, const int* idx, int len, int mode, const int* cursor, const void* pv) override {
        if (!kDiagCost) return goal_refuse("pddp_set_goal_path_problems");
        if (!gp_capacity) return fail(PDDP_EINVAL, "pddp_set_goal_path_problems: the handle has no goal path storage (pddp_reserve_goal_path)");
        const T* path = static_cast<const T*>(pv);
        const std::string complaint = goal_path_set_complaint<T>(count, idx, len, mode, cursor, path, cfg.batch, gp_capacity, NX);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_set_goal_path_problems: " + complaint);
        const size_t per = (size_t)len * NX, slot = (size_t)gp_capacity * NX;
        hipError_t e = hipSuccess;
        if (len == gp_capacity) {                                   // full blocks: runs of ascending slots are contiguous on both sides
            for_each_slot_run(count, idx, [&](int first, int run) {
                if (e == hipSuccess) e = hipMemcpyAsync(gpath_rows() + (size_t)idx[first] * slot, path + (size_t)first * per, (size_t)run * per * sizeof(T), hipMemcpyHostToDevice, stream);
            });
        } else {
            for (int i = 0; i < count && e == hipSuccess; i++)
                e = hipMemcpyAsync(gpath_rows() + (size_t)idx[i] * slot, path + (size_t)i * per, per * sizeof(T), hipMemcpyHostToDevice, stream);
        }
        gp_stage.resize((size_t)count);
        for (int i = 0; i < count; i++) gp_stage[i] = GoalPathRec{len, mode, cursor ? cursor[i] : 0};
        if (e == hipSuccess) e = goal_path_records_upload(count, idx);
        if (e != hipSuccess) { hipStreamSynchronize(stream); return fail(PDDP_ENODEVICE, std::string("pddp_set_goal_path_problems: transfer failed: ") + hipGetErrorString(e)); }
        int rc = goal_flags_upload(count, idx, 1);
        if (!rc && (e = goal_path_window_named(count, idx)) != hipSuccess) rc = fail(PDDP_ENODEVICE, std::string("pddp_set_goal_path_problems: the window kernel failed: ") + hipGetErrorString(e));
        for (int i = 0; i < count; i++) { if (!gp_host[idx[i]].len) gp_count++; gp_host[idx[i]] = GoalPathRec{len, mode, 0}; }      // (the records are on their way whatever follows)
        HIPCHK(hipStreamSynchronize(stream));
        return rc;
    }
    int set_goal_path_cursor_problems(int count, const int* idx, const int* cursor) override {
        if (!kDiagCost) return goal_refuse("pddp_set_goal_path_cursor_problems");
        if (!gp_capacity) return fail(PDDP_EINVAL, "pddp_set_goal_path_cursor_problems: the handle has no goal path storage (pddp_reserve_goal_path)");
        const std::string complaint = goal_path_cursor_complaint(count, idx, cursor, gp_host.data(), cfg.batch);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_set_goal_path_cursor_problems: " + complaint);
        gp_stage.resize((size_t)count);
        for (int i = 0; i < count; i++) gp_stage[i] = GoalPathRec{gp_host[idx[i]].len, gp_host[idx[i]].mode, cursor[i]};
        hipError_t e = goal_path_records_upload(count, idx);
        if (e == hipSuccess) e = goal_path_window_named(count, idx);
        const hipError_t es = hipStreamSynchronize(stream);
        if (e != hipSuccess || es != hipSuccess) return fail(PDDP_ENODEVICE, std::string("pddp_set_goal_path_cursor_problems: failed on the device: ") + hipGetErrorString(e != hipSuccess ? e : es));
        return 0;
    }
    int get_goal_path_problems(int count, const int* idx, int* len, int* mode, int* cursor, void* pv) override {
        if (!kDiagCost) return goal_refuse("pddp_get_goal_path_problems");
        if (!gp_capacity) return fail(PDDP_EINVAL, "pddp_get_goal_path_problems: the handle has no goal path storage (pddp_reserve_goal_path)");
        const std::string complaint = slots_complaint(count, idx, cfg.batch);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_get_goal_path_problems: " + complaint);
        T* path = static_cast<T*>(pv);
        const size_t slot = (size_t)gp_capacity * NX;
        gp_stage.assign((size_t)count, GoalPathRec{0, 0, 0});
        hipError_t e = hipSuccess;
        for_each_slot_run(count, idx, [&](int first, int run) {
            if (e == hipSuccess) e = hipMemcpyAsync(gp_stage.data() + first, gpmeta_rows() + idx[first], (size_t)run * sizeof(GoalPathRec), hipMemcpyDeviceToHost, stream);
            if (path && e == hipSuccess) e = hipMemcpyAsync(path + (size_t)first * slot, gpath_rows() + (size_t)idx[first] * slot, (size_t)run * slot * sizeof(T), hipMemcpyDeviceToHost, stream);
        });
        const hipError_t es = hipStreamSynchronize(stream);
        if (e != hipSuccess || es != hipSuccess) return fail(PDDP_ENODEVICE, std::string("pddp_get_goal_path_problems: transfer failed: ") + hipGetErrorString(e != hipSuccess ? e : es));
        for (int i = 0; i < count; i++) {
            const GoalPathRec& r = gp_stage[i];
            if (len) len[i] = r.len;
            if (mode) mode[i] = r.mode;
            if (cursor) cursor[i] = r.cursor;
            if (path) for (size_t k = (size_t)r.len * NX; k < slot; k++) path[(size_t)i * slot + k] = T(0);      // rows >= len: what an earlier, longer path left there is not part of this one
        }
        return 0;
    }
    // The load stage of a control cycle, enqueued: argument checks, pinned staging, the single input transfer and the k_mpc_load launch.  pddp_mpc_solve goes on
    // from here with the sweeps; pddp_mpc_load (teacher-forcing hook) waits for the stream and returns, so that what k_mpc_load leaves can be read before a sweep
    // overwrites it.  ONE place selects between the 512-thread pipeline (V = 0 / 1) and the 256-thread kernel.
    int mpc_enqueue_load(const char* who, const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout) {
        const size_t B = cfg.batch, N = cfg.N;
        for (size_t i = 0; i < B; i++) if (shift[i] < 0 || shift[i] >= (int)N - 1) return fail(PDDP_EINVAL, std::string(who) + ": shift must be in [0, N-2]");
        if (int rc = mpc_admit(who, clear_vars)) return rc;
        return mpc_launch_load(xActual, xGoal, shift, clear_vars, full_rollout);
    }
    // what a warm start means for the handle as a whole (the named-slot calls take it on the handle, their cycles run on its intake area).  whole = false: the call
    // clears or shifts the named slots only, so clear_vars = 1 there does not lift the refusal -- the other slots' interior cost-to-go is as stale as before; it stays in
    // force until pddp_mpc_solve / pddp_mpc_load clears every slot.
    int mpc_admit(const char* who, int clear_vars, bool whole = true) {
        if (lean_ctg_ran && !clear_vars)
            return fail(PDDP_EINVAL, std::string(who) + ": this handle iterated with boundary_cost_to_go_only = 1, so its interior cost-to-go slots are stale and a warm start "
                                     "(clear_vars = 0) would shift them into the block boundaries; call with clear_vars = 1 once, or create the handle without that option" +
                                     (whole ? "" : " (named slots: clear_vars = 1 clears the named slots only and is accepted, but the refusal stays in force for every slot "
                                                   "until pddp_mpc_solve or pddp_mpc_load with clear_vars = 1 has cleared the whole handle)"));
        if (whole) lean_ctg_ran = false;
        if (!mpc_used) { mpc_used = true; drop_graph(); }
        return 0;
    }
    size_t cap_batch = 0;      // problems the handle's buffers were allocated for (an intake area's cfg.batch is the chunk in flight, <= this)
    // inputs of cfg.batch problems -> device, then the k_mpc_load launch.  from: the previous solutions are read from slots d_idx[i] of another handle's buffers
    // (k_mpc_load_slots: an intake area loading named slots of its handle); the kernel form is selected the same way for both.
    int mpc_launch_load(const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout, const Buffers<T>* from = nullptr,
                        const int* d_idx = nullptr, int from_batch = 0) {
        const size_t B = cfg.batch, Bc = cap_batch;
        // one pinned staging area: pageable host memory would make every small transfer of the cycle a synchronous staging copy of its own.  It holds the input run,
        // then the result records (mpc_record.hpp) that overwrite it after the solve
        const MpcInputRun in = mpc_input_run(sizeof(T), NX, B);
        const size_t out_bytes = Bc * mpc_record_of<T>(NX, NU, cfg.N, (size_t)cfg.max_iter + 2).bytes, in_bytes = mpc_input_run(sizeof(T), NX, Bc).bytes;
        if (int rc = reserve(h_stage, out_bytes > in_bytes ? out_bytes : in_bytes, "hipHostMalloc failed for the staging area of the MPC call")) return rc;
        unsigned char* h = h_stage.as<unsigned char>();
        std::memcpy(h + in.x, xActual, in.x_bytes); std::memcpy(h + in.goal, xGoal, in.x_bytes); std::memcpy(h + in.shift, shift, in.shift_bytes);
        if (B == Bc) HIPCHK(hipMemcpyAsync(d_xActual, h, in.bytes, hipMemcpyHostToDevice, stream));   // the load kernel moves goals / shifts where the sweeps read them
        else {                                                  // a chunk smaller than the intake area: the three runs lie apart on the device
            HIPCHK(hipMemcpyAsync(d_xActual, h + in.x, in.x_bytes, hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemcpyAsync(d_goal_in, h + in.goal, in.x_bytes, hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemcpyAsync(d_shift, h + in.shift, in.shift_bytes, hipMemcpyHostToDevice, stream));
        }
        if (gp_count) goal_path_advance_enqueue((int)B, nullptr, d_shift);      // goal paths: cursors on by the shifts, the new windows in the goal table before anything reads a goal
        if constexpr (P::PLANT == 4 && INTEG == 1 && sizeof(T) == 4) {                // float arm with a built-in robot model: the warm-start rollout split over two waves
            if (plan.mpc_split_roll) {
                if (tl_variant == 0) launch_mpc_load<0>(clear_vars, full_rollout, from, d_idx, from_batch);
                else launch_mpc_load<1>(clear_vars, full_rollout, from, d_idx, from_batch);
                return 0;
            }
        }
        launch_mpc_load<-1>(clear_vars, full_rollout, from, d_idx, from_batch);
        return 0;
    }
    // k_mpc_load, or with `from` its slots form, in the form V: the 512-thread pipeline of built-in robot model V = 0 / 1, or (V = -1) the 256-thread kernel
    template <int V> void launch_mpc_load(int clear_vars, int full_rollout, const Buffers<T>* from, const int* d_idx, int from_batch) {
        const dim3 grid(cfg.batch), block(V < 0 ? 256 : 512);
        const int tsm = (cfg.ee_cost && cfg.ee_cost_shift) ? 1 : 0;
        if constexpr (kDiagCost) {
            if (b.dtab) {            // per-problem time steps: the warm-start rollout in its StepTab instantiation (the kernel reads no cost: P itself on every other handle)
                using Q = StepTab<P, T>;
                if (from) hipLaunchKernelGGL((k_mpc_load_slots<Q, INTEG, T, V>), grid, block, 0, stream, b, mb, *from, d_idx, from_batch, dm, dt, d_xActual, d_shift, clear_vars, full_rollout, d_goal_in, tsm);
                else hipLaunchKernelGGL((k_mpc_load<Q, INTEG, T, V>), grid, block, 0, stream, b, mb, dm, dt, d_xActual, d_shift, clear_vars, full_rollout, d_goal_in, tsm);
                return;
            }
        }
        if (from) hipLaunchKernelGGL((k_mpc_load_slots<P, INTEG, T, V>), grid, block, 0, stream, b, mb, *from, d_idx, from_batch, dm, dt, d_xActual, d_shift, clear_vars, full_rollout, d_goal_in, tsm);
        else hipLaunchKernelGGL((k_mpc_load<P, INTEG, T, V>), grid, block, 0, stream, b, mb, dm, dt, d_xActual, d_shift, clear_vars, full_rollout, d_goal_in, tsm);
    }
    int mpc_load(const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout) override {
        if (int rc = mpc_enqueue_load("mpc_load", xActual, xGoal, shift, clear_vars, full_rollout)) return rc;
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    int mpc_solve(const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout, int ifd, int max_iter, double budget_ms,
                  int poll_every, void* x, void* u, void* KT, void* Jout, int* alphaOut, int* success, int* iters) override {
        if (max_iter < 1 || max_iter > cfg.max_iter) return fail(PDDP_EINVAL, "mpc_solve: max_iter must be in [1, config.max_iter]");
        const double t0 = now_ms();
        if (int rc = mpc_enqueue_load("mpc_solve", xActual, xGoal, shift, clear_vars, full_rollout)) return rc;
        return mpc_cycle(t0, ifd, max_iter, budget_ms, poll_every, x, u, KT, Jout, alphaOut, success, iters, [] {});
    }
    // A control cycle behind its load stage, for the cfg.batch problems of this handle (pddp_mpc_solve: the whole handle; pddp_mpc_solve_problems: a chunk of named slots
    // on the intake area): initial cost and setup with alphaIndex kept, the iLQR loop under this call's iteration limit and time budget (t0: the start of the call),
    // fall-back and result records.  after_store() runs behind every k_mpc_store launch, before the wait: what the caller enqueues there rides the same synchronisation.
    template <typename AfterStore>
    int mpc_cycle(double t0, int ifd, int max_iter, double budget_ms, int poll_every, void* x, void* u, void* KT, void* Jout, int* alphaOut, int* success, int* iters,
                  AfterStore&& after_store) {
        const size_t B = cfg.batch;
        const MpcRecord rec = mpc_record_of<T>(NX, NU, cfg.N, (size_t)cfg.max_iter + 2);
        struct Restore { int& v; const int saved; ~Restore() { v = saved; } } limit{sp.max_iter, sp.max_iter};      // this call's iteration limit, until the function returns
        sp.max_iter = max_iter;                                  // acceptRejectTrajGPU(..., max_iter)
        launch_init_cost_and_setup(stream, ifd, 0, 1);
        HIPCHK(hipGetLastError());
        int rc = 0;
        const int chunk = poll_every > 0 ? poll_every : 4;
        bool all_exited = false;
        if (budget_ms <= 0 && chunk >= max_iter) {
            // no time budget and the whole iteration limit in one chunk: every problem is done after max_iter sweeps whatever happens (the limit forces the exit), so
            // nothing has to be polled -- sweeps, fall-back kernel and ALL result transfers are enqueued back to back and the cycle synchronises once
            if ((rc = iterate(max_iter))) return rc;
            // k_mpc_store also packs every problem's results into one device run of records: ONE transfer back instead of six
            if (!d_mpc_out) { int arc = alloc("mpc_out", &d_mpc_out, cap_batch * rec.bytes); if (arc) return arc; }
            hipLaunchKernelGGL((k_mpc_store<P, T>), dim3(B), dim3(256), 0, stream, b, mb, dm, 1, d_mpc_out, rec);
            HIPCHK(hipGetLastError());
            after_store();
            HIPCHK(hipMemcpyAsync(h_stage.ptr, d_mpc_out, B * rec.bytes, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            hstate.resize(B);
            all_exited = true;
            for (size_t pb = 0; pb < B; pb++) {
                mpc_record_unpack<T>(rec, h_stage.as<unsigned char>() + pb * rec.bytes, pb, hstate.data(), (T*)x, (T*)u, (T*)KT, (T*)Jout, alphaOut);
                all_exited &= (hstate[pb].done != 0);
            }
        }
        // (after the single synchronisation too: a sweep whose backward pass failed raises rho and repeats without advancing `iter` (backwardPassGPU's retry loop,
        // bpHelpers.cuh:497-511): such a problem is still running after max_iter sweeps -- go on in the polled loop, like the reference would)
        if (!all_exited) {
            std::vector<int> done(B);
            bool fresh = false;
            for (int guard = 0; guard < 100000; guard++) {
                if (budget_ms > 0 && now_ms() - t0 > budget_ms) break;   // time_budget (MPCHelpers.cuh:919,941,1001): checked between chunks of sweeps
                fresh = false;
                if ((rc = iterate(chunk))) break;
                if ((rc = status(done.data(), nullptr))) break;
                fresh = true;                                            // hstate reflects everything enqueued so far
                bool all = true;
                for (int v : done) all &= (v != 0);
                if (all) break;
            }
            if (rc) return rc;
            hipLaunchKernelGGL((k_mpc_store<P, T>), dim3(B), dim3(64), 0, stream, b, mb, dm, 0, (unsigned char*)nullptr, MpcRecord{});   // copies only: the states status() fetched above stay valid
            HIPCHK(hipGetLastError());
            after_store();
            if ((rc = store_impl(x, u, KT, Jout, alphaOut, nullptr, fresh))) return rc;
        }
        for (size_t i = 0; i < B; i++) { if (success) success[i] = hstate[i].took_step; if (iters) iters[i] = hstate[i].iter; }
        return 0;
    }
    std::vector<SolverState<T>> hstate;      // the solver states as last fetched by status()
    int status(int* done, int* iters) override {
        hstate.resize(cfg.batch);
        const size_t bytes = cfg.batch * sizeof(SolverState<T>);
        if (int rc = reserve(h_state, cap_batch * sizeof(SolverState<T>), "hipHostMalloc failed for the solver states")) return rc;   // pinned: the poll is one asynchronous copy + one wait
        HIPCHK(hipMemcpyAsync(h_state.ptr, b.state, bytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        std::memcpy(hstate.data(), h_state.ptr, bytes);
        for (int i = 0; i < cfg.batch; i++) { if (done) done[i] = hstate[i].done; if (iters) iters[i] = hstate[i].iter; }
        return 0;
    }
    int store(void* x, void* u, void* KT, void* Jout, int* alphaOut, void* dmax) override { return store_impl(x, u, KT, Jout, alphaOut, dmax, false); }
    // state_is_current: hstate was fetched after the last kernel that changes `cur` / `alphaIndex` (saves a round trip in the MPC cycle)
    int store_impl(void* x, void* u, void* KT, void* Jout, int* alphaOut, void* dmax, bool state_is_current) {
        const size_t B = cfg.batch, N = cfg.N;
        if (!state_is_current) {
            hstate.resize(B);
            HIPCHK(hipMemcpyAsync(hstate.data(), b.state, B * sizeof(SolverState<T>), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        const std::vector<SolverState<T>>& st = hstate;
        for (size_t pb = 0; pb < B; pb++) {
            if (x) HIPCHK(hipMemcpyAsync((T*)x + pb * N * NX, b.xb + (pb * 2 + st[pb].cur) * N * NX, N * NX * sizeof(T), hipMemcpyDeviceToHost, stream));
            if (dmax) HIPCHK(hipMemcpyAsync((T*)dmax + pb, b.dmax + pb * cfg.A + st[pb].alphaIndex, sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        if (u) HIPCHK(hipMemcpyAsync(u, b.ucur, B * N * NU * sizeof(T), hipMemcpyDeviceToHost, stream));
        if (KT) HIPCHK(hipMemcpyAsync(KT, b.KT, B * N * NX * NU * sizeof(T), hipMemcpyDeviceToHost, stream));
        if (Jout) HIPCHK(hipMemcpyAsync(Jout, b.Jout, B * (cfg.max_iter + 2) * sizeof(T), hipMemcpyDeviceToHost, stream));
        if (alphaOut) HIPCHK(hipMemcpyAsync(alphaOut, b.alphaOut, B * (cfg.max_iter + 2) * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    // ---- individual slots of a loaded handle between sweeps: pddp_load_problems / pddp_store_problems (slots.hpp)
    // The intake area: a second Solver of the same type for min(batch, kSlotIntakeMax) problems on this handle's stream, with this handle's RESOLVED kernel selection
    // (adopt_selection: the choices init() derives from the batch size are the handle's, not those of a 256-problem handle), created at the first refill.  load() of the
    // intake is the handle's own init path -- the same kernel families, the same bits.  Control cycles of named slots run sweeps on the same area (mpc_problems below), so
    // a refill does not rely on what the area holds: load_problems clears the solver states and the Jout / alphaOut rows of its chunk first.
    Solver* intake = nullptr;
    const Solver* intake_of = nullptr;             // set on the intake itself: the handle it serves
    DeviceBuf d_slot_idx;                        // [kSlotIntakeMax] the slot indices of the chunk in flight
    int* slot_idx() const { return d_slot_idx.as<int>(); }
    DeviceBuf d_slot_stage;                        // pddp_store_problems: the packed rows of one chunk
    void adopt_selection(const Solver& o) { plan = o.plan; tl_variant = o.tl_variant; tl_grav = o.tl_grav; }
    int slot_chunk() const { return cfg.batch < kSlotIntakeMax ? cfg.batch : kSlotIntakeMax; }
    int ensure_slot_idx() { return reserve(d_slot_idx, kSlotIntakeMax * sizeof(int), "hipMalloc failed for the slot indices"); }
    int ensure_intake() {
        // the arrays that exist only on some kernel families must exist on both sides (pddp_set_array("model_*") can move a handle to another family)
        if (intake && ((intake->b.xw != nullptr) != (b.xw != nullptr) || intake->b.xw_rec != b.xw_rec || (intake->b.ABc != nullptr) < (b.ABc != nullptr) ||
                       (intake->b.Hc != nullptr) < (b.Hc != nullptr) || intake->plan.fp_path != plan.fp_path)) {
            HIPCHK(hipStreamSynchronize(stream));
            delete intake; intake = nullptr;
        }
        if (!intake) {
            Solver* in = new Solver();
            in->cfg = cfg; in->cfg.batch = slot_chunk(); in->cfg.use_graph = 0; in->intake_of = this;
            if (int rc = in->init()) { delete in; return rc; }
            intake = in;
        }
        Solver& in = *intake;
        in.adopt_selection(*this);
        in.cw = cw; in.sp = sp; in.dt = dt; in.b.model = b.model; in.h_overridden = h_overridden;
        if (b.cwt && !in.b.cwt) {                                    // per-problem cost weights: the intake area gets a table of its own, filled per chunk from the slots' rows (load_problems)
            if (int rc = in.ensure_cost_table(slot_chunk())) return rc;
            in.b.cwt = in.cwt_rows();
        }
        if (b.gtab && !in.b.gtab) {                                  // goal trajectories: the same, rows and flags of the chunk's slots
            if (int rc = in.reserve_goal_table(slot_chunk())) return rc;
            in.b.gtab = in.gtab_rows(); in.b.gflag = in.gflag_rows();
        }
        if (b.dtab && !in.b.dtab) {                                  // per-problem time steps: the same, one entry per slot of the chunk
            if (int rc = in.reserve(in.d_dtab, (size_t)slot_chunk() * sizeof(T), "hipMalloc failed for the intake area's time steps")) return rc;
            in.b.dtab = in.dtab_rows();
        }
        if (b.utab && !in.b.utab) {                                  // control references: the same, blocks and flags of the chunk's slots behind the intake's own zero row
            if (int rc = in.reserve_ref_table(slot_chunk())) { in.d_utab.release(); in.d_uflag.release(); return rc; }      // (no half-made table stays behind, as in ensure_ref_table)
            in.b.utab = in.utab_rows(); in.b.uflag = in.uflag_rows();
        }
        if (!b.ABc) { in.b.ABc = nullptr; in.b.Hc = nullptr; }      // the handle left the compact layouts (ab_keep_reference_layout): so does its intake
        return ensure_slot_idx();
    }
    // what a refill moves (copy) or clears (zero) per slot; DESIGN.md "refilling slots" lists the bytes
    bool refill_table(SlotTable& t) {
        const Buffers<T>& ib = intake->b;
        const size_t N = cfg.N, M = cfg.M, A = cfg.A, out = (size_t)cfg.max_iter + 2, e = sizeof(T);
        t.n = 0; t.N = cfg.N; t.state = nullptr; t.state_stride = t.off_cur = t.off_alpha = 0;
        bool ok = true;
        auto copy = [&](const void* c, void* s, size_t cstride, size_t sstride, size_t bytes) { ok = ok && slot_add(t, c, s, cstride, sstride, bytes, kSlotCopy); };
        auto same = [&](const void* c, void* s, size_t bytes) { copy(c, s, bytes, bytes, bytes); };
        auto zero = [&](void* s, size_t bytes) { ok = ok && slot_add(t, nullptr, s, 0, bytes, bytes, kSlotZero); };
        copy(ib.xb, b.xb, 2 * N * NX * e, 2 * N * NX * e, N * NX * e);            // half 0: the fresh state's cur
        same(ib.ucur, b.ucur, N * NU * e); same(ib.xGoal, b.xGoal, NX * e);
        same(ib.state, b.state, sizeof(SolverState<T>));
        same(ib.Jout, b.Jout, out * e); same(ib.alphaOut, b.alphaOut, out * sizeof(int));      // (the intake's rows are zero behind element 0: load_problems clears them in front of the init path, which writes element 0)
        if (b.ABc) ok = ok && slot_add_abc(t, ib.ABc, b.ABc, cfg.N, e); else same(ib.AB, b.AB, N * NX * NM * e);
        same(ib.H, b.H, N * NM * NM * e); same(ib.g, b.g, N * NM * e);
        if (b.Hc) same(ib.Hc, b.Hc, N * 49 * e);
        same(ib.costk, b.costk, N * e);
        zero(b.P, N * NX * NX * e); zero(b.Pp, N * NX * NX * e); zero(b.p, N * NX * e); zero(b.pp, N * NX * e);
        zero(b.KT, N * NX * NU * e); zero(b.dcur, N * NX * e); zero(b.du, N * NU * e);
        zero(b.err, M * sizeof(int)); zero(b.dmax, A * e); zero(b.tshift, sizeof(int));
        return ok;
    }
    int load_problems(int count, const int* idx, const void* x0, const void* u0, const void* xg, int ignore_first_defect) override {
        if (int rc = ensure_intake()) return rc;
        Solver& in = *intake;
        SlotTable tab, fetch;
        if (!refill_table(tab)) return fail(PDDP_EINVAL, "pddp_load_problems: internal error (slot table)");
        fetch.n = 0; fetch.N = cfg.N; fetch.state = nullptr; fetch.state_stride = fetch.off_cur = fetch.off_alpha = 0;
        if (cfg.ee_cost) slot_add(fetch, in.b.xTarget, b.xTarget, NX * sizeof(T), NX * sizeof(T), NX * sizeof(T), kSlotCopy);      // the slots' own nominal-state targets: read by the setup kernel, not part of a load
        if (b.cwt) {                                                 // ... and their own cost weights: rows idx[c0 .. c0 + n) of the handle's table -> rows 0 .. n of the intake's
            const size_t rb = table_record_len() * sizeof(T);
            if (!slot_add(fetch, in.cwt_rows(), cwt_rows(), rb, rb, rb, kSlotCopy)) return fail(PDDP_EINVAL, "pddp_load_problems: internal error (slot table)");
        }
        if (b.gtab) {                                                // ... and their goal trajectories: block and flag of slot idx[c0 + i] -> problem i of the intake's table
            const size_t gb = goal_len() * sizeof(T);
            if (!slot_add(fetch, in.gtab_rows(), gtab_rows(), gb, gb, gb, kSlotCopy) || !slot_add(fetch, in.gflag_rows(), gflag_rows(), sizeof(int), sizeof(int), sizeof(int), kSlotCopy))
                return fail(PDDP_EINVAL, "pddp_load_problems: internal error (slot table)");
        }
        if (b.dtab) {                                                // ... and their time steps
            if (!slot_add(fetch, in.dtab_rows(), dtab_rows(), sizeof(T), sizeof(T), sizeof(T), kSlotCopy)) return fail(PDDP_EINVAL, "pddp_load_problems: internal error (slot table)");
        }
        if (b.utab) {                                                // ... and their control references: block and flag, next to the goal's
            const size_t ub = ref_len() * sizeof(T);
            if (!slot_add(fetch, in.utab_rows(), utab_rows(), ub, ub, ub, kSlotCopy) || !slot_add(fetch, in.uflag_rows(), uflag_rows(), sizeof(int), sizeof(int), sizeof(int), kSlotCopy))
                return fail(PDDP_EINVAL, "pddp_load_problems: internal error (slot table)");
        }
        const size_t N = cfg.N;
        const int C = slot_chunk();
        int rc = 0;
        for (int c0 = 0; c0 < count && !rc; c0 += C) {
            const int n = count - c0 < C ? count - c0 : C;
            in.cfg.batch = n;                                        // this chunk's view of the intake area: launches and transfers cover n problems
            if (hipMemcpyAsync(slot_idx(), idx + c0, n * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess) { rc = fail(PDDP_ENODEVICE, "pddp_load_problems: index transfer failed"); break; }
            if (fetch.n) hipLaunchKernelGGL((k_slots_scatter<T>), dim3(n, fetch.n), dim3(256), 0, stream, fetch, (const int*)slot_idx(), n, (int)cfg.batch, 1);
            // what the init path keeps or does not write, as on a fresh handle whatever ran on the intake before (a control cycle of named slots leaves some robot's
            // state and observables there): state.pw = 0, the rows of Jout / alphaOut zero behind element 0
            if (hipMemsetAsync(in.b.state, 0, (size_t)n * sizeof(SolverState<T>), stream) != hipSuccess || hipMemsetAsync(in.b.Jout, 0, (size_t)n * (cfg.max_iter + 2) * sizeof(T), stream) != hipSuccess ||
                hipMemsetAsync(in.b.alphaOut, 0, (size_t)n * (cfg.max_iter + 2) * sizeof(int), stream) != hipSuccess) { rc = fail(PDDP_ENODEVICE, "pddp_load_problems: clearing the intake area failed"); break; }
            rc = in.enqueue_load((const T*)x0 + (size_t)c0 * N * NX, (const T*)u0 + (size_t)c0 * N * NU, (const T*)xg + (size_t)c0 * NX, nullptr, nullptr, nullptr, nullptr, 0, 1,
                                 ignore_first_defect);
            if (!rc) hipLaunchKernelGGL((k_slots_scatter<T>), dim3(n, tab.n), dim3(256), 0, stream, tab, (const int*)slot_idx(), n, (int)cfg.batch, 0);
        }
        in.cfg.batch = C;
        if (rc) { hipStreamSynchronize(stream); return rc; }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    int store_problems(int count, const int* idx, void* x, void* u, void* KT, void* Jout, int* alphaOut, void* dmax) override {
        if (int rc = ensure_slot_idx()) return rc;
        const size_t N = cfg.N, out = (size_t)cfg.max_iter + 2, e = sizeof(T);
        const int C = slot_chunk();
        // one staging area per requested output, [C][row] each, 16-byte aligned
        void* host[6] = {x, u, KT, Jout, alphaOut, dmax};
        const size_t row[6] = {N * NX * e, N * NU * e, N * NX * NU * e, out * e, out * sizeof(int), e};
        size_t at[6], need = 0;
        for (int k = 0; k < 6; k++) { at[k] = need; if (host[k]) need += ((size_t)C * row[k] + 15) / 16 * 16; }
        if (!need) return 0;
        if (int rc = reserve(d_slot_stage, need, "pddp_store_problems: hipMalloc failed for the staging buffer")) return rc;
        unsigned char* const stage = d_slot_stage.as<unsigned char>();
        SlotTable t;
        t.n = 0; t.N = cfg.N; t.state = reinterpret_cast<const unsigned char*>(b.state); t.state_stride = sizeof(SolverState<T>);
        t.off_cur = offsetof(SolverState<T>, cur); t.off_alpha = offsetof(SolverState<T>, alphaIndex);
        void* src[6] = {b.xb, b.ucur, b.KT, b.Jout, b.alphaOut, b.dmax};
        const size_t sstride[6] = {2 * row[0], row[1], row[2], row[3], row[4], (size_t)cfg.A * e};
        const int op[6] = {kSlotCopyHalf, kSlotCopy, kSlotCopy, kSlotCopy, kSlotCopy, kSlotCopyAlpha};
        int which[6], nw = 0;
        for (int k = 0; k < 6; k++) if (host[k]) { if (!slot_add(t, stage + at[k], src[k], row[k], sstride[k], row[k], op[k])) return fail(PDDP_EINVAL, "pddp_store_problems: internal error (slot table)"); which[nw++] = k; }
        for (int c0 = 0; c0 < count; c0 += C) {
            const int n = count - c0 < C ? count - c0 : C;
            HIPCHK(hipMemcpyAsync(slot_idx(), idx + c0, n * sizeof(int), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL((k_slots_gather<T>), dim3(n, t.n), dim3(256), 0, stream, t, (const int*)slot_idx(), n, (int)cfg.batch);
            for (int w = 0; w < nw; w++) { const int k = which[w]; HIPCHK(hipMemcpyAsync((unsigned char*)host[k] + (size_t)c0 * row[k], stage + at[k], (size_t)n * row[k], hipMemcpyDeviceToHost, stream)); }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    // ---- control cycles of named slots: pddp_mpc_solve_problems / pddp_mpc_load_problems (DESIGN.md "control cycles of named slots")
    // The intake area is where the cycle runs: per chunk of up to slot_chunk() named slots their whole persistent state goes in (k_slots_scatter, to_compact = 1), the
    // intake runs the load stage and the cycle it would run as a handle of n problems (mpc_launch_load, mpc_cycle: the code pddp_mpc_solve runs), and every array goes
    // back to its slot (to_compact = 0).  No kernel of a sweep learns to skip problems; an unnamed slot is never an operand of anything.
    // what travels in and out per slot: mpc_slots.hpp
    bool cycle_tables(std::vector<SlotTable>& in_t, std::vector<SlotTable>& out_t) {
        const Solver& in = *intake;
        const bool gt = b.gtab != nullptr;
        const bool st = b.dtab != nullptr;
        const bool ut = b.utab != nullptr;
        const MpcSlotSide<T> is{b.cwt ? in.cwt_rows() : nullptr, in.d_xActual, in.d_goal_in, in.d_shift, gt ? in.gtab_rows() : nullptr, gt ? in.gflag_rows() : nullptr, st ? in.dtab_rows() : nullptr,
                                ut ? in.utab_rows() : nullptr, ut ? in.uflag_rows() : nullptr},
                             hs{b.cwt ? cwt_rows() : nullptr, d_xActual, d_goal_in, d_shift, gt ? gtab_rows() : nullptr, gt ? gflag_rows() : nullptr, st ? dtab_rows() : nullptr,
                                ut ? utab_rows() : nullptr, ut ? uflag_rows() : nullptr};
        return mpc_slot_tables<NX, NU, T>(in_t, out_t, in.b, in.mb, is, b, mb, hs, cfg.N, cfg.M, cfg.A, cfg.max_iter, cfg.ee_cost, table_record_len());
    }
    // pddp_mpc_slots_profile (measurement): HIP events around the in stage (movers + load kernel), the cycle and the out stage of every chunk
    bool slots_timing = false;
    hipEvent_t slots_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float slots_ms[3] = {0.f, 0.f, 0.f};
    int mpc_slots_profile(int on, float* ms3) override {
        if (on >= 0) {
            if (on && !slots_ev[0]) for (hipEvent_t& e : slots_ev) HIPCHK(hipEventCreate(&e));
            slots_timing = on != 0;
        }
        if (ms3) for (int k = 0; k < 3; k++) ms3[k] = slots_ms[k];
        return 0;
    }
    // solve = false: the load stage alone (pddp_mpc_load_problems), results left in the slots
    int mpc_problems(bool solve, int count, const int* idx, const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout, int ifd, int max_iter,
                     double budget_ms, int poll_every, void* x, void* u, void* KT, void* Jout, int* alphaOut, int* success, int* iters) {
        const double t0 = now_ms();                                  // the time budget runs from the start of the call, whatever the number of chunks
        const char* who = solve ? "pddp_mpc_solve_problems" : "pddp_mpc_load_problems";
        if (lean_ctg_ran && !clear_vars) return mpc_admit(who, clear_vars, false);      // (refused before the intake area is touched)
        if (int rc = ensure_intake()) return rc;
        if (int rc = mpc_admit(who, clear_vars, false)) return rc;
        Solver& in = *intake;
        in.mpc_used = true; in.lean_ctg_ran = false; in.bench_mode = bench_mode; in.cfg.ee_cost_shift = cfg.ee_cost_shift;
        slots_ms[0] = slots_ms[1] = slots_ms[2] = 0.f;
        std::vector<SlotTable> in_t, out_t;
        if (!cycle_tables(in_t, out_t)) return fail(PDDP_EINVAL, std::string(who) + ": internal error (slot table)");
        const size_t N = cfg.N, out = (size_t)cfg.max_iter + 2;
        const int C = slot_chunk();
        int rc = 0;
        for (int c0 = 0; c0 < count && !rc; c0 += C) {
            const int n = count - c0 < C ? count - c0 : C;
            in.cfg.batch = n;                                        // this chunk's view of the intake area, as in load_problems
            if (hipMemcpyAsync(slot_idx(), idx + c0, n * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess) { rc = fail(PDDP_ENODEVICE, std::string(who) + ": index transfer failed"); break; }
            if (slots_timing) hipEventRecord(slots_ev[0], stream);
            if (gp_count) {                                          // goal paths: the chunk's slots are windowed in the HANDLE's table by the chunk's shifts, before the movers fetch blocks and flags
                if (hipMemcpyAsync(d_gp_shift.ptr, shift + c0, n * sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess) { rc = fail(PDDP_ENODEVICE, std::string(who) + ": shift transfer failed"); break; }
                goal_path_advance_enqueue(n, slot_idx(), d_gp_shift.template as<int>());
            }
            for (const SlotTable& t : in_t) hipLaunchKernelGGL((k_slots_scatter<T>), dim3(n, t.n), dim3(256), 0, stream, t, (const int*)slot_idx(), n, (int)cfg.batch, 1);
            if ((rc = in.mpc_launch_load((const T*)xActual + (size_t)c0 * NX, (const T*)xGoal + (size_t)c0 * NX, shift + c0, clear_vars, full_rollout, &b,
                                         slot_idx(), (int)cfg.batch))) break;
            if (slots_timing) hipEventRecord(slots_ev[1], stream);
            const auto scatter_out = [&] {
                if (slots_timing) hipEventRecord(slots_ev[2], stream);
                for (const SlotTable& t : out_t) hipLaunchKernelGGL((k_slots_scatter<T>), dim3(n, t.n), dim3(256), 0, stream, t, (const int*)slot_idx(), n, (int)cfg.batch, 0);
                if (slots_timing) hipEventRecord(slots_ev[3], stream);
            };
            if (solve) {
                rc = in.mpc_cycle(t0, ifd, max_iter, budget_ms, poll_every, x ? (T*)x + (size_t)c0 * N * NX : nullptr, u ? (T*)u + (size_t)c0 * N * NU : nullptr,
                                  KT ? (T*)KT + (size_t)c0 * N * NX * NU : nullptr, Jout ? (T*)Jout + (size_t)c0 * out : nullptr, alphaOut ? alphaOut + (size_t)c0 * out : nullptr,
                                  success ? success + c0 : nullptr, iters ? iters + c0 : nullptr, scatter_out);
            } else {
                scatter_out();
                if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) rc = fail(PDDP_ENODEVICE, "pddp_mpc_load_problems: the load stage failed on the device");
            }
            if (slots_timing && !rc && hipEventSynchronize(slots_ev[3]) == hipSuccess)
                for (int k = 0; k < 3; k++) { float t = 0; if (hipEventElapsedTime(&t, slots_ev[k], slots_ev[k + 1]) == hipSuccess) slots_ms[k] += t; }
        }
        in.cfg.batch = C;
        if (rc) { hipStreamSynchronize(stream); return rc; }
        if (solve) { note_sweeps_enqueued(); note_setup_weights(); }      // the named slots hold what sweeps left: the handle's lazily rebuilt views are as stale as after pddp_mpc_solve
        HIPCHK(hipGetLastError());
        return 0;
    }
    int mpc_solve_problems(int count, const int* idx, const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout, int ifd, int max_iter,
                           double budget_ms, int poll_every, void* x, void* u, void* KT, void* Jout, int* alphaOut, int* success, int* iters) override {
        return mpc_problems(true, count, idx, xActual, xGoal, shift, clear_vars, full_rollout, ifd, max_iter, budget_ms, poll_every, x, u, KT, Jout, alphaOut, success, iters);
    }
    int mpc_load_problems(int count, const int* idx, const void* xActual, const void* xGoal, const int* shift, int clear_vars, int full_rollout) override {
        return mpc_problems(false, count, idx, xActual, xGoal, shift, clear_vars, full_rollout, 0, 1, 0.0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    int time_sweeps(int sweeps, float* ms_total, float* ms_phase) override {
        HIPCHK(hipStreamSynchronize(stream));
        if (!ms_phase) {                       // total only: the sweeps exactly as pddp_iterate enqueues them (graph replay if configured)
            int rc = need_events(2);                       // (the handle's own events: nothing to release on an error return)
            if (rc) return rc;
            HIPCHK(hipEventRecord(trace_ev[0], stream));
            if ((rc = iterate(sweeps))) return rc;
            HIPCHK(hipEventRecord(trace_ev[1], stream));
            HIPCHK(hipEventSynchronize(trace_ev[1]));
            if (ms_total) HIPCHK(hipEventElapsedTime(ms_total, trace_ev[0], trace_ev[1]));
            return 0;
        }
        // per phase: ONE pass, kernel by kernel, an event after every launch (the sweeps are not replayed a second time:
        // the state machine moves on, and later sweeps do different amounts of work)
        std::vector<double> ph(5 * (size_t)sweeps, 0.0);
        int rc = iterate_traced(sweeps, ph.data(), 0, sweeps);
        if (rc) return rc;
        double tot = 0;
        for (int k = 0; k < 4; k++) { double sum = 0; for (int i = 0; i < sweeps; i++) sum += ph[(size_t)k * sweeps + i]; ms_phase[k] = (float)sum; tot += sum; }
        if (ms_total) *ms_total = (float)tot;
        return 0;
    }
    int array(const char* name, void** ptr, size_t* bytes) override {
        auto it = arrays.find(name);
        if (it == arrays.end()) return fail(PDDP_EINVAL, std::string("unknown array ") + name);
        *ptr = it->second.first; *bytes = it->second.second;
        return 0;
    }
    int get_state(pddp_state* out) override {
        std::vector<SolverState<T>> st(cfg.batch);
        HIPCHK(hipStreamSynchronize(stream));        // the solver stream is non-blocking: order the copy after every enqueued sweep
        HIPCHK(hipMemcpy(st.data(), b.state, cfg.batch * sizeof(SolverState<T>), hipMemcpyDeviceToHost));
        for (int i = 0; i < cfg.batch; i++) to_public(st[i], out[i]);
        return 0;
    }
    int set_state(const pddp_state* in) override {
        std::vector<SolverState<T>> st(cfg.batch);
        for (int i = 0; i < cfg.batch; i++) from_public(in[i], st[i]);
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemcpy(b.state, st.data(), cfg.batch * sizeof(SolverState<T>), hipMemcpyHostToDevice));
        return 0;
    }
    int run_phase(int phase) override {
        const unsigned B = cfg.batch;
        if (std::getenv("PDDP_POISON_LDS")) {                       // debugging aid (tools/determinism_check.py): every CU's LDS holds NaNs when the phase starts -- a kernel that reads LDS it has not written shows
            static bool attr_set = false;
            if (!attr_set) { HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_poison_lds), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); attr_set = true; }
            hipLaunchKernelGGL(k_poison_lds, dim3(4096), dim3(256), 160 * 1024, stream, 160 * 256);
        }
        if (phase >= 0 && phase <= 3) {
            if (phase == PDDP_PHASE_BP) fs_vars_stale = false;     // (the hook's backward pass writes A - B K / B du itself)
            // the hook's rollouts sweep from A - B K / B du: after production sweeps that composed maps instead of writing them, rebuild them from [A B], K, du first
            if (phase == PDDP_PHASE_FP && fs_vars_stale && cfg.M > 1) { int rc = reference_views(1); if (rc) return rc; }
            launch_sweep(stream, phase, 1);                         // teacher-forcing hook: the forward pass also stores every candidate trajectory
            if (phase == PDDP_PHASE_FP) hipLaunchKernelGGL((k_reduce_parts<T>), dim3((B + 63) / 64), dim3(64), 0, stream, b, dm, (int)B);   // J / dmax readable right after the phase
        }
        else if (phase == PDDP_PHASE_BP_FUSED || phase == PDDP_PHASE_SWEEP_FUSED) {
            // the production sweep path under teacher forcing: the matrix-core backward pass composes the segment maps (and writes every cost-to-go slot, not
            // A - B K / B du); then k_sweep_maps alone -- the candidates' segment start states land in xs
            if (!plan.sweep_fused && !plan.mq_fused) return fail(PDDP_EINVAL, "PDDP_PHASE_BP_FUSED / _SWEEP_FUSED: this handle's selection has no fused sweep (matrix-core backward pass -- the KUKA arm's, or the 12-state plants' with the record rollouts --, M > 1, no kernels.sweep override)");
            if (phase == PDDP_PHASE_BP_FUSED) launch_bp(stream, 1, true);
            else launch_fp(stream, kFpHookFusedSweep);
        }
        else if (phase == PDDP_PHASE_ROLLOUT) {
            launch_fp(stream, kFpHookRollouts);
            hipLaunchKernelGGL((k_reduce_parts<T>), dim3((B + 63) / 64), dim3(64), 0, stream, b, dm, (int)B);
        }
        else if (phase == PDDP_PHASE_BP_COOP) { fs_vars_stale = false; hipLaunchKernelGGL((k_bp<P, T>), dim3(cfg.M, B), dim3(64), 0, stream, b, dm); }
        else if (phase == PDDP_PHASE_INIT_NIS) launch_nis(stream, 1);
        else if (phase == PDDP_PHASE_INIT_COST) launch_init_cost(stream, 1, 0, cfg.ee_cost ? 1 : 0, 0);
        else return fail(PDDP_EINVAL, "unknown phase");
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    // grow-only device scratch of the helper entry points below (owned by the handle: no allocation and release -- an implicit device synchronisation -- per call,
    // nothing to leak on an error return; released with the handle), never smaller than 4096 bytes
    DeviceBuf scratch_buf[3];
    int scratch(int slot, size_t bytes, void** out) {
        if (int rc = reserve(scratch_buf[slot], bytes, "hipMalloc failed for a helper's scratch buffer", 4096)) return rc;
        *out = scratch_buf[slot].ptr;
        return 0;
    }
    // ---- lock-step experiment helpers
    using PD = typename P::template Rebind<double>;
    const void* model_d = nullptr;                     // the plant's constants in double (the simulated robot runs in double); the block is one of `allocs`
    int ensure_model_d() {
        if (model_d) return 0;
        typename PD::Model hm; fill_model(hm, cfg);
        DeviceBuf blk;
        if (!blk.reserve(sizeof(hm))) return fail(PDDP_ENODEVICE, "hipMalloc failed for the simulated robot's model");
        HIPCHK(hipMemcpy(blk.ptr, &hm, sizeof(hm), hipMemcpyHostToDevice));
        model_d = blk.ptr; allocs.push_back(std::move(blk));
        return 0;
    }
    int simulate(const void* x, const void* u, const void* KT, double t0_us, double elapsed_us, int substeps, const void* goal, void* xActual,
                 double* avg_err, int* failed) override {
        if (substeps < 1 || !(elapsed_us >= 0)) return fail(PDDP_EINVAL, "pddp_simulate: substeps >= 1 and elapsed_us >= 0");
        const size_t N = cfg.N;
        if (int mrc = ensure_model_d()) return mrc;
        const size_t nx = N * NX, nu = N * NU, nk = N * NX * NU;
        T* buf = nullptr; double* dout = nullptr;
        int rc;
        if ((rc = scratch(0, (nx + nu + nk + NX + 3) * sizeof(T), (void**)&buf)) || (rc = scratch(1, 2 * sizeof(double), (void**)&dout))) return rc;
        HIPCHK(hipMemcpyAsync(buf, x, nx * sizeof(T), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(buf + nx, u, nu * sizeof(T), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(buf + nx + nu, KT, nk * sizeof(T), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(buf + nx + nu + nk, xActual, NX * sizeof(T), hipMemcpyHostToDevice, stream));
        if (goal) HIPCHK(hipMemcpyAsync(buf + nx + nu + nk + NX, goal, 3 * sizeof(T), hipMemcpyHostToDevice, stream));
        PlantSimArgs<T> a;
        a.x = buf; a.u = buf + nx; a.KT = buf + nx + nu; a.N = cfg.N; a.step_us = step_us(cfg);
        a.t0_us = t0_us; a.elapsed_us = elapsed_us; a.substeps = substeps; a.goal = goal ? buf + nx + nu + nk + NX : nullptr; a.ee_z = cfg.ee_on_link_z;
        a.xActual = buf + nx + nu + nk; a.out = dout;
        hipLaunchKernelGGL((k_plant_sim<PD, INTEG, T>), dim3(1), dim3(64), 0, stream, model_d, a);
        HIPCHK(hipGetLastError());
        double ho[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(ho, dout, sizeof(ho), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(xActual, buf + nx + nu + nk, NX * sizeof(T), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (avg_err) *avg_err = ho[0];
        if (failed) *failed = (int)ho[1];
        return 0;
    }
    // pddp_simulate_batch: the same body for every problem of the handle, one wavefront each (k_plant_sim_batch).  Its buffers are its own, grow-only and released with
    // the handle -- not the helpers' scratch slots above, not the MPC call's staging: whatever else is enqueued on the stream keeps what it owns.  Per call: one transfer
    // up (the packed per-problem records) + the three plans when they come from the host, one launch, one transfer back (state | error | failed), one synchronisation.
    DeviceBuf d_simb_buf;            // device: input records, then output records
    DeviceBuf d_simb_plan_buf;       // device: uploaded plans x | u | KT
    PinnedBuf h_simb_buf;            // pinned: the same two record areas
    int simulate_batch(const void* x, const void* u, const void* KT, const double* t0_us, const double* elapsed_us, int substeps, const void* goal, void* xActual,
                       double* avg_err, int* failed) override {
        using In = PlantSimBatchIn<PD, T>; using Out = PlantSimBatchOut<PD, T>;
        const size_t B = cfg.batch, N = cfg.N;
        if (b.dtab)                                                  // (the kernel interpolates every plan with ONE knot spacing, step_us: a refusal, not a silently wrong interpolation)
            return fail(PDDP_EINVAL, "pddp_simulate_batch: this handle has per-problem horizon times (pddp_set_horizon_time_problems), and the batched simulator takes one knot "
                                     "spacing for the whole launch; pddp_simulate_problems simulates every named slot at the spacing of its own horizon time");
        if ((x != nullptr) != (u != nullptr) || (x != nullptr) != (KT != nullptr))
            return fail(PDDP_EINVAL, "pddp_simulate_batch: x, u and KT are either all given (host plans) or all NULL (the solution the handle holds)");
        if (substeps < 1) return fail(PDDP_EINVAL, "pddp_simulate_batch: substeps >= 1");
        for (size_t i = 0; i < B; i++) if (!(elapsed_us[i] >= 0)) return fail(PDDP_EINVAL, "pddp_simulate_batch: elapsed_us[" + std::to_string(i) + "] must be >= 0");
        if (int mrc = ensure_model_d()) return mrc;
        const size_t in_bytes = (B * sizeof(In) + 15) / 16 * 16, rec_bytes = in_bytes + B * sizeof(Out);
        if (int rc = reserve(d_simb_buf, rec_bytes, "pddp_simulate_batch: hipMalloc failed for the per-problem records")) return rc;
        if (int rc = reserve(h_simb_buf, rec_bytes, "pddp_simulate_batch: hipHostMalloc failed for the per-problem records")) return rc;
        unsigned char* const d_simb = d_simb_buf.as<unsigned char>(); unsigned char* const h_simb = h_simb_buf.as<unsigned char>();
        const size_t nx = B * N * NX, nu = B * N * NU, nk = B * N * NX * NU;
        const T *px = nullptr, *pu = nullptr, *pKT = nullptr;
        if (x) {
            if (int rc = reserve(d_simb_plan_buf, (nx + nu + nk) * sizeof(T), "pddp_simulate_batch: hipMalloc failed for the uploaded plans")) return rc;
            T* const d_simb_plan = d_simb_plan_buf.as<T>();
            px = d_simb_plan; pu = px + nx; pKT = pu + nu;
            HIPCHK(hipMemcpyAsync(d_simb_plan, x, nx * sizeof(T), hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemcpyAsync(d_simb_plan + nx, u, nu * sizeof(T), hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemcpyAsync(d_simb_plan + nx + nu, KT, nk * sizeof(T), hipMemcpyHostToDevice, stream));
        }
        In* hin = reinterpret_cast<In*>(h_simb);
        for (size_t i = 0; i < B; i++) {
            In& r = hin[i];
            r.t0_us = t0_us[i]; r.elapsed_us = elapsed_us[i];
            for (int c = 0; c < 3; c++) r.goal[c] = goal ? ((const T*)goal)[3 * i + c] : T(0);
            std::memcpy(r.x, (const T*)xActual + i * NX, NX * sizeof(T));
        }
        HIPCHK(hipMemcpyAsync(d_simb, h_simb, B * sizeof(In), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL((k_plant_sim_batch<PD, INTEG, T>), dim3((unsigned)B), dim3(64), 0, stream, model_d, (const In*)d_simb, (Out*)(d_simb + in_bytes), px, pu, pKT, b,
                           (int)N, step_us(cfg), substeps, goal ? 1 : 0, cfg.ee_on_link_z);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_simb + in_bytes, d_simb + in_bytes, B * sizeof(Out), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        const Out* hout = reinterpret_cast<const Out*>(h_simb + in_bytes);
        for (size_t i = 0; i < B; i++) {
            std::memcpy((T*)xActual + i * NX, hout[i].x, NX * sizeof(T));
            if (avg_err) avg_err[i] = hout[i].out[0];
            if (failed) failed[i] = (int)hout[i].out[1];
        }
        return 0;
    }
    // pddp_simulate_problems (sim_slots.hpp): entry i is the simulated robot of slot idx[i] -- on the solution that slot holds, or on entry i of the uploaded plans --
    // with the knot spacing of the slot's own horizon time (the host mirror ht_host where the handle has a step table, cfg.total_time otherwise) and its own sub-step
    // count, both in the entry's record.  Slots are only read; an index may stand in many entries.  The same traffic as pddp_simulate_batch, sized by `count`: one
    // transfer up (+ the three plans when they come from the host), one launch -- a wavefront per entry, or a thread per entry on the closed-form plants --, one
    // transfer back, one synchronisation.  Buffers of its own, grow-only, released with the handle.
    DeviceBuf d_simp_buf;            // device: input records, then output records
    DeviceBuf d_simp_plan_buf;       // device: uploaded plans x | u | KT
    PinnedBuf h_simp_buf;            // pinned: the same two record areas
    int simulate_problems(int count, const int* idx, const void* x, const void* u, const void* KT, const double* t0_us, const double* elapsed_us, const int* substeps,
                          const void* goal, void* xActual, double* avg_err, int* failed, int family) override {
        using In = PlantSimSlotIn<PD, T>; using Out = PlantSimBatchOut<PD, T>;
        const std::string complaint = sim_slots_complaint(count, idx, x, u, KT, t0_us, elapsed_us, substeps, xActual, family, P::PLANT, cfg.batch, loaded);
        if (!complaint.empty()) return fail(PDDP_EINVAL, "pddp_simulate_problems: " + complaint);
        const int fam = sim_slots_family(family, P::PLANT, sizeof(T) == 8, count);
        if (int mrc = ensure_model_d()) return mrc;
        const size_t C = (size_t)count, N = cfg.N;
        const SimSlotsLayout lay = sim_slots_layout(C, sizeof(In), sizeof(Out));
        if (int rc = reserve(d_simp_buf, lay.rec_bytes, "pddp_simulate_problems: hipMalloc failed for the per-entry records")) return rc;
        if (int rc = reserve(h_simp_buf, lay.rec_bytes, "pddp_simulate_problems: hipHostMalloc failed for the per-entry records")) return rc;
        unsigned char* const d_rec = d_simp_buf.as<unsigned char>(); unsigned char* const h_rec = h_simp_buf.as<unsigned char>();
        const size_t nx = C * N * NX, nu = C * N * NU, nk = C * N * NX * NU;
        const T *px = nullptr, *pu = nullptr, *pKT = nullptr;
        if (x) {
            if (int rc = reserve(d_simp_plan_buf, (nx + nu + nk) * sizeof(T), "pddp_simulate_problems: hipMalloc failed for the uploaded plans")) return rc;
            T* const d_plan = d_simp_plan_buf.as<T>();
            px = d_plan; pu = px + nx; pKT = pu + nu;
            HIPCHK(hipMemcpyAsync(d_plan, x, nx * sizeof(T), hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemcpyAsync(d_plan + nx, u, nu * sizeof(T), hipMemcpyHostToDevice, stream));
            HIPCHK(hipMemcpyAsync(d_plan + nx + nu, KT, nk * sizeof(T), hipMemcpyHostToDevice, stream));
        }
        const bool tab = b.dtab != nullptr;
        const double handle_step_us = step_us(cfg);
        sim_slots_fill<In, T>(reinterpret_cast<In*>(h_rec), count, idx, t0_us, elapsed_us, substeps, (const T*)goal, (const T*)xActual, NX,
                              [&](int q) { return tab ? step_us(ht_host[(size_t)q], cfg.N) : handle_step_us; });
        HIPCHK(hipMemcpyAsync(d_rec, h_rec, C * sizeof(In), hipMemcpyHostToDevice, stream));
        const In* din = reinterpret_cast<const In*>(d_rec); Out* dout = reinterpret_cast<Out*>(d_rec + lay.in_bytes);
        bool launched = false;
        if constexpr (kDiagCost) {
            if (fam == kSimFamilyThread) {
                hipLaunchKernelGGL((k_plant_sim_ts<PD, INTEG, T>), dim3((unsigned)((C + 63) / 64)), dim3(64), 0, stream, model_d, din, dout, px, pu, pKT, b, (int)N, cfg.batch, count,
                                   goal ? 1 : 0, cfg.ee_on_link_z);
                launched = true;
            }
        }
        if (!launched)
            hipLaunchKernelGGL((k_plant_sim_slots<PD, INTEG, T>), dim3((unsigned)C), dim3(64), 0, stream, model_d, din, dout, px, pu, pKT, b, (int)N, cfg.batch, goal ? 1 : 0,
                               cfg.ee_on_link_z);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_rec + lay.in_bytes, d_rec + lay.in_bytes, C * sizeof(Out), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        const Out* hout = reinterpret_cast<const Out*>(h_rec + lay.in_bytes);
        for (size_t i = 0; i < C; i++) {
            std::memcpy((T*)xActual + i * NX, hout[i].x, NX * sizeof(T));
            if (avg_err) avg_err[i] = hout[i].out[0];
            if (failed) failed[i] = (int)hout[i].out[1];
        }
        return 0;
    }
    int ee_pos(int count, const void* x, void* out) override {
        if (P::PLANT != 4 || count <= 0) return fail(PDDP_EINVAL, "pddp_ee_pos: KUKA arm only, count >= 1");
        T *dx = nullptr, *dout = nullptr;
        int rc;
        if ((rc = scratch(0, (size_t)count * NX * sizeof(T), (void**)&dx)) || (rc = scratch(1, (size_t)count * 6 * sizeof(T), (void**)&dout))) return rc;
        HIPCHK(hipMemcpyAsync(dx, x, (size_t)count * NX * sizeof(T), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL((k_ee_pos<P, T>), dim3(count), dim3(64), 0, stream, b.model, (T)cfg.ee_on_link_z, (const T*)dx, dout);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, dout, (size_t)count * 6 * sizeof(T), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return 0;
    }
    int plant_eval(int what, int count, const void* x, const void* u, void* out) override {
        if (what < 0 || what > 9 || count <= 0 || (what >= 4 && P::PLANT != 4)) return fail(PDDP_EINVAL, "plant_eval: bad arguments");
        const size_t osz = what == 9 ? 48 : (what == 0 || what == 4 || what == 6 || what == 7 ? NP : (what == 1 || what == 5 || what == 8) ? NP * NM : what == 2 ? NX : NX * NM);
        T *dx, *du_, *dout;
        int rc;
        if ((rc = scratch(0, (size_t)count * NX * sizeof(T), (void**)&dx)) || (rc = scratch(1, (size_t)count * NU * sizeof(T), (void**)&du_)) ||
            (rc = scratch(2, (size_t)count * osz * sizeof(T), (void**)&dout))) return rc;
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemcpy(dx, x, (size_t)count * NX * sizeof(T), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(du_, u, (size_t)count * NU * sizeof(T), hipMemcpyHostToDevice));
        int grid = count < 4096 ? count : 4096;
        if (const char* g = std::getenv("PDDP_EVAL_GRID")) grid = std::atoi(g) > 0 ? std::atoi(g) : grid;   // micro-benchmarks (tools/)
        if (what >= 7) {
            if constexpr (P::PLANT == 4) {
                if (tl_variant < 0) { return fail(PDDP_EINVAL, "plant_eval: the thread-lane kernels need one of the built-in robot models"); }
                launch_plant_eval_tl<T>(stream, tl_variant, what == 9 ? (T)cfg.ee_on_link_z : tl_grav, count, dx, du_, dout, what == 9 ? 2 : what == 8 ? 1 : 0);
            }
        }
        else if (what >= 4) { if constexpr (P::PLANT == 4) hipLaunchKernelGGL((k_plant_eval_lg<T>), dim3(grid), dim3(64), 0, stream, b.model, count, dx, du_, dout, what == 5 ? 1 : (what == 6 ? 2 : 0)); }
        else hipLaunchKernelGGL((k_plant_eval<P, INTEG, T>), dim3(grid), dim3(64), 0, stream, b.model, what, count, dx, du_, dout, dt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemcpy(out, dout, (size_t)count * osz * sizeof(T), hipMemcpyDeviceToHost));
        return 0;
    }
};

template <template <typename> class PT, typename T>
static SolverBase* make_integ(int integ) {
    switch (integ) {
    case 1: return new Solver<PT<T>, 1, T>();
    case 2: return new Solver<PT<T>, 2, T>();
    case 3: return new Solver<PT<T>, 3, T>();
    }
    return nullptr;
}
template <template <typename> class PT>
static SolverBase* make_solver_of(const pddp_config& c) {
    return c.dtype == 0 ? make_integ<PT, float>(c.integrator) : c.dtype == 1 ? make_integ<PT, double>(c.integrator) : nullptr;
}
