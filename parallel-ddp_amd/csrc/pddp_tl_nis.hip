// Thread-lane setup kernels of the KUKA arm (fp_tl.hpp, plant_arm_tl.hpp): k_nis_tl (one thread per knot) and k_nis_tl7 (one thread per knot and joint).  gfx950 only.
// A translation unit of its own beside pddp_tl.hip (the rollout kernels), and compiled twice -- -DPDDP_TL_NIS_ELEM=0: the float instantiations, 1: the double ones
// (undefined: both) --: k_nis_tl's instantiations are the library's longest compile by far, and the halves build side by side.
#include <hip/hip_runtime.h>

#include "ab_compact.hpp"
#include "bodies.hpp"
#include "fp_lg.hpp"
#include "tl_launch.hpp"

#ifndef PDDP_TL_NIS_ELEM
#define PDDP_TL_NIS_ELEM 2
#endif

namespace pddp {

// k_nis_tl: grid ceil(B*N / 256), block 256.  Thread = knot (global knot index g = pb*N + k).  The Jacobian of a wave's 64 knots is staged in LDS and written out in
// THREE pieces as soon as their columns are complete (arm_tl_gradient's marks: columns {4..6, 11..13} first -- the composite sweep finishes the outer joints first --,
// then {0..3, 7..10}, then the controls {14..20}): 57 staged floats per knot at most, 14.6 KB per wave, so that two workgroups (two waves per SIMD -- the kernel needs
// all 256 registers) share a compute unit.
//   CAB (b.ABc != null, the sweep's default): the piece goes to the compact [A B] (ab_compact.hpp) -- the wave's 64 knots x the piece's columns x 7 dynamic rows are ONE
//                  contiguous 16-byte aligned run of the chunk; the producer stages finished elements knot-major, so the flush is a copy with 16 bytes per lane
//                  (37 groups per lane and knot instead of 147 elements with two divisions each: ~3 k of the kernel's ~13 k instructions per knot were index arithmetic);
//                  the constant rows are not written at all;
//   !CAB:          the reference layout, whole 56-byte columns, adjacent columns of a knot by adjacent lanes (224 / 168 / 392 contiguous bytes per knot and piece).
// double handles (PDDP_FP=tl: test selection) run the same code with two waves per workgroup.  Replaces integratorGradientKern + costGradientHessianKern + memcpyCurrAKern x3 (nisInitHelpers.cuh:247-279).
constexpr int kNisTlStage = 64 * 57;

template <typename T> struct NisTlCfg { static constexpr int kWaves = sizeof(T) == 4 ? 4 : 2, kThreads = 64 * kWaves; };   // double: two waves per workgroup (58 KB of staging)
template <typename T> struct NisTlVec { typedef T v4 __attribute__((ext_vector_type(4), aligned(16))); typedef T v4p __attribute__((ext_vector_type(16 / sizeof(T)), aligned(16))); };   // v4p: one 16-byte piece
// PC: per-problem cost weights (Buffers::cwt), an instantiation of its own as in k_fp_tl; the record is read once per knot (arm_tl_nis_cost_vals / arm_tl_nis_cost_ee_knot).
template <typename T, int V, bool EE, bool CAB, bool PC = false>
__global__ __launch_bounds__(NisTlCfg<T>::kThreads, sizeof(T) == 4 ? 2 : 1) void k_nis_tl(Buffers<T> b, Dims dm, CostWeights<T> cw, T dt, T grav, int mode, int batch) {
    if constexpr (!PC) b.cwt = nullptr;
    constexpr ArmTlModel<T> md = arm_tl_builtin<T>(V);
    constexpr int NX = 14, NM = 21;
    const int g = blockIdx.x * NisTlCfg<T>::kThreads + threadIdx.x, total = batch * dm.N;
    const int pb = g / dm.N, k = g - pb * dm.N;
    __shared__ __attribute__((aligned(16))) T stage_all[NisTlCfg<T>::kWaves * kNisTlStage];
    T* stage = stage_all + (threadIdx.x >> 6) * kNisTlStage;
    const int lane = threadIdx.x & 63;
    T x[NX], u[7];
#pragma unroll
    for (int i = 0; i < NX; i++) x[i] = T(0);                    // a lane without a knot differentiates the zero state (its columns are never flushed)
#pragma unroll
    for (int i = 0; i < 7; i++) u[i] = T(0);
    bool need = false;
    if (EE) { if (g < total) need = arm_tl_nis_cost_ee<T>(md, b, dm, cw, mode, k, pb, x, u); }
    else {
        // joint-space cost: the wave's 64 gradients g_k (21 elements each, consecutive knots = 84 x 64 contiguous bytes) leave through the staging area as 16-byte pieces
        T gl[NM];
        const int r = (g < total) ? arm_tl_nis_cost_vals<T>(b, dm, cw, mode, k, pb, x, u, gl, false) : 0;
        need = (r == 3);
        constexpr int per16 = 16 / (int)sizeof(T);                        // elements per 16-byte piece
        auto run_out = [&](T* dst, const T* v, auto cnt) {               // element i of lane l -> dst[l * n + i]: through the staging area, whole pieces per lane
            constexpr int n = decltype(cnt)::value;
#pragma unroll
            for (int i = 0; i < n; i++) stage[lane * n + i] = v[i];
            wsync();
            for (int c = lane; c < 64 * n / per16; c += 64)
                *reinterpret_cast<typename NisTlVec<T>::v4p*>(dst + c * per16) = *reinterpret_cast<const typename NisTlVec<T>::v4p*>(stage + c * per16);
            wsync();
        };
        const bool adopting = (mode == 0) && r != 0;                      // (uniform per problem) the accepted state / control are in x, u and still have to go out
        if (__ballot(r != 0) == ~0ull && (dm.N & 63) == 0) {              // the wave's 64 knots belong to ONE problem and all of them moved: contiguous runs
            const size_t k0 = (size_t)(g - lane);                         // global index of the wave's first knot
            if (adopting) {
                run_out(b.xb + ((size_t)pb * 2 + b.state[pb].cur) * dm.N * NX + (size_t)(k - lane) * NX, x, std::integral_constant<int, NX>{});
                run_out(b.ucur + k0 * 7, u, std::integral_constant<int, 7>{});
            }
            if (r & 1) run_out(b.g + k0 * NM, gl, std::integral_constant<int, NM>{});
        } else if (r) {
            if (adopting) {
                tl_store14(b.xb + (((size_t)pb * 2 + b.state[pb].cur) * dm.N + k) * NX, x);
#pragma unroll
                for (int i = 0; i < 7; i++) b.ucur[(size_t)g * 7 + i] = u[i];
            }
            if (r & 1) {
                T* gk = b.g + (size_t)g * NM;
#pragma unroll
                for (int i = 0; i < NM; i++) gk[i] = gl[i];
            }
        }
    }
    const unsigned long long mask = __ballot(need);
    if (!mask) return;                                          // (uniform) nothing to differentiate in this wave
    T* AB0 = b.AB + (size_t)(g - lane) * (NX * NM);            // [A B] of the wave's first knot (reference layout)
    T* ABc0 = CAB ? b.ABc + (size_t)((g - lane) >> 6) * kAbcChunk : nullptr;   // the wave's chunk of the compact array
    constexpr bool compact = CAB;
    // Staging.  Compact: the producer leaves the FINISHED element ([A B] = I + dt dqdd) at knot * P + (column in piece) * 7 + row, P = the piece's elements per knot
    // made odd (57 / 43 / 49: conflict-free writes) -- the flush is then a copy of the piece's run, 16 bytes per lane, whose only arithmetic is the step over the
    // pad at a knot boundary.  Reference layout: raw dqdd entry-major (entry * 65 + knot), finished by the lanes that write whole columns.
    auto emit = [&](int col, int row, T val) {
        const int ent = abc_col_in_piece(col) * 7 + row;
        if (compact) stage[lane * ((abc_piece_cols(abc_piece(col)) * 7) | 1) + ent] = T(col == 7 + row ? 1 : 0) + dt * val;
        else stage[ent * 65 + lane] = val;
    };
    auto flush = [&](auto pc) {
        constexpr int piece = decltype(pc)::value;
        wsync();
        constexpr int ncols = abc_piece_cols(piece);
        if (compact) {
            constexpr int per = ncols * 7, P = per | 1, count = 64 * per;      // elements of this piece per knot / staged stride / per wave (a multiple of 4)
            T* dst = ABc0 + abc_piece_off(piece);
            int kk = (4 * lane) / per, ent = 4 * lane - kk * per;
            const bool whole = (mask == ~0ull);
            // one group of four consecutive elements, every element tested against the mask (ragged waves: knots of several problems, some of them not moving)
            auto group = [&](int e0, int kk, int ent, int limit) {
                T out[4]; bool ok[4], all = true;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const bool over = ent + j >= per;
                    const int k2 = over ? kk + 1 : kk, en = over ? ent + j - per : ent + j;
                    out[j] = stage[k2 * P + en];
                    ok[j] = e0 + j < limit && (whole || ((mask >> k2) & 1ull)); all = all && ok[j];
                }
                if (all) { typename NisTlVec<T>::v4 v; v[0] = out[0]; v[1] = out[1]; v[2] = out[2]; v[3] = out[3]; *reinterpret_cast<typename NisTlVec<T>::v4*>(dst + e0) = v; }
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++) if (ok[j]) dst[e0 + j] = out[j];
                }
            };
            // The two masks a wave of ONE problem has when it moves: every knot, or every knot but the problem's terminal one (lane 63: it has no [A B]).  Then the wave's
            // first nk knots are one dense run of nk * per elements and the flush is a copy: staged index of element e = e + (knot of e) * (P - per), so a group of four
            // is five consecutive staged words with at most one step over a knot's pad (t = elements left in the knot) -- ~20 instructions per group where the tested
            // form costs ~75 (three 32-bit multiplies and four 64-bit mask shifts per group): a quarter of the kernel's instructions were this loop.
            const int nk = whole ? 64 : (mask == (~0ull >> 1) ? 63 : 0);
            if (nk) {
                const int cnt = nk * per;
                int e0 = 4 * lane, sb = e0 + kk * (P - per), t = per - ent;
#pragma unroll 2
                for (; e0 + 3 < cnt; e0 += 256) {
                    typename NisTlVec<T>::v4 v;
                    if constexpr (P == per) { v[0] = stage[sb]; v[1] = stage[sb + 1]; v[2] = stage[sb + 2]; v[3] = stage[sb + 3]; }
                    else {
                        const T r0 = stage[sb], r1 = stage[sb + 1], r2 = stage[sb + 2], r3 = stage[sb + 3], r4 = stage[sb + 4];
                        v[0] = r0; v[1] = t > 1 ? r1 : r2; v[2] = t > 2 ? r2 : r3; v[3] = t > 3 ? r3 : r4;
                    }
                    *reinterpret_cast<typename NisTlVec<T>::v4*>(dst + e0) = v;
                    sb += 256 + (256 / per) * (P - per); t -= 256 % per; kk += 256 / per;
                    if (t <= 0) { t += per; sb += P - per; kk++; }
                }
                if (e0 < cnt) group(e0, kk, per - t, cnt);                       // the group the run ends in (nk = 63: cnt need not be a multiple of four)
            } else {
                for (int e0 = 4 * lane; e0 < count; e0 += 256) {
                    group(e0, kk, ent, count);
                    ent += 256 % per; kk += 256 / per;
                    if (ent >= per) { ent -= per; kk++; }
                }
            }
        } else {
            for (int it = 0; it * 64 < 64 * ncols; it++) {
                const int pi = it * 64 + lane, kk = pi / ncols, ci = pi - kk * ncols;
                if (kk >= 64 || !((mask >> kk) & 1ull)) continue;
                const int col = abc_piece_col(piece, ci);
                T out[NX];
#pragma unroll
                for (int r = 0; r < 7; r++) {
                    out[r] = tl_AB_const<T>(r, col, dt);
                    out[7 + r] = T(col == 7 + r ? 1 : 0) + dt * stage[(ci * 7 + r) * 65 + kk];
                }
                tl_store14(AB0 + ((size_t)kk * NM + col) * NX, out);
            }
        }
        wsync();
    };
    arm_tl_nis_jac<T>(md, grav, x, u, emit, flush);
}

// k_nis_tl7: grid (ceil(B*N / 64), 7), block 64.  Next-iteration setup of a handle with FEW problems in flight (one MPC solve: 127 knots on a 256-CU device):
// thread = (knot, joint J); blockIdx.y = J, so a wave differentiates ONE joint of 64 knots -- every thread recomputes the knot's forward dynamics and nominal inverse
// dynamics (~2.3 k instructions) and then only joint J's tangent pass (columns J, 7 + J, 14 + J of [A B]): the longest instruction stream is ~4.5 k instead of the
// ~11 k of a whole knot on one thread (k_nis_tl), on 7 x as many waves.  Joint 0's threads also adopt the accepted candidate (a copy of its x, u, d from the
// candidate-major arrays the split rollout kernel k_fp_tl2 wrote) and write the cost gradient (mode 1: the cost Hessian).  Reference layout of [A B].
// Replaces integratorGradientKern + costGradientHessianKern + memcpyCurrAKern x3 (nisInitHelpers.cuh:247-279), like k_nis_lg.
// EE: the end-effector cost family -- an eighth row of workgroups (blockIdx.y == 7) evaluates the tool point, its Jacobian, g_k and the position block of H_k
// (arm_tl_nis_cost_ee_knot), one thread per knot.
template <typename T, int V, bool EE>
__global__ __launch_bounds__(64) void k_nis_tl7(Buffers<T> b, Dims dm, CostWeights<T> cw, T dt, T grav, int mode, int batch) {
    constexpr ArmTlModel<T> md = arm_tl_builtin<T>(V);
    constexpr int NX = 14, NU = 7, NM = 21;
    const int J = blockIdx.y, g = blockIdx.x * 64 + threadIdx.x, N = dm.N;
    if (g >= batch * N) return;
    const int pb = g / N, k = g - pb * N;
    const SolverState<T>& st = b.state[pb];
    const size_t knot = (size_t)pb * N + k;
    if (!EE && J == 0) cw = cost_weights_at(b, cw, pb);                   // (per lane; the end-effector row resolves its record itself: arm_tl_nis_cost_ee_knot)
    T x[NX], u[NU];
    if (mode == 0) {
        if (!st.win_pending) return;                                      // rejected / failed backward pass: trajectory and derivatives are unchanged
        const size_t src = ((size_t)pb * dm.A + st.alphaIndex) * N + k;   // this knot in the winner's candidate slot
        tl_load14(x, b.xs + src * NX);
#pragma unroll
        for (int i = 0; i < NU; i++) u[i] = b.us[src * NU + i];
        if (J == 0) {
            tl_store14(b.xb + (((size_t)pb * 2 + st.cur) * N + k) * NX, x);
#pragma unroll
            for (int i = 0; i < NU; i++) b.ucur[knot * NU + i] = u[i];
            if (dm.M > 1 && dm.on_defect_boundary(k)) { T d[NX]; tl_load14(d, b.ds + src * NX); tl_store14(b.dcur + knot * NX, d); }
        }
        if (st.done) return;                                              // final accepted step: solution copied, no derivatives needed
    } else {
        tl_load14(x, b.xb + (((size_t)pb * 2 + st.cur) * N + k) * NX);
#pragma unroll
        for (int i = 0; i < NU; i++) u[i] = b.ucur[knot * NU + i];
    }
    const bool fin = (k == N - 1);
    if (EE) {
        if (J == 7) { arm_tl_nis_cost_ee_knot<T>(md, b, dm, cw, mode, k, pb, x, u, true); return; }
    } else if (J == 0) {
        const T w1 = fin ? cw.QF1 : cw.Q1, w2 = fin ? cw.QF2 : cw.Q2, w3 = fin ? T(0) : cw.R;   // ArmPlant::weight
        T xg[NX];
        tl_load14(xg, b.xGoal + (size_t)pb * NX);
        T* gk = b.g + knot * NM;
#pragma unroll
        for (int i = 0; i < 7; i++) { gk[i] = w1 * (x[i] - xg[i]); gk[7 + i] = w2 * (x[7 + i] - xg[7 + i]); gk[14 + i] = w3 * u[i]; }
        if (cw.limits) { const int n = fin ? NX : NM; for (int i = 0; i < n; i++) gk[i] += arm_limit_term<T>(x, u, i, 1); }                     // USE_LIMITS_FLAG (cost_arm.cuh:176-199)
        if (mode == 1) {
            T* H = b.H + knot * (NM * NM);
            for (int e = 0; e < NM * NM; e++) { const int i = e / NM, j = e % NM; H[e] = i != j ? T(0) : (i < 7 ? w1 : (i < NX ? w2 : w3)); }
        }
    }
    if (fin) return;
    ArmTlState<T> ts;
    T qdd[7];
    arm_tl_dynamics<T>(md, grav, ts, qdd, x, x + 7, u);
    T* AB = b.AB + knot * (NX * NM);
    auto emit = [&](int col, int row, T val) { AB[col * NX + 7 + row] = T(col == 7 + row ? 1 : 0) + dt * val; };
    ArmTlNominal<T> nm;
    arm_tl_grad_nominal<T>(md, grav, ts, x + 7, qdd, nm);
    switch (J) {                                                          // uniform over the wave
#define PDDP_TL7_CASE(JJ) case JJ: arm_tl_grad_joint<JJ, T>(md, ts, x + 7, qdd, nm, emit); arm_tl_grad_control<JJ, T>(ts, emit); break;
        PDDP_TL7_CASE(0) PDDP_TL7_CASE(1) PDDP_TL7_CASE(2) PDDP_TL7_CASE(3) PDDP_TL7_CASE(4) PDDP_TL7_CASE(5) PDDP_TL7_CASE(6)
#undef PDDP_TL7_CASE
    }
#pragma unroll
    for (int r = 0; r < 7; r++) {                                         // the constant rows of this thread's three columns
        AB[J * NX + r] = tl_AB_const<T>(r, J, dt); AB[(7 + J) * NX + r] = tl_AB_const<T>(r, 7 + J, dt); AB[(14 + J) * NX + r] = tl_AB_const<T>(r, 14 + J, dt);
    }
}
template <typename T>
void launch_nis_tl7(hipStream_t s, int variant, const Buffers<T>& b, const Dims& dm, const CostWeights<T>& cw, T dt, T grav, int mode, int batch) {
    const dim3 grid(((unsigned)batch * dm.N + 63) / 64, cw.ee ? 8 : 7);
    if (cw.ee) {
        if (variant == 0) hipLaunchKernelGGL((k_nis_tl7<T, 0, true>), grid, dim3(64), 0, s, b, dm, cw, dt, grav, mode, batch);
        else hipLaunchKernelGGL((k_nis_tl7<T, 1, true>), grid, dim3(64), 0, s, b, dm, cw, dt, grav, mode, batch);
    } else if (variant == 0) hipLaunchKernelGGL((k_nis_tl7<T, 0, false>), grid, dim3(64), 0, s, b, dm, cw, dt, grav, mode, batch);
    else hipLaunchKernelGGL((k_nis_tl7<T, 1, false>), grid, dim3(64), 0, s, b, dm, cw, dt, grav, mode, batch);
}
#if PDDP_TL_NIS_ELEM != 1
template void launch_nis_tl7<float>(hipStream_t, int, const Buffers<float>&, const Dims&, const CostWeights<float>&, float, float, int, int);
#endif
#if PDDP_TL_NIS_ELEM != 0
template void launch_nis_tl7<double>(hipStream_t, int, const Buffers<double>&, const Dims&, const CostWeights<double>&, double, double, int, int);     // the parity instantiation (PDDP_FP=tl4)
#endif

template <typename T>
void launch_nis_tl(hipStream_t s, int variant, const Buffers<T>& b, const Dims& dm, const CostWeights<T>& cw, T dt, T grav, int mode, int batch) {
    const unsigned knots = (unsigned)batch * dm.N, th = NisTlCfg<T>::kThreads;
    const dim3 g((knots + th - 1) / th), t(th);
    // a handle without a table of per-problem cost weights launches the instantiation it always launched, whatever T / EE / CAB; with one, the PC instantiation
#define PDDP_NIS_TL(VV, EEV) do { if (b.cwt) { if (b.ABc) hipLaunchKernelGGL((k_nis_tl<T, VV, EEV, true, true>), g, t, 0, s, b, dm, cw, dt, grav, mode, batch); \
                                                 else hipLaunchKernelGGL((k_nis_tl<T, VV, EEV, false, true>), g, t, 0, s, b, dm, cw, dt, grav, mode, batch); } \
                                  else if (b.ABc) hipLaunchKernelGGL((k_nis_tl<T, VV, EEV, true>), g, t, 0, s, b, dm, cw, dt, grav, mode, batch); \
                                  else hipLaunchKernelGGL((k_nis_tl<T, VV, EEV, false>), g, t, 0, s, b, dm, cw, dt, grav, mode, batch); } while (0)
    if (cw.ee) { if (variant == 0) PDDP_NIS_TL(0, true); else PDDP_NIS_TL(1, true); }
    else { if (variant == 0) PDDP_NIS_TL(0, false); else PDDP_NIS_TL(1, false); }
#undef PDDP_NIS_TL
}
#if PDDP_TL_NIS_ELEM != 1
template void launch_nis_tl<float>(hipStream_t, int, const Buffers<float>&, const Dims&, const CostWeights<float>&, float, float, int, int);
#endif
#if PDDP_TL_NIS_ELEM != 0
template void launch_nis_tl<double>(hipStream_t, int, const Buffers<double>&, const Dims&, const CostWeights<double>&, double, double, int, int);
#endif

}  // namespace pddp
