// What a control cycle sends and what it gets back (pddp_mpc_solve / pddp_mpc_solve_problems), as bytes: the ONE definition of both layouts.
//
//   input run      measured states [B][NX] | goals [B][NX] | shifts [B] ints -- the device array "mpc_in" and the head of the pinned staging area; one transfer where the
//                  call covers the whole array (solver_impl.hpp init, mpc_launch_load)
//   result record  [SolverState, padded to 16 bytes][x: N * NX][u: N * NU][K: N * NX * NU][Jout: out_stride][alphaOut: out_stride ints], the record padded to 16 bytes;
//                  one per problem, back to back in "mpc_out" and in the staging area.  k_mpc_store (kernels.hpp) packs through mpc_record_pack, the host unpacks
//                  through mpc_record_unpack (solver_impl.hpp mpc_cycle)
//
// Host code a kernel can call: no HIP header, no environment (tests/native/mpc_record_host_check.cpp runs all of it on exactly-sized host buffers).
#pragma once
#include <cstddef>
#include <cstring>

#include "solver_state.hpp"

namespace pddp {

struct MpcRecord {
    unsigned state, x, u, K, J, alpha, end;      // byte offsets inside one problem's record; end: behind alphaOut
    unsigned bytes;                              // from one problem's record to the next: a multiple of 16, >= end
    unsigned out_stride;                         // numbers per row of Jout / alphaOut
};
PDDP_HD MpcRecord mpc_record(size_t state_bytes, size_t elem, size_t NX, size_t NU, size_t N, size_t out_stride) {
    MpcRecord r;
    r.state = 0; r.x = (unsigned)((state_bytes + 15) / 16 * 16);
    r.u = r.x + (unsigned)(N * NX * elem); r.K = r.u + (unsigned)(N * NU * elem); r.J = r.K + (unsigned)(N * NX * NU * elem);
    r.alpha = r.J + (unsigned)(out_stride * elem); r.end = r.alpha + (unsigned)(out_stride * sizeof(int));
    r.bytes = (r.end + 15) / 16 * 16; r.out_stride = (unsigned)out_stride;
    return r;
}
template <typename T> PDDP_HD MpcRecord mpc_record_of(size_t NX, size_t NU, size_t N, size_t out_stride) { return mpc_record(sizeof(SolverState<T>), sizeof(T), NX, NU, N, out_stride); }

struct MpcInputRun {
    size_t x, goal, shift;           // byte offsets inside the run of B problems
    size_t x_bytes, shift_bytes;     // length of the measured states (and of the goals), of the shifts
    size_t bytes;                    // the contiguous transfer
    size_t elems;                    // elements "mpc_in" is allocated with (>= bytes, in whole elements, and two to spare)
};
PDDP_HD MpcInputRun mpc_input_run(size_t elem, size_t NX, size_t B) {
    MpcInputRun r;
    r.x_bytes = B * NX * elem; r.shift_bytes = B * sizeof(int);
    r.x = 0; r.goal = r.x_bytes; r.shift = 2 * r.x_bytes; r.bytes = r.shift + r.shift_bytes;
    r.elems = 2 * B * NX + B * sizeof(int) / elem + 2;
    return r;
}
template <typename U> PDDP_HD U* mpc_at(void* base, size_t byte_offset) { return reinterpret_cast<U*>(static_cast<unsigned char*>(base) + byte_offset); }

// the five arrays of one problem into its record `r`, by lane `tid` of `nt` (a workgroup; 0 of 1 on the host)
template <typename T>
PDDP_HD void mpc_record_pack(const MpcRecord& rec, unsigned char* r, int tid, int nt, const T* x, const T* u, const T* K, const T* J, const int* alpha) {
    const auto run = [&](unsigned from, unsigned to, const T* src) { for (int e = tid, n = (int)((to - from) / sizeof(T)); e < n; e += nt) mpc_at<T>(r, from)[e] = src[e]; };
    run(rec.x, rec.u, x); run(rec.u, rec.K, u); run(rec.K, rec.J, K); run(rec.J, rec.alpha, J);
    for (int e = tid; e < (int)rec.out_stride; e += nt) mpc_at<int>(r, rec.alpha)[e] = alpha[e];
}
// record `r` of problem pb into row pb of the caller's arrays (a null array is left out)
template <typename T>
inline void mpc_record_unpack(const MpcRecord& rec, const unsigned char* r, size_t pb, SolverState<T>* state, T* x, T* u, T* K, T* J, int* alpha) {
    const auto row = [&](void* dst, unsigned from, unsigned to) { if (dst) std::memcpy(static_cast<unsigned char*>(dst) + pb * (to - from), r + from, to - from); };
    std::memcpy(state + pb, r + rec.state, sizeof(SolverState<T>));
    row(x, rec.x, rec.u); row(u, rec.u, rec.K); row(K, rec.K, rec.J); row(J, rec.J, rec.alpha); row(alpha, rec.alpha, rec.end);
}

}  // namespace pddp
