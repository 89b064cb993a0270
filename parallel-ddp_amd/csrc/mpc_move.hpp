// Data movement of the MPC warm start: the fall-back arrays of a handle and the knot shift every array of the previous solution goes through (mpc.hpp builds the load
// stage from it).  Depends on nothing but the wave scaffolding, so that tests/native/mpc_slots_host_check.cpp can replay the shift's addressing on the host.
#pragma once

#include "pddp_common.hpp"

namespace pddp {

template <typename T>
struct MpcBuffers {      // extra arrays of a handle that has been used for MPC: [B][N][.]
    T *x_old, *u_old, *KT_old;
};

// dst[k] = src[min(k + shift, DIM_N - 1)] (or 0 beyond the data when zero_fill) for k < DIM_N - 1.  dst2 (optional) receives the same values.  When
// copy_last, knot DIM_N - 1 of src is also copied to dst/dst2 (needed when dst is not src).  The array is walked as ONE flat run in ascending order in
// pieces of 8 elements per lane: a piece is read completely before it is written and only ever reads at or above what it writes, so shifting in place is
// safe -- and the loads of a piece are in flight together (one element per lane and knot at a time, as a first version did, spends one memory latency per
// knot: 0.3 ms of a 1.2 ms control cycle for the two cost-to-go arrays).
template <typename T>
PDDP_HD void mpc_shift(const Wave& w, T* dst, T* dst2, const T* src, int per_knot, int DIM_N, int shift, bool zero_fill, bool copy_last) {
    constexpr int U = 8;
    const int total = (DIM_N - 1) * per_knot, last = (DIM_N - 1) * per_knot, off = shift * per_knot;
    for (int base = 0; base < total; base += w.nlanes * U) {
        T v[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int e = base + j * w.nlanes + w.lane;
            if (e < total) {
                const int es = e + off;
                v[j] = es < last ? src[es] : (zero_fill ? T(0) : src[last + (e % per_knot)]);
            }
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int e = base + j * w.nlanes + w.lane;
            if (e < total) { dst[e] = v[j]; if (dst2) dst2[e] = v[j]; }
        }
    }
    if (copy_last) PDDP_FOR(i, per_knot) { const T val = src[last + i]; dst[last + i] = val; if (dst2) dst2[last + i] = val; }
}

}  // namespace pddp
