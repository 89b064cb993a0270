// Run-time diagonal cost weights of the pendulum, cart-pole and quadrotor: pddp_set_diag_cost / pddp_set_diag_cost_problems / pddp_get_diag_cost_problems.
//
// The record of a problem is the diagonal of its cost, [ q_0..q_{NX-1} | r_0..r_{NU-1} | qf_0..qf_{NX-1} ] (2 NX + NU numbers): running knots H_k = diag(q, r),
// final knot H = diag(qf, 0).  Until the first setter call a handle has no table and its kernels take the plant's literals (plants.hpp QR / Rw / QF); the first call
// allocates the device table [batch][record] in the handle's element type, every row the built-in record, and the kernels' DiagTab instantiations read it
// (plants.hpp).  This header is the host part, plain C++, next to cost_table.hpp whose pieces it reuses: what a list of records has to satisfy, the built-in record,
// and the packing -- one rounding, here and nowhere else.  tests/native/diag_cost_host_check.cpp runs it without a GPU.
#pragma once
#include <cmath>
#include <string>

#include "cost_table.hpp"

namespace pddp {

constexpr int diag_record_len(int nx, int nu) { return 2 * nx + nu; }

// "" or the complaint about the arguments of pddp_set_diag_cost_problems (check_w) / pddp_get_diag_cost_problems (w only has to be non-null).  The weights are
// judged as the kernels will see them, rounded to the element type T: finite, none negative, every r_j > 0 (Quu = R + B' P B has to stay invertible at rho = 0);
// q and qf may be zero.
template <typename T>
inline std::string diag_records_complaint(int count, const int* idx, const double* w, int batch, int nx, int nu, bool check_w = true) {
    const int rec = diag_record_len(nx, nu);
    const std::string c = cost_records_complaint(count, idx, w, batch, rec, check_w);      // count >= 1, idx and w non-null, indices inside [0, batch) and distinct, w finite
    if (!c.empty() || !check_w) return c;
    for (size_t i = 0; i < (size_t)count * rec; i++) {
        const T v = (T)w[i];
        const int e = (int)(i % rec);
        const std::string at = "w[" + std::to_string(i / rec) + "][" + std::to_string(e) + "]";
        if (!std::isfinite(v)) return at + " is not finite in the handle's element type";
        if (v < T(0)) return at + " is negative";
        if (e >= nx && e < nx + nu && !(v > T(0))) return at + " (a control weight) must be > 0";
    }
    return "";
}

// the built-in record of plant P at horizon N, rounded once to T; false: the plant's QR(NX + j, N) is not its Rw(N), so there is no single r (the gradient takes
// Rw, the Hessian QR -- a table could not reproduce both)
template <typename P, typename T>
inline bool diag_record_builtin(int N, T* row) {
    bool one_r = true;
    for (int i = 0; i < P::NX; i++) { row[i] = (T)P::QR(i, N); row[P::NX + P::NU + i] = (T)P::QF(N); }
    for (int j = 0; j < P::NU; j++) { row[P::NX + j] = (T)P::Rw(N); one_r = one_r && P::QR(P::NX + j, N) == P::Rw(N); }
    return one_r;
}

}  // namespace pddp
