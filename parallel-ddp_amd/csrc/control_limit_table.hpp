// Control limits of the pendulum, cart-pole and quadrotor: pddp_set_control_limits_problems / pddp_get_control_limits_problems / pddp_clear_control_limits_problems.
//
// A problem either has a limit row  lo_0..lo_{NU-1} | hi_0..hi_{NU-1}  -- its backward pass minimises every knot's control step over the box the row leaves around the
// current control, and every rollout clamps its control law to the row -- or has none.  -inf and +inf are legal entries: no bound on that side.  Until the first
// setter call a handle has no table; the first call allocates the device table [batch][2 NU] in the handle's element type, every row -inf.. | +inf.., which is also what
// a problem without limits holds afterwards: the kernels read a row, never a flag (plants.hpp LimTab, bp_box.hpp).  Which problems HAVE limits -- a row of infinities
// set by the caller counts -- is a host-side flag per problem, for the getter.
// This header is the host part, plain C++, next to control_ref_table.hpp: what the arguments of the three calls have to satisfy, the rounding to the element type and
// the layout.  The rows arrive as doubles.  tests/native/control_limit_host_check.cpp runs it without a GPU.
#pragma once
#include <cmath>
#include <limits>
#include <string>

#include "slots.hpp"

namespace pddp {

constexpr int control_limits_len(int nu) { return 2 * nu; }

// the row of a problem without limits, in the element type
template <typename T>
inline void control_limits_open_row(T* row, int nu) {
    for (int j = 0; j < nu; j++) { row[j] = -std::numeric_limits<T>::infinity(); row[nu + j] = std::numeric_limits<T>::infinity(); }
}

// "" or the complaint about (count, idx, lim): count >= 1, idx non-null, indices inside [0, batch) and distinct; with_lim: lim non-null (setter and getter; the clear
// call has none); check_values (setter): no NaN, and lo_j < hi_j AFTER rounding to the element type T -- a box that rounding closes has no interior for the step
template <typename T>
inline std::string control_limits_complaint(int count, const int* idx, const double* lim, int batch, int nu, bool with_lim = true, bool check_values = true) {
    const std::string c = slots_complaint(count, idx, batch);
    if (!c.empty()) return c;
    if (!with_lim) return "";
    if (!lim) return "lim is NULL";
    if (check_values) {
        const size_t len = (size_t)control_limits_len(nu);
        for (size_t i = 0; i < (size_t)count * len; i++)
            if (std::isnan(lim[i])) return "lim[" + std::to_string(i / len) + "][" + std::to_string(i % len) + "] is NaN";
        for (int i = 0; i < count; i++)
            for (int j = 0; j < nu; j++) {
                const T lo = (T)lim[(size_t)i * len + j], hi = (T)lim[(size_t)i * len + nu + j];
                if (!(lo < hi)) return "lim[" + std::to_string(i) + "]: lo_" + std::to_string(j) + " >= hi_" + std::to_string(j) + " in the handle's element type";
            }
    }
    return "";
}

// the rows as the table holds them
template <typename T>
inline void control_limits_round(T* dst, const double* lim, int count, int nu) {
    for (size_t i = 0; i < (size_t)count * control_limits_len(nu); i++) dst[i] = (T)lim[i];
}

}  // namespace pddp
