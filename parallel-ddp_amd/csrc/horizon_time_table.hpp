// Per-problem horizon times of the pendulum, cart-pole and quadrotor: pddp_set_horizon_time_problems / pddp_get_horizon_time_problems.
//
// Every problem of such a handle has a horizon time in seconds, cfg.total_time until a setter call names it.  What the kernels see is the problem's time STEP in the
// handle's element type, (T)(total_time / (N - 1)) -- the expression of time_step<T> (handle_setup.hpp), so that a problem given t computes the bits of a handle created
// with cfg.total_time = t.  Until the first setter call a handle has no table and every kernel takes the handle-wide step as its argument; the first call allocates the
// device table [batch] of steps, and the kernels' StepTab instantiations read it (plants.hpp problem_dt).
// This header is the host part, plain C++, next to goal_traj_table.hpp: what the arguments of the two calls have to satisfy and the conversion seconds -> step.
// tests/native/horizon_time_host_check.cpp runs it without a GPU.
#pragma once
#include <cmath>
#include <string>

#include "slots.hpp"

namespace pddp {

// the step of a problem whose horizon of N knots lasts total_time seconds, as the kernels see it
template <typename T>
inline T horizon_time_step(double total_time, int N) { return (T)(total_time / (N - 1)); }

// "" or the complaint about (count, idx, total_time): count >= 1, idx non-null, indices inside [0, batch) and distinct; with_times (the setter): total_time non-null,
// every time finite and > 0, and its step rounded to T finite and a normal positive number (a float step that underflows or overflows is refused, not stored)
template <typename T>
inline std::string horizon_times_complaint(int count, const int* idx, const double* total_time, int batch, int N, bool with_times = true) {
    const std::string c = slots_complaint(count, idx, batch);
    if (!c.empty()) return c;
    if (!with_times) return "";
    if (!total_time) return "total_time is NULL";
    for (int i = 0; i < count; i++) {
        const double t = total_time[i];
        if (!std::isfinite(t) || !(t > 0.0)) return "total_time[" + std::to_string(i) + "] must be finite and > 0";
        const T step = horizon_time_step<T>(t, N);
        if (!std::isfinite(step) || !std::isnormal(step) || !(step > T(0)))
            return "total_time[" + std::to_string(i) + "]: its step total_time / (N - 1) is not a normal positive number in the handle's element type";
    }
    return "";
}

}  // namespace pddp
