// Per-knot goal trajectories of the pendulum, cart-pole and quadrotor: pddp_set_goal_trajectory_problems / pddp_get_goal_trajectory_problems /
// pddp_clear_goal_trajectory_problems.
//
// A problem either has a goal trajectory G[N][NX] in the handle's element type or has none and is pulled towards xGoal[b] at every knot.  Until the first setter call a
// handle has no table; the first call allocates the device table [batch][N][NX] and a flag per problem, and the kernels' GoalTab instantiations read them (plants.hpp).
// This header is the host part, plain C++, next to diag_cost_table.hpp: what the arguments of the three calls have to satisfy, and the block the getter answers with for
// a problem without a trajectory (its xGoal, N times).  The rows arrive in the element type, so nothing is rounded here.  tests/native/goal_traj_host_check.cpp runs it
// without a GPU.
#pragma once
#include <cmath>
#include <string>

#include "slots.hpp"

namespace pddp {

constexpr int goal_trajectory_len(int N, int nx) { return N * nx; }

// "" or the complaint about (count, idx, G): count >= 1, idx non-null, indices inside [0, batch) and distinct; with_G: G non-null (setter and getter; the clear call has
// none); check_values: every number of G finite in the element type T (setter)
template <typename T>
inline std::string goal_rows_complaint(int count, const int* idx, const T* G, int batch, int N, int nx, bool with_G = true, bool check_values = true) {
    const std::string c = slots_complaint(count, idx, batch);
    if (!c.empty()) return c;
    if (!with_G) return "";
    if (!G) return "G is NULL";
    if (check_values) {
        const size_t len = (size_t)goal_trajectory_len(N, nx);
        for (size_t i = 0; i < (size_t)count * len; i++)
            if (!std::isfinite(G[i])) return "G[" + std::to_string(i / len) + "][" + std::to_string((i % len) / nx) + "][" + std::to_string(i % nx) + "] is not finite";
    }
    return "";
}

// the getter's answer for a problem without a trajectory: what its cost reads at every knot, xGoal N times
template <typename T>
inline void goal_rows_from_xgoal(const T* xg, int N, int nx, T* rows) {
    for (int k = 0; k < N; k++) for (int i = 0; i < nx; i++) rows[(size_t)k * nx + i] = xg[i];
}

}  // namespace pddp
