// Control references of the pendulum, cart-pole and quadrotor: pddp_set_control_reference_problems / pddp_get_control_reference_problems /
// pddp_clear_control_reference_problems.
//
// A problem either has a control reference U[N][NU] in the handle's element type -- the control term of its running knot k is then taken on u_k - U[k] -- or has none
// and pays for u_k itself, as always.  Until the first setter call a handle has no table; the first call allocates the device table [batch][N][NU] with its zero row in
// front (solver_state.hpp control_ref_pad) and a flag per problem, and the kernels' RefTab instantiations read them (plants.hpp).  Row N - 1 is stored and returned but
// never read: the final knot has no control term.
// This header is the host part, plain C++, next to goal_traj_table.hpp: what the arguments of the three calls have to satisfy, and the layout of the allocation.  The
// rows arrive in the element type, so nothing is rounded here.  tests/native/control_ref_host_check.cpp runs it without a GPU.
#pragma once
#include <cmath>
#include <string>

#include "slots.hpp"
#include "solver_state.hpp"

namespace pddp {

constexpr int control_reference_len(int N, int nu) { return N * nu; }

// elements of the allocation that holds `rows` problems' blocks: the zero row's pad in front, then [rows][N][nu]; Buffers::utab points at element control_ref_pad<T>(nu)
template <typename T>
constexpr size_t control_ref_table_elems(int rows, int N, int nu) { return (size_t)control_ref_pad<T>(nu) + (size_t)rows * (size_t)control_reference_len(N, nu); }

// "" or the complaint about (count, idx, U): count >= 1, idx non-null, indices inside [0, batch) and distinct; with_U: U non-null (setter and getter; the clear call has
// none); check_values: every number of U finite in the element type T (setter)
template <typename T>
inline std::string control_rows_complaint(int count, const int* idx, const T* U, int batch, int N, int nu, bool with_U = true, bool check_values = true) {
    const std::string c = slots_complaint(count, idx, batch);
    if (!c.empty()) return c;
    if (!with_U) return "";
    if (!U) return "U is NULL";
    if (check_values) {
        const size_t len = (size_t)control_reference_len(N, nu);
        for (size_t i = 0; i < (size_t)count * len; i++)
            if (!std::isfinite(U[i])) return "U[" + std::to_string(i / len) + "][" + std::to_string((i % len) / nu) + "][" + std::to_string(i % nu) + "] is not finite";
    }
    return "";
}

}  // namespace pddp
