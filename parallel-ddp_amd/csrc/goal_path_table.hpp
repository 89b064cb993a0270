// Goal paths of the pendulum, cart-pole and quadrotor: pddp_reserve_goal_path / pddp_set_goal_path_problems / pddp_set_goal_path_cursor_problems /
// pddp_get_goal_path_problems.
//
// A problem with a goal path keeps path[len][NX] (1 <= len <= capacity) in device memory with a mode and a cursor in [0, len).  The goal of horizon knot k is row
// goal_path_row(cursor, k, len, mode) of the path; a control cycle that shifts the previous solution by s moves the cursor to goal_path_advance(cursor, s, len, mode).
// The problem's block of the goal table (goal_traj_table.hpp) always holds that window, written by k_goal_window (kernels.hpp), so every kernel that reads a goal is
// the one a plain trajectory runs.  This header is the host part, plain C++ with no HIP include: the two index functions (kernel, host and tests share them), the
// record the device keeps per problem and what the arguments of the calls have to satisfy.  tests/native/goal_path_host_check.cpp runs it without a GPU.
#pragma once
#include <climits>
#include <cmath>
#include <string>

#include "pddp_common.hpp"
#include "slots.hpp"

namespace pddp {

constexpr int kGoalPathHold = 1;           // PDDP_GOAL_PATH_HOLD: the last row is held
constexpr int kGoalPathWrap = 2;           // PDDP_GOAL_PATH_WRAP: the path is a loop

// what the device keeps per problem; len = 0: no path
struct GoalPathRec { int len, mode, cursor; };

// row of the path that horizon knot k reads: cursor in [0, len), k >= 0, cursor + k fits an int (pddp_reserve_goal_path refuses a capacity for which capacity + N does not)
PDDP_HD int goal_path_row(int cursor, int k, int len, int mode) {
    const int r = cursor + k;
    if (mode == kGoalPathWrap) return r % len;                      // (a true modulo: len may be smaller than N, the window then laps the path)
    return r < len - 1 ? r : len - 1;
}
// the cursor after a shift by s knots, in canonical form ([0, len)): the row knot s read before the shift
PDDP_HD int goal_path_advance(int cursor, int s, int len, int mode) { return goal_path_row(cursor, s, len, mode); }

// "" or the complaint about a reserve: capacity >= 1, capacity + N an int; a handle that has one keeps it
inline std::string goal_path_reserve_complaint(int capacity, int N, int have) {
    if (capacity < 1) return "capacity must be >= 1";
    if (capacity > INT_MAX - N) return "capacity + N does not fit an int";
    if (have && have != capacity) return "the handle has a goal path capacity of " + std::to_string(have) + " rows; it cannot be changed";
    return "";
}
// "" or the complaint about (len, mode) of a setter call
inline std::string goal_path_shape_complaint(int len, int mode, int capacity) {
    if (len < 1 || len > capacity) return "len = " + std::to_string(len) + " is outside [1, capacity = " + std::to_string(capacity) + "]";
    if (mode != kGoalPathHold && mode != kGoalPathWrap) return "mode must be PDDP_GOAL_PATH_HOLD (1) or PDDP_GOAL_PATH_WRAP (2)";
    return "";
}
// "" or the complaint about the arguments of pddp_set_goal_path_problems: the slot list, len, mode, cursor[count] (NULL: every cursor 0) inside [0, len), path non-null
// and every number of path[count][len][nx] finite in the element type T
template <typename T>
inline std::string goal_path_set_complaint(int count, const int* idx, int len, int mode, const int* cursor, const T* path, int batch, int capacity, int nx) {
    std::string c = slots_complaint(count, idx, batch);
    if (!c.empty()) return c;
    if (!(c = goal_path_shape_complaint(len, mode, capacity)).empty()) return c;
    if (!path) return "path is NULL";
    if (cursor)
        for (int i = 0; i < count; i++)
            if (cursor[i] < 0 || cursor[i] >= len) return "cursor[" + std::to_string(i) + "] = " + std::to_string(cursor[i]) + " is outside [0, len = " + std::to_string(len) + ")";
    const size_t per = (size_t)len * nx;
    for (size_t i = 0; i < (size_t)count * per; i++)
        if (!std::isfinite(path[i])) return "path[" + std::to_string(i / per) + "][" + std::to_string((i % per) / nx) + "][" + std::to_string(i % nx) + "] is not finite";
    return "";
}
// "" or the complaint about the arguments of pddp_set_goal_path_cursor_problems; recs[q].len: the path length of problem q as the host knows it (0: no path)
inline std::string goal_path_cursor_complaint(int count, const int* idx, const int* cursor, const GoalPathRec* recs, int batch) {
    const std::string c = slots_complaint(count, idx, batch);
    if (!c.empty()) return c;
    if (!cursor) return "cursor is NULL";
    for (int i = 0; i < count; i++) {
        const int len = recs[idx[i]].len;
        if (!len) return "problem " + std::to_string(idx[i]) + " (idx[" + std::to_string(i) + "]) has no goal path";
        if (cursor[i] < 0 || cursor[i] >= len) return "cursor[" + std::to_string(i) + "] = " + std::to_string(cursor[i]) + " is outside [0, len = " + std::to_string(len) + ")";
    }
    return "";
}

// the window of one problem as k_goal_window writes it, on the host: rows[k] = path[goal_path_row(cursor, k)] for the N knots (tests and the stand-alone check)
template <typename T>
inline void goal_path_window(const T* path, const GoalPathRec& r, int N, int nx, T* rows) {
    for (int k = 0; k < N; k++) {
        const T* src = path + (size_t)goal_path_row(r.cursor, k, r.len, r.mode) * nx;
        for (int i = 0; i < nx; i++) rows[(size_t)k * nx + i] = src[i];
    }
}

}  // namespace pddp
