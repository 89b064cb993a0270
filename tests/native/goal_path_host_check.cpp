// Stand-alone host program over the host side of the goal paths (csrc/goal_path_table.hpp): every refusal of the argument checks on exactly-sized buffers, the two
// index functions goal_path_row / goal_path_advance against a brute-force statement (walk one knot at a time), and a kernel-shaped host loop -- k_goal_window's
// (knot, chunk) addressing over bytes -- that windows with them, against the same brute force.  It prints the windows of a list of cases as row numbers; the test
// suite holds its NumPy statement of the window against those lines, so that the GPU tests and the C++ share one definition.  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc goal_path_host_check.cpp -o goal_path_host_check && ./goal_path_host_check
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "goal_path_table.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// the statement: move one knot at a time
static int brute_step(int row, int len, int mode) {
    if (mode == kGoalPathWrap) return row + 1 == len ? 0 : row + 1;
    return row + 1 < len ? row + 1 : len - 1;
}
static int brute_row(int cursor, int k, int len, int mode) {
    int r = cursor;
    for (int j = 0; j < k; j++) r = brute_step(r, len, mode);
    return r;
}

static void check_index_functions() {
    for (int mode : {kGoalPathHold, kGoalPathWrap})
        for (int len = 1; len <= 9; len++)
            for (int cursor = 0; cursor < len; cursor++) {
                for (int k = 0; k <= 20; k++) {
                    const int r = goal_path_row(cursor, k, len, mode);
                    CHECK(r == brute_row(cursor, k, len, mode) && r >= 0 && r < len);
                }
                for (int s = 0; s <= 20; s++) {
                    const int c = goal_path_advance(cursor, s, len, mode);
                    CHECK(c == brute_row(cursor, s, len, mode) && c >= 0 && c < len);      // canonical
                    // the window after the advance is the old window moved up by s knots
                    for (int k = 0; k <= 20; k++) CHECK(goal_path_row(c, k, len, mode) == brute_row(cursor, s + k, len, mode));
                    // two advances are one
                    for (int s2 = 0; s2 <= 20; s2 += 5) CHECK(goal_path_advance(c, s2, len, mode) == brute_row(cursor, s + s2, len, mode));
                }
            }
    // the largest operands a reserve admits: capacity + N fits an int, so cursor + k does
    const int N = 1024, cap = INT_MAX - N;
    CHECK(goal_path_reserve_complaint(cap, N, 0).empty());
    CHECK(goal_path_row(cap - 1, N - 1, cap, kGoalPathHold) == cap - 1);
    CHECK(goal_path_row(cap - 1, N - 1, cap, kGoalPathWrap) == N - 2);
}

// k_goal_window's loop for one problem with `threads` threads: t runs over (knot, chunk) pairs, chunk width W bytes
template <typename T>
static void window_like_the_kernel(const T* path, GoalPathRec& rec, int shift, int N, int nx, T* gtab, int threads) {
    GoalPathRec r = rec;
    r.cursor = goal_path_advance(r.cursor, shift, r.len, r.mode);
    rec.cursor = r.cursor;                                          // (thread 0, behind the barrier)
    const unsigned row_bytes = (unsigned)nx * (unsigned)sizeof(T);
    const unsigned W = row_bytes % 16 == 0 ? 16 : row_bytes % 8 == 0 ? 8 : 4;
    const unsigned per = row_bytes / W, total = (unsigned)N * per;
    unsigned char* dst = reinterpret_cast<unsigned char*>(gtab);
    const unsigned char* src = reinterpret_cast<const unsigned char*>(path);
    for (int tid = 0; tid < threads; tid++)
        for (unsigned t = (unsigned)tid; t < total; t += (unsigned)threads) {
            const unsigned k = t / per, c = t - k * per;
            const size_t from = (size_t)goal_path_row(r.cursor, (int)k, r.len, r.mode) * row_bytes + (size_t)c * W;
            std::memcpy(dst + (size_t)t * W, src + from, W);
        }
}

template <typename T>
static void check_windows(int nx) {
    for (int mode : {kGoalPathHold, kGoalPathWrap})
        for (int len : {1, 2, 3, 8, 9})
            for (int N : {4, 8})
                for (int cursor = 0; cursor < len; cursor++)
                    for (int shift : {0, 1, 3, N - 2}) {
                        std::vector<T> path((size_t)len * nx), got((size_t)N * nx, T(-1)), lib((size_t)N * nx, T(-2));      // exactly sized
                        for (size_t i = 0; i < path.size(); i++) path[i] = (T)(1.0 + (double)i * 0.5);
                        GoalPathRec rec{len, mode, cursor};
                        window_like_the_kernel<T>(path.data(), rec, shift, N, nx, got.data(), 7);
                        CHECK(rec.cursor == brute_row(cursor, shift, len, mode));
                        goal_path_window<T>(path.data(), rec, N, nx, lib.data());
                        for (int k = 0; k < N; k++) {
                            const int want = brute_row(cursor, shift + k, len, mode);
                            for (int i = 0; i < nx; i++) {
                                CHECK(std::memcmp(&got[(size_t)k * nx + i], &path[(size_t)want * nx + i], sizeof(T)) == 0);
                                CHECK(std::memcmp(&lib[(size_t)k * nx + i], &path[(size_t)want * nx + i], sizeof(T)) == 0);
                            }
                        }
                    }
}

// every refusal of include/pddp.h, and what is accepted
template <typename T>
static void check_complaints(int nx) {
    const int B = 5, cap = 6, len = 4;
    std::vector<T> path(2 * (size_t)len * nx);                     // exactly sized: a read past the end is the sanitizer's
    for (size_t i = 0; i < path.size(); i++) path[i] = (T)(0.25 * (double)i - 3.0);
    std::vector<int> idx = {3, 0}, cur = {3, 0};
    auto set = [&](int count, const int* ix, int l, int mode, const int* c, const T* p) { return goal_path_set_complaint<T>(count, ix, l, mode, c, p, B, cap, nx); };
    CHECK(set(2, idx.data(), len, kGoalPathHold, cur.data(), path.data()).empty());
    CHECK(set(2, idx.data(), len, kGoalPathWrap, nullptr, path.data()).empty());      // cursor NULL: 0
    CHECK(set(1, idx.data(), len, kGoalPathWrap, cur.data(), path.data()).empty());
    CHECK(!set(0, idx.data(), len, kGoalPathHold, cur.data(), path.data()).empty());
    CHECK(!set(-3, idx.data(), len, kGoalPathHold, cur.data(), path.data()).empty());
    CHECK(!set(2, nullptr, len, kGoalPathHold, cur.data(), path.data()).empty());
    CHECK(!set(2, idx.data(), len, kGoalPathHold, cur.data(), nullptr).empty());
    std::vector<int> out_of = {0, B}, neg = {-1, 2}, twice = {2, 2};
    for (const std::vector<int>* bad : {&out_of, &neg, &twice}) CHECK(!set(2, bad->data(), len, kGoalPathHold, cur.data(), path.data()).empty());
    for (int l : {0, -1, cap + 1, INT_MAX}) CHECK(!set(2, idx.data(), l, kGoalPathHold, nullptr, path.data()).empty());      // (refused before a row is read)
    for (int mode : {0, 3, -1}) CHECK(!set(2, idx.data(), len, mode, cur.data(), path.data()).empty());
    for (int c : {-1, len, len + 7}) {
        std::vector<int> bc = {0, c};
        CHECK(!set(2, idx.data(), len, kGoalPathHold, bc.data(), path.data()).empty());
        CHECK(set(1, idx.data(), len, kGoalPathHold, bc.data(), path.data()).empty());      // (only count cursors are read)
    }
    { std::vector<T> full(2 * (size_t)cap * nx, T(1)); std::vector<int> last = {cap - 1, 0}; CHECK(goal_path_set_complaint<T>(2, idx.data(), cap, kGoalPathHold, last.data(), full.data(), B, cap, nx).empty()); }
    for (size_t e : {(size_t)0, (size_t)len * nx - 1, (size_t)len * nx, 2 * (size_t)len * nx - 1})
        for (T v : {std::numeric_limits<T>::quiet_NaN(), std::numeric_limits<T>::infinity(), -std::numeric_limits<T>::infinity()}) {
            std::vector<T> p = path;
            p[e] = v;
            CHECK(!set(2, idx.data(), len, kGoalPathHold, cur.data(), p.data()).empty());
            if (e >= (size_t)len * nx) CHECK(set(1, idx.data(), len, kGoalPathHold, cur.data(), p.data()).empty());      // (only count paths are read)
            p[e] = std::numeric_limits<T>::max();
            CHECK(set(2, idx.data(), len, kGoalPathHold, cur.data(), p.data()).empty());
        }
    // the cursor call: problems 0 and 3 have a path
    std::vector<GoalPathRec> recs(B, GoalPathRec{0, 0, 0});
    recs[0] = GoalPathRec{1, kGoalPathWrap, 0}; recs[3] = GoalPathRec{4, kGoalPathHold, 0};
    auto curs = [&](int count, const int* ix, const int* c) { return goal_path_cursor_complaint(count, ix, c, recs.data(), B); };
    std::vector<int> ok = {3, 0}, zero = {0, 0};
    CHECK(curs(2, idx.data(), ok.data()).empty() && curs(2, idx.data(), zero.data()).empty());
    CHECK(!curs(0, idx.data(), ok.data()).empty() && !curs(2, nullptr, ok.data()).empty() && !curs(2, idx.data(), nullptr).empty());
    for (const std::vector<int>* bad : {&out_of, &neg, &twice}) CHECK(!curs(2, bad->data(), zero.data()).empty());
    std::vector<int> no_path = {3, 1}, past = {4, 0}, past1 = {0, 1}, negc = {-1, 0};
    CHECK(!curs(2, no_path.data(), zero.data()).empty());          // problem 1 has none
    CHECK(!curs(2, idx.data(), past.data()).empty() && !curs(2, idx.data(), past1.data()).empty() && !curs(2, idx.data(), negc.data()).empty());
}

static void check_reserve() {
    CHECK(goal_path_reserve_complaint(1, 8, 0).empty() && goal_path_reserve_complaint(37, 8, 0).empty() && goal_path_reserve_complaint(37, 8, 37).empty());
    CHECK(!goal_path_reserve_complaint(0, 8, 0).empty() && !goal_path_reserve_complaint(-5, 8, 0).empty());
    CHECK(!goal_path_reserve_complaint(36, 8, 37).empty() && !goal_path_reserve_complaint(38, 8, 37).empty());
    CHECK(!goal_path_reserve_complaint(INT_MAX, 8, 0).empty() && !goal_path_reserve_complaint(INT_MAX - 7, 8, 0).empty() && goal_path_reserve_complaint(INT_MAX - 8, 8, 0).empty());
    CHECK(goal_path_shape_complaint(1, 1, 1).empty() && !goal_path_shape_complaint(2, 1, 1).empty());
}

// "window <len> <mode> <cursor> <shift> <N>: <cursor after> | <row of knot 0> ..." through the kernel-shaped loop on rows that hold their own number
static void print_windows() {
    const int nx = 2;
    for (int mode : {kGoalPathHold, kGoalPathWrap})
        for (int len : {1, 3, 8, 37})
            for (int cursor : {0, len / 2, len - 1})
                for (int shift : {0, 1, 3, 6}) {
                    const int N = 8;
                    std::vector<float> path((size_t)len * nx), got((size_t)N * nx);
                    for (int r = 0; r < len; r++) for (int i = 0; i < nx; i++) path[(size_t)r * nx + i] = (float)r;
                    GoalPathRec rec{len, mode, cursor};
                    window_like_the_kernel<float>(path.data(), rec, shift, N, nx, got.data(), 256);
                    std::printf("window %d %d %d %d %d: %d |", len, mode, cursor, shift, N, rec.cursor);
                    for (int k = 0; k < N; k++) { CHECK(got[(size_t)k * nx] == got[(size_t)k * nx + 1]); std::printf(" %d", (int)got[(size_t)k * nx]); }
                    std::printf("\n");
                }
}

int main() {
    static_assert(sizeof(GoalPathRec) == 3 * sizeof(int), "the record is three ints");
    check_index_functions();
    check_reserve();
    for (int nx : {2, 4, 12}) {
        check_complaints<float>(nx); check_complaints<double>(nx);
        check_windows<float>(nx); check_windows<double>(nx);
    }
    print_windows();
    std::printf("goal_path_host_check: ok\n");
    return 0;
}
