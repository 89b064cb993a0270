// Stand-alone host program over the host side of the per-knot goal trajectories (csrc/goal_traj_table.hpp): the argument checks of the three calls, the block the
// getter answers with for a problem without a trajectory, and what the kernels' GoalTab instantiations take the goal from (csrc/plants.hpp: problem_goal / goal_at)
// on exactly-sized host buffers.  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc goal_traj_host_check.cpp -o goal_traj_host_check && ./goal_traj_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "diag_cost_table.hpp"
#include "goal_traj_table.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

template <typename T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// every refusal of include/pddp.h, and what is accepted
template <typename T> static void check_complaints(int N, int nx) {
    const int B = 5, len = goal_trajectory_len(N, nx);
    CHECK(len == N * nx);
    std::vector<T> G(2 * (size_t)len);                          // exactly sized: a read past the end is the sanitizer's
    for (size_t i = 0; i < G.size(); i++) G[i] = (T)(0.25 * (double)i - 3.0);
    std::vector<int> idx = {3, 0};
    CHECK(goal_rows_complaint<T>(2, idx.data(), G.data(), B, N, nx).empty());
    CHECK(goal_rows_complaint<T>(1, idx.data(), G.data(), B, N, nx).empty());
    CHECK(!goal_rows_complaint<T>(0, idx.data(), G.data(), B, N, nx).empty());
    CHECK(!goal_rows_complaint<T>(-1, idx.data(), G.data(), B, N, nx).empty());
    CHECK(!goal_rows_complaint<T>(2, nullptr, G.data(), B, N, nx).empty());
    CHECK(!goal_rows_complaint<T>(2, idx.data(), nullptr, B, N, nx).empty());
    CHECK(!goal_rows_complaint<T>(2, idx.data(), nullptr, B, N, nx, true, false).empty());      // the getter's G has to be there too
    CHECK(goal_rows_complaint<T>(2, idx.data(), nullptr, B, N, nx, false).empty());             // the clear call has none
    std::vector<int> out_of = {0, B}, neg = {-1, 2}, twice = {2, 2};
    for (const std::vector<int>* bad : {&out_of, &neg, &twice}) {
        CHECK(!goal_rows_complaint<T>(2, bad->data(), G.data(), B, N, nx).empty());
        CHECK(!goal_rows_complaint<T>(2, bad->data(), G.data(), B, N, nx, true, false).empty());
        CHECK(!goal_rows_complaint<T>(2, bad->data(), nullptr, B, N, nx, false).empty());
    }
    for (size_t e : {(size_t)0, (size_t)len - 1, (size_t)len, 2 * (size_t)len - 1}) {      // first and last number of both trajectories
        for (T v : {std::numeric_limits<T>::quiet_NaN(), std::numeric_limits<T>::infinity(), -std::numeric_limits<T>::infinity()}) {
            std::vector<T> g = G;
            g[e] = v;
            CHECK(!goal_rows_complaint<T>(2, idx.data(), g.data(), B, N, nx).empty());
            CHECK(goal_rows_complaint<T>(2, idx.data(), g.data(), B, N, nx, true, false).empty());      // (the getter does not look at G's contents)
            if (e >= (size_t)len) CHECK(goal_rows_complaint<T>(1, idx.data(), g.data(), B, N, nx).empty());      // (only count trajectories are read)
        }
        std::vector<T> g = G;
        g[e] = std::numeric_limits<T>::max(); CHECK(goal_rows_complaint<T>(2, idx.data(), g.data(), B, N, nx).empty());
        g[e] = -T(0); CHECK(goal_rows_complaint<T>(2, idx.data(), g.data(), B, N, nx).empty());
    }
    // the getter's block for a problem without a trajectory
    std::vector<T> xg(nx), rows((size_t)len, T(-1));
    for (int i = 0; i < nx; i++) xg[i] = (T)(1.5 + i);
    goal_rows_from_xgoal<T>(xg.data(), N, nx, rows.data());
    for (int k = 0; k < N; k++) for (int i = 0; i < nx; i++) CHECK(same_bits(rows[(size_t)k * nx + i], xg[i]));
}

// what the kernels read: base and stride of a problem, the row of a knot; the policies without a goal table take xGoal + pb NX whatever the table holds
template <template <typename> class PT, typename T> static void check_goal_address(int N) {
    using P = PT<T>;
    using D = DiagTab<P, T>;
    using Gp = GoalTab<P, T>;
    constexpr int NX = P::NX, NU = P::NU, NM = NX + NU;
    static_assert(IsDiagTab<Gp>::value && IsGoalTab<Gp>::value && !IsGoalTab<D>::value && !IsGoalTab<P>::value && IsDiagTab<D>::value, "policy traits");
    static_assert(Gp::REC == D::REC && Gp::NX == NX && Gp::NU == NU, "the same record");
    const int B = 3;
    std::vector<T> table((size_t)B * N * NX), xGoal((size_t)B * NX);
    for (size_t i = 0; i < table.size(); i++) table[i] = (T)(100.0 + (double)i);
    for (size_t i = 0; i < xGoal.size(); i++) xGoal[i] = (T)(-1.0 - (double)i);
    std::vector<int> flag = {0, 1, 0};
    Buffers<T> b{};
    CHECK(b.gtab == nullptr && b.gflag == nullptr);
    b.xGoal = xGoal.data(); b.gtab = table.data(); b.gflag = flag.data();
    for (int pb = 0; pb < B; pb++) {
        const GoalRows<T> g = problem_goal<Gp, T>(b, pb, N);
        CHECK(g.stride == (flag[pb] ? NX : 0));
        for (int k = 0; k < N; k++) {
            const T* row = goal_at(g, k);
            const T* want = flag[pb] ? table.data() + ((size_t)pb * N + k) * NX : xGoal.data() + (size_t)pb * NX;
            CHECK(row == want);
            for (int i = 0; i < NX; i++) CHECK(same_bits(row[i], want[i]));      // (reads the whole row: the last row of the last problem ends with the buffer)
        }
        const T* plain = problem_goal<P, T>(b, pb, N);
        const T* diag = problem_goal<D, T>(b, pb, N);
        CHECK(plain == xGoal.data() + (size_t)pb * NX && diag == plain && goal_at(plain, N - 1) == plain);
    }
    // GoalTab evaluates DiagTab's cost: same record, same goal -> same bits
    std::vector<T> row(D::REC);
    CHECK((diag_record_builtin<P, T>(N, row.data())));
    CostWeights<T> cw;
    std::memset(&cw, 0, sizeof(cw));
    const DiagCostWeights<T> own = diag_cost_weights(cw, row.data());
    unsigned s = 7u + (unsigned)N;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (T)((double)(s >> 8) / 8388608.0 - 1.0); };
    for (int k : {0, 1, N - 2, N - 1}) {
        T x[NX], u[NU], H1[NM * NM], H2[NM * NM], g1[NM], g2[NM];
        for (int i = 0; i < NX; i++) x[i] = rnd();
        for (int j = 0; j < NU; j++) u[j] = rnd();
        const T* gk = goal_at(problem_goal<Gp, T>(b, 1, N), k);
        CHECK(same_bits(D::cost(own, x, u, gk, k, N), Gp::cost(own, x, u, gk, k, N)));
        D::cost_grad(own, H1, g1, x, u, gk, k, N);
        Gp::cost_grad(own, H2, g2, x, u, gk, k, N);
        for (int e = 0; e < NM * NM; e++) CHECK(same_bits(H1[e], H2[e]));
        for (int e = 0; e < NM; e++) CHECK(same_bits(g1[e], g2[e]));
        for (int i = 0; i < NX; i++) CHECK(same_bits(g2[i], (T)((k == N - 1 ? row[NX + NU + i] : row[i]) * (x[i] - table[((size_t)1 * N + k) * NX + i]))));
    }
}

int main() {
    for (int N : {4, 16}) {
        check_complaints<float>(N, 2); check_complaints<double>(N, 2);
        check_complaints<float>(N, 4); check_complaints<double>(N, 4);
        check_complaints<float>(N, 12); check_complaints<double>(N, 12);
    }
    CHECK(goal_trajectory_len(16, 2) == 32 && goal_trajectory_len(32, 12) == 384);
    for (int N : {16, 32}) {
        check_goal_address<PendPlant, float>(N); check_goal_address<PendPlant, double>(N);
        check_goal_address<CartPlant, float>(N); check_goal_address<CartPlant, double>(N);
        check_goal_address<QuadPlant, float>(N); check_goal_address<QuadPlant, double>(N);
    }
    std::printf("goal_traj_host_check: ok\n");
    return 0;
}
