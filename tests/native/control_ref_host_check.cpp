// Stand-alone host program over the host side of the control references (csrc/control_ref_table.hpp): the argument checks of the three calls and the layout of the
// allocation, and what the kernels' RefTab instantiations take the goal and the reference from (csrc/plants.hpp: problem_goal / goal_at / RefTab::cost / cost_grad /
// control_term) on exactly-sized host buffers.  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc control_ref_host_check.cpp -o control_ref_host_check && ./control_ref_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "control_ref_table.hpp"
#include "diag_cost_table.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

template <typename T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// every refusal of include/pddp.h, and what is accepted
template <typename T> static void check_complaints(int N, int nu) {
    const int B = 5, len = control_reference_len(N, nu);
    CHECK(len == N * nu);
    std::vector<T> U(2 * (size_t)len);                          // exactly sized: a read past the end is the sanitizer's
    for (size_t i = 0; i < U.size(); i++) U[i] = (T)(0.25 * (double)i - 3.0);
    std::vector<int> idx = {3, 0};
    CHECK(control_rows_complaint<T>(2, idx.data(), U.data(), B, N, nu).empty());
    CHECK(control_rows_complaint<T>(1, idx.data(), U.data(), B, N, nu).empty());
    CHECK(!control_rows_complaint<T>(0, idx.data(), U.data(), B, N, nu).empty());
    CHECK(!control_rows_complaint<T>(-1, idx.data(), U.data(), B, N, nu).empty());
    CHECK(!control_rows_complaint<T>(2, nullptr, U.data(), B, N, nu).empty());
    CHECK(!control_rows_complaint<T>(2, idx.data(), nullptr, B, N, nu).empty());
    CHECK(!control_rows_complaint<T>(2, idx.data(), nullptr, B, N, nu, true, false).empty());      // the getter's U has to be there too
    CHECK(control_rows_complaint<T>(2, idx.data(), nullptr, B, N, nu, false).empty());             // the clear call has none
    std::vector<int> out_of = {0, B}, neg = {-1, 2}, twice = {2, 2};
    for (const std::vector<int>* bad : {&out_of, &neg, &twice}) {
        CHECK(!control_rows_complaint<T>(2, bad->data(), U.data(), B, N, nu).empty());
        CHECK(!control_rows_complaint<T>(2, bad->data(), U.data(), B, N, nu, true, false).empty());
        CHECK(!control_rows_complaint<T>(2, bad->data(), nullptr, B, N, nu, false).empty());
    }
    for (size_t e : {(size_t)0, (size_t)len - 1, (size_t)len, 2 * (size_t)len - 1}) {      // first and last number of both references (the last: in row N - 1, stored if never read)
        for (T v : {std::numeric_limits<T>::quiet_NaN(), std::numeric_limits<T>::infinity(), -std::numeric_limits<T>::infinity()}) {
            std::vector<T> u = U;
            u[e] = v;
            CHECK(!control_rows_complaint<T>(2, idx.data(), u.data(), B, N, nu).empty());
            CHECK(control_rows_complaint<T>(2, idx.data(), u.data(), B, N, nu, true, false).empty());      // (the getter does not look at U's contents)
            if (e >= (size_t)len) CHECK(control_rows_complaint<T>(1, idx.data(), u.data(), B, N, nu).empty());      // (only count references are read)
        }
        std::vector<T> u = U;
        u[e] = std::numeric_limits<T>::max(); CHECK(control_rows_complaint<T>(2, idx.data(), u.data(), B, N, nu).empty());
        u[e] = -T(0); CHECK(control_rows_complaint<T>(2, idx.data(), u.data(), B, N, nu).empty());
    }
    // the layout: whole 16-byte pieces of zero row in front, at least one row long
    const int pad = control_ref_pad<T>(nu);
    CHECK(pad >= nu && (pad * sizeof(T)) % 16 == 0 && (pad - nu) * sizeof(T) < 16);
    CHECK(control_ref_table_elems<T>(B, N, nu) == (size_t)pad + (size_t)B * len);
}

// what the kernels read: goal base / stride and reference base / stride of a problem, the rows of a knot; the policies below RefTab see none of it
template <template <typename> class PT, typename T> static void check_reference_address(int N) {
    using P = PT<T>;
    using D = DiagTab<P, T>;
    using S = StepTab<P, T>;
    using R = RefTab<P, T>;
    constexpr int NX = P::NX, NU = P::NU, NM = NX + NU;
    static_assert(IsDiagTab<R>::value && IsGoalTab<R>::value && IsStepTab<R>::value && IsRefTab<R>::value && !IsRefTab<S>::value && !IsRefTab<D>::value && !IsRefTab<P>::value, "policy traits");
    static_assert(R::REC == D::REC && R::NX == NX && R::NU == NU, "the same record");
    const int B = 3, pad = control_ref_pad<T>(NU);
    std::vector<T> gtable((size_t)B * N * NX), xGoal((size_t)B * NX), alloc(control_ref_table_elems<T>(B, N, NU), T(0));      // exactly sized
    for (size_t i = 0; i < gtable.size(); i++) gtable[i] = (T)(100.0 + (double)i);
    for (size_t i = 0; i < xGoal.size(); i++) xGoal[i] = (T)(-1.0 - (double)i);
    T* utab = alloc.data() + pad;
    for (size_t i = 0; i < (size_t)B * N * NU; i++) utab[i] = (T)(0.5 + 0.125 * (double)i);
    std::vector<int> gflag = {0, 1, 0}, uflag = {0, 1, 1};
    Buffers<T> b{};
    CHECK(b.utab == nullptr && b.uflag == nullptr);
    b.xGoal = xGoal.data(); b.gtab = gtable.data(); b.gflag = gflag.data(); b.utab = utab; b.uflag = uflag.data();
    for (int pb = 0; pb < B; pb++) {
        const RefRows<T> g = problem_goal<R, T>(b, pb, N);
        CHECK(g.stride == (gflag[pb] ? NX : 0) && g.ustride == (uflag[pb] ? NU : 0));
        for (int k = 0; k < N; k++) {
            const KnotRef<T> row = goal_at(g, k);
            const T* want = gflag[pb] ? gtable.data() + ((size_t)pb * N + k) * NX : xGoal.data() + (size_t)pb * NX;
            const T* uwant = uflag[pb] ? utab + ((size_t)pb * N + k) * NU : alloc.data();
            CHECK(row.xg == want && row.ur == uwant && goal_row(row) == want);
            for (int i = 0; i < NX; i++) CHECK(same_bits(row.xg[i], want[i]));
            for (int j = 0; j < NU; j++) CHECK(same_bits(row.ur[j], uflag[pb] ? uwant[j] : T(0)));      // (reads the whole row: the last row of the last problem ends with the buffer)
        }
        // the layers below: what they always returned, whatever the reference table holds
        const GoalRows<T> gs = problem_goal<S, T>(b, pb, N);
        CHECK(gs.base == g.base && gs.stride == g.stride);
        const T* plain = problem_goal<P, T>(b, pb, N);
        CHECK(plain == xGoal.data() + (size_t)pb * NX && goal_at(plain, N - 1) == plain && goal_row(plain) == plain);
    }
    std::vector<T> rec(D::REC);
    CHECK((diag_record_builtin<P, T>(N, rec.data())));
    CostWeights<T> cw;
    std::memset(&cw, 0, sizeof(cw));
    const DiagCostWeights<T> own = diag_cost_weights(cw, rec.data());
    unsigned s = 11u + (unsigned)N;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (T)((double)(s >> 8) / 8388608.0 - 1.0); };
    for (int k : {0, 1, N - 2, N - 1}) {
        T x[NX], u[NU], du[NU], H1[NM * NM], H2[NM * NM], g1[NM], g2[NM];
        for (int i = 0; i < NX; i++) x[i] = rnd();
        for (int j = 0; j < NU; j++) u[j] = rnd();
        // an unflagged problem (0): RefTab evaluates StepTab's cost bit for bit -- u - 0 is u
        const KnotRef<T> r0 = goal_at(problem_goal<R, T>(b, 0, N), k);
        CHECK(same_bits(S::cost(own, x, u, r0.xg, k, N), R::cost(own, x, u, r0, k, N)));
        S::cost_grad(own, H1, g1, x, u, r0.xg, k, N);
        R::cost_grad(own, H2, g2, x, u, r0, k, N);
        for (int e = 0; e < NM * NM; e++) CHECK(same_bits(H1[e], H2[e]));
        for (int e = 0; e < NM; e++) CHECK(same_bits(g1[e], g2[e]));
        for (int j = 0; j < NU; j++) CHECK(same_bits(control_term(r0, u, j, k == N - 1), u[j]) && same_bits(control_term(r0.xg, u, j, k == N - 1), u[j]));
        // a flagged problem (1): StepTab's cost of u - U[k] at a running knot; the final knot reads no row
        const KnotRef<T> r1 = goal_at(problem_goal<R, T>(b, 1, N), k);
        for (int j = 0; j < NU; j++) du[j] = k == N - 1 ? u[j] : u[j] - utab[((size_t)1 * N + k) * NU + j];
        CHECK(same_bits(S::cost(own, x, du, r1.xg, k, N), R::cost(own, x, u, r1, k, N)));
        S::cost_grad(own, H1, g1, x, du, r1.xg, k, N);
        R::cost_grad(own, H2, g2, x, u, r1, k, N);
        for (int e = 0; e < NM * NM; e++) CHECK(same_bits(H1[e], H2[e]));
        for (int e = 0; e < NM; e++) CHECK(same_bits(g1[e], g2[e]));
        for (int j = 0; j < NU; j++) CHECK(same_bits(control_term(r1, u, j, k == N - 1), du[j]));
        if (k < N - 1) for (int j = 0; j < NU; j++) CHECK(same_bits(g2[NX + j], (T)(rec[NX + j] * (u[j] - utab[((size_t)1 * N + k) * NU + j]))));
    }
}

int main() {
    for (int N : {4, 16}) {
        check_complaints<float>(N, 1); check_complaints<double>(N, 1);
        check_complaints<float>(N, 4); check_complaints<double>(N, 4);
    }
    CHECK(control_reference_len(16, 1) == 16 && control_reference_len(32, 4) == 128);
    CHECK(control_ref_pad<float>(1) == 4 && control_ref_pad<float>(4) == 4 && control_ref_pad<double>(1) == 2 && control_ref_pad<double>(4) == 4);
    for (int N : {16, 32}) {
        check_reference_address<PendPlant, float>(N); check_reference_address<PendPlant, double>(N);
        check_reference_address<CartPlant, float>(N); check_reference_address<CartPlant, double>(N);
        check_reference_address<QuadPlant, float>(N); check_reference_address<QuadPlant, double>(N);
    }
    std::printf("control_ref_host_check: ok\n");
    return 0;
}
