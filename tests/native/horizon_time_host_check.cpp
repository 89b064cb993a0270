// Stand-alone host program over the host side of the per-problem horizon times (csrc/horizon_time_table.hpp): the argument checks of the two calls, the conversion
// seconds -> step held against time_step<T> (csrc/handle_setup.hpp) of a configuration with that total_time, and what the kernels' StepTab instantiations integrate
// with (csrc/plants.hpp: problem_dt) on exactly-sized host buffers.  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc horizon_time_host_check.cpp -o horizon_time_host_check && ./horizon_time_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "handle_setup.hpp"
#include "horizon_time_table.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

template <typename T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// every refusal of include/pddp.h, and what is accepted
template <typename T> static void check_complaints(int N) {
    const int B = 5;
    std::vector<double> t = {0.6, 1.37};                        // exactly sized: a read past the end is the sanitizer's
    std::vector<int> idx = {3, 0};
    CHECK(horizon_times_complaint<T>(2, idx.data(), t.data(), B, N).empty());
    CHECK(horizon_times_complaint<T>(1, idx.data(), t.data(), B, N).empty());
    CHECK(!horizon_times_complaint<T>(0, idx.data(), t.data(), B, N).empty());
    CHECK(!horizon_times_complaint<T>(-1, idx.data(), t.data(), B, N).empty());
    CHECK(!horizon_times_complaint<T>(2, nullptr, t.data(), B, N).empty());
    CHECK(!horizon_times_complaint<T>(2, idx.data(), nullptr, B, N).empty());
    CHECK(horizon_times_complaint<T>(2, idx.data(), nullptr, B, N, false).empty());             // the getter has no times to check
    CHECK(!horizon_times_complaint<T>(2, nullptr, nullptr, B, N, false).empty());
    CHECK(!horizon_times_complaint<T>(0, idx.data(), nullptr, B, N, false).empty());
    std::vector<int> out_of = {0, B}, neg = {-1, 2}, twice = {2, 2};
    for (const std::vector<int>* bad : {&out_of, &neg, &twice}) {
        CHECK(!horizon_times_complaint<T>(2, bad->data(), t.data(), B, N).empty());
        CHECK(!horizon_times_complaint<T>(2, bad->data(), nullptr, B, N, false).empty());
    }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // times that are not finite or not > 0; times whose step in T is not finite (overflow) or not normal (underflow to a subnormal or to zero)
    const double tiny = (double)std::numeric_limits<T>::min() * (N - 1) * 0.25, huge = sizeof(T) == 4 ? 1e39 * (N - 1) : inf;
    for (double v : {nan, inf, -inf, 0.0, -0.0, -1.0, tiny, std::numeric_limits<double>::denorm_min(), huge}) {
        for (int e = 0; e < 2; e++) {
            std::vector<double> bad = t;
            bad[e] = v;
            CHECK(!horizon_times_complaint<T>(2, idx.data(), bad.data(), B, N).empty());
            CHECK(horizon_times_complaint<T>(2, idx.data(), bad.data(), B, N, false).empty());      // (the getter does not look at them)
            if (e == 1) CHECK(horizon_times_complaint<T>(1, idx.data(), bad.data(), B, N).empty());  // (only count times are read)
        }
    }
    // the smallest and a large accepted step
    std::vector<double> edge = {(double)std::numeric_limits<T>::min() * (N - 1) * 2.0, 1e6};
    CHECK(horizon_times_complaint<T>(2, idx.data(), edge.data(), B, N).empty());
}

// the step of a given time is time_step<T> of a configuration with that total_time, bit for bit
template <typename T> static void check_step_is_time_step() {
    for (int plant : {1, 2, 3}) {
        for (int N : {4, 16, 32, 128, 513}) {
            pddp_config c;
            default_config(&c, plant);
            c.N = N;
            unsigned s = 99u + (unsigned)N;
            for (int trial = 0; trial < 200; trial++) {
                s = s * 1664525u + 1013904223u;
                static const double ladder[5] = {1.0, 0.6, 1.37, 0.8, 1.5};
                const double t = trial < 5 ? (N / 32.0) * ladder[trial] : 1e-3 + 20.0 * ((double)(s >> 8) / 16777216.0);
                c.total_time = t;
                CHECK(same_bits(horizon_time_step<T>(t, N), time_step<T>(c)));
                CHECK(same_bits(horizon_time_step<T>(t, N), (T)(t / (N - 1))));
            }
        }
    }
}

// what the kernels integrate with: entry pb of the table on a StepTab policy, the kernel argument on every other policy whatever the table holds
template <template <typename> class PT, typename T> static void check_problem_dt() {
    using P = PT<T>;
    using D = DiagTab<P, T>;
    using G = GoalTab<P, T>;
    using S = StepTab<P, T>;
    static_assert(IsStepTab<S>::value && IsGoalTab<S>::value && IsDiagTab<S>::value, "StepTab is every layer below it");
    static_assert(!IsStepTab<G>::value && !IsStepTab<D>::value && !IsStepTab<P>::value && IsGoalTab<G>::value && !IsGoalTab<D>::value, "policy traits");
    static_assert(S::REC == D::REC && S::NX == P::NX && S::NU == P::NU && S::NPOS == P::NPOS && S::PLANT == P::PLANT, "the same plant and record");
    static_assert(IsStepTab<typename S::template Rebind<double>>::value, "Rebind keeps the layer");
    const int B = 5;
    std::vector<T> table(B);                                    // exactly sized
    for (int i = 0; i < B; i++) table[i] = horizon_time_step<T>(0.3 + 0.21 * i, 16);
    const T arg = (T)0.03125;
    Buffers<T> b{};
    CHECK(b.dtab == nullptr);                                   // default-initialised: a handle without a table
    CHECK(same_bits(problem_dt<P, T>(b, 3, arg), arg) && same_bits(problem_dt<D, T>(b, 3, arg), arg) && same_bits(problem_dt<G, T>(b, 3, arg), arg));
    b.dtab = table.data();
    for (int pb = 0; pb < B; pb++) {
        CHECK(same_bits(problem_dt<S, T>(b, pb, arg), table[pb]));
        CHECK(same_bits(problem_dt<P, T>(b, pb, arg), arg) && same_bits(problem_dt<D, T>(b, pb, arg), arg) && same_bits(problem_dt<G, T>(b, pb, arg), arg));
    }
    // StepTab evaluates GoalTab's cost: same record, same goal -> same bits
    std::vector<T> row(D::REC);
    for (int i = 0; i < D::REC; i++) row[i] = (T)(0.5 + 0.25 * i);
    CostWeights<T> cw;
    std::memset(&cw, 0, sizeof(cw));
    const DiagCostWeights<T> own = diag_cost_weights(cw, row.data());
    T x[P::NX], u[P::NU], xg[P::NX];
    for (int i = 0; i < P::NX; i++) { x[i] = (T)(0.1 * i - 0.3); xg[i] = (T)(0.05 * i); }
    for (int j = 0; j < P::NU; j++) u[j] = (T)(0.7 - 0.2 * j);
    for (int k : {0, 14, 15}) CHECK(same_bits(G::cost(own, x, u, xg, k, 16), S::cost(own, x, u, xg, k, 16)));
}

int main() {
    for (int N : {4, 16, 32}) { check_complaints<float>(N); check_complaints<double>(N); }
    check_step_is_time_step<float>(); check_step_is_time_step<double>();
    check_problem_dt<PendPlant, float>(); check_problem_dt<PendPlant, double>();
    check_problem_dt<CartPlant, float>(); check_problem_dt<CartPlant, double>();
    check_problem_dt<QuadPlant, float>(); check_problem_dt<QuadPlant, double>();
    std::printf("horizon_time_host_check: ok\n");
    return 0;
}
