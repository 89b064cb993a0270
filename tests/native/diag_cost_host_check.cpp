// Stand-alone host program over the host side of the run-time diagonal cost weights (csrc/diag_cost_table.hpp): argument checks, the built-in record, the packing, and
// the DiagTab policy (csrc/plants.hpp: what the table instantiations of the kernels evaluate) against the literal policy it stands in for.  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc diag_cost_host_check.cpp -o diag_cost_host_check && ./diag_cost_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>
#include <utility>
#include <vector>

#include "diag_cost_table.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

template <typename T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// does policy D's weight() accept a record of type CW?  (DiagTab must take the record WITH a row and refuse the plain kernel argument at compile time)
template <typename D, typename CW, typename = void> struct takes_record : std::false_type {};
template <typename D, typename CW> struct takes_record<D, CW, std::void_t<decltype(D::weight(std::declval<const CW&>(), 0, 0, 1))>> : std::true_type {};

// the argument checks: every refusal of include/pddp.h, and what is accepted
template <typename T> static void check_complaints(int nx, int nu) {
    const int rec = diag_record_len(nx, nu), B = 5;
    CHECK(rec == 2 * nx + nu);
    std::vector<double> w(2 * (size_t)rec);                     // exactly sized: a read past the end is the sanitizer's
    for (size_t i = 0; i < w.size(); i++) w[i] = 0.25 + 0.5 * (double)i;
    std::vector<int> idx = {3, 0};
    CHECK(diag_records_complaint<T>(2, idx.data(), w.data(), B, nx, nu).empty());
    CHECK(!diag_records_complaint<T>(0, idx.data(), w.data(), B, nx, nu).empty());
    CHECK(!diag_records_complaint<T>(-1, idx.data(), w.data(), B, nx, nu).empty());
    CHECK(!diag_records_complaint<T>(2, nullptr, w.data(), B, nx, nu).empty());
    CHECK(!diag_records_complaint<T>(2, idx.data(), nullptr, B, nx, nu).empty());
    CHECK(!diag_records_complaint<T>(2, idx.data(), nullptr, B, nx, nu, false).empty());      // the getter's w has to be there too
    std::vector<int> out_of = {0, B}, neg = {-1, 2}, twice = {2, 2};
    CHECK(!diag_records_complaint<T>(2, out_of.data(), w.data(), B, nx, nu).empty());
    CHECK(!diag_records_complaint<T>(2, neg.data(), w.data(), B, nx, nu).empty());
    CHECK(!diag_records_complaint<T>(2, twice.data(), w.data(), B, nx, nu).empty());
    CHECK(!diag_records_complaint<T>(2, twice.data(), w.data(), B, nx, nu, false).empty());
    for (int e = 0; e < rec; e++) {                             // every entry of the second record in turn
        const bool control = e >= nx && e < nx + nu;
        std::vector<double> v = w;
        v[rec + e] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!diag_records_complaint<T>(2, idx.data(), v.data(), B, nx, nu).empty());
        CHECK(diag_records_complaint<T>(2, idx.data(), v.data(), B, nx, nu, false).empty());   // (the getter does not look at w's contents)
        v[rec + e] = std::numeric_limits<double>::infinity();
        CHECK(!diag_records_complaint<T>(2, idx.data(), v.data(), B, nx, nu).empty());
        v[rec + e] = -1e-3;
        CHECK(!diag_records_complaint<T>(2, idx.data(), v.data(), B, nx, nu).empty());
        v[rec + e] = 0.0;                                       // q and qf may be zero, r may not
        CHECK(diag_records_complaint<T>(2, idx.data(), v.data(), B, nx, nu).empty() == !control);
        v[rec + e] = -0.0;
        CHECK(diag_records_complaint<T>(2, idx.data(), v.data(), B, nx, nu).empty() == !control);
        if (sizeof(T) == 4) {                                   // judged in the element type: finite as a double, infinite as a float; positive as a double, zero as a float
            v[rec + e] = 1e39;
            CHECK(!diag_records_complaint<T>(2, idx.data(), v.data(), B, nx, nu).empty());
            v[rec + e] = 1e-60;
            CHECK(diag_records_complaint<T>(2, idx.data(), v.data(), B, nx, nu).empty() == !control);
        }
    }
}

// the built-in record is the policy's literals rounded once; DiagTab on that record evaluates the same numbers as the literal policy, bit for bit
template <template <typename> class PT, typename T> static void check_policy(int N) {
    using P = PT<T>;
    using D = DiagTab<P, T>;
    constexpr int NX = P::NX, NU = P::NU, NM = NX + NU, REC = D::REC;
    static_assert(REC == 2 * NX + NU, "record length");
    static_assert(takes_record<D, DiagCostWeights<T>>::value && !takes_record<D, CostWeights<T>>::value, "DiagTab takes a record with a row, never the plain one");
    static_assert(takes_record<P, CostWeights<T>>::value, "the literal policy takes the plain record");
    std::vector<T> row(REC);
    CHECK((diag_record_builtin<P, T>(N, row.data())));
    for (int i = 0; i < NX; i++) { CHECK(same_bits(row[i], (T)P::QR(i, N))); CHECK(same_bits(row[NX + NU + i], (T)P::QF(N))); }
    for (int j = 0; j < NU; j++) { CHECK(same_bits(row[NX + j], (T)P::Rw(N))); CHECK(P::QR(NX + j, N) == P::Rw(N)); }
    // packing: one rounding
    std::vector<double> wd(REC);
    for (int e = 0; e < REC; e++) wd[e] = 0.1 + 1.0 / 3.0 * e;
    std::vector<T> packed(REC);
    cost_records_pack<T>(1, REC, wd.data(), packed.data());
    for (int e = 0; e < REC; e++) CHECK(same_bits(packed[e], (T)wd[e]));
    CostWeights<T> cw;
    std::memset(&cw, 0, sizeof(cw));
    cw.fd_eps = 0.125;
    const DiagCostWeights<T> own = diag_cost_weights(cw, row.data());
    CHECK(own.row == row.data() && own.fd_eps == 0.125);
    unsigned s = 99u + (unsigned)N;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (T)((double)(s >> 8) / 8388608.0 - 1.0); };
    for (int k : {0, 1, N - 2, N - 1}) {
        T x[NX], u[NU], xg[NX], H1[NM * NM], H2[NM * NM], g1[NM], g2[NM];
        for (int i = 0; i < NX; i++) { x[i] = rnd(); xg[i] = rnd(); }
        for (int j = 0; j < NU; j++) u[j] = rnd();
        CHECK(same_bits(P::cost(cw, x, u, xg, k, N), D::cost(own, x, u, xg, k, N)));
        P::cost_grad(cw, H1, g1, x, u, xg, k, N);
        D::cost_grad(own, H2, g2, x, u, xg, k, N);
        for (int e = 0; e < NM * NM; e++) CHECK(same_bits(H1[e], H2[e]));
        for (int e = 0; e < NM; e++) CHECK(same_bits(g1[e], g2[e]));
        for (int i = 0; i < NM; i++) CHECK(same_bits(P::weight(cw, i, k, N), D::weight(own, i, k, N)));
        // knot_weight with a table: row pb of Buffers::cwt
        std::vector<T> table(3 * (size_t)REC, T(7));
        std::memcpy(table.data() + REC, row.data(), REC * sizeof(T));
        Buffers<T> b{};
        b.cwt = table.data();
        for (int i = 0; i < NM; i++) { CHECK(same_bits((knot_weight<D, T>(b, cw, 1, i, k, N)), P::weight(cw, i, k, N))); CHECK(same_bits((knot_weight<P, T>(b, cw, 1, i, k, N)), P::weight(cw, i, k, N))); }
    }
    // a record of its own: the formulas of include/pddp.h
    for (int e = 0; e < REC; e++) packed[e] = (T)(0.5 + 0.25 * e);
    const DiagCostWeights<T> mine = diag_cost_weights(cw, packed.data());
    T x[NX], u[NU], xg[NX], H[NM * NM], g[NM];
    for (int i = 0; i < NX; i++) { x[i] = rnd(); xg[i] = rnd(); }
    for (int j = 0; j < NU; j++) u[j] = rnd();
    for (int k : {0, N - 1}) {
        const bool fin = k == N - 1;
        D::cost_grad(mine, H, g, x, u, xg, k, N);
        for (int i = 0; i < NM; i++) for (int j = 0; j < NM; j++) {
            const T want = i != j ? T(0) : (fin ? (i < NX ? packed[NX + NU + i] : T(0)) : packed[i]);
            CHECK(same_bits(H[i * NM + j], want));
        }
        for (int i = 0; i < NX; i++) CHECK(same_bits(g[i], (T)((fin ? packed[NX + NU + i] : packed[i]) * (x[i] - xg[i]))));
        for (int j = 0; j < NU; j++) CHECK(same_bits(g[NX + j], (T)((fin ? T(0) : packed[NX + j]) * u[j])));
        double c = 0;
        for (int i = 0; i < NX; i++) c += (double)(fin ? packed[NX + NU + i] : packed[i]) * ((double)(x[i] - xg[i]) * (double)(x[i] - xg[i]));
        if (!fin) for (int j = 0; j < NU; j++) c += (double)packed[NX + j] * ((double)u[j] * (double)u[j]);
        const double got = (double)D::cost(mine, x, u, xg, k, N);
        CHECK(std::fabs(got - 0.5 * c) <= (sizeof(T) == 4 ? 1e-5 : 1e-13) * (std::fabs(0.5 * c) + 1.0));
    }
}

int main() {
    check_complaints<float>(2, 1); check_complaints<double>(2, 1);
    check_complaints<float>(4, 1); check_complaints<double>(4, 1);
    check_complaints<float>(12, 4); check_complaints<double>(12, 4);
    CHECK(diag_record_len(2, 1) == 5 && diag_record_len(4, 1) == 9 && diag_record_len(12, 4) == 28);
    for (int N : {16, 32, 512}) {
        check_policy<PendPlant, float>(N); check_policy<PendPlant, double>(N);
        check_policy<CartPlant, float>(N); check_policy<CartPlant, double>(N);
        check_policy<QuadPlant, float>(N); check_policy<QuadPlant, double>(N);
    }
    std::printf("diag_cost_host_check: ok\n");
    return 0;
}
