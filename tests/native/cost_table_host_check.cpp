// Stand-alone host program over the host side of the per-problem cost weights: cost_weights_at (csrc/plants.hpp: what every kernel calls) with and without a table,
// and validation / packing of csrc/cost_table.hpp.  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc cost_table_host_check.cpp -o cost_table_host_check && ./cost_table_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "cost_table.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

// a record whose every field differs from every other field, and from every entry of the rows below
template <typename T> static CostWeights<T> handle_record(int ee) {
    CostWeights<T> cw;
    std::memset(&cw, 0, sizeof(cw));
    cw.Q1 = T(1.5); cw.Q2 = T(2.5); cw.R = T(3.5); cw.QF1 = T(4.5); cw.QF2 = T(5.5);
    cw.ee = ee;
    cw.Q_EE1 = T(6.5); cw.Q_EE2 = T(7.5); cw.QF_EE1 = T(8.5); cw.QF_EE2 = T(9.5); cw.R_EE = T(10.5); cw.Q_xEE = T(11.5); cw.QF_xEE = T(12.5); cw.Q_xdEE = T(13.5); cw.QF_xdEE = T(14.5);
    cw.ee_z = T(15.5); cw.limits = 1; cw.smooth_abs = ee; cw.sa2 = T(16.5); cw.sa = T(17.5); cw.fd_eps = 18.5;
    return cw;
}

// every field, bit for bit (not one memcmp over the record: the double record has padding behind `ee`)
#define SAME_FIELD(f) (std::memcmp(&a.f, &c.f, sizeof(a.f)) == 0)
template <typename T> static bool same_record(const CostWeights<T>& a, const CostWeights<T>& c) {
    return SAME_FIELD(Q1) && SAME_FIELD(Q2) && SAME_FIELD(R) && SAME_FIELD(QF1) && SAME_FIELD(QF2) && SAME_FIELD(ee) && SAME_FIELD(Q_EE1) && SAME_FIELD(Q_EE2) && SAME_FIELD(QF_EE1) &&
           SAME_FIELD(QF_EE2) && SAME_FIELD(R_EE) && SAME_FIELD(Q_xEE) && SAME_FIELD(QF_xEE) && SAME_FIELD(Q_xdEE) && SAME_FIELD(QF_xdEE) && SAME_FIELD(ee_z) && SAME_FIELD(limits) &&
           SAME_FIELD(smooth_abs) && SAME_FIELD(sa2) && SAME_FIELD(sa) && SAME_FIELD(fd_eps);
}

template <typename T> static void check_weights_at(int ee) {
    const int rec = cost_record_len(ee), B = 4;
    CHECK(rec == (ee ? 9 : 5));
    const CostWeights<T> cw = handle_record<T>(ee);
    Buffers<T> b{};
    CHECK(b.cwt == nullptr);
    // null table: the handle's record, byte for byte, whatever the problem index
    for (int pb : {0, 3, 1000000}) {
        CHECK(same_record(cost_weights_at(b, cw, pb), cw));
    }
    // a table: exactly the family's fields from row pb, in the argument order of the handle-wide call; nothing else
    std::vector<T> rows((size_t)B * rec);
    for (size_t i = 0; i < rows.size(); i++) rows[i] = T(100 + i);
    b.cwt = rows.data();
    for (int pb = 0; pb < B; pb++) {
        const CostWeights<T> o = cost_weights_at(b, cw, pb);
        const T* r = rows.data() + (size_t)pb * rec;
        if (ee) {
            CHECK(o.Q_EE1 == r[0] && o.Q_EE2 == r[1] && o.QF_EE1 == r[2] && o.QF_EE2 == r[3] && o.R_EE == r[4] && o.Q_xEE == r[5] && o.QF_xEE == r[6] && o.Q_xdEE == r[7] && o.QF_xdEE == r[8]);
            CHECK(o.Q1 == cw.Q1 && o.Q2 == cw.Q2 && o.R == cw.R && o.QF1 == cw.QF1 && o.QF2 == cw.QF2);
        } else {
            CHECK(o.Q1 == r[0] && o.Q2 == r[1] && o.R == r[2] && o.QF1 == r[3] && o.QF2 == r[4]);
            CHECK(o.Q_EE1 == cw.Q_EE1 && o.Q_EE2 == cw.Q_EE2 && o.QF_EE1 == cw.QF_EE1 && o.QF_EE2 == cw.QF_EE2 && o.R_EE == cw.R_EE && o.Q_xEE == cw.Q_xEE && o.QF_xEE == cw.QF_xEE &&
                  o.Q_xdEE == cw.Q_xdEE && o.QF_xdEE == cw.QF_xdEE);
        }
        CHECK(o.ee == cw.ee && o.ee_z == cw.ee_z && o.limits == cw.limits && o.smooth_abs == cw.smooth_abs && o.sa == cw.sa && o.sa2 == cw.sa2 && o.fd_eps == cw.fd_eps);
        T hq1, hq2, hr;                                  // the diagonal the matrix-core backward pass takes
        cost_diag_weights_at<T>(b.cwt, ee, pb, hq1, hq2, hr);
        if (ee) CHECK(hq1 == o.Q_xEE && hq2 == o.Q_xdEE && hr == o.R_EE); else CHECK(hq1 == o.Q1 && hq2 == o.Q2 && hr == o.R);
    }
    // the handle-wide record as a row, and back through the table
    std::vector<T> row(rec);
    cost_record_of<T>(cw, row.data());
    b.cwt = row.data();
    CHECK(same_record(cost_weights_at(b, cw, 0), cw));
}

static void check_validation() {
    const int batch = 7, rec = 5;
    const int good[4] = {3, 0, 6, 2};                    // unsorted, unique
    std::vector<double> w(4 * rec, 0.25);
    CHECK(cost_records_complaint(4, good, w.data(), batch, rec).empty());
    CHECK(!cost_records_complaint(0, good, w.data(), batch, rec).empty());
    CHECK(!cost_records_complaint(-1, good, w.data(), batch, rec).empty());
    CHECK(!cost_records_complaint(4, nullptr, w.data(), batch, rec).empty());
    CHECK(!cost_records_complaint(4, good, nullptr, batch, rec).empty());
    const int outside[2] = {1, 7}, negative[2] = {-1, 2}, twice[3] = {2, 5, 2};
    CHECK(!cost_records_complaint(2, outside, w.data(), batch, rec).empty());
    CHECK(!cost_records_complaint(2, negative, w.data(), batch, rec).empty());
    CHECK(!cost_records_complaint(3, twice, w.data(), batch, rec).empty());
    for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()}) {
        std::vector<double> v = w;
        v[4 * rec - 1] = bad;                            // the last number of the last record
        CHECK(!cost_records_complaint(4, good, v.data(), batch, rec).empty());
        CHECK(cost_records_complaint(3, good, v.data(), batch, rec).empty());         // ... which a shorter list does not reach
        CHECK(cost_records_complaint(4, good, v.data(), batch, rec, false).empty());  // the getter's buffer is not looked at
    }
}

static void check_packing() {
    // a double that is no float: rounded ONCE, to the nearest float
    const double v = 0.1 + 1e-10, big = 1000.0 * (1.0 + 3e-8);
    const double w[10] = {v, 0.001, 0.0001, big, 1000.0, 2 * v, 0.5, 0.25, 3.0, -0.0};
    float f[10];
    cost_records_pack<float>(2, 5, w, f);
    for (int i = 0; i < 10; i++) CHECK(f[i] == (float)w[i]);
    CHECK((double)f[0] != v && std::fabs((double)f[0] - v) <= std::ldexp(1.0, -27));
    double d[10];
    cost_records_pack<double>(2, 5, w, d);
    for (int i = 0; i < 10; i++) CHECK(std::memcmp(&d[i], &w[i], sizeof(double)) == 0);
}

int main() {
    check_weights_at<float>(0); check_weights_at<float>(1);
    check_weights_at<double>(0); check_weights_at<double>(1);
    check_validation();
    check_packing();
    std::printf("cost_table_host_check: ok\n");
    return 0;
}
