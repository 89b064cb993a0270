// Stand-alone host program over the host side of the control limits (csrc/control_limit_table.hpp): the argument checks of the three calls, the rounding to the element
// type and the row of a problem without limits, on exactly-sized host buffers.  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc control_limit_host_check.cpp -o control_limit_host_check && ./control_limit_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "control_limit_table.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

template <typename T> static void check(int nu) {
    const int B = 5, len = control_limits_len(nu);
    const double inf = std::numeric_limits<double>::infinity();
    CHECK(len == 2 * nu);
    std::vector<double> lim(2 * (size_t)len);                   // exactly sized: a read past the end is the sanitizer's
    for (int i = 0; i < 2; i++) for (int j = 0; j < nu; j++) { lim[(size_t)i * len + j] = -1.0 - j; lim[(size_t)i * len + nu + j] = 0.5 + i; }
    std::vector<int> idx = {3, 0};
    CHECK(control_limits_complaint<T>(2, idx.data(), lim.data(), B, nu).empty());
    CHECK(control_limits_complaint<T>(1, idx.data(), lim.data(), B, nu).empty());
    CHECK(!control_limits_complaint<T>(0, idx.data(), lim.data(), B, nu).empty());
    CHECK(!control_limits_complaint<T>(-1, idx.data(), lim.data(), B, nu).empty());
    CHECK(!control_limits_complaint<T>(2, nullptr, lim.data(), B, nu).empty());
    CHECK(!control_limits_complaint<T>(2, idx.data(), nullptr, B, nu).empty());
    CHECK(!control_limits_complaint<T>(2, idx.data(), nullptr, B, nu, true, false).empty());      // the getter's lim has to be there too
    CHECK(control_limits_complaint<T>(2, idx.data(), nullptr, B, nu, false).empty());             // the clear call has none
    std::vector<int> out_of = {0, B}, neg = {-1, 2}, twice = {2, 2};
    for (const std::vector<int>* bad : {&out_of, &neg, &twice}) {
        CHECK(!control_limits_complaint<T>(2, bad->data(), lim.data(), B, nu).empty());
        CHECK(!control_limits_complaint<T>(2, bad->data(), lim.data(), B, nu, true, false).empty());
        CHECK(!control_limits_complaint<T>(2, bad->data(), nullptr, B, nu, false).empty());
    }
    for (size_t e : {(size_t)0, (size_t)len - 1, (size_t)len, 2 * (size_t)len - 1}) {      // first and last number of both rows
        std::vector<double> l = lim;
        l[e] = std::numeric_limits<double>::quiet_NaN();
        CHECK(!control_limits_complaint<T>(2, idx.data(), l.data(), B, nu).empty());
        CHECK(control_limits_complaint<T>(2, idx.data(), l.data(), B, nu, true, false).empty());      // (the getter does not look at lim's contents)
        if (e >= (size_t)len) CHECK(control_limits_complaint<T>(1, idx.data(), l.data(), B, nu).empty());      // (only count rows are read)
        l = lim;
        l[e] = (e % len) < (size_t)nu ? -inf : inf;              // no bound on that side: legal
        CHECK(control_limits_complaint<T>(2, idx.data(), l.data(), B, nu).empty());
        l[e] = (e % len) < (size_t)nu ? inf : -inf;              // lo = +inf or hi = -inf: an empty box
        CHECK(!control_limits_complaint<T>(2, idx.data(), l.data(), B, nu).empty());
    }
    {   // lo >= hi, as given and after rounding: 1 and 1 + 2^-40 are two doubles and one float
        std::vector<double> l = lim;
        l[0] = l[nu] = 0.25; CHECK(!control_limits_complaint<T>(2, idx.data(), l.data(), B, nu).empty());
        l[0] = 0.5; CHECK(!control_limits_complaint<T>(2, idx.data(), l.data(), B, nu).empty());
        l[0] = 1.0; l[nu] = 1.0 + std::ldexp(1.0, -40);
        CHECK(control_limits_complaint<T>(2, idx.data(), l.data(), B, nu).empty() == (sizeof(T) == 8));
    }
    std::vector<T> rows(2 * (size_t)len), open((size_t)len);
    control_limits_round<T>(rows.data(), lim.data(), 2, nu);
    for (size_t i = 0; i < rows.size(); i++) CHECK(rows[i] == (T)lim[i]);
    control_limits_open_row<T>(open.data(), nu);
    for (int j = 0; j < nu; j++) CHECK(open[j] == -std::numeric_limits<T>::infinity() && open[nu + j] == std::numeric_limits<T>::infinity());
}

int main() {
    for (int nu : {1, 4}) { check<float>(nu); check<double>(nu); }
    std::printf("control_limit_host_check: ok\n");
    return 0;
}
