// TEST TOOL -- NOT PRODUCT CODE.  The oracle's plant 5 as "plant 1, 2 or 3 with a run-time diagonal cost and a per-knot goal trajectory": an independent reference for
// pddp_set_goal_trajectory_problems.  Modelled on tests/plugin_diag/diag_shim.cpp:
//   dynamics / dynamics_gradient   forward to the oracle's own ora_dynamics_* / ora_dynamics_gradient_* with a stored configuration of plant 1, 2 or 3
//                                  (function pointers handed in by the test, which has the oracle loaded);
//   cost_func / cost_grad          are the diagonal formulas of include/pddp.h with a record the test sets, the goal taken from a table G[N][n] at the knot index k the
//                                  oracle passes -- the ABSOLUTE knot of the horizon -- when the test has set a table, and the routine's own xg argument when it has not.
// The plug-in signature carries no horizon length: the test sets it with the record.  Shares nothing with the library under test.
//   g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off goal_traj_shim.cpp
#include <math.h>

#include <vector>

#include "../../oracle/oracle.h"

namespace {
struct State {
    ora_cfg cfg;               // plant 1, 2 or 3: whose dynamics the plug-in forwards to
    int n = 0, m = 0, N = 0;
    double rec[2 * 14 + 7];    // [q | r | qf]
    bool has_table = false;
    std::vector<double> G;     // [N][n] (the values the solve's element type holds: the test rounds them)
    void* dyn32 = nullptr; void* grad32 = nullptr; void* dyn64 = nullptr; void* grad64 = nullptr;
} st;

template <typename T> struct Fn;
template <> struct Fn<float> { static void* dyn() { return st.dyn32; } static void* grad() { return st.grad32; } };
template <> struct Fn<double> { static void* dyn() { return st.dyn64; } static void* grad() { return st.grad64; } };

template <typename T> void dyn(T* qdd, const T* x, const T* u) {
    reinterpret_cast<void (*)(const ora_cfg*, T*, const T*, const T*)>(Fn<T>::dyn())(&st.cfg, qdd, x, u);
}
template <typename T> void grad(T* dqdd, T* qdd, const T* x, const T* u) {
    reinterpret_cast<void (*)(const ora_cfg*, T*, T*, const T*, const T*)>(Fn<T>::grad())(&st.cfg, dqdd, qdd, x, u);
}
// entry i of the goal of knot k
template <typename T> T goal(const T* xg, int k, int i) { return st.has_table ? (T)st.G[(size_t)k * st.n + i] : xg[i]; }
template <typename T> T cost(const T* xk, const T* uk, const T* xg, int k, T, T, T, T, T) {
    const int n = st.n, m = st.m;
    const bool fin = k == st.N - 1;
    T c = 0.0;
    for (int i = 0; i < n; i++) c += (T)(fin ? st.rec[n + m + i] : st.rec[i]) * pow(xk[i] - goal<T>(xg, k, i), 2);
    if (!fin) for (int j = 0; j < m; j++) c += (T)st.rec[n + j] * pow(uk[j], 2);
    return 0.5 * c;
}
template <typename T> void cgrad(T* Hk, T* gk, const T* xk, const T* uk, const T* xg, int k, int ld, T, T, T, T, T) {
    const int n = st.n, m = st.m;
    const bool fin = k == st.N - 1;
    for (int i = 0; i < n + m; i++) for (int j = 0; j < n + m; j++)
        Hk[i * ld + j] = (T)(i != j ? 0.0 : (fin ? (i < n ? st.rec[n + m + i] : 0.0) : st.rec[i]));
    for (int i = 0; i < n; i++) gk[i] = (T)(fin ? st.rec[n + m + i] : st.rec[i]) * (xk[i] - goal<T>(xg, k, i));
    for (int j = 0; j < m; j++) gk[n + j] = (T)(fin ? 0.0 : st.rec[n + j]) * uk[j];
}
ora_plugin_f32 p32;
ora_plugin_f64 p64;
}  // namespace

// plant_cfg: a configuration of plant 1, 2 or 3; N: the horizon of the solves that follow; rec: 2 n + m doubles; G: N n doubles or null (no table: the cost routines
// use their xg argument); the four oracle entry points by address
extern "C" void goal_traj_shim_set(const ora_cfg* plant_cfg, int n, int m, int N, const double* rec, const double* G, void* dyn32, void* grad32, void* dyn64, void* grad64) {
    st.cfg = *plant_cfg; st.n = n; st.m = m; st.N = N;
    for (int i = 0; i < 2 * n + m; i++) st.rec[i] = rec[i];
    st.has_table = G != nullptr;
    st.G.assign(G ? G : nullptr, G ? G + (size_t)N * n : nullptr);
    st.dyn32 = dyn32; st.grad32 = grad32; st.dyn64 = dyn64; st.grad64 = grad64;
    p32 = {n / 2, m, dyn<float>, grad<float>, cost<float>, cgrad<float>};
    p64 = {n / 2, m, dyn<double>, grad<double>, cost<double>, cgrad<double>};
}
extern "C" const ora_plugin_f32* plugin_f32(void) { return &p32; }
extern "C" const ora_plugin_f64* plugin_f64(void) { return &p64; }
