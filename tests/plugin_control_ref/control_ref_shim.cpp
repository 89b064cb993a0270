// TEST TOOL -- NOT PRODUCT CODE.  The oracle's plant 5 as "plant 1, 2 or 3 with a run-time diagonal cost, a per-knot goal trajectory and a control reference": an
// independent reference for pddp_set_control_reference_problems.  tests/plugin_goal_traj/goal_traj_shim.cpp with the control term taken on u_k - U[k]:
//   dynamics / dynamics_gradient   forward to the oracle's own ora_dynamics_* / ora_dynamics_gradient_* with a stored configuration of plant 1, 2 or 3
//                                  (function pointers handed in by the test, which has the oracle loaded);
//   cost_func / cost_grad          are the diagonal formulas of include/pddp.h with a record the test sets; the goal comes from a table G[N][n] and the control
//                                  reference from a table U[N][m], both at the knot index k the oracle passes -- the ABSOLUTE knot of the horizon -- when the test has
//                                  set them; without G the routine's own xg argument, without U zero.  The final knot has no control term and reads no row of U.
// The plug-in signature carries no horizon length: the test sets it with the record.  Shares nothing with the library under test.
//   g++ -O2 -std=c++17 -fPIC -shared -ffp-contract=off control_ref_shim.cpp
#include <math.h>

#include <vector>

#include "../../oracle/oracle.h"

namespace {
struct State {
    ora_cfg cfg;               // plant 1, 2 or 3: whose dynamics the plug-in forwards to
    int n = 0, m = 0, N = 0;
    double rec[2 * 14 + 7];    // [q | r | qf]
    bool has_G = false, has_U = false;
    std::vector<double> G;     // [N][n] (the values the solve's element type holds: the test rounds them)
    std::vector<double> U;     // [N][m] (the same)
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
// entry i of the goal of knot k, entry j of the control reference of knot k
template <typename T> T goal(const T* xg, int k, int i) { return st.has_G ? (T)st.G[(size_t)k * st.n + i] : xg[i]; }
template <typename T> T uref(int k, int j) { return st.has_U ? (T)st.U[(size_t)k * st.m + j] : (T)0; }
template <typename T> T cost(const T* xk, const T* uk, const T* xg, int k, T, T, T, T, T) {
    const int n = st.n, m = st.m;
    const bool fin = k == st.N - 1;
    T c = 0.0;
    for (int i = 0; i < n; i++) c += (T)(fin ? st.rec[n + m + i] : st.rec[i]) * pow(xk[i] - goal<T>(xg, k, i), 2);
    if (!fin) for (int j = 0; j < m; j++) c += (T)st.rec[n + j] * pow(uk[j] - uref<T>(k, j), 2);
    return 0.5 * c;
}
template <typename T> void cgrad(T* Hk, T* gk, const T* xk, const T* uk, const T* xg, int k, int ld, T, T, T, T, T) {
    const int n = st.n, m = st.m;
    const bool fin = k == st.N - 1;
    for (int i = 0; i < n + m; i++) for (int j = 0; j < n + m; j++)
        Hk[i * ld + j] = (T)(i != j ? 0.0 : (fin ? (i < n ? st.rec[n + m + i] : 0.0) : st.rec[i]));
    for (int i = 0; i < n; i++) gk[i] = (T)(fin ? st.rec[n + m + i] : st.rec[i]) * (xk[i] - goal<T>(xg, k, i));
    for (int j = 0; j < m; j++) gk[n + j] = fin ? (T)0.0 * uk[j] : (T)st.rec[n + j] * (uk[j] - uref<T>(k, j));
}
ora_plugin_f32 p32;
ora_plugin_f64 p64;
}  // namespace

// plant_cfg: a configuration of plant 1, 2 or 3; N: the horizon of the solves that follow; rec: 2 n + m doubles; G: N n doubles or null (no table: the cost routines
// use their xg argument); U: N m doubles or null (no reference); the four oracle entry points by address
extern "C" void control_ref_shim_set(const ora_cfg* plant_cfg, int n, int m, int N, const double* rec, const double* G, const double* U, void* dyn32, void* grad32, void* dyn64,
                                     void* grad64) {
    st.cfg = *plant_cfg; st.n = n; st.m = m; st.N = N;
    for (int i = 0; i < 2 * n + m; i++) st.rec[i] = rec[i];
    st.has_G = G != nullptr; st.has_U = U != nullptr;
    st.G.clear(); st.U.clear();
    if (G) st.G.assign(G, G + (size_t)N * n);
    if (U) st.U.assign(U, U + (size_t)N * m);
    st.dyn32 = dyn32; st.grad32 = grad32; st.dyn64 = dyn64; st.grad64 = grad64;
    p32 = {n / 2, m, dyn<float>, grad<float>, cost<float>, cgrad<float>};
    p64 = {n / 2, m, dyn<double>, grad<double>, cost<double>, cgrad<double>};
}
extern "C" const ora_plugin_f32* plugin_f32(void) { return &p32; }
extern "C" const ora_plugin_f64* plugin_f64(void) { return &p64; }
