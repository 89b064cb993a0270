// may_exit_within_two (csrc/solver_state.hpp) held against line_search_accept itself, on the host.
//
// The matrix-core backward pass leaves a problem's interior cost-to-go unwritten only where the rule says the problem cannot exit in this sweep or the next.  Here every
// state of a grid (iter, rho, drho) is run through line_search_accept for EVERY pair of outcomes of two sweeps (accepted / rejected, with tol_cost = 0 and a positive
// cost, the precondition the library checks before it launches a lean pass): whenever one of the four futures ends the problem within two sweeps, the rule must have said
// so.  And the rule must not be vacuous: a fresh problem far from its limits is lean.
#include <cassert>
#include <cstdio>
#include <initializer_list>

#include "solver_state.hpp"

using namespace pddp;

// one sweep's line search with a forced outcome: candidate 0 halves the cost (accepted: the expected reduction is set so that z = 1) or no candidate lowers it (rejected)
template <typename T>
static void sweep(SolverState<T>& st, const SolverParams& sp, bool accept) {
    Dims dm{}; dm.N = 8; dm.M = 1; dm.A = 1; dm.NB = 8;
    T alpha[1] = {T(1)}, J[1], dmax[1] = {T(0)}, dJexp[2], Jout[64] = {}; int alphaOut[64] = {};
    J[0] = accept ? st.prevJ / T(2) : st.prevJ * T(2);
    dJexp[0] = st.prevJ / T(2); dJexp[1] = T(0);
    line_search_accept<T>(st, sp, dm, 0, alpha, J, dmax, dJexp, Jout, alphaOut);
}

template <typename T>
static void check(int ignore_max_rho_exit) {
    SolverParams sp{};
    sp.max_iter = 12; sp.out_stride = 64; sp.ignore_max_rho_exit = ignore_max_rho_exit; sp.tol_cost = 0.0;
    sp.exp_red_min = 0.05; sp.exp_red_max = 1.25; sp.max_defect = 1.0; sp.rho_init = 12.5;
    const int flags = kMxLeanIfRunning | (ignore_max_rho_exit ? 0 : kMxMaxRhoExit) | lean_flags_max_iter(sp.max_iter);
    long lean = 0, kept = 0, exits = 0;
    for (int iter = 1; iter <= sp.max_iter; iter++)
        for (double rho = kRhoMin; rho <= kRhoMax * 1.0001; rho *= 1.19)
            for (double drho : {1.0 / 3.0, 0.64, 0.8, 1.0, 1.25, 1.5625, 2.44140625, 5.0}) {
                SolverState<T> s0{};
                s0.rho = T(rho > kRhoMax ? kRhoMax : rho); s0.drho = T(drho); s0.prevJ = T(100); s0.iter = iter; s0.accepted = 1;
                const bool says = may_exit_within_two(s0, flags);
                bool ends = false;
                for (int o = 0; o < 4; o++) {
                    SolverState<T> s = s0;
                    sweep(s, sp, (o & 1) != 0);
                    if (!s.done) sweep(s, sp, (o & 2) != 0);
                    ends |= s.done != 0;
                }
                exits += ends;
                if (ends) assert(says && "a problem that can exit within two sweeps must keep its interior cost-to-go");
                (says ? kept : lean)++;
            }
    assert(lean > 0 && exits > 0);
    // the benchmark's situation: a fresh problem, the default limits
    SolverState<T> fresh{};
    fresh.rho = T(12.5); fresh.drho = T(1); fresh.prevJ = T(100); fresh.iter = 1;
    assert(!may_exit_within_two(fresh, kMxLeanIfRunning | lean_flags_max_iter(100)));
    assert(may_exit_within_two(fresh, kMxLeanIfRunning | lean_flags_max_iter(2)));
    assert(lean_flags_max_iter(1 << 30) >> kMxMaxIterShift == (1 << 22) - 1);
    std::printf("%s ignore_max_rho_exit=%d: %ld states lean, %ld kept, %ld can exit within two sweeps\n", sizeof(T) == 4 ? "float" : "double", ignore_max_rho_exit, lean, kept, exits);
}

int main() {
    check<float>(0); check<float>(1); check<double>(0); check<double>(1);
    std::printf("ctg_lean_rule_host_check ok\n");
    return 0;
}
