// Control cycles of named slots (pddp_mpc_solve_problems / pddp_mpc_load_problems): what travels between a slot of the handle and a problem of its intake area.
//
// The cycle of a chunk of named slots runs on the intake area (solver_impl.hpp mpc_problems): IN -- every per-problem array of slot idx[i] goes to intake problem i
// (k_slots_scatter, to_compact = 1) --, the intake runs the load stage and the cycle as a handle of n problems, OUT -- every array goes back (to_compact = 0).
// Copies only, nothing zeroed: a warm start lives on what the slot holds.  There are more arrays than one SlotTable has entries, so each direction is a short list of
// tables, one launch each.
//   in and out   the solver state, derivatives ([A B] in both layouts where the compact one exists), sweep operands, candidates (and their knot-major records / segment
//                maps where the family keeps them), line-search inputs, observables
//   in only      what a cycle reads and never writes: xTarget, the slot's row of the cost table, its goal trajectory and flag, its time step, its control reference and flag
//   out only     what the load stage writes whole before anything reads it: du, dmax, err, the fall-back copies, xGoal, tshift; the cycle's inputs as the arrays
//                "xActual" / "shift" / "mpc_in" show them after a whole-handle call; and the previous solution the load stage shifts -- both halves of xb, u, d, the
//                cost-to-go double buffer, the gains --, which does not go in through the movers at all: k_mpc_load_slots (kernels.hpp) reads it from the slot while
//                it shifts
// Host code only (tests/native/mpc_slots_host_check.cpp replays the tables on exactly-sized host buffers).
#pragma once
#include <vector>

#include "slots.hpp"
#include "solver_state.hpp"

namespace pddp {

template <typename T> struct MpcBuffers;      // mpc.hpp

template <typename T>
struct MpcSlotSide {                 // one side (handle or intake area) of the arrays that are not part of Buffers / MpcBuffers
    T* cwt_rows;                     // the cost table, or null (both sides or neither)
    T *xActual, *goal_in; int* shift;      // the three runs of "mpc_in"
    T* gtab; int* gflag;             // the goal trajectories [.][N][NX] and their flags, or null (both sides or neither)
    T* dtab = nullptr;               // the per-problem time steps [.], or null (both sides or neither)
    T* utab = nullptr; int* uflag = nullptr;      // the control references [.][N][NU] (row 0 of problem 0: behind the side's own zero row) and their flags, or null (both sides or neither)
};

template <int NX, int NU, typename T>
bool mpc_slot_tables(std::vector<SlotTable>& in_t, std::vector<SlotTable>& out_t, const Buffers<T>& ib, const MpcBuffers<T>& imb, const MpcSlotSide<T>& is,
                     const Buffers<T>& b, const MpcBuffers<T>& mb, const MpcSlotSide<T>& hs, int Nk, int Mk, int Ak, int max_iter, int ee_cost, int cwt_rec = 0) {      // cwt_rec: numbers per row of the cost table; 0: the arm's record of its cost family
    constexpr size_t NM = NX + NU;
    const size_t N = Nk, M = Mk, A = Ak, out = (size_t)max_iter + 2, e = sizeof(T);
    bool ok = true;
    auto room = [&](std::vector<SlotTable>& v, int need) -> SlotTable& {
        if (v.empty() || v.back().n + need > kSlotMaxDesc) { v.emplace_back(); SlotTable& t = v.back(); t.n = 0; t.N = Nk; t.state = nullptr; t.state_stride = t.off_cur = t.off_alpha = 0; }
        return v.back();
    };
    auto add = [&](int dir, const void* c, void* s, size_t bytes) {
        if (dir & 1) ok = ok && slot_add(room(in_t, 1), c, s, bytes, bytes, bytes, kSlotCopy);
        if (dir & 2) ok = ok && slot_add(room(out_t, 1), c, s, bytes, bytes, bytes, kSlotCopy);
    };
    add(3, ib.state, b.state, sizeof(SolverState<T>));
    const int prev = 2;                  // read from the slot by the gathering load kernel
    add(prev, ib.xb, b.xb, 2 * N * NX * e); add(prev, ib.ucur, b.ucur, N * NU * e); add(prev, ib.dcur, b.dcur, N * NX * e);
    add(prev, ib.P, b.P, N * NX * NX * e); add(prev, ib.Pp, b.Pp, N * NX * NX * e); add(prev, ib.p, b.p, N * NX * e); add(prev, ib.pp, b.pp, N * NX * e);
    add(prev, ib.KT, b.KT, N * NX * NU * e); add(2, ib.du, b.du, N * NU * e);
    add(2, imb.x_old, mb.x_old, N * NX * e); add(2, imb.u_old, mb.u_old, N * NU * e); add(2, imb.KT_old, mb.KT_old, N * NX * NU * e);
    add(3, ib.AB, b.AB, N * NX * NM * e);
    if (b.ABc) { ok = ok && slot_add_abc(room(in_t, 3), ib.ABc, b.ABc, Nk, e); ok = ok && slot_add_abc(room(out_t, 3), ib.ABc, b.ABc, Nk, e); }
    add(3, ib.H, b.H, N * NM * NM * e); add(3, ib.g, b.g, N * NM * e);
    if (b.Hc) add(3, ib.Hc, b.Hc, N * 49 * e);
    add(3, ib.ApBK, b.ApBK, N * NX * NX * e); add(3, ib.Bdu, b.Bdu, N * NX * e);
    add(3, ib.xs, b.xs, A * N * NX * e); add(3, ib.us, b.us, A * N * NU * e); add(3, ib.ds, b.ds, A * N * NX * e);
    if (b.xw) add(3, ib.xw, b.xw, N * A * (size_t)b.xw_rec * e);
    if (b.segmap) add(3, ib.segmap, b.segmap, M * 256 * e);
    add(3, ib.J, b.J, A * e); add(2, ib.dmax, b.dmax, A * e); add(3, ib.dJexp, b.dJexp, 2 * M * e); add(2, ib.err, b.err, M * sizeof(int));
    add(3, ib.Jpart, b.Jpart, A * M * e); add(3, ib.dpart, b.dpart, A * M * e); add(3, ib.parts_fresh, b.parts_fresh, sizeof(int));
    add(2, ib.xGoal, b.xGoal, NX * e); add(2, ib.tshift, b.tshift, sizeof(int)); add(3, ib.costk, b.costk, N * e);
    add(3, ib.Jout, b.Jout, out * e); add(3, ib.alphaOut, b.alphaOut, out * sizeof(int));
    add(1, ib.xTarget, b.xTarget, NX * e);
    if (hs.cwt_rows) add(1, is.cwt_rows, hs.cwt_rows, (cwt_rec ? cwt_rec : cost_record_len(ee_cost)) * e);
    if (hs.gtab) { add(1, is.gtab, hs.gtab, N * NX * e); add(1, is.gflag, hs.gflag, sizeof(int)); }      // in only: a cycle does not change a trajectory
    if (hs.dtab) add(1, is.dtab, hs.dtab, e);                                                            // in only: nor its slot's time step
    if (hs.utab) { add(1, is.utab, hs.utab, N * NU * e); add(1, is.uflag, hs.uflag, sizeof(int)); }      // in only: nor its control reference
    add(2, is.xActual, hs.xActual, NX * e); add(2, is.goal_in, hs.goal_in, NX * e); add(2, is.shift, hs.shift, sizeof(int));
    return ok;
}

}  // namespace pddp
