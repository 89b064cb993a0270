// Per-problem cost weights of the KUKA arm: pddp_set_cost_problems / pddp_get_cost_problems.
//
// A handle keeps ONE CostWeights record, a kernel argument (plants.hpp).  The first pddp_set_cost_problems gives it a device table [batch][record] in the handle's
// element type and points Buffers::cwt at it; the kernels then take every problem's weights from its row (cost_weights_at).  This header is the host part, plain C++:
// what a list of records has to satisfy, the handle-wide record as a row, and the packing of double records into rows of the element type -- one rounding, here and
// nowhere else.  tests/native/cost_table_host_check.cpp runs it without a GPU.
#pragma once
#include <cmath>
#include <string>

#include "plants.hpp"
#include "slots.hpp"

namespace pddp {

// "" or the complaint about the arguments of pddp_set_cost_problems (w non-null) / pddp_get_cost_problems (w not looked at: check_w = false)
inline std::string cost_records_complaint(int count, const int* idx, const double* w, int batch, int rec, bool check_w = true) {
    const std::string c = slots_complaint(count, idx, batch);      // count >= 1, idx non-null, every index inside [0, batch), none twice
    if (!c.empty()) return c;
    if (!w) return "w is NULL";
    if (check_w)
        for (size_t i = 0; i < (size_t)count * rec; i++)
            if (!std::isfinite(w[i])) return "w[" + std::to_string(i / rec) + "][" + std::to_string(i % rec) + "] is not finite";
    return "";
}

// the handle-wide record as one row of the table (the argument order of pddp_set_cost / pddp_set_cost_ee)
template <typename T>
inline void cost_record_of(const CostWeights<T>& cw, T* row) {
    if (cw.ee) { row[0] = cw.Q_EE1; row[1] = cw.Q_EE2; row[2] = cw.QF_EE1; row[3] = cw.QF_EE2; row[4] = cw.R_EE; row[5] = cw.Q_xEE; row[6] = cw.QF_xEE; row[7] = cw.Q_xdEE; row[8] = cw.QF_xdEE; }
    else { row[0] = cw.Q1; row[1] = cw.Q2; row[2] = cw.R; row[3] = cw.QF1; row[4] = cw.QF2; }
}

// `count` records of doubles -> rows of the element type: each number rounded once, as cost_weights_of rounds the configuration's
template <typename T>
inline void cost_records_pack(int count, int rec, const double* w, T* rows) {
    for (size_t i = 0; i < (size_t)count * rec; i++) rows[i] = (T)w[i];
}

}  // namespace pddp
