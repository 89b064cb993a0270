// The simulated robots of named slots (pddp_simulate_problems): what the arguments have to satisfy, how the per-entry records are laid out and filled, and which of
// the two kernel families a call runs on.
//
// Entry i of a call is the robot of slot idx[i].  Everything that differs per entry travels in ONE packed input record (sim.hpp PlantSimSlotIn: the measured state,
// t0, the elapsed time, the goal, and -- what pddp_simulate_batch takes once per launch -- the slot, the sub-step count and the knot spacing of the slot's own horizon
// time), so the kernels read no table and the call costs what `count` costs, not what `batch` costs.  The call only READS slots: an index may be named more than once
// (one plan under many start states), which the calls that write slots refuse (slots.hpp slots_complaint).
//   family 1 (k_plant_sim_slots): one wavefront per entry, every plant
//   family 2 (k_plant_sim_ts)   : one THREAD per entry, the same body under a one-lane wave, pendulum / cart-pole / quadrotor only
//   family 0                    : the library's choice -- sim_slots_family below, thresholds measured in profiles/sim_problems.md
// Host code only, no HIP header: the library (solver_impl.hpp) and tests/native/sim_slots_host_check.cpp both include it.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>

namespace pddp {

enum SimFamily : int { kSimFamilyAuto = 0, kSimFamilyWave = 1, kSimFamilyThread = 2 };

// "" or the complaint about the arguments of pddp_simulate_problems (answered as PDDP_EINVAL, the handle unchanged).  plant: 1..5; loaded: pddp_load / pddp_solve
// filled the handle (a device-resident plan exists)
inline std::string sim_slots_complaint(int count, const int* idx, const void* x, const void* u, const void* KT, const double* t0_us, const double* elapsed_us,
                                       const int* substeps, const void* xActual, int family, int plant, int batch, bool loaded) {
    if (count < 1) return "count must be >= 1";
    if (!idx) return "idx is NULL";
    if (!t0_us) return "t0_us is NULL";
    if (!elapsed_us) return "elapsed_us is NULL";
    if (!substeps) return "substeps is NULL";
    if (!xActual) return "xActual_inout is NULL";
    if (family < kSimFamilyAuto || family > kSimFamilyThread) return "family must be 0 (the library's choice), 1 (a wavefront per problem) or 2 (a thread per problem)";
    if (family == kSimFamilyThread && !(plant >= 1 && plant <= 3))
        return "family 2 (a thread per problem) belongs to the pendulum, cart-pole and quadrotor (plants 1-3); the arm and plug-in plants run a wavefront per problem";
    if ((x != nullptr) != (u != nullptr) || (x != nullptr) != (KT != nullptr)) return "x, u and KT are either all given (host plans) or all NULL (the solutions the slots hold)";
    if (!x && !loaded) return "x, u and KT are NULL, but the handle has never been loaded (pddp_load / pddp_solve): its slots hold no solution to follow";
    for (int i = 0; i < count; i++) {
        if (idx[i] < 0 || idx[i] >= batch) return "idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is outside [0, batch = " + std::to_string(batch) + ")";
        if (substeps[i] < 1) return "substeps[" + std::to_string(i) + "] must be >= 1";
        if (!(elapsed_us[i] >= 0)) return "elapsed_us[" + std::to_string(i) + "] must be >= 0";
        if (!std::isfinite(t0_us[i])) return "t0_us[" + std::to_string(i) + "] must be finite";
    }
    return "";
}

// ---- the library's choice.  The thread family pays off from some number of entries on, per plant and element type: the smallest measured count from which it stays
// faster than the wave family by more than the run-to-run spread of the two rows compared (tools/sim_problems_time.py on one MI355X, 150 sub-steps, device-resident
// plans: profiles/sim_problems.md holds the table, the spread and these values).  kSimTsNever: it never did, family 0 never picks it there.
constexpr int kSimTsNever = INT_MAX;
inline int sim_ts_threshold(int plant, bool f64) {
    switch (plant) {                                   // profiles/sim_problems.md, "chosen thresholds": the thread family was faster at EVERY measured count, 1 included
    case 1: return f64 ? 1 : 1;                        // (a wavefront's lanes buy a 2- to 12-state robot nothing, and its stage boundaries cost; one lane runs the same
    case 2: return f64 ? 1 : 1;                        //  serial sub-steps without them)
    case 3: return f64 ? 1 : 1;
    }
    return kSimTsNever;                                // the arm and plug-in plants have no thread family
}
// the family a call runs on: kSimFamilyWave or kSimFamilyThread (family and plant as accepted by sim_slots_complaint)
inline int sim_slots_family(int family, int plant, bool f64, int count) {
    if (family == kSimFamilyWave || family == kSimFamilyThread) return family;
    return (plant >= 1 && plant <= 3 && count >= sim_ts_threshold(plant, f64)) ? kSimFamilyThread : kSimFamilyWave;
}

// ---- the records of one call: `count` input records, then (from a 16-byte boundary) `count` output records, the same on the device and in pinned memory
struct SimSlotsLayout { size_t in_bytes, rec_bytes; };
inline SimSlotsLayout sim_slots_layout(size_t count, size_t in_size, size_t out_size) {
    SimSlotsLayout l;
    l.in_bytes = (count * in_size + 15) / 16 * 16;
    l.rec_bytes = l.in_bytes + count * out_size;
    return l;
}
// fills rec[0 .. count): entry i is slot idx[i] in the caller's order, duplicates included.  goal [count][3] or null (zeros), xActual [count][NX];
// spacing_us(slot) = the knot spacing of that slot's horizon time in microseconds (handle_setup.hpp step_us(total_time, N))
template <typename In, typename T, typename Spacing>
inline void sim_slots_fill(In* rec, int count, const int* idx, const double* t0_us, const double* elapsed_us, const int* substeps, const T* goal, const T* xActual,
                           int NX, Spacing&& spacing_us) {
    for (int i = 0; i < count; i++) {
        In& r = rec[i];
        r.t0_us = t0_us[i]; r.elapsed_us = elapsed_us[i];
        for (int c = 0; c < 3; c++) r.goal[c] = goal ? goal[3 * (size_t)i + c] : T(0);
        std::memcpy(r.x, xActual + (size_t)i * NX, (size_t)NX * sizeof(T));
        r.slot = idx[i]; r.substeps = substeps[i]; r.step_us = spacing_us(idx[i]);
    }
}

}  // namespace pddp
