// Stand-alone host program over the host side of pddp_simulate_problems (csrc/sim_slots.hpp): every refusal of include/pddp.h, the knot spacing of a given horizon time
// held against step_us (csrc/handle_setup.hpp) of a configuration with that total_time, the fill of the per-entry records (csrc/sim.hpp PlantSimSlotIn) for duplicate
// and out-of-order indices on exactly-sized buffers, and the family choice for every plant.  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc sim_slots_host_check.cpp -o sim_slots_host_check && ./sim_slots_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "handle_setup.hpp"
#include "sim.hpp"
#include "sim_slots.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

template <typename T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

struct Args {                                                   // one call's arguments, every array exactly sized: a read past `count` entries is the sanitizer's
    std::vector<int> idx{3, 0, 3};
    std::vector<double> t0{0.0, 250.0, -16129.5}, el{1000.0, 0.0, 31.25};
    std::vector<int> sub{4, 7, 40};
    int plan = 1, state = 1;                                    // stand-ins for non-null plan / state pointers (the checks do not read through them)
    int count = 3, family = 0, plant = 3, batch = 5;
    bool loaded = true, px = true, pu = true, pk = true, has_idx = true, has_t0 = true, has_el = true, has_sub = true, has_xa = true;
    std::string complaint() const {
        return sim_slots_complaint(count, has_idx ? idx.data() : nullptr, px ? &plan : nullptr, pu ? &plan : nullptr, pk ? &plan : nullptr, has_t0 ? t0.data() : nullptr,
                                   has_el ? el.data() : nullptr, has_sub ? sub.data() : nullptr, has_xa ? &state : nullptr, family, plant, batch, loaded);
    }
};

// every refusal, and what is accepted
static void check_complaints() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(Args().complaint().empty());
    { Args a; a.px = a.pu = a.pk = false; CHECK(a.complaint().empty()); }                        // the solutions the slots hold
    { Args a; a.idx = {4, 4, 4}; CHECK(a.complaint().empty()); }                                  // a slot may be named more than once; the last slot is inside
    { Args a; a.count = 1; CHECK(a.complaint().empty()); }
    for (int c : {0, -1}) { Args a; a.count = c; CHECK(!a.complaint().empty()); }
    { Args a; a.has_idx = false; CHECK(!a.complaint().empty()); }
    { Args a; a.has_t0 = false; CHECK(!a.complaint().empty()); }
    { Args a; a.has_el = false; CHECK(!a.complaint().empty()); }
    { Args a; a.has_sub = false; CHECK(!a.complaint().empty()); }
    { Args a; a.has_xa = false; CHECK(!a.complaint().empty()); }
    for (int e = 0; e < 3; e++) {
        for (int v : {-1, 5, 1 << 30}) { Args a; a.idx[e] = v; CHECK(!a.complaint().empty()); if (e == 2) { a.count = 2; CHECK(a.complaint().empty()); } }     // (only count entries are read)
        for (int v : {0, -3}) { Args a; a.sub[e] = v; CHECK(!a.complaint().empty()); }
        for (double v : {-1.0, -1e-300, nan, -inf}) { Args a; a.el[e] = v; CHECK(!a.complaint().empty()); }
        { Args a; a.el[e] = inf; CHECK(a.complaint().empty()); }                                  // (>= 0: such an entry leaves its plan and aborts on the device)
        for (double v : {nan, inf, -inf}) { Args a; a.t0[e] = v; CHECK(!a.complaint().empty()); }
    }
    for (int f : {-1, 3, 64}) { Args a; a.family = f; CHECK(!a.complaint().empty()); }
    for (int plant = 1; plant <= 5; plant++) {
        for (int f = 0; f <= 2; f++) { Args a; a.plant = plant; a.family = f; CHECK(a.complaint().empty() == !(f == 2 && plant >= 4)); }
    }
    // a mixture of NULL and non-NULL plans, in every combination
    for (int m = 1; m < 7; m++) { Args a; a.px = m & 1; a.pu = m & 2; a.pk = m & 4; CHECK(!a.complaint().empty()); }
    // NULL plans need a loaded handle; host plans do not
    { Args a; a.loaded = false; CHECK(a.complaint().empty()); a.px = a.pu = a.pk = false; CHECK(!a.complaint().empty()); }
}

// the spacing of a slot given t is step_us of a configuration with that total_time, bit for bit
static void check_spacing() {
    for (int plant : {1, 2, 3}) {
        for (int N : {4, 16, 32, 128, 1024}) {
            pddp_config c;
            default_config(&c, plant);
            c.N = N;
            CHECK(same_bits(step_us(c.total_time, N), step_us(c)));
            unsigned s = 7u + (unsigned)N;
            for (int trial = 0; trial < 200; trial++) {
                s = s * 1664525u + 1013904223u;
                static const double ladder[6] = {1.0, 0.6, 1.37, 0.8, 1.5, 0.11};
                const double t = trial < 6 ? (N / 32.0) * ladder[trial] : 1e-3 + 20.0 * ((double)(s >> 8) / 16777216.0);
                c.total_time = t;
                CHECK(same_bits(step_us(t, N), step_us(c)));
                CHECK(same_bits(step_us(t, N), t / (N - 1) * 1000.0 * 1000.0));
            }
        }
    }
}

// entry i of the records is slot idx[i] in the caller's order, duplicates included, with that slot's spacing
template <template <typename> class PT, typename T> static void check_fill() {
    using PD = PT<double>;
    using In = PlantSimSlotIn<PD, T>;
    using Out = PlantSimBatchOut<PD, T>;
    constexpr int NX = PD::NX;
    const int B = 5, N = 16;
    const std::vector<double> times = {0.5, 0.3, 0.685, 0.4, 0.055};        // the host mirror of a step table
    const std::vector<int> idx = {4, 1, 4, 0, 3, 1, 4};
    const int count = (int)idx.size();
    CHECK((int)times.size() == B && count > B);
    std::vector<double> t0(count), el(count);
    std::vector<int> sub(count);
    std::vector<T> goal((size_t)count * 3), xa((size_t)count * NX);
    for (int i = 0; i < count; i++) {
        t0[i] = 100.0 * i - 7.5; el[i] = 1000.0 + i; sub[i] = 4 + 3 * i;
        for (int c = 0; c < 3; c++) goal[3 * i + c] = (T)(0.1 * i + c);
        for (int c = 0; c < NX; c++) xa[(size_t)i * NX + c] = (T)(i + 0.01 * c);
    }
    const SimSlotsLayout lay = sim_slots_layout((size_t)count, sizeof(In), sizeof(Out));
    CHECK(lay.in_bytes % 16 == 0 && lay.in_bytes >= count * sizeof(In) && lay.in_bytes < count * sizeof(In) + 16 && lay.rec_bytes == lay.in_bytes + count * sizeof(Out));
    std::vector<In> rec((size_t)count);                                       // exactly sized
    for (int with_goal = 0; with_goal < 2; with_goal++) {
        for (int tab = 0; tab < 2; tab++) {
            std::memset((void*)rec.data(), 0xff, rec.size() * sizeof(In));
            sim_slots_fill<In, T>(rec.data(), count, idx.data(), t0.data(), el.data(), sub.data(), with_goal ? goal.data() : nullptr, xa.data(), NX,
                                  [&](int q) { return step_us(tab ? times[(size_t)q] : 0.5, N); });
            for (int i = 0; i < count; i++) {
                const In& r = rec[i];
                CHECK(r.slot == idx[i] && r.substeps == sub[i] && same_bits(r.t0_us, t0[i]) && same_bits(r.elapsed_us, el[i]));
                CHECK(same_bits(r.step_us, step_us(tab ? times[(size_t)idx[i]] : 0.5, N)));
                for (int c = 0; c < 3; c++) CHECK(same_bits(r.goal[c], with_goal ? goal[3 * i + c] : T(0)));
                CHECK(std::memcmp(r.x, xa.data() + (size_t)i * NX, NX * sizeof(T)) == 0);
            }
            if (tab) CHECK(same_bits(rec[0].step_us, rec[2].step_us) && same_bits(rec[0].step_us, rec[6].step_us) && !same_bits(rec[0].step_us, rec[1].step_us));
        }
    }
    const PlantSimBatchIn<PD, T>& base = rec[1];                               // the body takes the batched record: the same leading fields
    CHECK(same_bits(base.t0_us, t0[1]) && same_bits(base.x[NX - 1], xa[(size_t)1 * NX + NX - 1]));
}

// the family a call runs on: forced values as given; the library's choice never leaves the wave family on plants 4 and 5 and follows the count threshold elsewhere
static void check_family() {
    const int counts[] = {1, 63, 64, 65, 256, 1024, 4096, 16384, 1 << 20};
    for (int plant = 1; plant <= 5; plant++) {
        for (int f64 = 0; f64 < 2; f64++) {
            const int thr = sim_ts_threshold(plant, f64 != 0);
            CHECK(thr >= 1);
            if (plant >= 4) CHECK(thr == kSimTsNever);
            for (int count : counts) {
                CHECK(sim_slots_family(kSimFamilyWave, plant, f64 != 0, count) == kSimFamilyWave);
                if (plant <= 3) CHECK(sim_slots_family(kSimFamilyThread, plant, f64 != 0, count) == kSimFamilyThread);
                const int chosen = sim_slots_family(kSimFamilyAuto, plant, f64 != 0, count);
                CHECK(chosen == ((plant <= 3 && count >= thr) ? kSimFamilyThread : kSimFamilyWave));
                if (plant >= 4) CHECK(chosen == kSimFamilyWave);
            }
            if (thr != kSimTsNever) {                            // the threshold itself is the first count on the thread family
                CHECK(sim_slots_family(kSimFamilyAuto, plant, f64 != 0, thr) == kSimFamilyThread);
                if (thr > 1) CHECK(sim_slots_family(kSimFamilyAuto, plant, f64 != 0, thr - 1) == kSimFamilyWave);
            }
        }
    }
}

int main() {
    check_complaints();
    check_spacing();
    check_fill<PendPlant, float>(); check_fill<PendPlant, double>();
    check_fill<CartPlant, float>(); check_fill<CartPlant, double>();
    check_fill<QuadPlant, float>(); check_fill<QuadPlant, double>();
    check_family();
    std::printf("sim_slots_host_check: ok\n");
    return 0;
}
