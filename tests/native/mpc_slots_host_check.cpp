// Stand-alone host program over the host-only part of the control cycles of named slots: the in / out descriptor tables of csrc/mpc_slots.hpp replayed by memcpy on
// exactly-sized host arrays (the compact [A B] with N < 64 and N >= 64), and the gathering shift's addressing (csrc/mpc_move.hpp mpc_shift with separate source and
// destination: shift 0 and shift N-2 included) -- built with -fsanitize=address,undefined, an entry or a shift that reaches past an array is reported.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc mpc_slots_host_check.cpp -o mpc_slots_host_check && ./mpc_slots_host_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mpc_move.hpp"
#include "mpc_slots.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

constexpr int NX = 14, NU = 7, NM = NX + NU;

// one side (handle of `B` problems, or intake area of `B` problems): every array exactly as large as the library allocates it, in 4-byte words
struct Side {
    int B;
    Buffers<float> b{};
    MpcBuffers<float> mb{};
    MpcSlotSide<float> s{};
    struct Arr { const char* name; std::unique_ptr<unsigned[]> mem; size_t per, words; bool abc; };      // per: words per problem (abc: addressed through abc_index)
    std::vector<Arr> arrs;
    template <typename U> void make(const char* name, U*& p, size_t per, size_t words = 0, bool abc = false) {
        static_assert(sizeof(U) % 4 == 0, "whole words");      // (per and words count 4-byte words)
        if (!words) words = per * B;
        arrs.push_back(Arr{name, std::unique_ptr<unsigned[]>(new unsigned[words]), per, words, abc});      // (new[]: exactly-sized, what the sanitizer guards)
        p = reinterpret_cast<U*>(arrs.back().mem.get());
    }
    Side(int B_, int N, int M, int A, int max_iter, bool compact, bool ee, bool table) : B(B_) {
        const size_t out = max_iter + 2;
        make("xs", b.xs, (size_t)A * N * NX); make("us", b.us, (size_t)A * N * NU); make("ds", b.ds, (size_t)A * N * NX);
        make("xb", b.xb, 2 * N * NX); make("ucur", b.ucur, N * NU); make("dcur", b.dcur, N * NX);
        make("P", b.P, N * NX * NX); make("Pp", b.Pp, N * NX * NX); make("p", b.p, N * NX); make("pp", b.pp, N * NX);
        make("AB", b.AB, N * NX * NM); make("H", b.H, N * NM * NM); make("g", b.g, N * NM);
        make("KT", b.KT, N * NX * NU); make("du", b.du, N * NU); make("ApBK", b.ApBK, N * NX * NX); make("Bdu", b.Bdu, N * NX);
        make("J", b.J, A); make("dmax", b.dmax, A); make("dJexp", b.dJexp, 2 * M); make("xGoal", b.xGoal, NX);
        make("Jout", b.Jout, out); make("err", b.err, M); make("alphaOut", b.alphaOut, out); make("state", b.state, sizeof(SolverState<float>) / 4);
        make("x_old", mb.x_old, N * NX); make("u_old", mb.u_old, N * NU); make("KT_old", mb.KT_old, N * NX * NU);
        make("xTarget", b.xTarget, NX); make("costk", b.costk, N); make("tshift", b.tshift, 1);
        make("Jpart", b.Jpart, A * M); make("dpart", b.dpart, A * M); make("parts_fresh", b.parts_fresh, 1);
        if (compact) {
            b.xw_rec = 22; make("xw", b.xw, (size_t)N * A * 22); make("segmap", b.segmap, M * 256);
            make("ABc", b.ABc, (size_t)N * 147, abc_floats((size_t)B * N), true);
            if (ee) make("Hc", b.Hc, N * 49, (size_t)B * N * 49 + 16);
        }
        if (table) make("cwt", s.cwt_rows, cost_record_len(ee));
        make("xActual", s.xActual, NX); make("goal_in", s.goal_in, NX); make("shift", s.shift, 1);
    }
    // word `e` of problem `q` of an array
    unsigned& at(Arr& a, int N, size_t q, size_t e) {
        if (!a.abc) return a.mem[q * a.per + e];
        const size_t k = e / 147, c = (e % 147) / 7, r = e % 7;
        return a.mem[abc_index(q * (size_t)N + k, (int)c, (int)r)];
    }
};
static unsigned code(size_t arr, size_t q, size_t e, unsigned salt) { return (unsigned)(((arr * 131 + q) * 1000003u + e) * 2654435761u + salt); }

static void replay(const std::vector<SlotTable>& ts, const std::vector<int>& idx, bool to_compact) {
    for (const SlotTable& t : ts)
        for (size_t i = 0; i < idx.size(); i++)
            for (int k = 0; k < t.n; k++) {
                const SlotDesc& d = t.d[k];
                CHECK(d.op == kSlotCopy);                                       // copies only: nothing of a warm start is zeroed by the movers
                unsigned char* s = d.slot + (d.abc ? slot_abc_offset(d.abc, (size_t)idx[i], t.N, 4) : (size_t)idx[i] * d.sstride);
                unsigned char* c = d.compact + (d.abc ? slot_abc_offset(d.abc, i, t.N, 4) : i * d.cstride);
                CHECK(d.bytes % d.vec == 0 && (uintptr_t)s % d.vec == 0 && (uintptr_t)c % d.vec == 0);
                if (to_compact) std::memcpy(c, s, d.bytes); else std::memcpy(s, c, d.bytes);
            }
}

static void tables_case(int N, int M, int A, bool compact, bool ee, bool table) {
    const int B = 7, C = 3, max_iter = 4;
    Side h(B, N, M, A, max_iter, compact, ee, table), in(C, N, M, A, max_iter, compact, ee, table);
    const std::vector<int> idx = {6, 0, 3};
    std::vector<char> named(B, 0);
    for (int q : idx) named[q] = 1;
    for (size_t a = 0; a < h.arrs.size(); a++) {
        for (size_t w = 0; w < h.arrs[a].words; w++) h.arrs[a].mem[w] = 0xdeadbeefu;
        for (size_t w = 0; w < in.arrs[a].words; w++) in.arrs[a].mem[w] = 0xfeedf00du;
        for (int q = 0; q < B; q++) for (size_t e = 0; e < h.arrs[a].per; e++) h.at(h.arrs[a], N, q, e) = code(a, q, e, 1);
    }
    std::vector<SlotTable> in_t, out_t;
    CHECK((mpc_slot_tables<NX, NU, float>(in_t, out_t, in.b, in.mb, in.s, h.b, h.mb, h.s, N, M, A, max_iter, ee)));
    size_t n_in = 0, n_out = 0;
    for (const SlotTable& t : in_t) { CHECK(t.n >= 1 && t.n <= kSlotMaxDesc); n_in += t.n; }
    for (const SlotTable& t : out_t) { CHECK(t.n >= 1 && t.n <= kSlotMaxDesc); n_out += t.n; }
    CHECK(out_t.size() >= 2);                                                  // (more arrays than one table holds)
    // ---- in: intake problem i holds slot idx[i] of every array but the cycle's own inputs; the handle is only read
    replay(in_t, idx, true);
    for (size_t a = 0; a < h.arrs.size(); a++) {
        const std::string nm = h.arrs[a].name;
        bool inputs = nm == "xActual" || nm == "goal_in" || nm == "shift";                      // out only: the movers leave the intake's values alone on the way in
        for (const char* k : {"du", "dmax", "err", "x_old", "u_old", "KT_old", "xGoal", "tshift"}) inputs = inputs || nm == k;      // (written whole by the load stage)
        for (const char* k : {"xb", "ucur", "dcur", "P", "Pp", "p", "pp", "KT"}) inputs = inputs || nm == k;                // (read from the slot by the gathering kernel)
        for (size_t i = 0; i < idx.size(); i++) for (size_t e = 0; e < in.arrs[a].per; e++)
            CHECK(in.at(in.arrs[a], N, i, e) == (inputs ? 0xfeedf00du : code(a, idx[i], e, 1)));
        for (int q = 0; q < B; q++) for (size_t e = 0; e < h.arrs[a].per; e++) CHECK(h.at(h.arrs[a], N, q, e) == code(a, q, e, 1));
    }
    // ---- the cycle rewrites everything in the intake area; out: named slots hold the intake's values, unnamed slots and the in-only arrays are untouched
    for (size_t a = 0; a < in.arrs.size(); a++) for (int i = 0; i < C; i++) for (size_t e = 0; e < in.arrs[a].per; e++) in.at(in.arrs[a], N, i, e) = code(a, i, e, 2);
    replay(out_t, idx, false);
    for (size_t a = 0; a < h.arrs.size(); a++) {
        const std::string nm = h.arrs[a].name;
        const bool in_only = nm == "xTarget" || nm == "cwt";
        size_t coded = 0;
        for (int q = 0; q < B; q++) for (size_t e = 0; e < h.arrs[a].per; e++) {
            size_t i = 0;
            while (i < idx.size() && idx[i] != q) i++;
            CHECK(h.at(h.arrs[a], N, q, e) == ((named[q] && !in_only) ? code(a, i, e, 2) : code(a, q, e, 1)));
            coded++;
        }
        size_t untouched = 0;                                                   // padding of the compact layouts: not a word of it written
        for (size_t w = 0; w < h.arrs[a].words; w++) untouched += h.arrs[a].mem[w] == 0xdeadbeefu;
        CHECK(untouched == h.arrs[a].words - coded);
    }
    std::printf("tables N %3d M %d A %2d compact %d ee %d table %d: %zu entries in (%zu tables), %zu out (%zu tables)\n", N, M, A, compact, ee, table, n_in, in_t.size(), n_out, out_t.size());
}

// the gathering shift: dst in another buffer than src, every lane of a 64-lane wave in turn; buffers exactly N * per words
static void shift_case(int N, int per, int shift, bool zero_fill, int dim_n) {
    std::unique_ptr<float[]> src(new float[(size_t)N * per]), dst(new float[(size_t)N * per]), dst2(new float[(size_t)N * per]);
    for (int e = 0; e < N * per; e++) { src[e] = 1.f + e; dst[e] = -1.f; dst2[e] = -2.f; }
    for (int lane = 0; lane < 64; lane++) mpc_shift<float>(Wave{lane, 64, 0}, dst.get(), dst2.get(), src.get(), per, dim_n, shift, zero_fill, true);
    for (int k = 0; k < N; k++) for (int i = 0; i < per; i++) {
        float want;
        if (k < dim_n - 1) want = (k + shift >= dim_n - 1) ? (zero_fill ? 0.f : src[(dim_n - 1) * per + i]) : src[(k + shift) * per + i];
        else if (k == dim_n - 1) want = src[k * per + i];                        // copy_last: the knot an in-place shift leaves alone
        else want = -1.f;                                                       // beyond DIM_N (ucur / KT: knot N-1 is a copy of its own in the gathering kernel)
        CHECK(dst[k * per + i] == want);
        CHECK(dst2[k * per + i] == (want == -1.f ? -2.f : want));
    }
}

int main() {
    for (int N : {8, 32, 64, 128})
        for (int ee : {0, 1}) tables_case(N, 4, 8, true, ee != 0, ee != 0);
    tables_case(32, 2, 8, false, false, false);      // a family without compact layouts, records or maps (cart-pole shaped: the entry list is the same, the sizes the arm's)
    tables_case(16, 1, 3, true, false, true);
    for (int N : {4, 16, 64})
        for (int per : {7, 14, 98, 196})
            for (int shift : {0, 1, N / 2, N - 2}) {
                shift_case(N, per, shift, false, N);             // x, d, P, p, Pp, pp
                shift_case(N, per, shift, true, N - 1);          // u, KT: their own last knot is N-2 (shift N-2: everything below it zero-filled)
            }
    std::printf("mpc_slots_host_check: ok\n");
    return 0;
}
