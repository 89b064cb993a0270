// Stand-alone host program over the host-only part of csrc/slots.hpp: index validation and descriptor-table construction, with the kernels' addressing replayed by
// memcpy on exactly-sized host arrays -- built with -fsanitize=address,undefined, an entry that reaches past an array is reported.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc slots_host_check.cpp -o slots_host_check && ./slots_host_check
#include <algorithm>
#include <cassert>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "slots.hpp"

using namespace pddp;

static void replay(const SlotTable& t, const std::vector<int>& idx, size_t elem) {
    for (size_t i = 0; i < idx.size(); i++)
        for (int k = 0; k < t.n; k++) {
            const SlotDesc& d = t.d[k];
            unsigned char* s = d.slot + (d.abc ? slot_abc_offset(d.abc, (size_t)idx[i], t.N, elem) : (size_t)idx[i] * d.sstride);
            assert(d.bytes % d.vec == 0 && (uintptr_t)s % d.vec == 0);
            if (d.op == kSlotZero) { std::memset(s, 0, d.bytes); continue; }
            unsigned char* c = d.compact + (d.abc ? slot_abc_offset(d.abc, i, t.N, elem) : i * d.cstride);
            assert((uintptr_t)c % d.vec == 0);
            std::memcpy(s, c, d.bytes);
        }
}

int main() {
    // ---- index validation
    const int good[4] = {3, 0, 6, 2};
    assert(slots_complaint(4, good, 7).empty());
    assert(!slots_complaint(0, good, 7).empty() && !slots_complaint(-1, good, 7).empty() && !slots_complaint(4, nullptr, 7).empty());
    const int high[2] = {1, 7}, low[2] = {-1, 1}, twice[3] = {5, 2, 5};
    assert(slots_complaint(2, high, 7).find("outside") != std::string::npos);
    assert(slots_complaint(2, low, 7).find("outside") != std::string::npos);
    assert(slots_complaint(3, twice, 7).find("twice") != std::string::npos);
    assert(slots_complaint(1, good + 1, 1).empty());
    // ---- the compact [A B] through abc_index: every (N, batch) puts each knot's 147 floats where abc_index says, and nothing else moves
    for (int N : {4, 8, 16, 32, 64, 128}) {
        for (int batch : {1, 3, 67}) {
            const int C = batch < 5 ? batch : 5;
            std::vector<float> main_abc(abc_floats((size_t)batch * N), -1.f), in_abc(abc_floats((size_t)C * N), -1.f);
            std::vector<int> idx;
            for (int i = 0; i < C; i++) idx.push_back((batch - 1 - 2 * i + 4 * batch) % batch);
            std::sort(idx.begin(), idx.end()); idx.erase(std::unique(idx.begin(), idx.end()), idx.end());
            for (size_t i = 0; i < idx.size(); i++)
                for (int k = 0; k < N; k++) for (int col = 0; col < 21; col++) for (int r = 0; r < 7; r++) in_abc[abc_index(i * N + k, col, r)] = (float)(1000 * idx[i] + k) + 0.01f * (col * 7 + r);
            SlotTable t{}; t.N = N;
            assert(slot_add_abc(t, in_abc.data(), main_abc.data(), N, sizeof(float)));
            assert(t.n == (N >= 64 ? 1 : 3));
            replay(t, idx, sizeof(float));
            std::vector<char> named(batch, 0);
            for (int q : idx) named[q] = 1;
            size_t written = 0;
            for (int q = 0; q < batch; q++)
                for (int k = 0; k < N; k++) for (int col = 0; col < 21; col++) for (int r = 0; r < 7; r++) {
                    const float v = main_abc[abc_index((size_t)q * N + k, col, r)];
                    if (named[q]) { assert(v == (float)(1000 * q + k) + 0.01f * (col * 7 + r)); written++; } else assert(v == -1.f);
                }
            size_t changed = 0;
            for (float v : main_abc) changed += v != -1.f;
            assert(changed == written);
        }
    }
    // ---- plain entries: strides, the half-row copy of xb, zero fill, access widths
    {
        const int B = 9, C = 4, N = 8, NX = 3;
        std::vector<float> xb(B * 2 * N * NX, 7.f), ixb(C * 2 * N * NX, 1.f), P(B * N * NX * NX + B * N * NX * NX, 5.f);
        SlotTable t{}; t.N = N;
        assert(slot_add(t, ixb.data(), xb.data(), 2 * N * NX * 4, 2 * N * NX * 4, N * NX * 4, kSlotCopy));
        assert(slot_add(t, nullptr, P.data() + B * N * NX * NX, 0, N * NX * NX * 4, N * NX * NX * 4, kSlotZero));
        assert(!slot_add(t, nullptr, xb.data(), 4, 4, 4, kSlotCopy) && !slot_add(t, ixb.data(), xb.data(), 4, 4, 6, kSlotCopy) && !slot_add(t, ixb.data(), nullptr, 4, 4, 4, kSlotCopy));
        replay(t, {8, 0, 5}, 4);
        for (int q = 0; q < B; q++) {
            const bool named = q == 8 || q == 0 || q == 5;
            for (int e = 0; e < 2 * N * NX; e++) assert(xb[q * 2 * N * NX + e] == ((named && e < N * NX) ? 1.f : 7.f));
            for (int e = 0; e < N * NX * NX; e++) { assert(P[q * N * NX * NX + e] == 5.f); assert(P[(B + q) * N * NX * NX + e] == (named ? 0.f : 5.f)); }
        }
        SlotTable full{};
        for (int k = 0; k < kSlotMaxDesc; k++) assert(slot_add(full, ixb.data(), xb.data(), 4, 4, 4, kSlotCopy));
        assert(!slot_add(full, ixb.data(), xb.data(), 4, 4, 4, kSlotCopy));
        assert(slot_vec((void*)16, (void*)32, 48, 64, 16) == 16 && slot_vec((void*)16, (void*)40, 48, 64, 16) == 8 && slot_vec((void*)16, (void*)32, 48, 64, 12) == 4);
    }
    // ---- for_each_slot_run: the runs tile [0, count) in order, the slots inside a run ascend by one, and no run could have taken its successor's first element
    {
        const std::vector<std::vector<int>> lists = {{3}, {0, 1, 2, 3}, {5, 0, 1, 2, 4}, {4, 3, 2}, {1, 3, 5}, {0, 1, 7, 8, 9, 2}};
        const size_t runs_of[6] = {1, 1, 3, 3, 3, 3};
        for (size_t l = 0; l < lists.size(); l++) {
            const std::vector<int>& idx = lists[l];
            std::vector<std::pair<int, int>> runs;
            for_each_slot_run((int)idx.size(), idx.data(), [&](int first, int len) { runs.push_back({first, len}); });
            int next = 0;
            for (size_t r = 0; r < runs.size(); r++) {
                const int first = runs[r].first, len = runs[r].second;
                assert(first == next && len >= 1 && first + len <= (int)idx.size());
                for (int j = first + 1; j < first + len; j++) assert(idx[j] == idx[j - 1] + 1);
                if (r + 1 < runs.size()) assert(idx[first + len] != idx[first + len - 1] + 1);
                next = first + len;
            }
            assert(next == (int)idx.size() && runs.size() == runs_of[l]);
        }
        int calls = 0;
        for_each_slot_run(0, nullptr, [&](int, int) { calls++; });
        assert(calls == 0);
    }
    std::printf("slots_host_check: ok\n");
    return 0;
}
