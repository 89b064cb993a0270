// Replacing and collecting individual problems ("slots") of a loaded handle between sweeps: pddp_load_problems / pddp_store_problems.
//
// A refill runs the handle's own init path on a compact INTAKE AREA (a second set of buffers for min(batch, 256) problems on the same kernel families, solver_impl.hpp)
// and k_slots_scatter then moves every per-problem array of the intake's problem i into slot idx[i] of the handle -- or clears it there, where a load clears it.
// k_slots_gather goes the other way for a store: the requested rows of x (the half of xb that state.cur names), u, KT, Jout, alphaOut and dmax[alphaIndex] are packed
// into one staging buffer, [count][...] per output, which the host fetches with one transfer per output.
//
// Both kernels are driven by a small descriptor table (SlotTable, a kernel argument): one entry per array, in BYTES, so that element types do not matter.
// They are pure HBM movers: one workgroup per (problem, array), consecutive lanes on consecutive 16-byte words (8 / 4 bytes where an array's per-problem size or
// base does not allow 16: slot_vec).  No LDS, no cross-lane operation.
//
// The compact [A B] (ab_compact.hpp) is chunked by 64 GLOBAL knots: with N < 64 one chunk holds knots of several problems, and inside it the three column pieces lie
// apart.  Its entries therefore carry `abc` = piece + 1 and are addressed through abc_index: the N knots of a problem are one contiguous run per piece
// (N * 56 / 42 / 49 floats, a multiple of 16 bytes for every N >= 4); with N >= 64 a problem owns N / 64 whole chunks and the entry is an ordinary per-problem slice.
//
// The host part (descriptor construction, index validation) is plain C++: tests/native/slots_host_check.cpp runs it under the address / undefined-behaviour sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ab_compact.hpp"

namespace pddp {

constexpr int kSlotIntakeMax = 256;        // problems of the intake area (and of one chunk of a refill / a store)
constexpr int kSlotMaxDesc = 32;

enum SlotOp : int { kSlotCopy = 0, kSlotZero = 1, kSlotCopyHalf = 2, kSlotCopyAlpha = 3 };

struct SlotDesc {
    unsigned char* compact;          // base on the compact side (intake area / staging buffer): problem i of the chunk at compact + i * cstride
    unsigned char* slot;             // base on the handle's side: slot q at slot + q * sstride
    unsigned long long cstride, sstride;
    unsigned bytes;                  // bytes moved (or cleared) per problem
    int vec;                         // bytes per lane and access: 16, 8 or 4
    int op;                          // SlotOp.  kSlotCopyHalf: + state.cur * bytes on the handle's side (xb); kSlotCopyAlpha: + state.alphaIndex * bytes (dmax)
    int abc;                         // 0, or 1 + column piece of the compact [A B] (N < 64): both sides addressed through abc_index
};
struct SlotTable {
    SlotDesc d[kSlotMaxDesc];
    int n;
    int N;                           // knots per problem (the abc entries)
    const unsigned char* state;      // the handle's solver states (gather: cur / alphaIndex of a slot)
    unsigned state_stride, off_cur, off_alpha;
};

// widest access (16 / 8 / 4 bytes) that every address of an entry is a multiple of
inline int slot_vec(const void* a, const void* b, unsigned long long s0, unsigned long long s1, unsigned long long bytes) {
    const unsigned long long m = (unsigned long long)(uintptr_t)a | (unsigned long long)(uintptr_t)b | s0 | s1 | bytes;
    return (m % 16 == 0) ? 16 : (m % 8 == 0) ? 8 : 4;
}
// appends an entry; false when the table is full or the sizes are not whole 4-byte words (every array of a handle is)
inline bool slot_add(SlotTable& t, const void* compact, void* slot, size_t cstride, size_t sstride, size_t bytes, int op, int abc = 0) {
    if (t.n >= kSlotMaxDesc || bytes == 0 || bytes % 4 || cstride % 4 || sstride % 4 || bytes > 0xffffffffull || (!slot) || (op != kSlotZero && !compact)) return false;
    SlotDesc& d = t.d[t.n++];
    d.compact = (unsigned char*)compact; d.slot = (unsigned char*)slot; d.cstride = cstride; d.sstride = sstride; d.bytes = (unsigned)bytes; d.op = op; d.abc = abc;
    d.vec = slot_vec(op == kSlotZero ? nullptr : compact, slot, op == kSlotZero ? 0 : cstride, sstride, bytes);
    return true;
}
// the compact [A B] of `N` knots per problem, `elem` bytes per element: one entry (N >= 64: whole chunks) or one per column piece
inline bool slot_add_abc(SlotTable& t, const void* compact, void* slot, int N, size_t elem) {
    if (N >= 64) { const size_t per = (size_t)(N / 64) * kAbcChunk * elem; return slot_add(t, compact, slot, per, per, per, kSlotCopy); }
    for (int p = 0; p < 3; p++) if (!slot_add(t, compact, slot, 0, 0, (size_t)N * abc_piece_cols(p) * 7 * elem, kSlotCopy, p + 1)) return false;
    return true;
}
// byte offset of a problem's run of piece `abc - 1` (N < 64)
PDDP_HD size_t slot_abc_offset(int abc, size_t problem, int N, size_t elem) { return abc_index(problem * (size_t)N, abc_piece_col(abc - 1, 0), 0) * elem; }

// "" or the complaint about a list of slot indices: count >= 1, every index inside [0, batch), none twice
inline std::string slots_complaint(int count, const int* idx, int batch) {
    if (count < 1) return "count must be >= 1";
    if (!idx) return "idx is NULL";
    std::vector<unsigned char> seen((size_t)batch, 0);
    for (int i = 0; i < count; i++) {
        if (idx[i] < 0 || idx[i] >= batch) return "idx[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " is outside [0, batch = " + std::to_string(batch) + ")";
        if (seen[idx[i]]) return "slot " + std::to_string(idx[i]) + " is named twice (idx[" + std::to_string(i) + "])";
        seen[idx[i]] = 1;
    }
    return "";
}

// f(first, len) for every maximal run of positions [first, first + len) of idx[0 .. count) whose slots ascend by one, in order: what names such a run moves rows of
// a per-slot table with one transfer (the cost-weight tables, solver_impl.hpp)
template <typename F>
inline void for_each_slot_run(int count, const int* idx, F&& f) {
    for (int i = 0; i < count;) {
        int j = i + 1;
        while (j < count && idx[j] == idx[j - 1] + 1) j++;
        f(i, j - i);
        i = j;
    }
}

#ifdef __HIPCC__
// `bytes` bytes from src to dst (src null: zeros) by one workgroup, `vec` bytes per lane and access
__device__ inline void slot_move(unsigned char* dst, const unsigned char* src, unsigned bytes, int vec) {
    if (vec == 16) {
        const uint4 z = make_uint4(0, 0, 0, 0);
        for (unsigned o = threadIdx.x * 16u; o < bytes; o += blockDim.x * 16u) *reinterpret_cast<uint4*>(dst + o) = src ? *reinterpret_cast<const uint4*>(src + o) : z;
    } else if (vec == 8) {
        const uint2 z = make_uint2(0, 0);
        for (unsigned o = threadIdx.x * 8u; o < bytes; o += blockDim.x * 8u) *reinterpret_cast<uint2*>(dst + o) = src ? *reinterpret_cast<const uint2*>(src + o) : z;
    } else {
        for (unsigned o = threadIdx.x * 4u; o < bytes; o += blockDim.x * 4u) *reinterpret_cast<unsigned*>(dst + o) = src ? *reinterpret_cast<const unsigned*>(src + o) : 0u;
    }
}
// grid (problems of the chunk, entries of the table), block 256.  to_compact = 0: intake problem i -> slot idx[i] (or zeros into the slot); 1: the reverse for the
// copy entries (the refill fetches what the init kernels read per problem but a load does not upload, the end-effector cost's xTarget)
template <typename T>
__global__ __launch_bounds__(256) void k_slots_scatter(SlotTable t, const int* __restrict__ idx, int n, int batch, int to_compact) {
    const int i = blockIdx.x;
    if (i >= n || (int)blockIdx.y >= t.n) return;
    const SlotDesc d = t.d[blockIdx.y];
    const int q = idx[i];
    if (q < 0 || q >= batch) return;                               // (validated on the host; a stale index must not become a stray write)
    unsigned char* s = d.slot + (d.abc ? slot_abc_offset(d.abc, (size_t)q, t.N, sizeof(T)) : (size_t)q * d.sstride);
    unsigned char* c = d.compact + (d.abc ? slot_abc_offset(d.abc, (size_t)i, t.N, sizeof(T)) : (size_t)i * d.cstride);
    if (d.op == kSlotZero) { if (!to_compact) slot_move(s, nullptr, d.bytes, d.vec); }
    else if (to_compact) slot_move(c, s, d.bytes, d.vec);
    else slot_move(s, c, d.bytes, d.vec);
}
// grid (problems of the chunk, entries), block 256: slot idx[i] -> row i of the entry's staging area
template <typename T>
__global__ __launch_bounds__(256) void k_slots_gather(SlotTable t, const int* __restrict__ idx, int n, int batch) {
    const int i = blockIdx.x;
    if (i >= n || (int)blockIdx.y >= t.n) return;
    const SlotDesc d = t.d[blockIdx.y];
    const int q = idx[i];
    if (q < 0 || q >= batch) return;
    const unsigned char* st = t.state + (size_t)q * t.state_stride;
    size_t off = (size_t)q * d.sstride;
    if (d.op == kSlotCopyHalf) off += (size_t)(*reinterpret_cast<const int*>(st + t.off_cur) ? 1 : 0) * d.bytes;
    if (d.op == kSlotCopyAlpha) {                                  // (clamped to the row: a state record set from outside must not become a stray read)
        const int a = *reinterpret_cast<const int*>(st + t.off_alpha), amax = (int)(d.sstride / d.bytes) - 1;
        off += (size_t)(a < 0 ? 0 : a > amax ? amax : a) * d.bytes;
    }
    slot_move(d.compact + (size_t)i * d.cstride, d.slot + off, d.bytes, d.vec);
}
#endif

}  // namespace pddp
