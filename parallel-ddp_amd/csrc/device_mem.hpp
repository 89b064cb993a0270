// One grow-only owning block of memory: what a handle keeps in device or pinned host memory (solver_impl.hpp) is a MemBuf, a plain member or an element of a vector,
// and is released with its owner -- no capacity field beside a raw pointer, no line in a destructor, nothing to leak on an error return.
// The memory kind is a policy with  static bool alloc(void** p, size_t bytes)  and  static void release(void* p);  solver_base.hpp has the two HIP policies (DeviceMem,
// PinnedMem).  Host code only, no HIP header, no environment (tests/native/device_mem_host_check.cpp holds it with a counting host policy under the sanitizers).
#pragma once
#include <cstddef>

namespace pddp {

template <typename Mem>
struct MemBuf {
    void* ptr = nullptr;
    size_t cap = 0;              // bytes allocated; 0 with ptr == nullptr: empty
    MemBuf() = default;
    MemBuf(const MemBuf&) = delete;
    MemBuf& operator=(const MemBuf&) = delete;
    MemBuf(MemBuf&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr; o.cap = 0; }
    MemBuf& operator=(MemBuf&& o) noexcept {
        if (this != &o) { release(); ptr = o.ptr; cap = o.cap; o.ptr = nullptr; o.cap = 0; }
        return *this;
    }
    ~MemBuf() { release(); }
    void release() {
        if (ptr) Mem::release(ptr);
        ptr = nullptr; cap = 0;
    }
    bool holds(size_t bytes) const { return ptr && bytes <= cap; }
    // a block of at least `bytes` bytes: the one the buffer has if it is large enough, otherwise a new one of max(bytes, min_cap) -- the old block is released first and
    // its contents are not kept.  false: the allocation failed and the buffer is empty.
    bool reserve(size_t bytes, size_t min_cap = 0) {
        if (holds(bytes)) return true;
        release();
        const size_t want = bytes < min_cap ? min_cap : bytes;
        void* p = nullptr;
        if (!Mem::alloc(&p, want) || !p) return false;
        ptr = p; cap = want;
        return true;
    }
    template <typename U> U* as() const { return static_cast<U*>(ptr); }
};

}  // namespace pddp
