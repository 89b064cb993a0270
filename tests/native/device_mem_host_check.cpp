// Stand-alone host program over csrc/device_mem.hpp: the owning buffer with a counting host policy -- every allocation and release is counted and every live block
// is known, so a block released twice, never, or while another owner still names it fails an assertion (and, built with -fsanitize=address,undefined, the sanitizer).
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc device_mem_host_check.cpp -o device_mem_host_check && ./device_mem_host_check
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

#include "device_mem.hpp"

using namespace pddp;

struct CountingMem {
    static int allocs, releases;
    static size_t last_bytes;
    static bool fail_next;
    static std::set<void*> live;
    static bool alloc(void** p, size_t bytes) {
        if (fail_next) { fail_next = false; *p = nullptr; return false; }
        *p = std::malloc(bytes);
        std::memset(*p, 0xab, bytes);                    // (every byte of the capacity is the owner's to write)
        allocs++; last_bytes = bytes; live.insert(*p);
        return true;
    }
    static void release(void* p) {
        assert(live.erase(p) == 1);                      // a block that is live, once
        releases++;
        std::free(p);
    }
};
int CountingMem::allocs = 0, CountingMem::releases = 0;
size_t CountingMem::last_bytes = 0;
bool CountingMem::fail_next = false;
std::set<void*> CountingMem::live;

using Buf = MemBuf<CountingMem>;
static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "one owner per block");
static_assert(std::is_nothrow_move_constructible<Buf>::value && std::is_nothrow_move_assignable<Buf>::value, "a vector of buffers moves its elements when it grows");

int main() {
    int& A = CountingMem::allocs; int& R = CountingMem::releases;
    {   // ---- reserve: empty -> max(bytes, min_cap); smaller or equal keeps the block; larger releases once and allocates once
        Buf b;
        assert(b.ptr == nullptr && b.cap == 0 && !b.holds(0) && !b.holds(1));
        assert(b.reserve(100) && b.ptr && b.cap == 100 && CountingMem::last_bytes == 100 && A == 1 && R == 0);
        void* const p0 = b.ptr;
        assert(b.reserve(100) && b.ptr == p0 && b.reserve(1) && b.ptr == p0 && b.reserve(0) && b.ptr == p0 && b.reserve(50, 4096) && b.ptr == p0);
        assert(b.cap == 100 && A == 1 && R == 0);      // (a floor does not regrow a block that is large enough for the request)
        assert(b.reserve(101) && b.cap == 101 && A == 2 && R == 1 && CountingMem::live.size() == 1 && CountingMem::live.count(b.ptr));
        std::memset(b.ptr, 1, b.cap);
        Buf f;
        assert(f.reserve(16, 4096) && f.cap == 4096 && CountingMem::last_bytes == 4096);
        std::memset(f.ptr, 2, f.cap);
        assert(f.reserve(4096) && A == 3 && f.reserve(5000, 4096) && f.cap == 5000 && A == 4 && R == 2);
        assert(f.as<unsigned char>() == static_cast<unsigned char*>(f.ptr));
    }
    assert(A == 4 && R == 4 && CountingMem::live.empty());
    {   // ---- a policy that fails: the buffer is empty afterwards (the old block is gone, once), and a later reserve works
        Buf b;
        CountingMem::fail_next = true;
        assert(!b.reserve(64) && b.ptr == nullptr && b.cap == 0 && A == 4 && R == 4);
        assert(b.reserve(64) && b.cap == 64 && A == 5);
        CountingMem::fail_next = true;
        assert(!b.reserve(128) && b.ptr == nullptr && b.cap == 0 && A == 5 && R == 5 && CountingMem::live.empty());
        assert(b.reserve(8) && b.cap == 8 && A == 6);
        b.release();
        assert(b.ptr == nullptr && b.cap == 0 && R == 6);
        b.release();                                     // (an empty buffer releases nothing)
        assert(R == 6);
    }
    assert(A == 6 && R == 6 && CountingMem::live.empty());
    {   // ---- moves transfer ownership: the source is empty, the target's old block is released
        Buf a;
        assert(a.reserve(32));
        void* const pa = a.ptr;
        Buf b(std::move(a));
        assert(a.ptr == nullptr && a.cap == 0 && b.ptr == pa && b.cap == 32 && A == 7 && R == 6);
        Buf c;
        assert(c.reserve(48));
        void* const pc = c.ptr;
        c = std::move(b);
        assert(b.ptr == nullptr && b.cap == 0 && c.ptr == pa && c.cap == 32 && R == 7 && !CountingMem::live.count(pc) && CountingMem::live.count(pa));
        Buf& self = c;
        c = std::move(self);                             // (self-assignment keeps the block)
        assert(c.ptr == pa && c.cap == 32 && R == 7);
        assert(a.reserve(8) && a.cap == 8);              // a moved-from buffer is an empty one
        Buf e;
        c = std::move(e);                                // an empty source empties the target
        assert(c.ptr == nullptr && c.cap == 0 && R == 8);
    }
    assert(A == 9 && R == 9 && CountingMem::live.empty());
    {   // ---- a vector of buffers (the handle's named arrays): growth moves the owners, every block is released once
        std::vector<Buf> v;
        std::set<void*> blocks;
        for (int i = 0; i < 37; i++) {
            Buf blk;
            assert(blk.reserve(8 + i));
            blocks.insert(blk.ptr);
            if (i % 2) v.push_back(std::move(blk)); else { v.emplace_back(); v.back() = std::move(blk); }
            assert(blk.ptr == nullptr);
        }
        assert(A == 9 + 37 && R == 9 && CountingMem::live == blocks);
        for (int i = 0; i < 37; i++) assert(v[i].cap == (size_t)(8 + i) && blocks.count(v[i].ptr));
        CountingMem::fail_next = true;                   // an allocation that fails between two registrations leaves what is registered alone
        { Buf blk; assert(!blk.reserve(8)); }
        assert(CountingMem::live == blocks);
    }
    assert(A == 46 && R == 46 && CountingMem::live.empty());
    std::printf("device_mem_host_check: ok\n");
    return 0;
}
