// Stand-alone host program over csrc/mpc_record.hpp: the byte layouts of what a control cycle sends (the input run) and gets back (one result record per problem).
// Offsets against values written out by hand, the structure of every record, the input run against the expression the handle allocated "mpc_in" with before the
// header existed, and a round trip through the functions k_mpc_store and mpc_cycle call, on buffers sized with no slack.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc mpc_record_host_check.cpp -o mpc_record_host_check && ./mpc_record_host_check
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpc_record.hpp"

using namespace pddp;

static_assert(sizeof(SolverState<float>) == 64 && sizeof(SolverState<double>) == 88, "the table below is written out for these sizes (padded to 16: 64 and 96)");

struct Case { size_t elem, NX, NU, N, out_stride; MpcRecord want; };
// elem, NX, NU, N, out_stride, {state, x, u, K, J, alpha, end, bytes, out_stride}: pendulum (2, 1) and arm (14, 7), N in {2, 8, 32}, an odd and an even out_stride
static const Case kCases[] = {
    {4,  2, 1,  2,  3, {0, 64, 80, 88, 104, 116, 128, 128, 3}},
    {4,  2, 1,  2, 10, {0, 64, 80, 88, 104, 144, 184, 192, 10}},
    {4,  2, 1,  8,  3, {0, 64, 128, 160, 224, 236, 248, 256, 3}},
    {4,  2, 1,  8, 10, {0, 64, 128, 160, 224, 264, 304, 304, 10}},
    {4,  2, 1, 32,  3, {0, 64, 320, 448, 704, 716, 728, 736, 3}},
    {4,  2, 1, 32, 10, {0, 64, 320, 448, 704, 744, 784, 784, 10}},
    {4, 14, 7,  2,  3, {0, 64, 176, 232, 1016, 1028, 1040, 1040, 3}},
    {4, 14, 7,  2, 10, {0, 64, 176, 232, 1016, 1056, 1096, 1104, 10}},
    {4, 14, 7,  8,  3, {0, 64, 512, 736, 3872, 3884, 3896, 3904, 3}},
    {4, 14, 7,  8, 10, {0, 64, 512, 736, 3872, 3912, 3952, 3952, 10}},
    {4, 14, 7, 32,  3, {0, 64, 1856, 2752, 15296, 15308, 15320, 15328, 3}},
    {4, 14, 7, 32, 10, {0, 64, 1856, 2752, 15296, 15336, 15376, 15376, 10}},
    {8,  2, 1,  2,  3, {0, 96, 128, 144, 176, 200, 212, 224, 3}},
    {8,  2, 1,  2, 10, {0, 96, 128, 144, 176, 256, 296, 304, 10}},
    {8,  2, 1,  8,  3, {0, 96, 224, 288, 416, 440, 452, 464, 3}},
    {8,  2, 1,  8, 10, {0, 96, 224, 288, 416, 496, 536, 544, 10}},
    {8,  2, 1, 32,  3, {0, 96, 608, 864, 1376, 1400, 1412, 1424, 3}},
    {8,  2, 1, 32, 10, {0, 96, 608, 864, 1376, 1456, 1496, 1504, 10}},
    {8, 14, 7,  2,  3, {0, 96, 320, 432, 2000, 2024, 2036, 2048, 3}},
    {8, 14, 7,  2, 10, {0, 96, 320, 432, 2000, 2080, 2120, 2128, 10}},
    {8, 14, 7,  8,  3, {0, 96, 992, 1440, 7712, 7736, 7748, 7760, 3}},
    {8, 14, 7,  8, 10, {0, 96, 992, 1440, 7712, 7792, 7832, 7840, 10}},
    {8, 14, 7, 32,  3, {0, 96, 3680, 5472, 30560, 30584, 30596, 30608, 3}},
    {8, 14, 7, 32, 10, {0, 96, 3680, 5472, 30560, 30640, 30680, 30688, 10}},
};

template <typename T>
static void check_case(const Case& c) {
    const MpcRecord r = mpc_record_of<T>(c.NX, c.NU, c.N, c.out_stride), &w = c.want;
    assert(r.state == w.state && r.x == w.x && r.u == w.u && r.K == w.K && r.J == w.J && r.alpha == w.alpha && r.end == w.end && r.bytes == w.bytes && r.out_stride == w.out_stride);
    const MpcRecord g = mpc_record(sizeof(SolverState<T>), sizeof(T), c.NX, c.NU, c.N, c.out_stride);      // (the typed form is the general one)
    assert(std::memcmp(&g, &r, sizeof r) == 0);
    // the documented order, every field as long as its array, none overlapping the next
    assert(r.state == 0 && r.state + sizeof(SolverState<T>) <= r.x);
    assert(r.u - r.x == c.N * c.NX * sizeof(T) && r.K - r.u == c.N * c.NU * sizeof(T) && r.J - r.K == c.N * c.NX * c.NU * sizeof(T));
    assert(r.alpha - r.J == c.out_stride * sizeof(T) && r.end - r.alpha == c.out_stride * sizeof(int));
    assert(r.x < r.u && r.u < r.K && r.K < r.J && r.J < r.alpha && r.alpha < r.end);
    assert(r.x % 16 == 0 && r.x % sizeof(T) == 0 && r.u % sizeof(T) == 0 && r.K % sizeof(T) == 0 && r.J % sizeof(T) == 0 && r.alpha % sizeof(int) == 0);
    assert(r.bytes % 16 == 0 && r.bytes >= r.end && r.bytes - r.end < 16);
}

template <typename T>
static void check_input_run(size_t NX) {
    for (size_t B = 1; B <= 9; B++) {
        const MpcInputRun in = mpc_input_run(sizeof(T), NX, B);
        assert(in.elems == 2 * B * NX + B * sizeof(int) / sizeof(T) + 2);            // what init() allocated "mpc_in" with: the named array keeps its size
        assert(in.x == 0 && in.goal == B * NX * sizeof(T) && in.shift == 2 * B * NX * sizeof(T));      // the views "xActual" / "shift" keep their addresses
        assert(in.x_bytes == B * NX * sizeof(T) && in.shift_bytes == B * sizeof(int) && in.bytes == in.shift + in.shift_bytes);
        assert(in.bytes <= in.elems * sizeof(T));
        assert(in.shift % sizeof(int) == 0 && in.goal % sizeof(T) == 0);
        assert(in.bytes <= mpc_input_run(sizeof(T), NX, B + 1).bytes);               // (a chunk's run fits the staging of a larger handle)
    }
}

// two problems packed the way k_mpc_store packs them (lane tid of nt) into 2 * bytes with nothing behind, unpacked the way mpc_cycle unpacks them
template <typename T>
static void round_trip(size_t NX, size_t NU, size_t N, size_t os, int nt) {
    const MpcRecord rec = mpc_record_of<T>(NX, NU, N, os);
    const size_t B = 2, nx = N * NX, nu = N * NU, nk = N * NX * NU;
    std::vector<T> x(B * nx), u(B * nu), K(B * nk), J(B * os);
    std::vector<int> a(B * os);
    std::vector<SolverState<T>> st(B);
    int v = 1;                                                       // distinct integer values: exact in float, no two arrays share one
    for (T& e : x) e = T(v++);
    for (T& e : u) e = T(v++);
    for (T& e : K) e = T(v++);
    for (T& e : J) e = T(v++);
    for (int& e : a) e = v++;
    for (size_t pb = 0; pb < B; pb++) { std::memset(&st[pb], 0, sizeof st[pb]); st[pb].rho = T(v++); st[pb].iter = v++; st[pb].done = 2; st[pb].took_step = (int)pb; st[pb].win_pending = v++; }
    unsigned char* out = static_cast<unsigned char*>(std::malloc(B * rec.bytes));
    std::memset(out, 0xab, B * rec.bytes);
    for (size_t pb = 0; pb < B; pb++) {
        unsigned char* r = out + pb * rec.bytes;
        *mpc_at<SolverState<T>>(r, rec.state) = st[pb];
        for (int tid = 0; tid < nt; tid++) mpc_record_pack<T>(rec, r, tid, nt, &x[pb * nx], &u[pb * nu], &K[pb * nk], &J[pb * os], &a[pb * os]);
    }
    std::vector<T> x2(B * nx), u2(B * nu), K2(B * nk), J2(B * os);
    std::vector<int> a2(B * os);
    std::vector<SolverState<T>> st2(B), st3(B);
    for (size_t pb = 0; pb < B; pb++) mpc_record_unpack<T>(rec, out + pb * rec.bytes, pb, st2.data(), x2.data(), u2.data(), K2.data(), J2.data(), a2.data());
    assert(x2 == x && u2 == u && K2 == K && J2 == J && a2 == a && std::memcmp(st2.data(), st.data(), B * sizeof(SolverState<T>)) == 0);
    for (size_t pb = 0; pb < B; pb++) mpc_record_unpack<T>(rec, out + pb * rec.bytes, pb, st3.data(), (T*)nullptr, (T*)nullptr, (T*)nullptr, (T*)nullptr, (int*)nullptr);   // outputs the caller left out
    assert(std::memcmp(st3.data(), st.data(), B * sizeof(SolverState<T>)) == 0);
    for (size_t pb = 0; pb < B; pb++) for (size_t o = rec.end; o < rec.bytes; o++) assert(out[pb * rec.bytes + o] == 0xab);      // the padding is nobody's
    std::free(out);
}

int main() {
    for (const Case& c : kCases) { if (c.elem == 4) check_case<float>(c); else check_case<double>(c); }
    check_input_run<float>(2); check_input_run<float>(14); check_input_run<double>(2); check_input_run<double>(14);
    for (int nt : {1, 3, 64, 256}) {
        round_trip<double>(2, 1, 8, 5, nt);          // the GPU test's shapes: an odd out_stride under doubles
        round_trip<float>(14, 7, 16, 6, nt);
        round_trip<float>(2, 1, 2, 3, nt);
        round_trip<double>(14, 7, 2, 10, nt);
    }
    std::printf("mpc_record_host_check: ok\n");
    return 0;
}
