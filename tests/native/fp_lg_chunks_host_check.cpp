// Stand-alone host program over the candidates-per-workgroup rule of k_fp_lg (csrc/kernel_plan.hpp fp_lg_chunks).  No GPU, no library.
//   g++ -std=c++17 -g -fsanitize=address,undefined -I ../../parallel-ddp_amd/csrc fp_lg_chunks_host_check.cpp -o fp_lg_chunks_host_check
// Every (M, A) config_complaint accepts (M in 1 .. 16, A in 1 .. 64; M = 3, 5, ... never divide a horizon, and are swept all the same) and the initial rollout's one
// candidate: no workgroup above 1024 threads, the chunks tile A exactly, the instantiation covers the workgroup, and every (M, A) pddp_create accepted under the rule
// before this function -- one workgroup per 8 candidates when A is a multiple of 8 above 8, one workgroup otherwise, refused at create beyond 128 lane groups (1024
// threads) -- keeps its grid and workgroup size, so the kernel computes the same bits there.  Prints how many (M, A) create refused before.
#include <cstdio>
#include <cstdlib>

#include "kernel_plan.hpp"

using namespace pddp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d (M %d A %d): %s\n", __LINE__, M, A, #cond); std::exit(1); } } while (0)

int main() {
    int refused_before = 0;
    for (int M = 1; M <= 16; M++) {
        for (int A = 1; A <= 64; A++) {
            const FpLgChunks c = fp_lg_chunks(A, M);
            CHECK(c.chunks >= 1 && c.per_wg >= 1 && c.chunks * c.per_wg == A);
            CHECK(c.per_wg * M <= kFpLgMaxGroups);
            CHECK(c.waves == (c.per_wg * M + 7) / 8 && c.waves >= 1 && 64 * c.waves <= 1024);
            const int maxt[3] = {256, 512, 1024};
            CHECK(c.size >= 0 && c.size <= 2 && 64 * c.waves <= maxt[c.size] && (c.size == 0 || 64 * c.waves > maxt[c.size - 1]));
            // the rule before: chunks, candidates per workgroup and waves as launch_fp_rollouts computed them
            const int was_chunks = (A > 8 && A % 8 == 0) ? A / 8 : 1, was_per_wg = A / was_chunks, was_waves = (was_per_wg * M + 7) / 8;
            if (64 * was_waves <= 1024) {
                CHECK(c.chunks == was_chunks && c.per_wg == was_per_wg && c.waves == was_waves && c.size == (was_waves <= 4 ? 0 : was_waves <= 8 ? 1 : 2));
            } else {
                refused_before++;
                CHECK(c.chunks > 1);
                for (int d = c.per_wg + 1; d <= A; d++) CHECK(A % d != 0 || d * M > kFpLgMaxGroups);      // the largest divisor that fits
            }
        }
        const int A = 1;
        CHECK(fp_lg_chunks(1, M).chunks == 1 && fp_lg_chunks(1, M).per_wg == 1);                          // the initial rollout
    }
    // the shapes the rule was written for
    { const int M = 16, A = 12; CHECK(fp_lg_chunks(A, M).per_wg == 6 && fp_lg_chunks(A, M).chunks == 2 && fp_lg_chunks(A, M).waves == 12); }
    { const int M = 16, A = 13; CHECK(fp_lg_chunks(A, M).per_wg == 1 && fp_lg_chunks(A, M).chunks == 13); }
    { const int M = 8, A = 17; CHECK(fp_lg_chunks(A, M).per_wg == 1 && fp_lg_chunks(A, M).chunks == 17); }
    { const int M = 4, A = 33; CHECK(fp_lg_chunks(A, M).per_wg == 11 && fp_lg_chunks(A, M).chunks == 3); }
    { const int M = 16, A = 8; CHECK(fp_lg_chunks(A, M).per_wg == 8 && fp_lg_chunks(A, M).chunks == 1 && fp_lg_chunks(A, M).waves == 16); }
    std::printf("fp_lg_chunks_host_check: ok (%d of %d (M, A) were refused at create before)\n", refused_before, 16 * 64);
    return 0;
}
