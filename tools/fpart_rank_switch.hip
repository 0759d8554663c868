// Where the count of the fiber partition pre-pass (c3sc_amd/csrc/fiber_partition_rank.hpp) should switch from counting the smaller
// positions in a bin's list to sorting the block: FPART_RANK_SORT_MIN.  2^20 fibers of a 7-D batch at K = 3 on 41 x 41 + 1 bins,
// one fiber in eight dead; in EVERY block of 1024 one key bin holds exactly n fibers at random positions and the other live
// fibers have keys of their own, so n is the fullest bin of every block.  For each n the count kernel is timed with the sort
// forced and with the sort forbidden (device events around 20 launches, after 3 warm-up launches), and the whole pass is held
// to a stable sort on the host with either path.  Then the three kernels are timed on a batch with every index uniform.
//   hipcc -std=c++20 -O3 --offload-arch=gfx950 -I c3sc_amd/csrc -I include tools/fpart_rank_switch.hip -o fpart_rank_switch
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "fiber_partition_rank.hpp"

using namespace c3sc;

#define CHECK(x)                                                                          \
    do {                                                                                  \
        const hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                           \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

constexpr int D = 7, K = 3, N = 41, KMAJ = 2, KMIN = 4;

static std::vector<int32_t> make_batch(long F, int n, unsigned seed, std::vector<int> &bin)
{
    std::mt19937 rng(seed);
    std::vector<int32_t> idx((size_t)F * D);
    bin.assign(F, 0);
    std::vector<int> pos(FPART_BLOCK);
    for (long fb = 0; fb < F; fb += FPART_BLOCK) {
        const int len = (int)std::min<long>(FPART_BLOCK, F - fb);
        std::iota(pos.begin(), pos.begin() + len, 0);
        std::shuffle(pos.begin(), pos.begin() + len, rng);
        const int full = (int)(rng() % (N * N)); // the block's full bin
        int next = 0;
        for (int q = 0; q < len; q++) {
            const long f = fb + pos[q];
            int32_t *row = &idx[(size_t)f * D];
            for (int m = 0; m < D; m++) row[m] = 1 + (int)(rng() % (N - 2));
            int key = full;
            if (q >= n) {
                if (next == full) next++;
                key = next++;
            }
            row[KMAJ] = key / N;
            row[KMIN] = key % N;
            row[K] = 0;
            const bool dead = q >= n && rng() % 8 == 0;
            if (dead) row[rng() % 2] = rng() % 2 ? N - 1 : 0; // dimensions 0 and 1 absorb
            bin[f] = dead ? N * N : key;
        }
    }
    return idx;
}

int main(int argc, char **argv)
{
    const long F = argc > 1 ? std::atol(argv[1]) : 1L << 20;
    PartArgs P{};
    P.d = D;
    P.k = K;
    P.F = F;
    for (int m = 0; m < MAXD; m++) {
        P.ngrid[m] = N;
        P.bctype[m] = m < 2 ? C3SC_ABSORB : C3SC_REFLECT;
    }
    P.kmaj = KMAJ;
    P.kmin = KMIN;
    P.nmin = N;
    P.nbins = N * N + 1;
    void *block = nullptr;
    int32_t *d_idx = nullptr;
    CHECK(hipMalloc(&block, fpart_bytes(F, P.nbins)));
    CHECK(hipMalloc((void **)&d_idx, (size_t)F * D * 4));
    const PartScratch s = fpart_carve(block, F, P.nbins);
    const long nb = fpart_blocks(F);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::printf("F %ld, %ld blocks, %d bins, FPART_RANK_SORT_MIN %d\n", F, nb, P.nbins, FPART_RANK_SORT_MIN);
    std::printf("%6s %14s %14s   us per launch of k_fpart_rank_count\n", "n", "count lists", "sort");
    const int sizes[] = {1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 256, 512, 896};
    bool ok = true;
    for (const int n : sizes) {
        std::vector<int> bin;
        const std::vector<int32_t> idx = make_batch(F, n, 1000u + n, bin);
        CHECK(hipMemcpy(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
        std::vector<int32_t> want(F);
        std::iota(want.begin(), want.end(), 0);
        std::stable_sort(want.begin(), want.end(), [&](int32_t a, int32_t b) { return bin[a] < bin[b]; });
        float us[2];
        for (int path = 0; path < 2; path++) {
            const int sort_min = path == 0 ? 1 << 20 : 1;
            for (int it = 0; it < 23; it++) {
                if (it == 3) CHECK(hipEventRecord(e0, nullptr));
                hipLaunchKernelGGL(k_fpart_rank_count, dim3((unsigned)nb), dim3(FPART_THREADS), 0, nullptr, P, (const int32_t *)d_idx, s.bins, s.rank, s.counts,
                                   sort_min);
            }
            CHECK(hipEventRecord(e1, nullptr));
            CHECK(hipEventSynchronize(e1));
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            us[path] = ms * 1000.f / 20.f;
            // the whole pass behind the last count
            hipLaunchKernelGGL(k_fpart_rank_scan, dim3((unsigned)((P.nbins + FPART_RSCAN_BINS - 1) / FPART_RSCAN_BINS)), dim3(FPART_RSCAN_THREADS), 0, nullptr, s.counts,
                               nb, P.nbins, s.totals);
            hipLaunchKernelGGL(k_fpart_rank_scatter, dim3((unsigned)((nb + 7) / 8 * 8)), dim3(FPART_THREADS), 0, nullptr, F, P.nbins, (const uint16_t *)s.bins,
                               (const uint16_t *)s.rank, (const int32_t *)s.counts, (const int32_t *)s.totals, s.nlive, s.perm);
            CHECK(hipGetLastError());
            std::vector<int32_t> perm(F);
            CHECK(hipMemcpy(perm.data(), s.perm, (size_t)F * 4, hipMemcpyDeviceToHost));
            if (perm != want) {
                std::printf("n %d path %d: perm differs from the stable sort\n", n, path);
                ok = false;
            }
        }
        std::printf("%6d %14.2f %14.2f\n", n, us[0], us[1]);
        std::fflush(stdout);
    }
    {   // the three kernels on a batch like the benchmark's: every index uniform over the grid (a fiber in ten dead)
        std::mt19937 rng(7);
        std::vector<int32_t> idx((size_t)F * D);
        for (auto &v : idx) v = (int32_t)(rng() % N);
        for (long f = 0; f < F; f++) idx[f * D + K] = 0;
        CHECK(hipMemcpy(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
        auto timed = [&](const char *what, auto &&launch) {
            for (int it = 0; it < 23; it++) {
                if (it == 3) CHECK(hipEventRecord(e0, nullptr));
                launch();
            }
            CHECK(hipEventRecord(e1, nullptr));
            CHECK(hipEventSynchronize(e1));
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            std::printf("uniform batch, %-21s %8.2f us per launch, back to back\n", what, ms * 1000.f / 20.f);
        };
        timed("k_fpart_rank_count", [&] {
            hipLaunchKernelGGL(k_fpart_rank_count, dim3((unsigned)nb), dim3(FPART_THREADS), 0, nullptr, P, (const int32_t *)d_idx, s.bins, s.rank, s.counts,
                               FPART_RANK_SORT_MIN);
        });
        timed("k_fpart_rank_scan", [&] { // in place: every launch scans what the one before left, the same work
            hipLaunchKernelGGL(k_fpart_rank_scan, dim3((unsigned)((P.nbins + FPART_RSCAN_BINS - 1) / FPART_RSCAN_BINS)), dim3(FPART_RSCAN_THREADS), 0, nullptr, s.counts,
                               nb, P.nbins, s.totals);
        });
        // the scans above have scanned their own output over and over: count and scan once more, so that the scatter reads prefixes
        hipLaunchKernelGGL(k_fpart_rank_count, dim3((unsigned)nb), dim3(FPART_THREADS), 0, nullptr, P, (const int32_t *)d_idx, s.bins, s.rank, s.counts,
                           FPART_RANK_SORT_MIN);
        hipLaunchKernelGGL(k_fpart_rank_scan, dim3((unsigned)((P.nbins + FPART_RSCAN_BINS - 1) / FPART_RSCAN_BINS)), dim3(FPART_RSCAN_THREADS), 0, nullptr, s.counts, nb,
                           P.nbins, s.totals);
        timed("k_fpart_rank_scatter", [&] {
            hipLaunchKernelGGL(k_fpart_rank_scatter, dim3((unsigned)((nb + 7) / 8 * 8)), dim3(FPART_THREADS), 0, nullptr, F, P.nbins, (const uint16_t *)s.bins,
                               (const uint16_t *)s.rank, (const int32_t *)s.counts, (const int32_t *)s.totals, s.nlive, s.perm);
        });
        CHECK(hipDeviceSynchronize());
    }
    std::printf(ok ? "every permutation equals the stable sort\n" : "FAILED\n");
    return ok ? 0 : 1;
}
