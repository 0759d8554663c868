// fiber_partition_sort.hpp -- the sorting kernels of the fiber partition pre-pass (fiber_partition.hpp), compiled in c3sc_hip.hip alone:
// per-block histograms, a scan of every bin over the blocks, and a scatter in which every block sorts its (bin, position) words.
// C3SC_FIBER_RANK=0 runs them; otherwise the ranking kernels of fiber_partition_rank.hpp run.
#pragma once
#include "fiber_partition.hpp"

namespace c3sc {

__global__ void __launch_bounds__(FPART_THREADS) k_fpart_count(const PartArgs P, const int32_t *__restrict__ idx, uint16_t *__restrict__ bins,
                                                               int32_t *__restrict__ counts)
{
    __shared__ int hist[FPART_MAX_BINS];
    for (int b = threadIdx.x; b < P.nbins; b += FPART_THREADS) hist[b] = 0;
    __syncthreads();
    // a wave instruction takes 64 consecutive fibers (the histogram does not care about the order): 64 x d consecutive indices
    const long f0 = (long)blockIdx.x * FPART_BLOCK + threadIdx.x;
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        const long f = f0 + (long)i * FPART_THREADS;
        if (f < P.F) {
            int bin = P.nbins - 1;
            if (!fiber_dead(P, idx, f)) {
                bin = P.kmaj >= 0 ? idx[f * P.d + P.kmaj] : 0;
                if (P.kmin >= 0) bin = bin * P.nmin + idx[f * P.d + P.kmin];
                bin = min(max(bin, 0), P.nbins - 2); // an index off the grid must not leave the histogram
            }
            bins[f] = (uint16_t)bin;
            atomicAdd(&hist[bin], 1); // a count: its value does not depend on the order
        }
    }
    __syncthreads();
    int32_t *row = counts + (size_t)blockIdx.x * P.nbins;
    for (int b = threadIdx.x; b < P.nbins; b += FPART_THREADS) row[b] = hist[b];
}

// workgroup g scans the bins [16 g, 16 g + 16) over the blocks: counts[b][bin] <- fibers of the bin in the blocks before b,
// totals[bin] <- all of them.  Thread (s, c) takes bin c of the s-th 64th of the blocks: a row's 16 bins are one 64-byte read.  The
// loads of a chunk are issued together (the pass is latency: 16 rows per thread at 2^20 fibers), then summed or rewritten.  Traced
// at 2^20 fibers and 1682 bins: 12.8 us, against 16.9 us for the count and 23.6 us for the scatter, whose sort is the larger cost
// (with 256 threads and one row in flight the scan took 29.7 us); keeping the first walk's partial sums is what is left here.
constexpr int FPART_SCAN_THREADS = 1024, FPART_SCAN_CHUNK = 8;
__global__ void __launch_bounds__(FPART_SCAN_THREADS) k_fpart_scan(int32_t *__restrict__ counts, long nblocks, int nbins, int32_t *__restrict__ totals)
{
    constexpr int NS = FPART_SCAN_THREADS / FPART_SCAN_BINS;
    __shared__ int part[NS][FPART_SCAN_BINS];
    const int c = threadIdx.x % FPART_SCAN_BINS, s = threadIdx.x / FPART_SCAN_BINS;
    const int bin = blockIdx.x * FPART_SCAN_BINS + c;
    const bool on = bin < nbins;
    const long per = (nblocks + NS - 1) / NS, b0 = s * per < nblocks ? s * per : nblocks, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    int sum = 0;
    if (on)
        for (long b = b0; b < b1; b += FPART_SCAN_CHUNK) {
            int v[FPART_SCAN_CHUNK];
#pragma unroll
            for (int q = 0; q < FPART_SCAN_CHUNK; q++) v[q] = b + q < b1 ? counts[(size_t)(b + q) * nbins + bin] : 0;
#pragma unroll
            for (int q = 0; q < FPART_SCAN_CHUNK; q++) sum += v[q];
        }
    part[s][c] = sum;
    __syncthreads();
    int run = 0, total = 0;
    for (int q = 0; q < NS; q++) {
        const int v = part[q][c];
        if (q < s) run += v;
        total += v;
    }
    if (on) {
        for (long b = b0; b < b1; b += FPART_SCAN_CHUNK) {
            int v[FPART_SCAN_CHUNK];
#pragma unroll
            for (int q = 0; q < FPART_SCAN_CHUNK; q++) v[q] = b + q < b1 ? counts[(size_t)(b + q) * nbins + bin] : 0;
#pragma unroll
            for (int q = 0; q < FPART_SCAN_CHUNK; q++) {
                if (b + q < b1) counts[(size_t)(b + q) * nbins + bin] = run;
                run += v[q];
            }
        }
        if (s == 0) totals[bin] = total;
    }
}

__global__ void __launch_bounds__(FPART_THREADS) k_fpart_scatter(long F, int nbins, const uint16_t *__restrict__ bins, const int32_t *__restrict__ counts,
                                                                 const int32_t *__restrict__ totals, int32_t *__restrict__ nlive,
                                                                 int32_t *__restrict__ perm)
{
    __shared__ int base[FPART_MAX_BINS];  // first position of a bin in perm: the prefix over the bin totals
    __shared__ int start[FPART_MAX_BINS]; // where a bin's run starts in the sorted block
    __shared__ unsigned srt[FPART_BLOCK]; // (bin << 10 | position in the block), sorted: stable by construction
    const int tid = threadIdx.x;
    {
        int v[FPART_BIN_PER_THREAD], sum = 0;
#pragma unroll
        for (int i = 0; i < FPART_BIN_PER_THREAD; i++) {
            const int b = tid * FPART_BIN_PER_THREAD + i;
            v[i] = b < nbins ? totals[b] : 0;
            sum += v[i];
        }
        int total;
        int ex = fpart_block_scan(sum, total);
#pragma unroll
        for (int i = 0; i < FPART_BIN_PER_THREAD; i++) {
            base[tid * FPART_BIN_PER_THREAD + i] = ex;
            ex += v[i];
        }
    }
    const long fb = (long)blockIdx.x * FPART_BLOCK;
    if (nbins == 2) { // live and dead only (no key level, or grouping off): the rank is a prefix count, nothing to sort
        if (blockIdx.x == 0 && tid == 0) *nlive = base[1];
        bool dead[FPART_PER_THREAD];
        int live = 0;
#pragma unroll
        for (int i = 0; i < FPART_PER_THREAD; i++) {
            const long f = fb + tid * FPART_PER_THREAD + i;
            dead[i] = f < F ? bins[f] != 0 : true;
            live += dead[i] ? 0 : 1;
        }
        int total;
        const int ex = fpart_block_scan(live, total);
        const int32_t *row = counts + (size_t)blockIdx.x * 2;
        long lpos = (long)row[0] + ex, dpos = (long)base[1] + row[1] + (tid * FPART_PER_THREAD - ex);
#pragma unroll
        for (int i = 0; i < FPART_PER_THREAD; i++) {
            const long f = fb + tid * FPART_PER_THREAD + i;
            if (f < F) {
                if (dead[i]) perm[dpos++] = (int32_t)f;
                else perm[lpos++] = (int32_t)f;
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        const int p = tid * FPART_PER_THREAD + i;
        srt[p] = fb + p < F ? ((unsigned)bins[fb + p] << 10) | (unsigned)p : 0xffffffffu;
    }
    // bitonic sort, ascending: two compare-exchanges per thread and step
    for (int k = 2; k <= FPART_BLOCK; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
#pragma unroll
            for (int e = tid; e < FPART_BLOCK / 2; e += FPART_THREADS) {
                const int lo = ((e & ~(j - 1)) << 1) | (e & (j - 1)), hi = lo | j;
                const unsigned a = srt[lo], b = srt[hi];
                const bool up = (lo & k) == 0;
                if ((a > b) == up) {
                    srt[lo] = b;
                    srt[hi] = a;
                }
            }
        }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) *nlive = base[nbins - 1]; // the dead bin is the last one
    unsigned w[FPART_PER_THREAD];
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        const int s = tid * FPART_PER_THREAD + i;
        w[i] = srt[s];
        if (w[i] != 0xffffffffu && (s == 0 || (srt[s - 1] >> 10) != (w[i] >> 10))) start[w[i] >> 10] = s;
    }
    __syncthreads();
    const int32_t *row = counts + (size_t)blockIdx.x * nbins;
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        if (w[i] != 0xffffffffu) {
            const int s = tid * FPART_PER_THREAD + i, bin = (int)(w[i] >> 10);
            perm[(long)base[bin] + row[bin] + (s - start[bin])] = (int32_t)(fb + (w[i] & 1023u));
        }
    }
}

// enqueue the partition of idx[F][d] on `stream` with the sorting kernels above; s has been carved for (F, P.nbins)
hipError_t fpart_launch_sorting(const PartArgs &P, const int32_t *idx, const PartScratch &s, hipStream_t stream)
{
    const long nb = fpart_blocks(P.F);
    hipLaunchKernelGGL(k_fpart_count, dim3((unsigned)nb), dim3(FPART_THREADS), 0, stream, P, idx, s.bins, s.counts);
    hipLaunchKernelGGL(k_fpart_scan, dim3((unsigned)((P.nbins + FPART_SCAN_BINS - 1) / FPART_SCAN_BINS)), dim3(FPART_SCAN_THREADS), 0, stream, s.counts, nb,
                       P.nbins, s.totals);
    hipLaunchKernelGGL(k_fpart_scatter, dim3((unsigned)nb), dim3(FPART_THREADS), 0, stream, P.F, P.nbins, (const uint16_t *)s.bins,
                       (const int32_t *)s.counts, (const int32_t *)s.totals, s.nlive, s.perm);
    return hipGetLastError();
}

} // namespace c3sc
