// fiber_partition.hpp -- stable partition of a fiber batch for the fiber-pair kernel: live fibers first, absorbed ones last, and
// the live ones grouped by the indices of the fold levels next to K.
//
// A fiber with a FIXED index on an absorbing face is absorbed at every node (fixed_neighbors returns true for that dimension):
// its values are Model::boundcost, whatever the fold and the node loop compute.  k_fiber_pair maps one fiber to a lane, so it
// can only leave that work out for 64 such fibers at a time: the batch is reordered so that they share tiles.  In the same way a
// tile whose 64 fibers share the index of a fold level applies ONE matrix at that level, from SGPRs instead of through a staged
// core (kernel_fiber_pair.hpp: grouped fold), so the live fibers are ordered by the indices of up to two such levels
// (kernel_common.hpp: fpp_key_levels; fpart_plan below says how many).
//   perm[0 .. nlive)  the live fibers, keys (major index, minor index) ascending, batch order inside a key
//   perm[nlive .. F)  the dead ones, in batch order
// A stable counting sort over bins (key, then one bin for the dead) in three launches on the caller's stream, no host
// synchronisation: per-block histograms (and one bin number per fiber); an exclusive scan of every bin over the blocks, 16 bins per
// workgroup; the scatter, where a block sorts its (bin, position) words in LDS to rank each fiber among the block's own.  The
// order is a function of the batch alone -- the histogram's LDS atomics only count, no atomic decides a position: discounted
// models choose the form of their discount factor by wave vote, so a fiber's bits may depend on its tile-mates, and tile-mates
// must not change from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_common.hpp"

namespace c3sc {

constexpr int FPART_THREADS = 256, FPART_PER_THREAD = 4, FPART_BLOCK = FPART_THREADS * FPART_PER_THREAD;
static_assert(FPART_BLOCK == 1024, "the scatter packs (bin, position in the block) into one word with 10 position bits");
// Cap on the bins of one pass.  The counter scratch is blocks x bins x 4 B = 4 bins B per fiber: at the cap 8 B per fiber, under a
// third of what the pass reads anyway (the index list of a 7-D batch: 28 B per fiber).  It is also what the scatter keeps in LDS
// (8 bins per thread, two tables of 8 KB) and holds car7d's 41 x 41 + 1 bins.
constexpr int FPART_BIN_PER_THREAD = 8, FPART_MAX_BINS = FPART_THREADS * FPART_BIN_PER_THREAD;
// Floor on the mean number of live fibers per bin below which the minor key is dropped (and the major one where it alone falls
// below it).  A bin of s fibers covers s / 64 tiles and one tile straddles each bin boundary, so about 1 - 64 / s of the tiles are
// uniform: counted on the CPU with car7d's random fibers, 2^20 fibers (624 per bin) give 88.8-89.9 % of the tiles uniform in both
// keys, 2^19 (312 per bin) 77.5-79.8 %.  Below 128 per bin most tiles straddle two bins.
constexpr long FPART_MIN_PER_BIN = 128;
constexpr int FPART_SCAN_BINS = 16; // bins per workgroup of the scan: one 64-byte piece of a histogram row

struct PartArgs {
    int d, k;
    long F;
    int ngrid[MAXD];
    int bctype[MAXD];
    int kmaj = -1, kmin = -1; // key dimensions, -1: none
    int nmin = 1;             // bins per major index
    int nbins = 2;            // keys + the dead bin (the last one)
};

// How many key levels a launch groups by: two, one or none, from F and the grid alone.  floor: fibers per bin (< 0: no grouping).
constexpr void fpart_plan(PartArgs &P, KeyLevels kl, long floor)
{
    P.kmaj = P.kmin = -1;
    P.nmin = 1;
    P.nbins = 2;
    if (floor < 0 || kl.n < 1) return;
    const long nmaj = P.ngrid[kl.major];
    if (nmaj + 1 > FPART_MAX_BINS || P.F < floor * nmaj) return;
    P.kmaj = kl.major;
    P.nbins = (int)nmaj + 1;
    if (kl.n < 2) return;
    const long nkeys = nmaj * P.ngrid[kl.minor];
    if (nkeys + 1 > FPART_MAX_BINS || P.F < floor * nkeys) return;
    P.kmin = kl.minor;
    P.nmin = P.ngrid[kl.minor];
    P.nbins = (int)nkeys + 1;
}

// scratch of one partition, carved from a block of fpart_bytes(F, nbins) (the context keeps one block per stream a batch may run on)
struct PartScratch {
    int32_t *perm = nullptr;   // [F]
    int32_t *counts = nullptr; // [nblocks][nbins] fibers of a bin in a block, then those in the blocks before it
    int32_t *totals = nullptr; // [nbins]
    int32_t *nlive = nullptr;  // [1]
    uint16_t *bins = nullptr;  // [F] bin of a fiber
};

__host__ __device__ constexpr size_t fpart_align(size_t b) { return (b + 255) & ~(size_t)255; }
constexpr long fpart_blocks(long F) { return (F + FPART_BLOCK - 1) / FPART_BLOCK; }
// byte offsets of the regions in that block, in PartScratch's order; end: the size of the block
struct PartOffsets {
    size_t perm, counts, totals, nlive, bins, end;
};
constexpr PartOffsets fpart_offsets(long F, int nbins)
{
    PartOffsets o{};
    o.perm = 0;
    o.counts = o.perm + fpart_align((size_t)F * 4);
    o.totals = o.counts + fpart_align((size_t)fpart_blocks(F) * nbins * 4);
    o.nlive = o.totals + fpart_align((size_t)nbins * 4);
    o.bins = o.nlive + fpart_align(4);
    o.end = o.bins + fpart_align((size_t)F * 2);
    return o;
}
constexpr size_t fpart_bytes(long F, int nbins) { return fpart_offsets(F, nbins).end; }
inline PartScratch fpart_carve(void *base, long F, int nbins)
{
    const PartOffsets o = fpart_offsets(F, nbins);
    PartScratch s;
    char *p = (char *)base;
    s.perm = (int32_t *)(p + o.perm);
    s.counts = (int32_t *)(p + o.counts);
    s.totals = (int32_t *)(p + o.totals);
    s.nlive = (int32_t *)(p + o.nlive);
    s.bins = (uint16_t *)(p + o.bins);
    return s;
}

// the fiber is absorbed at every node: exactly what the kernels accumulate into fiber_abs
__device__ inline bool fiber_dead(const PartArgs &P, const int32_t *__restrict__ idx, long f)
{
    bool dead = false;
    for (int m = 0; m < P.d; m++) {
        if (m == P.k) continue;
        int lo, hi;
        dead = fixed_neighbors(idx[f * P.d + m], P.ngrid[m], P.bctype[m], lo, hi) || dead;
    }
    return dead;
}

// exclusive prefix of v over the workgroup (FPART_THREADS threads, thread order); total: the sum
__device__ inline int fpart_block_scan(int v, int &total)
{
    __shared__ int wsum[FPART_THREADS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads(); // wsum of a previous call has been read
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < FPART_THREADS / 64; q++) {
        if (q < w) before += wsum[q];
        total += wsum[q];
    }
    return before + inc - v;
}

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

// enqueue the partition of idx[F][d] on `stream`; s has been carved for (F, P.nbins)
inline hipError_t fpart_launch(const PartArgs &P, const int32_t *idx, const PartScratch &s, hipStream_t stream)
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
