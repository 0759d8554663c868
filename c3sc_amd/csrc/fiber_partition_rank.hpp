// fiber_partition_rank.hpp -- the kernels fpart_launch enqueues (fiber_partition.hpp says what the pre-pass is for and what it
// must produce; this file is compiled in prepass.hip alone).
//
// A stable counting sort over bins (key, then one bin for the dead) in three launches on the caller's stream, no host
// synchronisation:
//   count    per-block histograms, one bin number per fiber, and one RANK per fiber: how many fibers of its bin stand in front of
//            it in its own block of 1024;
//   scan     an exclusive scan of every bin over the blocks, 32 bins per workgroup, the rows of a thread kept in registers;
//   scatter  perm[base[bin] + counts[block][bin] + rank] = fiber: a gather and a store, every XCD on an eighth of the batch.
// The rank is a function of the batch alone.  The histogram's LDS atomics count, and the slot a live fiber draws from them only
// says where in its bin's list it writes its position; its rank is the number of SMALLER positions in that list, whatever their
// order.  A dead fiber's rank is a prefix count by wave ballots (the dead bin holds a tenth of a random car7d batch, far more than any
// key's bin).  A block whose fullest key bin reaches FPART_RANK_SORT_MIN fibers sorts its (bin, position) words instead, at a cost
// that does not grow with the bin.  No atomic decides a position: discounted models choose the form of their discount factor by
// wave vote, so a fiber's bits may depend on its tile-mates, and tile-mates must not change from run to run.
// With two bins (no key level, or the grouping off) the count ranks nothing and the scatter ranks by a prefix count of its own.
#pragma once
#include "fiber_partition.hpp"

namespace c3sc {

// Fibers in the fullest key bin of a block from which the count ranks by sorting: below it every fiber counts the smaller
// positions in its bin's list, a loop as long as the bin (1024 fibers over 1681 keys: 0.6 per bin, the fullest holds 4 or 5).
// Chosen by timing both paths at 2^20 fibers with n fibers in the fullest bin of EVERY block (tools/fpart_rank_switch.hip,
// profiles/r10_car7d_prepass.txt): the lists take 15.8 us per launch at n = 1, 19.6 at 16, 23.7 at 32, 27.8 at 48, 31.8 at 64,
// 39.6 at 96, 80 at 256, 238 at 896; the sort 32.6-33.0 whatever n.  They cross at 64.
constexpr int FPART_RANK_SORT_MIN = 64;

// Thread t takes the fibers at the block's positions t, 256 + t, 512 + t, 768 + t: a wave instruction takes 64 consecutive fibers,
// 64 x d consecutive indices.  sort_min: FPART_RANK_SORT_MIN (an argument so that both paths can be timed on one batch).
__global__ void __launch_bounds__(FPART_THREADS) k_fpart_rank_count(const PartArgs P, const int32_t *__restrict__ idx, uint16_t *__restrict__ bins,
                                                               uint16_t *__restrict__ rank, int32_t *__restrict__ counts, int sort_min)
{
    __shared__ int hist[FPART_MAX_BINS];
    __shared__ int start[FPART_MAX_BINS];  // where a bin's list (or its run in the sorted block) starts
    __shared__ unsigned list[FPART_BLOCK]; // positions of the live fibers, bin after bin; or (bin << 10 | position), sorted
    __shared__ int ndead[FPART_PER_THREAD][FPART_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int b = tid; b < P.nbins; b += FPART_THREADS) hist[b] = 0;
    __syncthreads();
    const long fb = (long)blockIdx.x * FPART_BLOCK;
    const int deadbin = P.nbins - 1;
    int bin[FPART_PER_THREAD], slot[FPART_PER_THREAD], dbefore[FPART_PER_THREAD];
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        const long f = fb + i * FPART_THREADS + tid;
        bin[i] = -1;
        slot[i] = 0;
        if (f < P.F) {
            int b = deadbin;
            if (!fiber_dead(P, idx, f)) {
                b = P.kmaj >= 0 ? idx[f * P.d + P.kmaj] : 0;
                if (P.kmin >= 0) b = b * P.nmin + idx[f * P.d + P.kmin];
                b = min(max(b, 0), P.nbins - 2); // an index off the grid must not leave the histogram
            }
            bin[i] = b;
            bins[f] = (uint16_t)b;
            slot[i] = atomicAdd(&hist[b], 1); // a count, and a place in the bin's list: neither decides a position
        }
        const unsigned long long dm = __ballot(bin[i] == deadbin);
        dbefore[i] = __popcll(dm & ((1ull << lane) - 1ull));
        if (lane == 0) ndead[i][wv] = __popcll(dm);
    }
    __syncthreads();
    int32_t *row = counts + (size_t)blockIdx.x * fpart_stride(P.nbins);
    for (int b = tid; b < P.nbins; b += FPART_THREADS) row[b] = hist[b];
    if (P.nbins == 2) return; // live and dead only: the scatter ranks by a prefix count
    // the dead: those at smaller positions, by the ballots
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        int r = dbefore[i];
#pragma unroll
        for (int q = 0; q < FPART_PER_THREAD * (FPART_THREADS / 64); q++)
            if (q < i * (FPART_THREADS / 64) + wv) r += ndead[q / (FPART_THREADS / 64)][q % (FPART_THREADS / 64)];
        if (bin[i] == deadbin) rank[fb + i * FPART_THREADS + tid] = (uint16_t)r;
    }
    // the live: every key bin's list starts at the prefix over the histogram; the fullest one picks the path for the block
    int v[FPART_BIN_PER_THREAD], sum = 0, most = 0;
#pragma unroll
    for (int i = 0; i < FPART_BIN_PER_THREAD; i++) {
        const int b = tid * FPART_BIN_PER_THREAD + i;
        v[i] = b < deadbin ? hist[b] : 0;
        sum += v[i];
        most = max(most, v[i]);
    }
    if (!__syncthreads_or(most >= sort_min)) {
        int total;
        int ex = fpart_block_scan(sum, total);
#pragma unroll
        for (int i = 0; i < FPART_BIN_PER_THREAD; i++) {
            start[tid * FPART_BIN_PER_THREAD + i] = ex;
            ex += v[i];
        }
        __syncthreads();
        int s0[FPART_PER_THREAD], n[FPART_PER_THREAD], r[FPART_PER_THREAD], nmost = 0;
#pragma unroll
        for (int i = 0; i < FPART_PER_THREAD; i++) {
            const bool live = bin[i] >= 0 && bin[i] != deadbin;
            s0[i] = live ? start[bin[i]] : 0;
            n[i] = live ? hist[bin[i]] : 0;
            r[i] = 0;
            nmost = max(nmost, n[i]);
            if (live) list[s0[i] + slot[i]] = (unsigned)(i * FPART_THREADS + tid);
        }
        __syncthreads();
        // the four fibers of a thread walk their lists together: four LDS reads in flight
        for (int j = 0; j < nmost; j++) {
#pragma unroll
            for (int i = 0; i < FPART_PER_THREAD; i++)
                if (j < n[i]) r[i] += list[s0[i] + j] < (unsigned)(i * FPART_THREADS + tid) ? 1 : 0;
        }
#pragma unroll
        for (int i = 0; i < FPART_PER_THREAD; i++)
            if (n[i] > 0) rank[fb + i * FPART_THREADS + tid] = (uint16_t)r[i];
        return;
    }
    // a full bin: bitonic sort of the live fibers' (bin << 10 | position) words, ascending and stable by construction; two
    // compare-exchanges per thread and step
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        const int p = i * FPART_THREADS + tid;
        list[p] = bin[i] >= 0 && bin[i] != deadbin ? ((unsigned)bin[i] << 10) | (unsigned)p : 0xffffffffu;
    }
    for (int k = 2; k <= FPART_BLOCK; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
#pragma unroll
            for (int e = tid; e < FPART_BLOCK / 2; e += FPART_THREADS) {
                const int lo = ((e & ~(j - 1)) << 1) | (e & (j - 1)), hi = lo | j;
                const unsigned a = list[lo], b = list[hi];
                const bool up = (lo & k) == 0;
                if ((a > b) == up) {
                    list[lo] = b;
                    list[hi] = a;
                }
            }
        }
    __syncthreads();
    unsigned w[FPART_PER_THREAD];
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        const int s = tid * FPART_PER_THREAD + i;
        w[i] = list[s];
        if (w[i] != 0xffffffffu && (s == 0 || (list[s - 1] >> 10) != (w[i] >> 10))) start[w[i] >> 10] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++)
        if (w[i] != 0xffffffffu) rank[fb + (w[i] & 1023u)] = (uint16_t)(tid * FPART_PER_THREAD + i - start[w[i] >> 10]);
}

// workgroup g scans the bins [32 g, 32 g + 32) over the blocks: counts[b][bin] <- fibers of the bin in the blocks before b,
// totals[bin] <- all of them.  Thread (s, c) takes bin c of the s-th 32nd of the blocks: a row's 32 bins are one 128-byte piece.  Up
// to FPART_RSCAN_KEEP rows per thread (2^20 fibers: 32) are loaded once, all loads issued together (the pass is latency), kept in
// registers and rewritten from them; a longer batch walks its rows twice, 8 at a time.  Rows of counts are fpart_stride ints
// apart, whole 128-byte lines, so a workgroup's pieces are lines of its own.  Timed back to back at 2^20 fibers and 1682 bins
// (tools/fpart_rank_switch.hip): 8.4 us; with rows 1682 ints apart, where neighbouring workgroups on different XCDs share every
// line, 12.1 us, and there with 16 bins and 16 rows 13.7 (two walks: 13.8), with 8 bins and 512 threads 16.0, with 4 bins and 256
// threads 16.3 -- the fewer bytes of a row a workgroup takes, the more workgroups fetch the same lines.
constexpr int FPART_RSCAN_BINS = FPART_LINE_INTS; // bins per workgroup of the scan: one 128-byte line of a histogram row
constexpr int FPART_RSCAN_THREADS = 1024, FPART_RSCAN_CHUNK = 8, FPART_RSCAN_SEGS = FPART_RSCAN_THREADS / FPART_RSCAN_BINS, FPART_RSCAN_KEEP = 32;
__global__ void __launch_bounds__(FPART_RSCAN_THREADS) k_fpart_rank_scan(int32_t *__restrict__ counts, long nblocks, int nbins, int32_t *__restrict__ totals)
{
    constexpr int NS = FPART_RSCAN_SEGS;
    __shared__ int part[NS][FPART_RSCAN_BINS];
    const int c = threadIdx.x % FPART_RSCAN_BINS, s = threadIdx.x / FPART_RSCAN_BINS;
    const int bin = blockIdx.x * FPART_RSCAN_BINS + c;
    const bool on = bin < nbins;
    const int stride = fpart_stride(nbins);
    const long per = (nblocks + NS - 1) / NS, b0 = s * per < nblocks ? s * per : nblocks, b1 = b0 + per < nblocks ? b0 + per : nblocks;
    const bool keep = per <= FPART_RSCAN_KEEP; // the same for every thread of the launch
    int kept[FPART_RSCAN_KEEP];
    int sum = 0;
    if (on && keep) {
        // a row past the segment is read at the batch's last row and dropped: loads without a branch between them
#pragma unroll
        for (int q = 0; q < FPART_RSCAN_KEEP; q++) {
            const long b = b0 + q < b1 ? b0 + q : nblocks - 1;
            kept[q] = counts[(size_t)b * stride + bin];
        }
#pragma unroll
        for (int q = 0; q < FPART_RSCAN_KEEP; q++) {
            kept[q] = b0 + q < b1 ? kept[q] : 0;
            sum += kept[q];
        }
    } else if (on) {
        for (long b = b0; b < b1; b += FPART_RSCAN_CHUNK) {
            int v[FPART_RSCAN_CHUNK];
#pragma unroll
            for (int q = 0; q < FPART_RSCAN_CHUNK; q++) v[q] = b + q < b1 ? counts[(size_t)(b + q) * stride + bin] : 0;
#pragma unroll
            for (int q = 0; q < FPART_RSCAN_CHUNK; q++) sum += v[q];
        }
    }
    part[s][c] = sum;
    __syncthreads();
    int run = 0, total = 0;
    for (int q = 0; q < NS; q++) {
        const int v = part[q][c];
        if (q < s) run += v;
        total += v;
    }
    if (!on) return;
    if (s == 0) totals[bin] = total;
    if (keep) {
#pragma unroll
        for (int q = 0; q < FPART_RSCAN_KEEP; q++) {
            if (b0 + q < b1) counts[(size_t)(b0 + q) * stride + bin] = run;
            run += kept[q];
        }
        return;
    }
    for (long b = b0; b < b1; b += FPART_RSCAN_CHUNK) {
        int v[FPART_RSCAN_CHUNK];
#pragma unroll
        for (int q = 0; q < FPART_RSCAN_CHUNK; q++) v[q] = b + q < b1 ? counts[(size_t)(b + q) * stride + bin] : 0;
#pragma unroll
        for (int q = 0; q < FPART_RSCAN_CHUNK; q++) {
            if (b + q < b1) counts[(size_t)(b + q) * stride + bin] = run;
            run += v[q];
        }
    }
}

// perm[base[bin] + counts[block][bin] + rank] = fiber, with base[] the prefix over the bin totals; thread t takes the positions of
// the count's thread t
__global__ void __launch_bounds__(FPART_THREADS) k_fpart_rank_scatter(long F, int nbins, const uint16_t *__restrict__ bins, const uint16_t *__restrict__ rank,
                                                                 const int32_t *__restrict__ counts, const int32_t *__restrict__ totals,
                                                                 int32_t *__restrict__ nlive, int32_t *__restrict__ perm)
{
    __shared__ int base[FPART_MAX_BINS]; // first position of a bin in perm
    const int tid = threadIdx.x;
    // Workgroups with the same index modulo 8 share an XCD and its L2 (a matter of speed alone): each such group takes one eighth
    // of the batch in a piece.  A 128-byte line of perm collects the fibers of one bin from some 58 consecutive blocks; written
    // from one L2 it is combined there, written from eight it leaves each of them as a partial line.  Timed back to back at 2^20
    // fibers and 1682 bins: 10.3 us, against 16.2 with block b taken by workgroup b.
    const long blk = (long)(blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;
    if (blk * FPART_BLOCK >= F) return;
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
    const long fb = blk * FPART_BLOCK;
    if (nbins == 2) { // live and dead only (no key level, or grouping off): the rank is a prefix count
        if (blk == 0 && tid == 0) *nlive = base[1];
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
        const int32_t *row = counts + (size_t)blk * fpart_stride(2);
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
    __syncthreads();
    if (blk == 0 && tid == 0) *nlive = base[nbins - 1]; // the dead bin is the last one
    const int32_t *row = counts + (size_t)blk * fpart_stride(nbins);
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        const long f = fb + i * FPART_THREADS + tid;
        if (f < F) {
            const int bin = bins[f];
            const long at = (long)base[bin] + row[bin] + rank[f];
            if (at >= 0 && at < F) perm[at] = (int32_t)f; // always, by construction: a store outside perm must not depend on it

        }
    }
}

} // namespace c3sc
