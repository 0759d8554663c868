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
// synchronisation: count, scan, scatter.  The order is a function of the batch alone -- the histogram's LDS atomics only count, no
// atomic decides a position: discounted models choose the form of their discount factor by wave vote, so a fiber's bits may depend
// on its tile-mates, and tile-mates must not change from run to run.
// Two sets of kernels produce it.  fpart_launch enqueues the ranking ones (fiber_partition_rank.hpp, compiled in prepass.hip): the
// count ranks every fiber among its block's fibers of its bin and the scatter is a gather and a store.  The kernels of
// fiber_partition_sort.hpp are the ones before them -- per-block histograms (and one bin number per fiber); an exclusive scan of
// every bin over the blocks, 16 bins per workgroup; the scatter, where a block sorts its (bin, position) words in LDS to rank each
// fiber among the block's own -- and stay as fpart_launch_sorting, which C3SC_FIBER_RANK=0 selects in the same build (c3sc_hip.hip:
// partition_fibers).
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
    uint16_t *rank = nullptr;  // [F] fibers of its bin in front of it in its block of 1024 (the ranking kernels with keys only)
};

__host__ __device__ constexpr size_t fpart_align(size_t b) { return (b + 255) & ~(size_t)255; }
constexpr long fpart_blocks(long F) { return (F + FPART_BLOCK - 1) / FPART_BLOCK; }
// ints from one row of counts to the next for the ranking kernels: whole 128-byte lines, so that no two workgroups of their scan
// share a line (the sorting kernels keep their rows nbins ints apart, in the same region)
constexpr int FPART_LINE_INTS = 32;
__host__ __device__ constexpr int fpart_stride(int nbins) { return (nbins + FPART_LINE_INTS - 1) / FPART_LINE_INTS * FPART_LINE_INTS; }
// byte offsets of the regions in that block, in PartScratch's order; end: the size of the block
struct PartOffsets {
    size_t perm, counts, totals, nlive, bins, rank, end;
};
constexpr PartOffsets fpart_offsets(long F, int nbins)
{
    PartOffsets o{};
    o.perm = 0;
    o.counts = o.perm + fpart_align((size_t)F * 4);
    o.totals = o.counts + fpart_align((size_t)fpart_blocks(F) * fpart_stride(nbins) * 4);
    o.nlive = o.totals + fpart_align((size_t)nbins * 4);
    o.bins = o.nlive + fpart_align(4);
    o.rank = o.bins + fpart_align((size_t)F * 2);
    o.end = o.rank + fpart_align((size_t)F * 2);
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
    s.rank = (uint16_t *)(p + o.rank);
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

// the sorting kernels: fiber_partition_sort.hpp (c3sc_hip.hip)
hipError_t fpart_launch_sorting(const PartArgs &P, const int32_t *idx, const PartScratch &s, hipStream_t stream);
// the same with the ranking kernels (prepass.hip)
hipError_t fpart_launch(const PartArgs &P, const int32_t *idx, const PartScratch &s, hipStream_t stream);

} // namespace c3sc
