// fiber_partition.hpp -- stable partition of a fiber batch for the fiber-pair kernel: live fibers first, absorbed ones last.
//
// A fiber with a FIXED index on an absorbing face is absorbed at every node (fixed_neighbors returns true for that dimension):
// its values are Model::boundcost, whatever the fold and the node loop compute.  k_fiber_pair maps one fiber to a lane, so it
// can only leave that work out for 64 such fibers at a time: the batch is reordered so that they share tiles.
//   perm[0 .. nlive)  the live fibers, in batch order
//   perm[nlive .. F)  the dead ones, in batch order
// Three launches on the caller's stream, no host synchronisation: per-block counts (and one flag byte per fiber), an exclusive
// scan of the counts by one workgroup, the scatter.  The order is a function of the batch alone -- no atomics: discounted models
// choose the form of their discount factor by wave vote, so a fiber's bits may depend on its tile-mates, and tile-mates must not
// change from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_common.hpp"

namespace c3sc {

constexpr int FPART_THREADS = 256, FPART_PER_THREAD = 4, FPART_BLOCK = FPART_THREADS * FPART_PER_THREAD;

struct PartArgs {
    int d, k;
    long F;
    int ngrid[MAXD];
    int bctype[MAXD];
};

// scratch of one partition, carved from a block of fpart_bytes(F) (the context keeps one block per stream a batch may run on)
struct PartScratch {
    int32_t *perm = nullptr;   // [F]
    int32_t *blocks = nullptr; // [nblocks] live count per block, then its exclusive prefix
    int32_t *nlive = nullptr;  // [1]
    uint8_t *flags = nullptr;  // [F] 1: dead
};

__host__ __device__ constexpr size_t fpart_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline long fpart_blocks(long F) { return (F + FPART_BLOCK - 1) / FPART_BLOCK; }
inline size_t fpart_bytes(long F)
{
    return fpart_align((size_t)F * 4) + fpart_align((size_t)fpart_blocks(F) * 4) + fpart_align(4) + fpart_align((size_t)F);
}
inline PartScratch fpart_carve(void *base, long F)
{
    PartScratch s;
    char *p = (char *)base;
    s.perm = (int32_t *)p;
    p += fpart_align((size_t)F * 4);
    s.blocks = (int32_t *)p;
    p += fpart_align((size_t)fpart_blocks(F) * 4);
    s.nlive = (int32_t *)p;
    p += fpart_align(4);
    s.flags = (uint8_t *)p;
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

__global__ void __launch_bounds__(FPART_THREADS) k_fpart_count(const PartArgs P, const int32_t *__restrict__ idx, uint8_t *__restrict__ flags,
                                                               int32_t *__restrict__ blocks)
{
    const long f0 = (long)blockIdx.x * FPART_BLOCK + (long)threadIdx.x * FPART_PER_THREAD;
    int live = 0;
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        const long f = f0 + i;
        if (f < P.F) {
            const bool dead = fiber_dead(P, idx, f);
            flags[f] = dead ? 1 : 0;
            live += dead ? 0 : 1;
        }
    }
    int total;
    (void)fpart_block_scan(live, total);
    if (threadIdx.x == 0) blocks[blockIdx.x] = total;
}

// one workgroup: blocks[b] <- live fibers in the blocks before b; *nlive <- all of them
__global__ void __launch_bounds__(FPART_THREADS) k_fpart_scan(int32_t *__restrict__ blocks, long nblocks, int32_t *__restrict__ nlive)
{
    int carry = 0;
    for (long b0 = 0; b0 < nblocks; b0 += FPART_THREADS) {
        const long b = b0 + threadIdx.x;
        const int v = b < nblocks ? blocks[b] : 0;
        int total;
        const int ex = fpart_block_scan(v, total);
        if (b < nblocks) blocks[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *nlive = carry;
}

__global__ void __launch_bounds__(FPART_THREADS) k_fpart_scatter(long F, const uint8_t *__restrict__ flags, const int32_t *__restrict__ blocks,
                                                                 const int32_t *__restrict__ nlive, int32_t *__restrict__ perm)
{
    const long fb = (long)blockIdx.x * FPART_BLOCK, f0 = fb + (long)threadIdx.x * FPART_PER_THREAD;
    bool dead[FPART_PER_THREAD];
    int live = 0;
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        dead[i] = (f0 + i < F) ? flags[f0 + i] != 0 : true;
        live += dead[i] ? 0 : 1;
    }
    int total;
    const int ex = fpart_block_scan(live, total);
    const long live_before = blocks[blockIdx.x];
    long lpos = live_before + ex;                                                    // live fibers before f0
    long dpos = (long)*nlive + (fb - live_before) + ((long)threadIdx.x * FPART_PER_THREAD - ex); // nlive + dead fibers before f0
#pragma unroll
    for (int i = 0; i < FPART_PER_THREAD; i++) {
        if (f0 + i < F) {
            if (dead[i]) perm[dpos++] = (int32_t)(f0 + i);
            else perm[lpos++] = (int32_t)(f0 + i);
        }
    }
}

// enqueue the partition of idx[F][d] on `stream`; s has been carved for F
inline hipError_t fpart_launch(const PartArgs &P, const int32_t *idx, const PartScratch &s, hipStream_t stream)
{
    const long nb = fpart_blocks(P.F);
    hipLaunchKernelGGL(k_fpart_count, dim3((unsigned)nb), dim3(FPART_THREADS), 0, stream, P, idx, s.flags, s.blocks);
    hipLaunchKernelGGL(k_fpart_scan, dim3(1), dim3(FPART_THREADS), 0, stream, s.blocks, nb, s.nlive);
    hipLaunchKernelGGL(k_fpart_scatter, dim3((unsigned)nb), dim3(FPART_THREADS), 0, stream, P.F, (const uint8_t *)s.flags, (const int32_t *)s.blocks,
                       (const int32_t *)s.nlive, s.perm);
    return hipGetLastError();
}

} // namespace c3sc
