// The launches in front of the fiber-pair kernels of a step that are not the pair kernels' own: the ranking kernels of the fiber
// partition pre-pass (fiber_partition_rank.hpp) and the padding of all cores in one launch.  A translation unit of its own, with
// its resource remarks apart in prepass_res/ (Makefile), as the chain kernels have theirs in chain_res/.
#include "fiber_partition_rank.hpp"
#include "pad_cores.hpp"

namespace c3sc {

hipError_t fpart_launch(const PartArgs &P, const int32_t *idx, const PartScratch &s, hipStream_t stream)
{
    const long nb = fpart_blocks(P.F);
    hipLaunchKernelGGL(k_fpart_rank_count, dim3((unsigned)nb), dim3(FPART_THREADS), 0, stream, P, idx, s.bins, s.rank, s.counts, FPART_RANK_SORT_MIN);
    hipLaunchKernelGGL(k_fpart_rank_scan, dim3((unsigned)((P.nbins + FPART_RSCAN_BINS - 1) / FPART_RSCAN_BINS)), dim3(FPART_RSCAN_THREADS), 0, stream,
                       s.counts, nb, P.nbins, s.totals);
    hipLaunchKernelGGL(k_fpart_rank_scatter, dim3((unsigned)((nb + 7) / 8 * 8)), dim3(FPART_THREADS), 0, stream, P.F, P.nbins, (const uint16_t *)s.bins,
                       (const uint16_t *)s.rank, (const int32_t *)s.counts, (const int32_t *)s.totals, s.nlive, s.perm);
    return hipGetLastError();
}

// k_pad_core (c3sc_hip.hip) for every core at once, blockIdx.y = core, as k_core_images takes its jobs: first core [N][RP] (index
// b), last core [N][RP] (index a), middle cores [N][RP*RP] (a + b*RP); padding entries are zero
__global__ void k_pad_cores(double *__restrict__ arena, const PadJobs J, int RP)
{
    const int m = blockIdx.y;
    const int kind = (m == 0) ? 0 : (m == J.d - 1 ? 2 : 1); // 0 first, 1 middle, 2 last
    const double *__restrict__ src = J.src[m];
    double *__restrict__ dst = arena + J.dst[m];
    const int N = J.N[m], r0 = J.r0[m], r1 = J.r1[m];
    const int per = (kind == 1) ? RP * RP : RP;
    const long total = (long)N * per;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int j = (int)(e / per), w = (int)(e - (long)j * per);
        int a, b;
        if (kind == 0) { a = 0; b = w; }
        else if (kind == 2) { a = w; b = 0; }
        else { a = w % RP; b = w / RP; }
        double v = 0.0;
        if (a < r0 && b < r1) v = src[(size_t)j * r0 * r1 + a + (size_t)b * r0];
        dst[e] = v;
    }
}

hipError_t pad_cores_launch(double *arena, const PadJobs &J, int rp, unsigned gridx, hipStream_t stream)
{
    hipLaunchKernelGGL(k_pad_cores, dim3(gridx, (unsigned)J.d), dim3(256), 0, stream, arena, J, rp);
    return hipGetLastError();
}

} // namespace c3sc
