// launch_fpp.hpp -- host launcher + registration macro for the fiber-pair (rank-split) kernels.
#pragma once
#include <cstdio>
#include <cstdlib>

#include "kernel_fiber_pair.hpp"
#include "registry.hpp"

namespace c3sc {

// LDS doubles a tile needs apart from its staged cores: max(vector exchange after the fold, node-loop rows).
//   rank split: half-swap buffer [NV][RH] rows; L, R rows + three partial-sum blocks + the parked rows (<= NP)
//   node split: the hand-over moves one half of the components at a time through the same [NV][RH] rows; L, R rows + four rows of
//               node values + the parked rows, which stay where the rank split has them
//   parked node split: the hand-over of the register-held vectors; L, R + four rows of node values + the parked rows + the homes
//               (kernel_fiber_pair.hpp: fpp_parked_rows, which is the larger of the two by construction)
template <class Model, int RP, int K>
__host__ __device__ constexpr size_t fpp_tile_doubles(bool node_split, bool pk = false)
{
    if (pk) return (size_t)fpp_parked_rows<Model, RP, K>() * 64;
    constexpr int NV = PairMap<Model, K>::nv(), NP = NV + 1, RH = RP / 2; // the kernel's own count of folded vectors
    const size_t swap = (size_t)NV * RH * 64;
    const size_t parked = (size_t)(2 * RP + (NP + 1) * 2 + NP) * 64; // where the parked rows start (PX in the kernel)
    const size_t rows = node_split ? parked + (size_t)PairPark<Model, K>::rows() * 64 : parked + (size_t)NP * 64;
    return swap > rows ? swap : rows;
}

// Three-core instantiations (k_fiber_pair_part3) exist where an instantiation file says so, ahead of its registrations:
// C3SC_FPP_TABLE3(Model, RP).  fpp_table3_registered (kernel_common.hpp) tells the host which (dimension count, padded rank) get
// the tables; the two are held together by a static assert in the macro.
template <class Model, int RP>
struct FppTable3 {
    static constexpr bool value = false;
};
#define C3SC_FPP_TABLE3(MODEL, RP)                                                                                              \
    template <>                                                                                                                 \
    struct FppTable3<MODEL, RP> {                                                                                               \
        static constexpr bool value = true;                                                                                     \
        static_assert(fpp_table3_registered(MODEL::D, RP) && fpp_edge_tables<MODEL, RP>(), "the host reserves no tables here"); \
    };
// ... and run for the K that are not on the opt-out list
template <class Model, int RP, int K>
constexpr bool fpp_table3() { return FppTable3<Model, RP>::value && !fpp_table3_optout(Model::D, RP, K); }

// Parked node split (kernel_fiber_pair.hpp: fpp_parked): its kernels stand in a translation unit of their own, which says so with
// C3SC_FPP_PARKED_KERNELS(Model, RP, K); the file that registers the K declares the same launcher with C3SC_FPP_PARKED(Model, RP, K)
// ahead of its registrations and instantiates none of them.
template <class Model, int RP, int K>
struct FppParked {
    static constexpr bool value = false;
};
template <class Model, int RP, int K>
constexpr bool fpp_parked_registered() { return FppParked<Model, RP, K>::value && fpp_parked<Model, RP, K>() > 0; }

template <class Model, int RP, int K, bool FORCED, bool PART, bool T3 = false, bool PK = false>
hipError_t launch_fpp_impl(const KArgs &A, const LaunchIO &io)
{
    constexpr int D = Model::D;
    if (A.ncand > 64) return hipErrorNotSupported; // one lane per candidate fills the table: the per-wave kernel walks longer lists
    // LDS: max(largest staged fixed core, vector exchange, node-loop rows)
    constexpr bool NS = fpp_node_split<Model, RP, K>();
    static_assert(fpp_tile_doubles<Model, RP, K>(NS) <= fpp_tile_doubles<Model, RP, K>(false), "the node split must not need more LDS than the rank split");
    static_assert(!NS || 4 * fpp_tile_doubles<Model, RP, K>(NS) * sizeof(double) <= 160 * 1024, "four node-split workgroups per CU must fit the LDS");
    size_t doubles = fpp_tile_doubles<Model, RP, K>(false); // the rank-split figure in both forms: the footprint does not move
    if constexpr (PK) {
        static_assert(!T3 && fpp_parked<Model, RP, K>() > 0, "a parked kernel where the form is used, behind the two-core tables");
        constexpr size_t pk = fpp_tile_doubles<Model, RP, K>(true, true);
        // four workgroups per CU with the tables of the bench grid (N = 41, nine candidates) behind the rows
        static_assert(4 * (pk * sizeof(double) + 1560) <= 160 * 1024, "four parked workgroups per CU must fit the LDS");
        if (pk > doubles) doubles = pk;
    }
    for (int m = 0; m < D; m++) {
        if (m == K || fpp_direct<Model, RP>()) continue; // no staged core when the fold reads the cores directly
        const int elems = (m == 0 || m == D - 1) ? RP : RP * RP;
        const size_t need = ((size_t)A.ngrid[m] * fpl_lds_stride(elems) + 1) & ~(size_t)1; // whole 16-byte LDS-DMA pieces
        if (need > doubles) doubles = need;
    }
    // wave-uniform tables (candidates, nodes of dim K) behind everything else: they persist across tiles
    KArgs B = A;
    B.tbl_off = (int)doubles;
    doubles += (size_t)CandLds<Model>::doubles(A.ncand) + (size_t)NodeLds<Model, K>::doubles(A.N);
    const size_t shmem = doubles * sizeof(double);
    static_assert(!T3 || PART, "the three-core kernel is a partitioned one");
    const void *kern = nullptr;
    if constexpr (PK) // ... and the parked kernels' file instantiates none of the kernels they stand in for
        kern = PART ? (const void *)k_fiber_pair_part_pk<Model, RP, K, FORCED> : (const void *)k_fiber_pair_pk<Model, RP, K, FORCED>;
    else if constexpr (T3) kern = (const void *)k_fiber_pair_part3<Model, RP, K, FORCED>; // instantiated only where it is registered
    else kern = PART ? (const void *)k_fiber_pair_part<Model, RP, K, FORCED> : (const void *)k_fiber_pair<Model, RP, K, FORCED>;
    static LaunchCache cache;
    int blocks_per_cu = 1, num_cu = 256;
    hipError_t e = cache.prepare(kern, FPP_THREADS, shmem, blocks_per_cu, num_cu);
    if (e != hipSuccess) return e;
    if (PK && getenv("C3SC_VERBOSE")) fprintf(stderr, "c3sc: parked node split K=%d: %zu B of LDS, %d workgroups per CU\n", K, shmem, blocks_per_cu);
    const long ntiles = (A.F + 63) / 64;
    const long cap = (long)num_cu * blocks_per_cu;
    // Persistent workgroups (one per resident slot, striding over the tiles) amortise the per-workgroup set-up, but a
    // static split leaves the slots that drew the slow tiles running at the end.  Once there are many tiles per slot the
    // hardware dispatcher balances better with one workgroup per tile (car7d, 2^20 fibers = 16 tiles per slot: 1.84 vs
    // 1.92 ms; at 2 tiles per slot it is the other way round, 0.290 vs 0.270 ms, and at 4 they are equal).  In between is worse
    // still: 2 / 4 / 8 tiles per workgroup at 2^20 fibers take 1.85 / 1.92 / 2.05 ms against 1.82 (the last round of a coarser
    // grid leaves slots idle).
    int grid = (int)(ntiles < cap ? ntiles : cap);
    if (ntiles >= 8 * cap && ntiles < 0x7fffffffL) grid = (int)ntiles;
    if (grid < 1) grid = 1;
    if constexpr (PK && PART)
        hipLaunchKernelGGL((k_fiber_pair_part_pk<Model, RP, K, FORCED>), dim3(grid), dim3(FPP_THREADS), shmem, io.stream, B, io.ro, io.idx, io.out,
                           io.uidx, io.absorbed, io.perm, io.nlive);
    else if constexpr (PK)
        hipLaunchKernelGGL((k_fiber_pair_pk<Model, RP, K, FORCED>), dim3(grid), dim3(FPP_THREADS), shmem, io.stream, B, io.ro, io.idx, io.out, io.uidx,
                           io.absorbed);
    else if constexpr (T3)
        hipLaunchKernelGGL((k_fiber_pair_part3<Model, RP, K, FORCED>), dim3(grid), dim3(FPP_THREADS), shmem, io.stream, B, io.ro, io.idx, io.out,
                           io.uidx, io.absorbed, io.perm, io.nlive);
    else if constexpr (PART)
        hipLaunchKernelGGL((k_fiber_pair_part<Model, RP, K, FORCED>), dim3(grid), dim3(FPP_THREADS), shmem, io.stream, B, io.ro, io.idx, io.out,
                           io.uidx, io.absorbed, io.perm, io.nlive);
    else
        hipLaunchKernelGGL((k_fiber_pair<Model, RP, K, FORCED>), dim3(grid), dim3(FPP_THREADS), shmem, io.stream, B, io.ro, io.idx, io.out, io.uidx,
                           io.absorbed);
    return hipGetLastError();
}

// all four parked kernels of a K (plain and partitioned, minimising and policy evaluation) behind one function, so that one
// explicit instantiation carries them
template <class Model, int RP, int K>
hipError_t launch_fpp_parked(const KArgs &A, const LaunchIO &io)
{
    if (io.perm) return A.forced ? launch_fpp_impl<Model, RP, K, true, true, false, true>(A, io) : launch_fpp_impl<Model, RP, K, false, true, false, true>(A, io);
    return A.forced ? launch_fpp_impl<Model, RP, K, true, false, false, true>(A, io) : launch_fpp_impl<Model, RP, K, false, false, false, true>(A, io);
}
#define C3SC_FPP_PARKED(MODEL, RP, K)                                                                        \
    template <>                                                                                              \
    struct FppParked<MODEL, RP, K> {                                                                         \
        static constexpr bool value = true;                                                                  \
        static_assert(fpp_parked<MODEL, RP, K>() > 0, "no parked node split for this instantiation");        \
    };                                                                                                       \
    extern template hipError_t launch_fpp_parked<MODEL, RP, K>(const KArgs &, const LaunchIO &);
#define C3SC_FPP_PARKED_KERNELS(MODEL, RP, K) template hipError_t launch_fpp_parked<MODEL, RP, K>(const KArgs &, const LaunchIO &);

template <class Model, int RP, int K>
hipError_t launch_fpp(const KArgs &A, const LaunchIO &io)
{
    static_assert(!(fpp_parked_registered<Model, RP, K>() && fpp_table3<Model, RP, K>()), "one replacement kernel per K");
    if constexpr (fpp_parked_registered<Model, RP, K>()) // io.parked: not switched off (C3SC_PAIR_PARKED=0 runs the rank-split kernels)
        if (io.parked) return launch_fpp_parked<Model, RP, K>(A, io);
    if constexpr (fpp_table3<Model, RP, K>()) // io.tab3: the host reserved the tables, built them and did not switch them off
        if (io.perm && io.tab3) return A.forced ? launch_fpp_impl<Model, RP, K, true, true, true>(A, io) : launch_fpp_impl<Model, RP, K, false, true, true>(A, io);
    if (io.perm) return A.forced ? launch_fpp_impl<Model, RP, K, true, true>(A, io) : launch_fpp_impl<Model, RP, K, false, true>(A, io);
    return A.forced ? launch_fpp_impl<Model, RP, K, true, false>(A, io) : launch_fpp_impl<Model, RP, K, false, false>(A, io);
}

#define C3SC_REG_FPP1(MODEL_ID, RP, K, ...)                                                                   \
    static Registrar C3SC_CAT(reg_fpp_, __COUNTER__)(KernelEntry{                                             \
        MODEL_ID, __VA_ARGS__::D, RP, 0, C3SC_VARIANT_FIBER_PAIR, 128, K, &launch_fpp<__VA_ARGS__, RP, K>, \
        "k_fiber_pair<" #__VA_ARGS__ "," #RP ",K=" #K ">"});

} // namespace c3sc
