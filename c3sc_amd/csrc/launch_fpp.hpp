// launch_fpp.hpp -- host launcher + registration macro for the fiber-pair (rank-split) kernels.
#pragma once
#include "kernel_fiber_pair.hpp"
#include "registry.hpp"

namespace c3sc {

// LDS doubles a tile needs apart from its staged cores: max(vector exchange after the fold, node-loop rows).
//   rank split: half-swap buffer [NV][RH] rows; L, R rows + three partial-sum blocks + the parked rows (<= NP)
//   node split: the hand-over moves one half of the components at a time through the same [NV][RH] rows; L, R rows + four rows of
//               node values + the parked rows, which stay where the rank split has them
template <class Model, int RP, int K>
__host__ __device__ constexpr size_t fpp_tile_doubles(bool node_split)
{
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

template <class Model, int RP, int K, bool FORCED, bool PART, bool T3 = false>
hipError_t launch_fpp_impl(const KArgs &A, const LaunchIO &io)
{
    constexpr int D = Model::D;
    if (A.ncand > 64) return hipErrorNotSupported; // one lane per candidate fills the table: the per-wave kernel walks longer lists
    // LDS: max(largest staged fixed core, vector exchange, node-loop rows)
    constexpr bool NS = fpp_node_split<Model, RP, K>();
    static_assert(fpp_tile_doubles<Model, RP, K>(NS) <= fpp_tile_doubles<Model, RP, K>(false), "the node split must not need more LDS than the rank split");
    static_assert(!NS || 4 * fpp_tile_doubles<Model, RP, K>(NS) * sizeof(double) <= 160 * 1024, "four node-split workgroups per CU must fit the LDS");
    size_t doubles = fpp_tile_doubles<Model, RP, K>(false); // the rank-split figure in both forms: the footprint does not move
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
    const void *kern = PART ? (const void *)k_fiber_pair_part<Model, RP, K, FORCED> : (const void *)k_fiber_pair<Model, RP, K, FORCED>;
    if constexpr (T3) kern = (const void *)k_fiber_pair_part3<Model, RP, K, FORCED>; // instantiated only where it is registered
    static LaunchCache cache;
    int blocks_per_cu = 1, num_cu = 256;
    hipError_t e = cache.prepare(kern, FPP_THREADS, shmem, blocks_per_cu, num_cu);
    if (e != hipSuccess) return e;
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
    if constexpr (T3)
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

template <class Model, int RP, int K>
hipError_t launch_fpp(const KArgs &A, const LaunchIO &io)
{
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
