// kernel_fiber_pair.hpp -- "one fiber per lane, two wavefronts per 64 fibers" Bellman kernel (gfx950).
//
// Fold-once algebra (fold everything that is constant along a fiber into
// L, R and the 2(d-1) neighbour vectors w_m^{-+} / z_m^{-+}; per node only c = G_k[j] R, a = L G_k[j]
// and 2d-1 short dots remain), but the folded vectors do not fit the 256 VALU-addressable VGPRs of a
// lane (2(d-1) r doubles = 240 VGPRs at d = 7, r = 10).  So a WORKGROUP OF TWO WAVEFRONTS owns 64
// fibers and the rank index is split in halves: wave h holds components [h r/2, (h+1) r/2) of every
// neighbour vector (60 doubles), computes the matching half of c and a with the wave-uniform matrix
// element as an SGPR operand (both waves see the same j, their element offsets differ by a wave-uniform
// constant), and produces PARTIAL dots; the two waves exchange the 2d-1 partial sums per node through
// LDS and take turns running the control minimisation (wave 0: even nodes, wave 1: odd nodes, delayed
// by one node pair so the dim-k neighbours are known).  One s_barrier pair per two nodes.
//
// Merged rates (PairPark::merged, PairMap): a control-independent dimension whose rates are constants of the fiber does not
// keep its two vectors -- they are summed rate-weighted into one vector per side of K, so car7d carries 5 to 11 vectors per
// launch instead of 12.
//
// Folding (once per 64-fiber tile): each wave folds the neighbour vectors of half of the dims (full
// length, 6 x r doubles in registers) through the fixed cores staged in LDS -- exactly as the
// fiber-per-lane kernel does -- and the halves are swapped through LDS afterwards.  What is mirrored about K is described once
// (PairMap::Side) and the staged core steps of both sides are one routine (fold_step); the table rows and the lone edge core of
// a side stand in fiber_pair_body once per side (moved into a callable they compile to the same instructions in another order).
//
// Budget: 128-thread workgroups, <= 256 VGPRs (2 waves per SIMD with 4 workgroups per CU), LDS = one
// staged core (33 KB at N = 41, r = 10), reused as the exchange buffer during the node loop.
#pragma once
#include <utility>

#include "fold_lds.hpp"

#ifndef FPP_CGD
#define FPP_CGD 3
#endif
#ifndef FPP_PIPE2
#define FPP_PIPE2 1
#endif
#ifndef FPP_CG
#define FPP_CG 1 // candidates in flight in the discounted scan (one division + exp chain each); 1 where registers are tight
#endif
#ifndef FPP_NV
#define FPP_NV 4 // vectors per pass over a staged matrix in the folding phase (2: 0.361 ms, 3: 0.343, 4: 0.340 on car7d)
#endif

#ifndef FPP_DIRECT_MAXD
#define FPP_DIRECT_MAXD 3
#endif
#ifndef FPP_EDGE_TABLES
#define FPP_EDGE_TABLES 1 // the two outer cores of each side enter through their product table (fpp_edge_tables); 0: a diagnostic build folds them
#endif

#ifndef FPP_NODE_SPLIT
#define FPP_NODE_SPLIT 1 // one node per wavefront at full rank where few vectors remain (fpp_node_split); 0: a diagnostic build splits the rank everywhere
#endif
#ifndef FPP_NODE_SPLIT_VGPRS
#define FPP_NODE_SPLIT_VGPRS 140 // what the full-length vectors of a lane may take: 7 vectors at rank 10, the half-length cost of 12 + merging
#endif
#ifndef FPP_PARKED_K4
#define FPP_PARKED_K4 1 // vectors car7d's K = 4 keeps in LDS under the parked node split (fpp_parked_count): 1 leaves six in registers, 2 five
#endif

namespace c3sc {

constexpr int FPP_THREADS = 128;

// Fold straight from the cores in global memory (fold_lds.hpp: apply_glb) instead of through a staged copy: a 3-D problem
// folds through ONE matrix level at most, and the staged core (30 KB for dubins3d, per 64 fibers) is what holds its
// workgroups at two wavefronts per SIMD -- without it the exchange rows are the LDS footprint (21 KB: three to four).
template <class Model, int RP>
__host__ __device__ constexpr bool fpp_direct() { return Model::D <= FPP_DIRECT_MAXD && RP <= 8; }

// Edge tables.  The first matrix level of a side -- L = G_0[i_0] G_1[i_1] with its four neighbour vectors G_0[i_0 +- 1] G_1[i_1],
// G_0[i_0] G_1[i_1 +- 1], and the same from the right with G_{d-2}, G_{d-1} -- is one function of an index pair, T(a, b), and the
// cores change once per upload, not per fiber: the host builds T over all N_0 N_1 (N_{d-2} N_{d-1}) pairs at the upload
// (k_core_images; kernel_common.hpp: pair_tabL_off / pair_tabR_off; 2 x 134 KB for car7d: L2-resident) and a tile gathers up to five rows of
// RP doubles per side instead of staging two cores and pushing its vectors through one of them.  Where a side consists of the
// edge core alone (K = 1, K = d-2) its rows are read straight from the arena.  Only the staged kernels from d = 4 on: a
// 3-D problem has no side with two cores.
template <class Model, int RP>
__host__ __device__ constexpr bool fpp_edge_tables() { return FPP_EDGE_TABLES && !fpp_direct<Model, RP>() && Model::D >= 4; }

// one table row (16-byte aligned: even RP, 16-double aligned table) as 16-byte loads
template <int RP>
__device__ __forceinline__ void load_row16(const double *__restrict__ p, double (&r)[RP])
{
    typedef double v2d __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < RP / 2; i++) {
        const v2d v = *reinterpret_cast<const v2d *>(p + 2 * i);
        r[2 * i] = v.x;
        r[2 * i + 1] = v.y;
    }
}

// apply the staged matrix G to W[FIRST .. FIRST+COUNT) AND to one extra vector E in the same passes: every pass
// re-reads the 100-element matrix of the lane's node from LDS, and LDS (gathered rows, ~2x bank conflicts) is the
// busiest unit of the folding phase, so the running prefix/suffix rides along instead of taking a pass of its own
template <int RP, int NW, int FIRST, int COUNT, bool ROWVEC>
__device__ inline void apply_core_and(const double *G, double (&W)[NW][RP], double (&E)[RP])
{
    constexpr int N1 = COUNT >= FPP_NV - 1 ? FPP_NV - 1 : COUNT;
    double tmp[N1 + 1][RP];
#pragma unroll
    for (int a = 0; a < RP; a++) tmp[0][a] = E[a];
#pragma unroll
    for (int s = 0; s < N1; s++)
#pragma unroll
        for (int a = 0; a < RP; a++) tmp[s + 1][a] = W[FIRST + s][a];
    if constexpr (ROWVEC) vecmat_lds<RP, N1 + 1>(G, tmp);
    else matvec_lds<RP, N1 + 1>(G, tmp);
#pragma unroll
    for (int a = 0; a < RP; a++) E[a] = tmp[0][a];
#pragma unroll
    for (int s = 0; s < N1; s++)
#pragma unroll
        for (int a = 0; a < RP; a++) W[FIRST + s][a] = tmp[s + 1][a];
    apply_core<RP, NW, FIRST + N1, COUNT - N1, ROWVEC, FPP_NV>(G, W);
}

// apply_core_and with a wave-uniform matrix (fold_lds.hpp: apply_uni): the same vectors per pass, the same sums
template <int RP, int NW, int FIRST, int COUNT, bool ROWVEC>
__device__ __forceinline__ void apply_uni_and(const double *__restrict__ G, double (&W)[NW][RP], double (&E)[RP])
{
    constexpr int N1 = COUNT >= FPP_NV - 1 ? FPP_NV - 1 : COUNT;
    double tmp[N1 + 1][RP];
#pragma unroll
    for (int a = 0; a < RP; a++) tmp[0][a] = E[a];
#pragma unroll
    for (int s = 0; s < N1; s++)
#pragma unroll
        for (int a = 0; a < RP; a++) tmp[s + 1][a] = W[FIRST + s][a];
    apply_uni<RP, N1 + 1, ROWVEC>(G, tmp);
#pragma unroll
    for (int a = 0; a < RP; a++) E[a] = tmp[0][a];
#pragma unroll
    for (int s = 0; s < N1; s++)
#pragma unroll
        for (int a = 0; a < RP; a++) W[FIRST + s][a] = tmp[s + 1][a];
    apply_range_uni<RP, NW, FIRST + N1, COUNT - N1, ROWVEC, FPP_NV>(G, W);
}

// f(std::integral_constant<int, 0>{}), ..., f(std::integral_constant<int, N - 1>{}) in this order
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    [&]<int... Is>(std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }(std::make_integer_sequence<int, N>{});
}

// One staged fold level: `body(uniform, index)` runs the level.  At a key level of the grouped fold (KEY) the tile is asked whether
// its 64 lanes share the level's index v -- the first lane's value and a ballot of the lanes that differ: an SGPR condition and a
// scalar branch, no lane-divergent control flow -- and a tile that does runs the uniform form with that index.
template <bool KEY, class Body>
__device__ __forceinline__ void fold_level(int v, Body &&body)
{
    if constexpr (KEY) {
        const int u = __builtin_amdgcn_readfirstlane(v);
        if (__ballot(v != u) == 0ull) body(std::true_type{}, u);
        else body(std::false_type{}, 0);
    } else
        body(std::false_type{}, 0);
}

__device__ inline void pair_barrier()
{ // workgroup barrier + LDS visibility between the two wavefronts.  Only LDS traffic is exchanged, so only
  // lgkmcnt is drained: a workgroup-scope release fence would also wait (vmcnt(0)) for the scattered
  // output stores of the previous node, which costs microseconds per barrier.
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// One fixed core into LDS by LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane straight into LDS at wave base + 16 lane).
// The source is the core's LDS image in HBM (padded node stride, k_core_image), so the copy is lane-linear.  No VGPRs and
// every piece of the core in flight at once -- the register-staged copy it replaces took three rounds of L2 latency per core
// with eight 16-byte loads per thread in flight.
// `img` must come from KArgs::img_base, not from the kernel's `ro` argument: the intrinsic counts as a memory write, and once a
// pointer based on the __restrict__ `ro` has been handed to it every later load from `ro` is "possibly clobbered" -- the
// wave-uniform core rows of the node loop would stop being scalar loads.
template <int H>
__device__ inline void stage_core_image(double *sK, const double *img, int n_doubles)
{
    typedef __attribute__((address_space(3))) char lds_char;
    typedef __attribute__((address_space(3))) void lds_void;
    typedef const __attribute__((address_space(1))) void glb_void;
    const int pieces = (n_doubles + 1) >> 1;
    const int lane = threadIdx.x & 63;
    // A wave-instruction writes 64 consecutive pieces.  The last round is moved back so that it ends with the image (it
    // re-copies a few pieces: same data to the same place) instead of switching lanes off -- the kernel keeps EXEC untouched
    // (tests/test_kernel_uniform_control_flow.py).  An image of fewer than 64 pieces is followed by repeats of its last piece;
    // the staging area is never smaller than the 11 KB exchange block, so those stay inside it.
    for (int base = H * 64; base < pieces; base += FPP_THREADS) {
        const int b = max(min(base, pieces - 64), 0);
        const int p = min(b + lane, pieces - 1);
        __builtin_amdgcn_global_load_lds((glb_void *)(img + 2 * p), (lds_void *)((lds_char *)sK + 16 * b), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// which wave folds the neighbour pair of dim m (m != K) where nothing is merged (PairMap::owner): alternate by distance from K
// so the O(distance) propagation work is balanced
template <int K>
__host__ __device__ constexpr int pair_owner(int m) { return m < K ? ((K - 1 - m) & 1) : ((m - K) & 1); }

// What a fiber parks in LDS for the moment its nodes are finalised (rows of 64 lanes behind the exchange rows).  Without
// dependency information (Model::HAS_DEPS absent): every fixed coordinate and every table value.  With it: the upwind rates of
// the control-independent dimensions whose drift does not read the varying dimension are constants of the fiber -- formed once
// (upwind_rates, the node loop's own arithmetic) and parked INSTEAD of the coordinates / table values only they needed; the node
// then reads the sum of those rates (and one rate-weighted total of their neighbour values, PairMap) where it formed a drift, two
// compares, four selects and three flops per such dimension (car7d: 3.7 of the 5 control-independent dimensions on average over K).
template <class Model, int K>
struct PairPark {
    static constexpr int D = Model::D, NTAB = Model::NTAB;
    static constexpr unsigned UM = Model::UDEP_MASK, UC = Model::UCONST_MASK, ALL = (1u << D) - 1u;
    __host__ __device__ static constexpr bool has_deps()
    {
        if constexpr (requires { Model::HAS_DEPS; }) return Model::HAS_DEPS;
        else return false;
    }
    __host__ __device__ static constexpr unsigned dep(int m)
    {
        if constexpr (has_deps()) return Model::dep_mask(m);
        else return ALL;
    }
    __host__ __device__ static constexpr unsigned cost_dep()
    {
        if constexpr (has_deps()) return Model::COST_DEP;
        else return ALL;
    }
    // control-independent dimensions (other than K... K itself may be one too) whose rates are constants of the fiber
    __host__ __device__ static constexpr unsigned constd()
    {
        unsigned c = 0;
        if (has_deps())
            for (int m = 0; m < D; m++)
                if (!((UM >> m) & 1u) && !((dep(m) >> K) & 1u)) c |= 1u << m;
        return c;
    }
    // state dimensions whose coordinate (or tables) a node still needs: the costs', the non-constant control-independent drifts',
    // the state-dependent controlled drifts'
    __host__ __device__ static constexpr unsigned need()
    {
        unsigned n = cost_dep();
        for (int m = 0; m < D; m++) {
            const bool ctl = (UM >> m) & 1u, cst = (constd() >> m) & 1u;
            if ((!ctl && !cst) || (ctl && !((UC >> m) & 1u))) n |= dep(m);
        }
        return n & ALL;
    }
    __host__ __device__ static constexpr bool need_x(int m) { return m != K && ((need() >> m) & 1u); }
    __host__ __device__ static constexpr bool need_t(int t) { return Model::tab_dim(t) != K && ((need() >> Model::tab_dim(t)) & 1u); }
    __host__ __device__ static constexpr int row_x(int m)
    {
        int r = 0;
        for (int q = 0; q < m; q++) r += need_x(q);
        return r;
    }
    __host__ __device__ static constexpr int nx() { return row_x(D); }
    __host__ __device__ static constexpr int row_t(int t)
    {
        int r = nx();
        for (int q = 0; q < t; q++) r += need_t(q);
        return r;
    }
    __host__ __device__ static constexpr int nt() { return row_t(NTAB) - nx(); }
    // ... of which every one but K is MERGED: its stencil values enter a node only as pm V- + pp V+, with (pm, pp) constants of
    // the fiber, so its two neighbour vectors are folded rate-weighted into one vector per side of K (PairMap) and the node
    // reads one total PVc and one Qc = sum (pm + pp) for all of them.  K's own rates (its stencil values are the node values
    // of the fiber itself) stay a parked pair.
    __host__ __device__ static constexpr unsigned merged() { return constd() & ~(1u << K); }
    __host__ __device__ static constexpr unsigned rates() { return constd() & (1u << K); }
    __host__ __device__ static constexpr int row_pm(int m)
    {
        int r = nx() + nt();
        for (int q = 0; q < m; q++) r += 2 * ((rates() >> q) & 1u);
        return r;
    }
    __host__ __device__ static constexpr int row_q() { return row_pm(D); }
    __host__ __device__ static constexpr int rows() { return row_q() + (merged() != 0u); }
};

// Slot map of the folded vectors.  Items: the +- pair of every non-merged dimension m != K (item m), the merged vector U_L of
// the merged dimensions left of K (item D) and U_R of those right of it (item D + 1).  Node-loop order (Wh, the exchange rows):
// [U_L] pairs of m < K ascending | [U_R] pairs of m > K ascending; the first nvl() are dotted with c = G_K[j] R, the others
// with a = L G_K[j].
//   U_L = sum_{m merged, m < K} (pm_m w_m^- + pp_m w_m^+): carried through the later cores as ONE vector, U <- U G_m[i_m], plus
//   pm (L G_m[i_m - 1]) + pp (L G_m[i_m + 1]) where m is itself merged; U_R likewise from the right.
// TAB (fpp_edge_tables): the product tables absorb each side's first matrix level -- the fold plan (plan()) and the cost count
// follow it; the slots, NV and the exchange layout do not depend on it.
struct FoldPlan {
    int lfirst, rfirst; // the staged left steps are the cores lfirst .. K-1, the right ones rfirst .. K+1 (descending)
    bool ledge, redge;  // a side's edge core is staged on its own (else: absorbed by a table, read from the arena, or no such side)
    int staged;         // staging rounds per tile
    int products;       // vector-matrix products per tile, both wavefronts, L / R carried once
};
template <class Model, int K, bool TAB = false, bool TAB3 = false>
struct PairMap {
    typedef PairPark<Model, K> PK;
    static constexpr int D = Model::D, NIT = D + 2, UL = D, UR = D + 1;
    __host__ __device__ static constexpr bool mg(int m) { return (PK::merged() >> m) & 1u; }
    // One side of K: the cores 0 .. K-1, folded ascending into the row vector L (LEFT), or D-1 .. K+1, folded descending into
    // the column R.  Everything that is mirrored about K is written here once, in the side's own coordinate: the depth of a
    // core, 0 at the edge core and NC at K.  The kernel runs the staged steps of both sides through it (fold_step).
    template <bool LEFT>
    struct Side {
        static constexpr bool ROWVEC = LEFT;                                  // L <- L G_m, R <- G_m R
        static constexpr int NC = LEFT ? K : D - 1 - K;                       // cores of the side
        static constexpr int EDGE = LEFT ? 0 : D - 1;                         // the edge core
        static constexpr int U = LEFT ? UL : UR;                              // the merged item
        __host__ __device__ static constexpr int depth(int m) { return LEFT ? m : D - 1 - m; }
        __host__ __device__ static constexpr int core(int q) { return LEFT ? q : D - 1 - q; }
        // the product table (tabL: cores 0, 1; tabR: cores d-2, d-1) absorbs the edge core and the next; with TAB3 a side of three
        // cores or more enters through tab3L / tab3R (kernel_common.hpp), which absorb one more.  td(): the cores a table absorbs
        __host__ __device__ static constexpr bool tab() { return TAB && NC >= 2; }
        __host__ __device__ static constexpr int td() { return !tab() ? 0 : (TAB3 && NC >= 3 ? 3 : 2); }
        // the staged steps: first(), then towards K
        __host__ __device__ static constexpr int first() { return core(tab() ? td() : 1); }
        __host__ __device__ static constexpr int nsteps() { return NC - depth(first()) > 0 ? NC - depth(first()) : 0; }
        __host__ __device__ static constexpr int step(int i) { return core(depth(first()) + i); }
        __host__ __device__ static constexpr int first_merged()
        { // the merged dimension at which U is created (the nearest to the edge), -1: none
            for (int q = 0; q < NC; q++)
                if (mg(core(q))) return core(q);
            return -1;
        }
        __host__ __device__ static constexpr int nv()
        {
            int c = count(U);
            for (int q = 0; q < NC; q++) c += count(core(q));
            return c;
        }
        // fold work of U and of the pair of m in vector-matrix products (edge cores combine rows, the tables' levels are
        // gathered rows: free)
        __host__ __device__ static constexpr int cost_u()
        {
            int c = NC - 1 - depth(first_merged()); // U through every core behind the one that creates it ...
            if (td() > depth(first_merged()) + 1) c = NC - td(); // ... that no table absorbs
            for (int q = depth(first()); q < NC; q++) c += 2 * mg(core(q));
            return c;
        }
        __host__ __device__ static constexpr int cost_pair(int m)
        {
            return depth(m) < td() ? 2 * (NC - td()) : (m != EDGE ? 2 : 0) + 2 * (NC - 1 - depth(m));
        }
        // the item the core step m creates: the pair of m, or U at its first merged dimension; -1: none
        __host__ __device__ static constexpr int created(int m) { return !mg(m) ? m : (m == first_merged() ? U : -1); }
        // own vectors of wave H that exist before the step m (created nearer to the edge): a wave keeps its vectors in creation
        // order, left ones first
        template <int H>
        __host__ __device__ static constexpr int before(int m)
        {
            int c = 0;
            for (int q = 0; q < depth(m) && q < NC; q++)
                if (created(core(q)) >= 0 && owner(created(core(q))) == H) c += count(created(core(q)));
            return c;
        }
        template <int H>
        __host__ __device__ static constexpr int base() { return LEFT ? 0 : Side<true>::template before<H>(K); } // first slot in W
        template <int H>
        __host__ __device__ static constexpr int slot(int it) { return base<H>() + before<H>(it == U ? first_merged() : it); }
        // wave H folds what the core step m creates or adds to: the pair of m, or the merged vector
        template <int H>
        __host__ __device__ static constexpr bool owns(int m) { return owner(mg(m) ? U : m) == H; }
    };
    typedef Side<true> SL;
    typedef Side<false> SR;
    __host__ __device__ static constexpr bool valid(int it)
    {
        return it == UL ? SL::first_merged() >= 0 : (it == UR ? SR::first_merged() >= 0 : (it != K && !mg(it)));
    }
    __host__ __device__ static constexpr int count(int it) { return !valid(it) ? 0 : (it < D ? 2 : 1); }
    __host__ __device__ static constexpr int nv() { return SL::nv() + SR::nv(); }
    __host__ __device__ static constexpr int gslot(int it)
    { // first node-loop slot of an item
        if (it == UL) return 0;
        if (it == UR) return SL::nv();
        int c = it < K ? count(UL) : SL::nv() + count(UR);
        for (int m = it < K ? 0 : K + 1; m < it; m++) c += count(m);
        return c;
    }
    __host__ __device__ static constexpr int cost(int it)
    {
        if (!valid(it)) return 0;
        if (it == UL) return SL::cost_u();
        if (it == UR) return SR::cost_u();
        return it < K ? SL::cost_pair(it) : SR::cost_pair(it);
    }
    // What the fold of a tile does: the kernel takes its step ranges from here, the tests its counts.
    __host__ __device__ static constexpr FoldPlan plan()
    {
        // an edge core on its own is staged too unless the tables are on (then it is read from the arena)
        FoldPlan p{SL::first(), SR::first(), K > 0 && !TAB, K < D - 1 && !TAB, 0, 0};
        p.staged = SL::nsteps() + SR::nsteps() + p.ledge + p.redge;
        p.products = SL::nsteps() + SR::nsteps(); // L and R through every staged middle core
        for (int it = 0; it < NIT; it++) p.products += cost(it);
        return p;
    }
    // Grouped fold: the products of the staged level m, both wavefronts -- L or R, the new pair (or the merged share), and every
    // vector created before it; those of the key levels (fpp_key_levels) run from SGPRs in a tile that shares the level's index,
    // and the level's staging round is left out.  The sum over all staged levels is plan().products.
    __host__ __device__ static constexpr int level_products(int m)
    {
        return 3 + (m < K ? SL::template before<0>(m) + SL::template before<1>(m) : SR::template before<0>(m) + SR::template before<1>(m));
    }
    // a key level counts where it is still staged: the three-core tables absorb the minor one of K = 2, 3, 4 (and both of K = 3)
    __host__ __device__ static constexpr bool staged(int m) { return m < K ? m >= SL::first() : (m > K && m <= SR::first()); }
    __host__ __device__ static constexpr int uniform_rounds()
    {
        constexpr KeyLevels kl = fpp_key_levels(D, K, TAB);
        return (kl.n > 0 && staged(kl.major)) + (kl.n > 1 && staged(kl.minor));
    }
    __host__ __device__ static constexpr int uniform_products()
    {
        constexpr KeyLevels kl = fpp_key_levels(D, K, TAB);
        return (kl.n > 0 && staged(kl.major) ? level_products(kl.major) : 0) + (kl.n > 1 && staged(kl.minor) ? level_products(kl.minor) : 0);
    }
    // Which wave folds an item.  Nothing merged: pair_owner (alternate by distance from K).  Otherwise that is no longer balanced
    // -- a side that collapsed to one carried vector costs a fraction of its pairs -- and the items are dealt by their cost
    // count, the most expensive first, each to the wave with less work so far.
    __host__ __device__ static constexpr int owner(int it)
    {
        if (PK::merged() == 0u) return pair_owner<K>(it);
        int load[2] = {0, 0}, own[NIT] = {};
        bool done[NIT] = {};
        for (int n = 0; n < NIT; n++) {
            int best = -1;
            for (int q = 0; q < NIT; q++)
                if (valid(q) && !done[q] && (best < 0 || cost(q) > cost(best))) best = q;
            if (best < 0) break;
            const int h = load[1] < load[0] ? 1 : 0;
            own[best] = h;
            load[h] += cost(best);
            done[best] = true;
        }
        return own[it];
    }
    template <int H>
    __host__ __device__ static constexpr int lslot(int it)
    { // slot of an item in its owner's W
        return (it == UL || it < K) ? SL::template slot<H>(it) : SR::template slot<H>(it);
    }
};

// Node split.  The rank is split over the two wavefronts because 2(d-1) full-length vectors do not fit a lane; where merging left
// few enough of them that they do (car7d at rank 10: K = 0, 1, 4, 5, 6 carry 5 / 6 / 7 / 5 / 5 = 100-140 VGPRs, what the half-length
// ones cost before merging), the split only makes work: every node's NV + 1 partial sums cross through LDS, each wavefront
// fetches 3/4 of G_K[j] for both nodes of a pair, both re-read L and R for both nodes, and there are two barriers per pair.  There
// wavefront h owns the nodes j = h (mod 2) outright: all vectors at full length, the full c, a and NV + 1 dots, one set of scalar
// loads for both products, and only v[j] crosses (one barrier per pair).  Staged instantiations with something merged only;
// everything else compiles as before.
// The opt-out list: instantiations (dimension count, padded rank, K) that measured no faster, or whose node loop gained scratch
// reloads, under the node split.
//   d = 7, rank 10, K = 4 (car7d, 7 vectors): the node loop of wavefront 0 reloads five registers from scratch per node (60 B per
//   lane against none in the rank split) -- taken off before it was timed
//   padded ranks below 10: the rank split leaves those kernels at 130-170 VGPRs, the full-length vectors take 180-230 and with
//   them the third wavefront per SIMD (car7d and lqg6d at rank 4), and lqg6d at rank 8 gains scratch at K = 2, 3 -- none of them
//   has been timed, so they stay as they are
__host__ __device__ constexpr bool fpp_node_split_optout(int d, int rp, int k) { return rp < 10 || (d == 7 && rp == 10 && k == 4); }
template <class Model, int RP, int K>
__host__ __device__ constexpr bool fpp_node_split()
{
    if constexpr (!FPP_NODE_SPLIT || fpp_direct<Model, RP>()) return false;
    else
        return PairPark<Model, K>::merged() != 0u && PairMap<Model, K>::nv() * RP * 2 <= FPP_NODE_SPLIT_VGPRS &&
               !fpp_node_split_optout(Model::D, RP, K);
}

// Parked node split.  A middle K carries more vectors than a lane holds at full length (car7d at rank 10: K = 2, 3, 4 carry
// 9 / 11 / 7; six is what compiles without scratch in the node loop, K = 1's count), but in the node split both wavefronts hold
// identical copies of every vector -- the same 64 fibers, alternate nodes -- so a vector kept in LDS is kept once for both, and
// the node-split node loop needs far fewer rows than the rank split's three partial-sum blocks.  The last P node-loop slots (right
// of K: dotted with a, behind the register dots) are written by their owner straight to home rows above L, R, VX and PX and
// read back inside `stencil`; the other NV - P stay in Wf.  P by (dimension count, padded rank, K), 0 = form not used; the kernels
// of the form are k_fiber_pair_pk / k_fiber_pair_part_pk, instantiated where an instantiation file says so (launch_fpp.hpp:
// C3SC_FPP_PARKED).
__host__ __device__ constexpr int fpp_parked_count(int d, int rp, int k) { return (d == 7 && rp == 10) ? (k == 2 ? 3 : (k == 4 ? FPP_PARKED_K4 : 0)) : 0; }
template <class Model, int RP, int K>
__host__ __device__ constexpr int fpp_parked()
{
    if constexpr (!FPP_NODE_SPLIT || fpp_direct<Model, RP>() || fpp_node_split<Model, RP, K>()) return 0;
    else {
        constexpr int P = PairPark<Model, K>::merged() != 0u ? fpp_parked_count(Model::D, RP, K) : 0;
        // every parked slot lies right of K, and something stays in registers
        return (P > 0 && PairMap<Model, K>::nv() - P >= PairMap<Model, K>::SL::nv() && PairMap<Model, K>::nv() - P > 0) ? P : 0;
    }
}
// LDS rows (64 doubles) of a parked tile: the hand-over X[g][RH] of the register-held vectors from row 0; in the node loop L, R
// (2 RP rows), VX (4), PX from fpp_parked_px_row; the homes above all of them, so the barrier that closes the hand-over closes
// them too.  A home keeps the elements 2i, 2i + 1 of a lane side by side: RP / 2 reads of 16 bytes per vector.
template <int RP>
__host__ __device__ constexpr int fpp_parked_px_row() { return 2 * RP + 4; }
template <class Model, int RP, int K>
__host__ __device__ constexpr int fpp_parked_home_row()
{
    constexpr int hand = (PairMap<Model, K>::nv() - fpp_parked<Model, RP, K>()) * (RP / 2);
    constexpr int low = fpp_parked_px_row<RP>() + PairPark<Model, K>::rows();
    return hand > low ? hand : low;
}
template <class Model, int RP, int K>
__host__ __device__ constexpr int fpp_parked_rows() { return fpp_parked_home_row<Model, RP, K>() + fpp_parked<Model, RP, K>() * RP; }

// the parked rates as node_backup's Pre
template <class Model, int K>
struct PairPre {
    static constexpr unsigned MASK = PairPark<Model, K>::merged(), RATES = PairPark<Model, K>::rates();
    const double *PX;
    int lane;
    double pvc; // the merged slots' totals of this node
    __device__ inline double q() const { return PX[PairPark<Model, K>::row_q() * 64 + lane]; }
    __device__ inline double pv() const { return pvc; }
    __device__ inline double pm(int m) const { return PX[PairPark<Model, K>::row_pm(m) * 64 + lane]; }
    __device__ inline double pp(int m) const { return PX[(PairPark<Model, K>::row_pm(m) + 1) * 64 + lane]; }
};

#define FPP_STAMP(slot)                                                   \
    if (C3SC_STAMPS_ON && (A.dbg & 128)) {                                \
        const unsigned long long now__ = clock64();                       \
        seg[slot] += now__ - tlast;                                       \
        tlast = now__;                                                    \
    }

// One staged core step m of a side (PairMap::Side): the side's running vector V (L or R) and the own vectors W[BASE ..) of wavefront
// H through G_m[i_m]; `combine` is the side's table combine, run behind the side's first staging round.  The tile's locals come as
// arguments and fiber_pair_body calls it from one small lambda per side (left_step, right_step): with the closures of the body
// where they were when each side had its own copy, every pair kernel compiles to the instructions it compiled to then.
template <class Model, int RP, int K, int H, bool PART, bool T3, bool LEFT, int m, int NOWN, class Combine>
__device__ __attribute__((always_inline)) inline void fold_step(const KArgs &A, const double *__restrict__ ro, double *sK,
                                                               const int (&fi)[Model::D], const int (&nbm)[Model::D], const int (&nbp)[Model::D],
                                                               const double (&rpm)[Model::D], const double (&rpp)[Model::D], double (&V)[RP],
                                                               double (&W)[NOWN][RP], unsigned long long (&seg)[12], unsigned long long &tlast,
                                                               Combine &&combine)
{
    constexpr int D = Model::D;
    constexpr bool DIRECT = fpp_direct<Model, RP>();
    typedef PairMap<Model, K, fpp_edge_tables<Model, RP>(), T3> PM;
    typedef typename PM::template Side<LEFT> SD;
    constexpr bool RV = SD::ROWVEC;
    constexpr int BASE = SD::template base<H>();
    constexpr KeyLevels KL = fpp_group_levels(D, RP, K);
    constexpr bool GROUP = PART && KL.n > 0;
    // UNI: the tile shares fi[m] = iu -- one matrix per product, from the arena on the scalar path, nothing staged
    auto body = [&](auto uc, int iu) __attribute__((always_inline)) {
        constexpr bool UNI = decltype(uc)::value;
        constexpr int str = (DIRECT || UNI) ? RP * RP : fpl_lds_stride(RP * RP);
        constexpr int before = SD::template before<H>(m); // own vectors created so far
        constexpr bool PAIR = !PM::mg(m) && PM::owner(m) == H, ACC = PM::mg(m) && PM::owner(SD::U) == H;
        double nw[RP]; // a merged dimension's share of U
        const double *src = sK;
        FPP_STAMP(1)
        if constexpr (DIRECT || UNI) src = ro + A.core_off[m];
        else {
            pair_barrier();
            stage_core_image<H>(sK, A.img_base + A.pair_img_off[m], A.ngrid[m] * str);
            pair_barrier();
        }
        if constexpr (SD::tab() && m == SD::first()) combine();
        FPP_STAMP(7)
        const double *G = src + (UNI ? iu : fi[m]) * str;
        if constexpr (PAIR || ACC) { // the new pair first: it needs the prefix (suffix) BEFORE this core
            double t0[1][RP], t1[1][RP];
#pragma unroll
            for (int a = 0; a < RP; a++) { t0[0][a] = V[a]; t1[0][a] = V[a]; }
            if constexpr (DIRECT) {
                apply_glb<RP, 1, RV>(src + nbm[m] * str, t0);
                apply_glb<RP, 1, RV>(src + nbp[m] * str, t1);
            } else if constexpr (UNI) { // functions of the shared index: uniform too
                apply_uni<RP, 1, RV>(src + __builtin_amdgcn_readfirstlane(nbm[m]) * str, t0);
                apply_uni<RP, 1, RV>(src + __builtin_amdgcn_readfirstlane(nbp[m]) * str, t1);
            } else if constexpr (RV) {
                vecmat_lds<RP, 1>(src + nbm[m] * str, t0);
                vecmat_lds<RP, 1>(src + nbp[m] * str, t1);
            } else {
                matvec_lds<RP, 1>(src + nbm[m] * str, t0);
                matvec_lds<RP, 1>(src + nbp[m] * str, t1);
            }
#pragma unroll
            for (int a = 0; a < RP; a++) {
                if constexpr (PAIR) { W[BASE + before][a] = t0[0][a]; W[BASE + before + 1][a] = t1[0][a]; }
                else nw[a] = fma(rpp[m], t1[0][a], rpm[m] * t0[0][a]);
            }
        }
        if constexpr (DIRECT) {
            double tl[1][RP];
#pragma unroll
            for (int a = 0; a < RP; a++) tl[0][a] = V[a];
            apply_glb<RP, 1, RV>(G, tl);
#pragma unroll
            for (int a = 0; a < RP; a++) V[a] = tl[0][a];
            apply_range_glb<RP, NOWN, BASE, before, RV>(G, W);
        } else if constexpr (UNI)
            apply_uni_and<RP, NOWN, BASE, before, RV>(G, W, V);
        else
            apply_core_and<RP, NOWN, BASE, before, RV>(G, W, V);
        if constexpr (ACC) { // U: created here, or carried through this core above and added to
            constexpr int su = SD::template slot<H>(SD::U);
#pragma unroll
            for (int a = 0; a < RP; a++) W[su][a] = (m == SD::first_merged()) ? nw[a] : W[su][a] + nw[a];
        }
    };
    fold_level<GROUP && (m == KL.major || (KL.n > 1 && m == KL.minor))>(fi[m], body);
}

template <class Model, int RP, int K, int H, bool FORCED, bool PART, bool T3 = false, int PKD = 0>
__device__ __attribute__((always_inline)) inline void fiber_pair_body(const KArgs &A, const double *__restrict__ ro,
                                                                     const int32_t *__restrict__ idx, double *__restrict__ outv,
                                                                     int32_t *__restrict__ uidx, int32_t *__restrict__ absorbed,
                                                                     const int32_t *__restrict__ perm, const int32_t *__restrict__ nlive_p,
                                                                     double *sK, unsigned &st)
{
    constexpr int D = Model::D;
    constexpr int S = 2 * D + 1;
    constexpr int RH = RP / 2;
    typedef PairPark<Model, K> PK;
    constexpr bool ET = fpp_edge_tables<Model, RP>();
    typedef PairMap<Model, K, ET, T3> PM;
    static_assert(!T3 || (PART && ET), "the three-core tables serve the partitioned kernels with edge tables");
    static_assert(PM::nv() == PairMap<Model, K, ET>::nv() && PM::gslot(D + 1) == PairMap<Model, K, ET>::gslot(D + 1),
                  "the table depth moves no slot of the node loop");
    constexpr FoldPlan PL = PM::plan();
    constexpr int NV = PM::nv();                            // folded vectors in total: 2(D-1) when nothing is merged
    constexpr int NVL = PM::SL::nv();                       // ... of which left of K (dotted with c)
    constexpr int NOL = PM::SL::template before<H>(K);      // own left vectors (slots [0, NOL))
    constexpr int NOR = PM::SR::template before<H>(K);      // own right vectors (slots [NOL, NOL+NOR))
    constexpr int NOWN = (NOL + NOR) > 0 ? (NOL + NOR) : 1;
    constexpr int NP = NV + 1; // partial sums per node: NV neighbour values + the node value
    constexpr bool DIRECT = fpp_direct<Model, RP>();
    // Grouped fold (PART only: the pre-pass orders the live fibers by these levels' indices, fiber_partition.hpp).  At a key
    // level both wavefronts ask whether the tile's 64 lanes share fi[m] -- the first lane's value and a ballot of the lanes that
    // differ: an SGPR condition, a scalar branch, the same answer in both wavefronts (they read the same perm entries), so both
    // pass the same barriers.  A tile that does takes the level's matrices from the arena on the scalar path and skips the
    // staging round; each level decides on its own, a mixed one runs the staged code.  Skipping the round is safe for the LDS
    // reuse around it: every read of sK by a wavefront precedes that wavefront's next barrier, and everything that writes sK
    // (a later staging round, the half swap) starts behind a barrier of its own.
    constexpr KeyLevels KL = fpp_group_levels(D, RP, K);
    constexpr bool GROUP = PART && KL.n > 0;
    static_assert(!GROUP || fpp_key_levels(D, K, ET).major == KL.major, "the key levels follow the kernel's own fold plan");
    static_assert(RP % 2 == 0, "rank-split kernel needs an even padded rank");
    const int lane = threadIdx.x & 63;
    const int N = A.N;
    const long ntiles = (A.F + 63) / 64;
    // Absorbed tiles.  With a permutation of the batch (fiber_partition.hpp: live fibers first) lane l of tile t takes fiber
    // perm[64 t + l], and every tile from ceil(nlive / 64) on holds only fibers with a fixed index on an absorbing face: each of
    // their nodes is absorbed (finalize: ab = 1) and its value is Model::boundcost, except the two end nodes of a reflecting or
    // periodic K under the literal end-point rule (vary_neighbors, keep_ends = 0).  Wave-uniform: one scalar load, the same
    // value in both wavefronts, so both pass the same barriers.  PART = false (k_fiber_pair: launches without a partition) compiles
    // none of it.
    int first_dead = 0x7fffffff;
    if constexpr (PART) first_dead = __builtin_amdgcn_readfirstlane((int)(((long)*nlive_p + 63) >> 6));
    unsigned long long seg[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tlast = clock64();
    // candidate and node tables: computed lane-distributed once, then kept in LDS behind the exchange rows and read
    // with wave-uniform addresses -- 16 VGPRs less in the node loop than keeping them in lanes, and no dependence on
    // what a spill does to inactive lanes
    CandLds<Model> cr;
    NodeLds<Model, K> nr;
    {
        CandRegs<Model> cr0;
        cr0.load(A, ro);
        NodeRegs<Model, K> nr0;
        nr0.load(A, ro);
        double *tb = sK + A.tbl_off;
        cr.fill(tb, cr0, A.ncand);
        nr.fill(tb + CandLds<Model>::doubles(A.ncand), nr0, N);
        pair_barrier();
    }

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        FPP_STAMP(7)
        const long f_raw = tile * 64 + lane;
        const bool live = f_raw < A.F;
        const long f_pos = live ? f_raw : A.F - 1;
        long f = f_pos;
        if constexpr (PART) f = (long)perm[f_pos];
        const bool dead_tile = PART && tile >= (long)first_dead;

        if constexpr (PART) if (dead_tile) {
            // the nodes whose value is boundcost whatever the stencil holds: all of them where K absorbs or the ends are
            // consistent -- the tile is done, nothing is staged or folded --, else the interior ones; the wavefronts split them
            // by parity as in the node loop.  x as finalize forms it (PairPark: a coordinate no node reads is not kept).  The
            // block stands in front of the tile set-up and reads its own coordinates: nothing of a live tile is live across it.
            const bool whole = A.bctype[K] == C3SC_ABSORB || A.cends != 0;
            int jb = whole ? 0 : 1;
            const int je = whole ? N : N - 1;
            // parked node split: the first node's output addresses are formed here, per absorbed tile; as constants of the launch
            // they are hoisted out of the tile loop and spilled for the whole kernel (three VGPR pairs)
            if constexpr (PKD > 0) {
                asm volatile("" : "+v"(jb));
                jb = __builtin_amdgcn_readfirstlane(jb);
            }
            double xb[D];
#pragma unroll
            for (int m = 0; m < D; m++) xb[m] = (m != K && PK::need_x(m)) ? ro[A.xg_off[m] + idx[f * D + m]] : 0.0;
            for (int j = jb + ((jb ^ H) & 1); j < je; j += 2) {
                xb[K] = nr.x_at(j);
                outv[(size_t)f * N + j] = Model::boundcost(A.prm, xb);
                if (uidx) uidx[(size_t)f * N + j] = -1;
                if (absorbed) absorbed[(size_t)f * N + j] = 1;
            }
            if (whole) continue;
        }

        int fi[D], nbm[D], nbp[D];
        bool fiber_abs = false;
        double x[D];
#pragma unroll
        for (int m = 0; m < D; m++) {
            fi[m] = (m == K) ? 0 : idx[f * D + m];
            const bool face = fixed_neighbors(fi[m], A.ngrid[m], A.bctype[m], nbm[m], nbp[m]);
            if (m != K) fiber_abs = fiber_abs || face;
            x[m] = ro[A.xg_off[m] + fi[m]];
        }

        const unsigned obs_fixed = obstacle_mask_fixed<D>(A, ro, x, K);
        double tv[Model::NTAB > 0 ? Model::NTAB : 1]; // model tables: constant along the fiber unless indexed by dim K
        table_values<Model>(A, ro, fi, tv);

        // (p-, p+) of the fiber-constant dimensions, before the fold: the merged vectors are weighted with them
        double rpm[D], rpp[D];
#pragma unroll
        for (int m = 0; m < D; m++) { rpm[m] = 0.0; rpp[m] = 0.0; }
        if constexpr (PK::constd() != 0) {
            // x[K] and the K-indexed tables are node 0's here (fi[K] = 0): the rates kept do not read them
            typename Model::Node nd0;
            Model::prep(A.prm, x, tv, nd0);
            double u0[Model::DU], cf0[Model::NCF > 0 ? Model::NCF : 1], b0[D], s0[D];
#pragma unroll
            for (int i = 0; i < Model::DU; i++) u0[i] = cr.get_u(i, 0);
            cf0[0] = 0.0;
#pragma unroll
            for (int i = 0; i < Model::NCF; i++) cf0[i] = cr.get_cf(i, 0);
            Model::drift(A.prm, nd0, x, u0, cf0, b0);
            Model::sigma(A.prm, x, u0, s0);
#pragma unroll
            for (int m = 0; m < D; m++)
                if ((PK::constd() >> m) & 1u) {
                    if constexpr (PKD > 0) {
                        // parked node split: t2 sigma^2 / 2 of a constant sigma is a constant of the launch, and hoisted out of the
                        // tile loop it sits in a VGPR pair that is spilled for the whole kernel; formed per tile it is one product
                        double t2 = A.t[2 * m + 1];
                        asm volatile("" : "+s"(t2));
                        upwind_rates(A.t[2 * m], t2, b0[m], s0[m], rpm[m], rpp[m]);
                    } else
                        upwind_rates(A.t[2 * m], A.t[2 * m + 1], b0[m], s0[m], rpm[m], rpp[m]);
                }
        }

        // parked node split: Qc (the merged dimensions' share of Q = sum p, parked behind the hand-over) is summed here, in the order
        // it is summed there, so that the merged rates are not held across the hand-over for it
        double qc_pk = 0.0;
        if constexpr (PKD > 0 && PK::merged() != 0u) {
#pragma unroll
            for (int m = 0; m < D; m++)
                if (PM::mg(m)) { qc_pk += rpm[m]; qc_pk += rpp[m]; }
        }

        double L[RP], R[RP], W[NOWN][RP];
#pragma unroll
        for (int a = 0; a < RP; a++) { L[a] = (a == 0) ? 1.0 : 0.0; R[a] = (a == 0) ? 1.0 : 0.0; }

        // A side whose three outer cores enter through tab3L / tab3R (PairMap::Side::td() == 3): V (L or R) is the row of the side's
        // index triple, the pair of each absorbed dimension the two rows with that index moved to its neighbours, a merged one's
        // share of U the same rows rate-weighted -- the expression of the two-core rows.  As there, all loads of the side are
        // issued ahead of its first remaining staging round and combined behind it; the cores left run through fold_step.
        auto side3 = [&](auto lc, double (&V)[RP]) __attribute__((always_inline)) {
            constexpr bool LEFT = decltype(lc)::value;
            typedef typename PM::template Side<LEFT> SD;
            constexpr int c0 = SD::core(0), c1 = SD::core(1), c2 = SD::core(2); // by depth: the edge core first
            constexpr int BASE = SD::template base<H>();
            const double *T = ro + (LEFT ? pair_tab3L_off(A, RP) : pair_tab3R_off(A, RP));
            const int n0 = A.ngrid[c0], n1 = A.ngrid[c1];
            auto row = [&](int j0, int j1, int j2) __attribute__((always_inline)) -> const double * { // the index of core c2 slowest
                return T + (LEFT ? ((long)j2 * n0 + j0) * n1 + j1 : ((long)j2 * n1 + j1) * n0 + j0) * RP;
            };
            constexpr bool OWN0 = SD::template owns<H>(c0), OWN1 = SD::template owns<H>(c1), OWN2 = SD::template owns<H>(c2);
            double tm[3][RP], tp[3][RP]; // rows of a dimension this wavefront does not fold are never loaded
            load_row16<RP>(row(fi[c0], fi[c1], fi[c2]), V);
            if constexpr (OWN0) {
                load_row16<RP>(row(nbm[c0], fi[c1], fi[c2]), tm[0]);
                load_row16<RP>(row(nbp[c0], fi[c1], fi[c2]), tp[0]);
            }
            if constexpr (OWN1) {
                load_row16<RP>(row(fi[c0], nbm[c1], fi[c2]), tm[1]);
                load_row16<RP>(row(fi[c0], nbp[c1], fi[c2]), tp[1]);
            }
            if constexpr (OWN2) {
                load_row16<RP>(row(fi[c0], fi[c1], nbm[c2]), tm[2]);
                load_row16<RP>(row(fi[c0], fi[c1], nbp[c2]), tp[2]);
            }
            __builtin_amdgcn_sched_barrier(0);
            auto combine = [&]() __attribute__((always_inline)) { // what the edge block and the steps of c1, c2 leave in W
                static_for<3>([&](auto qc) __attribute__((always_inline)) {
                    constexpr int q = decltype(qc)::value, m = SD::core(q);
                    if constexpr (SD::template owns<H>(m)) {
                        constexpr int before = SD::template before<H>(m);
#pragma unroll
                        for (int b = 0; b < RP; b++) {
                            if constexpr (PM::mg(m)) {
                                constexpr int su = PM::template lslot<H>(SD::U);
                                const double nw = fma(rpp[m], tp[q][b], rpm[m] * tm[q][b]);
                                W[su][b] = (m == SD::first_merged()) ? nw : W[su][b] + nw;
                            } else { W[BASE + before][b] = tm[q][b]; W[BASE + before + 1][b] = tp[q][b]; }
                        }
                    }
                });
            };
            if constexpr (SD::nsteps() == 0) combine(); // no staged core on this side
            static_for<SD::nsteps()>([&](auto ic) __attribute__((always_inline)) {
                fold_step<Model, RP, K, H, PART, T3, LEFT, SD::step(decltype(ic)::value)>(A, ro, sK, fi, nbm, nbp, rpm, rpp, V, W, seg, tlast, combine);
            });
        };

        // ------------------------------------------------------------ fold the prefix side
        FPP_STAMP(0) // tile setup
        if (!(C3SC_STAMPS_ON && (A.dbg & 1))) {
        if constexpr (K > 0 && PM::SL::td() == 3) side3(std::true_type{}, L);
        else if constexpr (K > 0) {
            // rows of tabL: T(a, b) = G_0[a] G_1[b].  All loads of the side are issued here, ahead of the first staging round,
            // and combined (left_combine) behind it: their L2 round trip runs under the staging wait.
            constexpr bool OWN0 = PM::SL::tab() && (PM::mg(0) ? PM::owner(PM::UL) == H : PM::owner(0) == H);
            constexpr bool OWN1 = PM::SL::tab() && (PM::mg(1) ? PM::owner(PM::UL) == H : PM::owner(1) == H);
            double t0m[OWN0 ? RP : 1], t0p[OWN0 ? RP : 1], t1m[OWN1 ? RP : 1], t1p[OWN1 ? RP : 1];
            if constexpr (PM::SL::tab()) {
                const double *T = ro + pair_tabL_off(A, RP);
                const int n1 = A.ngrid[1];
                load_row16<RP>(T + ((long)fi[0] * n1 + fi[1]) * RP, L);
                if constexpr (OWN0) {
                    load_row16<RP>(T + ((long)nbm[0] * n1 + fi[1]) * RP, t0m);
                    load_row16<RP>(T + ((long)nbp[0] * n1 + fi[1]) * RP, t0p);
                }
                if constexpr (OWN1) {
                    load_row16<RP>(T + ((long)fi[0] * n1 + nbm[1]) * RP, t1m);
                    load_row16<RP>(T + ((long)fi[0] * n1 + nbp[1]) * RP, t1p);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            auto left_combine = [&]() __attribute__((always_inline)) { // what the edge block and the step of core 1 leave in W
                if constexpr (OWN0) {
#pragma unroll
                    for (int b = 0; b < RP; b++) {
                        if constexpr (PM::mg(0)) W[0][b] = fma(rpp[0], t0p[b], rpm[0] * t0m[b]);
                        else { W[0][b] = t0m[b]; W[1][b] = t0p[b]; }
                    }
                }
                if constexpr (OWN1) {
                    constexpr int before = PM::SL::template before<H>(1);
#pragma unroll
                    for (int b = 0; b < RP; b++) {
                        if constexpr (PM::mg(1)) {
                            constexpr int su = PM::template lslot<H>(PM::UL);
                            const double nw = fma(rpp[1], t1p[b], rpm[1] * t1m[b]);
                            W[su][b] = (1 == PM::SL::first_merged()) ? nw : W[su][b] + nw;
                        } else { W[before][b] = t1m[b]; W[before + 1][b] = t1p[b]; }
                    }
                }
            };
            if constexpr (PM::SL::tab() && K == PL.lfirst) left_combine(); // no staged core on this side
            if constexpr (!PM::SL::tab()) {
                constexpr bool GLB = DIRECT || !PL.ledge; // tables on, K = 1: the lone edge core straight from the arena
                constexpr int str = GLB ? RP : fpl_lds_stride(RP);
                const double *src = sK;
                FPP_STAMP(1)
                if constexpr (GLB) src = ro + A.core_off[0];
                else {
                    pair_barrier();
                    stage_core_image<H>(sK, A.img_base + A.pair_img_off[0], A.ngrid[0] * str);
                    pair_barrier();
                }
                FPP_STAMP(7)
#pragma unroll
                for (int b = 0; b < RP; b++) {
                    L[b] = src[fi[0] * str + b];
                    if constexpr (PM::mg(0)) { // an edge core: U_L starts as the weighted rows
                        if constexpr (PM::owner(PM::UL) == H) W[0][b] = fma(rpp[0], src[nbp[0] * str + b], rpm[0] * src[nbm[0] * str + b]);
                    } else if constexpr (PM::owner(0) == H) {
                        W[0][b] = src[nbm[0] * str + b];
                        W[1][b] = src[nbp[0] * str + b];
                    }
                }
            }
            auto left_step = [&](auto mc) __attribute__((always_inline)) {
                fold_step<Model, RP, K, H, PART, T3, true, decltype(mc)::value>(A, ro, sK, fi, nbm, nbp, rpm, rpp, L, W, seg, tlast, left_combine);
            };
            static_for<PM::SL::nsteps()>([&](auto ic) __attribute__((always_inline)) { left_step(std::integral_constant<int, PM::SL::step(decltype(ic)::value)>{}); });
        }

        // ------------------------------------------------------------ fold the suffix side
        if constexpr (K < D - 1 && PM::SR::td() == 3) side3(std::false_type{}, R);
        else if constexpr (K < D - 1) {
            // rows of tabR: T(a, b) = G_{d-2}[a] G_{d-1}[b], as on the left
            constexpr bool OWN0 = PM::SR::tab() && (PM::mg(D - 1) ? PM::owner(PM::UR) == H : PM::owner(D - 1) == H);
            constexpr bool OWN1 = PM::SR::tab() && (PM::mg(D - 2) ? PM::owner(PM::UR) == H : PM::owner(D - 2) == H);
            double t0m[OWN0 ? RP : 1], t0p[OWN0 ? RP : 1], t1m[OWN1 ? RP : 1], t1p[OWN1 ? RP : 1];
            if constexpr (PM::SR::tab()) {
                const double *T = ro + pair_tabR_off(A, RP);
                const int n1 = A.ngrid[D - 1];
                load_row16<RP>(T + ((long)fi[D - 2] * n1 + fi[D - 1]) * RP, R);
                if constexpr (OWN0) {
                    load_row16<RP>(T + ((long)fi[D - 2] * n1 + nbm[D - 1]) * RP, t0m);
                    load_row16<RP>(T + ((long)fi[D - 2] * n1 + nbp[D - 1]) * RP, t0p);
                }
                if constexpr (OWN1) {
                    load_row16<RP>(T + ((long)nbm[D - 2] * n1 + fi[D - 1]) * RP, t1m);
                    load_row16<RP>(T + ((long)nbp[D - 2] * n1 + fi[D - 1]) * RP, t1p);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            auto right_combine = [&]() __attribute__((always_inline)) { // what the edge block and the step of core d-2 leave in W
                if constexpr (OWN0) {
#pragma unroll
                    for (int a = 0; a < RP; a++) {
                        if constexpr (PM::mg(D - 1)) W[NOL][a] = fma(rpp[D - 1], t0p[a], rpm[D - 1] * t0m[a]);
                        else { W[NOL][a] = t0m[a]; W[NOL + 1][a] = t0p[a]; }
                    }
                }
                if constexpr (OWN1) {
                    constexpr int after = PM::SR::template before<H>(D - 2);
#pragma unroll
                    for (int a = 0; a < RP; a++) {
                        if constexpr (PM::mg(D - 2)) {
                            constexpr int su = PM::template lslot<H>(PM::UR);
                            const double nw = fma(rpp[D - 2], t1p[a], rpm[D - 2] * t1m[a]);
                            W[su][a] = (D - 2 == PM::SR::first_merged()) ? nw : W[su][a] + nw;
                        } else { W[NOL + after][a] = t1m[a]; W[NOL + after + 1][a] = t1p[a]; }
                    }
                }
            };
            if constexpr (PM::SR::tab() && K == PL.rfirst) right_combine(); // no staged core on this side
            if constexpr (!PM::SR::tab()) {
                constexpr bool GLB = DIRECT || !PL.redge; // tables on, K = d-2: the lone edge core straight from the arena
                constexpr int str = GLB ? RP : fpl_lds_stride(RP);
                const double *src = sK;
                FPP_STAMP(1)
                if constexpr (GLB) src = ro + A.core_off[D - 1];
                else {
                    pair_barrier();
                    stage_core_image<H>(sK, A.img_base + A.pair_img_off[D - 1], A.ngrid[D - 1] * str);
                    pair_barrier();
                }
                FPP_STAMP(7)
#pragma unroll
                for (int a = 0; a < RP; a++) {
                    R[a] = src[fi[D - 1] * str + a];
                    if constexpr (PM::mg(D - 1)) {
                        if constexpr (PM::owner(PM::UR) == H)
                            W[NOL][a] = fma(rpp[D - 1], src[nbp[D - 1] * str + a], rpm[D - 1] * src[nbm[D - 1] * str + a]);
                    } else if constexpr (PM::owner(D - 1) == H) {
                        W[NOL][a] = src[nbm[D - 1] * str + a];
                        W[NOL + 1][a] = src[nbp[D - 1] * str + a];
                    }
                }
            }
            auto right_step = [&](auto mc) __attribute__((always_inline)) {
                fold_step<Model, RP, K, H, PART, T3, false, decltype(mc)::value>(A, ro, sK, fi, nbm, nbp, rpm, rpp, R, W, seg, tlast, right_combine);
            };
            static_for<PM::SR::nsteps()>([&](auto ic) __attribute__((always_inline)) { right_step(std::integral_constant<int, PM::SR::step(decltype(ic)::value)>{}); });
        }

        } // dbg & 1
        FPP_STAMP(1) // folding
        // ------------------------------------------------------------ swap halves: Wh[g][i] = component H*RH + i of vector g
        constexpr bool NS = fpp_node_split<Model, RP, K>() || PKD > 0;
        constexpr int NR = NV - PKD; // parked node split (PKD > 0): the slots [NR, NV) live in LDS homes, not in Wf
        static_assert(PKD == 0 || (PKD == fpp_parked<Model, RP, K>() && K > 0 && K < D - 1 && NR >= NVL && !T3), "parked slots are right of a middle K");
        double Wh[NS ? 1 : NV][RH];
        double Wf[NS ? NR : 1][RP]; // node split: every vector at full length in both wavefronts
        double *HM = sK;            // parked node split: the homes
        if constexpr (PKD > 0) {
            // the hand-over of the node split for the NR register-held vectors; a parked vector goes whole from its owner to its
            // home rows in the first pass -- it never enters X and is not read back.  The homes lie above X and above everything
            // the node loop keeps below them, so the barriers of the hand-over order them as well.
            typedef double v2d __attribute__((ext_vector_type(2)));
            double *X = sK; // [NR][RH][64]
            HM = sK + fpp_parked_home_row<Model, RP, K>() * 64;
            static_assert(fpp_parked_home_row<Model, RP, K>() >= NR * RH, "homes above the hand-over rows");
            auto put_get_own = [&](auto ic, auto pc) __attribute__((always_inline)) {
                constexpr int it = decltype(ic)::value, P = decltype(pc)::value;
                if constexpr (PM::valid(it) && PM::owner(it) == H) {
                    constexpr int slot = PM::template lslot<H>(it);
                    static_for<PM::count(it)>([&](auto sc) __attribute__((always_inline)) {
                        constexpr int s = decltype(sc)::value, g = PM::gslot(it) + s;
                        if constexpr (g < NR) {
#pragma unroll
                            for (int i = 0; i < RH; i++) {
                                X[(g * RH + i) * 64 + lane] = W[slot + s][P * RH + i];
                                Wf[g][P * RH + i] = W[slot + s][P * RH + i];
                            }
                        } else if constexpr (P == 0) {
#pragma unroll
                            for (int i = 0; i < RH; i++) {
                                v2d t;
                                t.x = W[slot + s][2 * i];
                                t.y = W[slot + s][2 * i + 1];
                                *reinterpret_cast<v2d *>(HM + (((g - NR) * RH + i) * 64 + lane) * 2) = t;
                            }
                        }
                    });
                }
            };
            auto get_other = [&](auto ic, auto pc) __attribute__((always_inline)) {
                constexpr int it = decltype(ic)::value, P = decltype(pc)::value;
                if constexpr (PM::valid(it) && PM::owner(it) != H) {
                    static_for<PM::count(it)>([&](auto sc) __attribute__((always_inline)) {
                        constexpr int g = PM::gslot(it) + decltype(sc)::value;
                        if constexpr (g < NR) {
#pragma unroll
                            for (int i = 0; i < RH; i++) Wf[g][P * RH + i] = X[(g * RH + i) * 64 + lane];
                        }
                    });
                }
            };
            auto half = [&](auto pc) __attribute__((always_inline)) {
                pair_barrier();
                static_for<PM::NIT>([&](auto ic) __attribute__((always_inline)) { put_get_own(ic, pc); });
                pair_barrier();
                static_for<PM::NIT>([&](auto ic) __attribute__((always_inline)) { get_other(ic, pc); });
            };
            half(std::integral_constant<int, 0>{});
            half(std::integral_constant<int, 1>{});
            pair_barrier();
        } else if constexpr (NS) {
            // hand-over of whole vectors, one half of the components at a time: each wavefront writes the vectors it folded and
            // reads the ones its partner folded, so NV * RH rows are in flight -- the half swap's buffer
            double *X = sK; // [NV][RH][64]
            auto put_get_own = [&](auto ic, auto pc) __attribute__((always_inline)) {
                constexpr int it = decltype(ic)::value, P = decltype(pc)::value;
                if constexpr (PM::valid(it) && PM::owner(it) == H) {
                    constexpr int slot = PM::template lslot<H>(it);
#pragma unroll
                    for (int s = 0; s < PM::count(it); s++) {
                        const int g = PM::gslot(it) + s;
#pragma unroll
                        for (int i = 0; i < RH; i++) {
                            X[(g * RH + i) * 64 + lane] = W[slot + s][P * RH + i];
                            Wf[g][P * RH + i] = W[slot + s][P * RH + i];
                        }
                    }
                }
            };
            auto get_other = [&](auto ic, auto pc) __attribute__((always_inline)) {
                constexpr int it = decltype(ic)::value, P = decltype(pc)::value;
                if constexpr (PM::valid(it) && PM::owner(it) != H) {
#pragma unroll
                    for (int s = 0; s < PM::count(it); s++) {
                        const int g = PM::gslot(it) + s;
#pragma unroll
                        for (int i = 0; i < RH; i++) Wf[g][P * RH + i] = X[(g * RH + i) * 64 + lane];
                    }
                }
            };
            auto half = [&](auto pc) __attribute__((always_inline)) {
                pair_barrier();
                static_for<PM::NIT>([&](auto ic) __attribute__((always_inline)) { put_get_own(ic, pc); });
                pair_barrier();
                static_for<PM::NIT>([&](auto ic) __attribute__((always_inline)) { get_other(ic, pc); });
            };
            half(std::integral_constant<int, 0>{});
            half(std::integral_constant<int, 1>{});
            pair_barrier();
        } else {
            double *X = sK; // [NV][RH][64]
            pair_barrier();
            auto put_get_own = [&](auto ic) __attribute__((always_inline)) {
                constexpr int it = decltype(ic)::value;
                if constexpr (PM::valid(it) && PM::owner(it) == H) {
                    constexpr int slot = PM::template lslot<H>(it);
#pragma unroll
                    for (int s = 0; s < PM::count(it); s++) {
                        const int g = PM::gslot(it) + s;
#pragma unroll
                        for (int i = 0; i < RH; i++) {
                            X[(g * RH + i) * 64 + lane] = W[slot + s][(1 - H) * RH + i];
                            Wh[g][i] = W[slot + s][H * RH + i];
                        }
                    }
                }
            };
            static_for<PM::NIT>(put_get_own);
            pair_barrier();
            auto get_other = [&](auto ic) __attribute__((always_inline)) {
                constexpr int it = decltype(ic)::value;
                if constexpr (PM::valid(it) && PM::owner(it) != H) {
#pragma unroll
                    for (int s = 0; s < PM::count(it); s++) {
                        const int g = PM::gslot(it) + s;
#pragma unroll
                        for (int i = 0; i < RH; i++) Wh[g][i] = X[(g * RH + i) * 64 + lane];
                    }
                }
            };
            static_for<PM::NIT>(get_other);
            pair_barrier();
        }
        // L and R move to LDS (rows of 64 lanes): both waves hold the same values, wave 0 stores L, wave 1 R.
        // The node loop re-reads them per use; that frees 2*RP*2 VGPRs for the 256-register budget.
        double *sL = sK, *sR = sK + RP * 64;
        if constexpr (PKD > 0) {
            // parked node split: the fiber number is read again rather than held across the fold and the hand-over (neither uses it)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const long fr2 = tile * 64 + ln;
            const long fp2 = fr2 < A.F ? fr2 : A.F - 1;
            f = fp2;
            if constexpr (PART) f = (long)perm[fp2];
        }
        {
#pragma unroll
            for (int a = 0; a < RP; a++) {
                if constexpr (H == 0) sL[a * 64 + lane] = L[a];
                else sR[a * 64 + lane] = R[a];
            }
            // the fiber's coordinates and table values are only needed when a node is finalised: parked in LDS
            // (wave 0 writes; both waves hold the same numbers) they do not occupy VGPRs during the partial sums
            if constexpr (H == 0) {
                static_assert(PK::rows() <= NP, "parking rows exceed the reserved block");
                double *PXw = sK + (PKD > 0 ? fpp_parked_px_row<RP>() : 2 * RP + 2 * (NP + 1) + NP) * 64; // parked node split: behind VX
                if constexpr (PKD > 0) {
                    // parked node split: coordinates and table values are read again here (the same loads, through a fiber
                    // number the compiler cannot match with the first one) and not held across the fold and the hand-over
                    long fr = f;
                    asm volatile("" : "+v"(fr));
                    int fi2[D];
#pragma unroll
                    for (int m = 0; m < D; m++) fi2[m] = (m == K || !(PK::need_x(m) || PK::nt() > 0)) ? 0 : idx[fr * D + m];
                    double tv2[Model::NTAB > 0 ? Model::NTAB : 1];
                    table_values<Model>(A, ro, fi2, tv2);
#pragma unroll
                    for (int m = 0; m < D; m++)
                        if (PK::need_x(m)) PXw[PK::row_x(m) * 64 + lane] = ro[A.xg_off[m] + fi2[m]];
#pragma unroll
                    for (int t = 0; t < Model::NTAB; t++)
                        if (PK::need_t(t)) PXw[PK::row_t(t) * 64 + lane] = tv2[t];
                } else {
#pragma unroll
                for (int m = 0; m < D; m++)
                    if (PK::need_x(m)) PXw[PK::row_x(m) * 64 + lane] = x[m];
#pragma unroll
                for (int t = 0; t < Model::NTAB; t++)
                    if (PK::need_t(t)) PXw[PK::row_t(t) * 64 + lane] = tv[t];
                }
#pragma unroll
                for (int m = 0; m < D; m++)
                    if ((PK::rates() >> m) & 1u) {
                        PXw[PK::row_pm(m) * 64 + lane] = rpm[m];
                        PXw[(PK::row_pm(m) + 1) * 64 + lane] = rpp[m];
                    }
                if constexpr (PKD > 0 && PK::merged() != 0u) PXw[PK::row_q() * 64 + lane] = qc_pk;
                else if constexpr (PK::merged() != 0u) { // Qc: the merged dimensions' share of Q = sum p
                    double qc = 0.0;
#pragma unroll
                    for (int m = 0; m < D; m++)
                        if (PM::mg(m)) { qc += rpm[m]; qc += rpp[m]; }
                    PXw[PK::row_q() * 64 + lane] = qc;
                }
            }
            pair_barrier();
        }
        FPP_STAMP(2) // half swap

        // ------------------------------------------------------------ node loop
        const int bck = A.bctype[K];
        const double *Gk = ro + A.core_off[K];
        // partial sums of node j owned by this wave, stored straight to LDS rows dst[g*64 + lane]:
        // g < NV neighbour values, g = NV the node value; the node-value partial is also returned
        auto partials = [&](int j, auto &&sink) __attribute__((always_inline)) -> double {
            double pv;
            if constexpr (K == 0) { // G_0[j] is a 1 x r row: a = row, no left vectors
                double ah[RH];
#pragma unroll
                for (int i = 0; i < RH; i++) ah[i] = Gk[(size_t)j * RP + H * RH + i];
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < RH; i++) v = fma(ah[i], sR[(H * RH + i) * 64 + lane], v);
                pv = v;
#pragma unroll
                for (int g = 0; g < NV; g++) sink(g, dot_reg<RH>(ah, Wh[g]));
            } else if constexpr (K == D - 1) { // G_{d-1}[j] is an r x 1 column: c = column, no right vectors
                double ch[RH];
#pragma unroll
                for (int i = 0; i < RH; i++) ch[i] = Gk[(size_t)j * RP + H * RH + i];
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < RH; i++) v = fma(sL[(H * RH + i) * 64 + lane], ch[i], v);
                pv = v;
#pragma unroll
                for (int g = 0; g < NV; g++) sink(g, dot_reg<RH>(Wh[g], ch));
            } else {
                // This wave's rows / columns of G_K[j] on the scalar path: c_h[i] = sum_b G[hi, b] R[b] (stride RP),
                // a_h[i] = sum_a L[a] G[a, hi] (contiguous).  A second, row-major copy of the core made the c-part
                // contiguous too and was 2.5 % faster in isolation, but it doubles what a workgroup pulls through the
                // 16 KB scalar cache (28 % of the requests missed or waited on a miss): without it 0.299 -> 0.282 ms.
                // (Walking the rows one at a time with the next row's s_load in flight was tried as well: SMEM
                // returns out of order, every wait is lgkmcnt(0), ten short waits lose to the compiler's bulk issue.)
                const double *GC0 = Gk + (size_t)j * RP * RP;
                const double *GC = GC0 + (size_t)H * RH * RP;
                double ch[RH], ah[RH];
#pragma unroll
                for (int i = 0; i < RH; i++) { ch[i] = 0.0; ah[i] = 0.0; }
#pragma unroll
                for (int b = 0; b < RP; b++) {
                    const double rb = sR[b * 64 + lane];
#pragma unroll
                    for (int i = 0; i < RH; i++) ch[i] = fma(GC0[H * RH + i + b * RP], rb, ch[i]);
                }
#pragma unroll
                for (int a = 0; a < RP; a++) {
                    const double la = sL[a * 64 + lane];
#pragma unroll
                    for (int i = 0; i < RH; i++) ah[i] = fma(la, GC[a + i * RP], ah[i]);
                }
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < RH; i++) v = fma(sL[(H * RH + i) * 64 + lane], ch[i], v);
                pv = v;
#pragma unroll
                for (int g = 0; g < NVL; g++) sink(g, dot_reg<RH>(Wh[g], ch));
#pragma unroll
                for (int g = NVL; g < NV; g++) sink(g, dot_reg<RH>(ah, Wh[g]));
            }
            sink(NV, pv);
            return pv;
        };
        auto to_lds = [&](double *dst) __attribute__((always_inline)) {
            return [dst, lane](int g, double v) __attribute__((always_inline)) { dst[g * 64 + lane] = v; };
        };
        // The same for a middle core in two halves, so that two nodes can be software-pipelined: the scalar loads and
        // FMAs of the second node's (c, a) are in the instruction stream BEFORE the register-only dots of the first
        // node, which then cover the scalar-memory latency.
        auto ca_part = [&](int j, double (&ch)[RH], double (&ah)[RH], auto &&filler) __attribute__((always_inline)) {
            // Scalar loads return out of order, so every wait on one is lgkmcnt(0): nothing can stay in flight across a
            // wait.  Left alone the compiler loads just in time and waits ~8 times per node; here the 75 values a wave
            // needs are fetched in four batches of <= 25 doubles (50 SGPRs), each issued back to back and waited for once.
            const double *GC0 = Gk + (size_t)j * RP * RP;
            const double *GC = GC0 + (size_t)H * RH * RP;
#pragma unroll
            for (int i = 0; i < RH; i++) { ch[i] = 0.0; ah[i] = 0.0; }
            constexpr int BH = (RP + 1) / 2; // columns per batch
            double vec[RP]; // R, then L: read from LDS ahead of the scalar batch so that one wait covers both
#pragma unroll
            for (int b = 0; b < RP; b++) vec[b] = sR[b * 64 + lane];
#pragma unroll
            for (int b0 = 0; b0 < RP; b0 += BH) {
                double g[BH][RH];
#pragma unroll
                for (int b = 0; b < BH; b++)
#pragma unroll
                    for (int i = 0; i < RH; i++) g[b][i] = (b0 + b < RP) ? GC0[H * RH + i + (b0 + b) * RP] : 0.0;
                __builtin_amdgcn_sched_barrier(0); // loads stay above, the filler (register-only work) below
                filler(b0 / BH);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int b = 0; b < BH; b++)
#pragma unroll
                    for (int i = 0; i < RH; i++) asm volatile("" : "+s"(g[b][i]));
#pragma unroll
                for (int b = 0; b < BH; b++) {
                    if (b0 + b < RP) {
                        const double rb = vec[b0 + b];
#pragma unroll
                        for (int i = 0; i < RH; i++) ch[i] = fma(g[b][i], rb, ch[i]);
                    }
                }
            }
#pragma unroll
            for (int a = 0; a < RP; a++) vec[a] = sL[a * 64 + lane];
#pragma unroll
            for (int a0 = 0; a0 < RP; a0 += BH) {
                double g[RH][BH];
#pragma unroll
                for (int i = 0; i < RH; i++)
#pragma unroll
                    for (int a = 0; a < BH; a++) g[i][a] = (a0 + a < RP) ? GC[a0 + a + i * RP] : 0.0;
                __builtin_amdgcn_sched_barrier(0);
                filler(2 + a0 / BH);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < RH; i++)
#pragma unroll
                    for (int a = 0; a < BH; a++) asm volatile("" : "+s"(g[i][a]));
#pragma unroll
                for (int a = 0; a < BH; a++) {
                    if (a0 + a < RP) {
                        const double la = vec[a0 + a];
#pragma unroll
                        for (int i = 0; i < RH; i++) ah[i] = fma(la, g[i][a], ah[i]);
                    }
                }
            }
        };
        // quarter q (0..3) of the 2d-1 dots of a node: register-only work that fills the scalar-load waits of the next node
        auto dots_quarter = [&](int q, const double (&ch)[RH], const double (&ah)[RH], auto &&sink) __attribute__((always_inline)) {
#pragma unroll
            for (int g = 0; g < NV; g++)
                if (g * 4 / NV == q) sink(g, (g < NVL) ? dot_reg<RH>(Wh[g], ch) : dot_reg<RH>(ah, Wh[g]));
        };
        auto dots_part = [&](const double (&ch)[RH], const double (&ah)[RH], auto &&sink) __attribute__((always_inline)) -> double {
            double v = 0.0;
#pragma unroll
            for (int i = 0; i < RH; i++) v = fma(sL[(H * RH + i) * 64 + lane], ch[i], v);
#pragma unroll
            for (int g = 0; g < NVL; g++) sink(g, dot_reg<RH>(Wh[g], ch));
#pragma unroll
            for (int g = NVL; g < NV; g++) sink(g, dot_reg<RH>(ah, Wh[g]));
            sink(NV, v);
            return v;
        };
        // LDS exchange rows after L/R
        double *B0 = sK + 2 * RP * 64;    // wave 0 -> wave 1 : P_0(j1)[NP], then v_0(j0)
        double *B1 = B0 + (NP + 1) * 64;  // wave 1 -> wave 0 : P_1(j0)[NP], then v_1(j1)
        double *B2 = B1 + (NP + 1) * 64;  // wave 1 own       : P_1(j1)[NP]
        double *PX = B2 + NP * 64;        // parked per-fiber constants: x[m] (m != K) rows 0..D-1, model tables after
        if constexpr (PKD > 0) PX = sK + fpp_parked_px_row<RP>() * 64; // no partial-sum blocks: behind the four rows of VX
        static_assert(PKD == 0 || fpp_parked_px_row<RP>() + PK::rows() <= fpp_parked_home_row<Model, RP, K>(), "the parked rows end below the homes");

        // finalise one node from its assembled stencil (NV totals in PairMap order, node value last)
        auto finalize = [&](int jn, const double (&Vt)[NP], double vlo, double vhi) __attribute__((always_inline)) {
            double V[S];
#pragma unroll
            for (int m = 0; m < D; m++) {
                if (m == K) { V[2 * m] = vlo; V[2 * m + 1] = vhi; }
                else if (PM::mg(m)) { V[2 * m] = 0.0; V[2 * m + 1] = 0.0; } // not formed: it enters through PVc
                else { V[2 * m] = Vt[PM::gslot(m)]; V[2 * m + 1] = Vt[PM::gslot(m) + 1]; }
            }
            V[2 * D] = Vt[NV];
            double pvc = 0.0; // sum over the merged dimensions of pm V- + pp V+
            if constexpr (PM::valid(PM::UL)) pvc += Vt[PM::gslot(PM::UL)];
            if constexpr (PM::valid(PM::UR)) pvc += Vt[PM::gslot(PM::UR)];
            double x[D], tv[Model::NTAB > 0 ? Model::NTAB : 1];
            tv[0] = 0.0;
#pragma unroll
            for (int m = 0; m < D; m++) // a coordinate nothing per node reads any more is not parked (PairPark)
                x[m] = (m == K) ? nr.x_at(jn) : (PairPark<Model, K>::need_x(m) ? PX[PairPark<Model, K>::row_x(m) * 64 + lane] : 0.0);
#pragma unroll
            for (int t = 0; t < Model::NTAB; t++)
                tv[t] = (Model::tab_dim(t) == K) ? nr.tab_at(t, jn) /* wave-uniform */
                                                 : (PairPark<Model, K>::need_t(t) ? PX[PairPark<Model, K>::row_t(t) * 64 + lane] : 0.0);
            int ab = (obs_fixed & nr.mask_at(jn)) ? -1 : 0;
            if (fiber_abs) ab = 1;
            int lo, hi;
            ab = vary_neighbors(jn, N, bck, ab, lo, hi, A.cends);
            int ui;
            FPP_STAMP(8) // exchange reads + stencil assembly + flags
            // FORCED (policy evaluation) is a separate instantiation: as a run-time flag it costs the minimising kernel 4 %
            int fu = -1;
            if constexpr (FORCED) fu = A.forced[(size_t)f * N + jn];
            const PairPre<Model, K> pre{PX, lane, pvc};
            const double val = node_backup<Model, FPP_CG, FPP_CGD, CandLds<Model>, true, PairPre<Model, K>>(A, ro, x, tv, cr, V, ab, ui, st, FORCED, fu, pre);
            FPP_STAMP(9) // control scan
            // lanes past the last fiber duplicate fiber F-1 and store the same numbers to the same place: no
            // divergent branch in the node loop (see node_backup on spilled lane tables)
            outv[(size_t)f * N + jn] = val;
            if (uidx) uidx[(size_t)f * N + jn] = ui;
            if (absorbed) absorbed[(size_t)f * N + jn] = ab;
        };

        if constexpr (NS) {
        // ------------------------------------------------------------ node split: wavefront H owns the nodes j = H (mod 2)
        // the whole stencil of node j: Vt[g] = dot g in PairMap order, Vt[NV] = v[j].  Element e = p RP + q of G_K[j] enters both
        // products, c[q] += G[e] R[p] and a[p] += L[q] G[e] (the summed index ascending in each, as in the rank split), so the
        // matrix is fetched once: four batches of scalar loads, each issued back to back and waited for once.
        auto stencil = [&](int j, double (&Vt)[NP]) __attribute__((always_inline)) {
            double v = 0.0;
            if constexpr (K == 0) { // G_0[j] is a 1 x r row: a = row, no left vectors
                double a[RP];
#pragma unroll
                for (int i = 0; i < RP; i++) a[i] = Gk[(size_t)j * RP + i];
#pragma unroll
                for (int i = 0; i < RP; i++) v = fma(a[i], sR[i * 64 + lane], v);
#pragma unroll
                for (int g = 0; g < NV; g++) Vt[g] = dot_reg<RP>(a, Wf[g]);
            } else if constexpr (K == D - 1) { // G_{d-1}[j] is an r x 1 column: c = column, no right vectors
                double c[RP];
#pragma unroll
                for (int i = 0; i < RP; i++) c[i] = Gk[(size_t)j * RP + i];
#pragma unroll
                for (int i = 0; i < RP; i++) v = fma(sL[i * 64 + lane], c[i], v);
#pragma unroll
                for (int g = 0; g < NV; g++) Vt[g] = dot_reg<RP>(Wf[g], c);
            } else {
                const double *G0 = Gk + (size_t)j * RP * RP;
                constexpr int NE = RP * RP, NB = (NE + 3) / 4; // elements per batch (25 doubles = 50 SGPRs at rank 10)
                double c[RP], a[RP], lv[RP];
#pragma unroll
                for (int i = 0; i < RP; i++) lv[i] = sL[i * 64 + lane];
#pragma unroll
                for (int i = 0; i < RP; i++) { c[i] = 0.0; a[i] = 0.0; }
#pragma unroll
                for (int b0 = 0; b0 < NE; b0 += NB) {
                    double g[NB];
#pragma unroll
                    for (int e = 0; e < NB; e++) g[e] = (b0 + e < NE) ? G0[b0 + e] : 0.0;
                    double rv[RP]; // R: only the rows this batch touches (three at rank 10), read under the same wait
#pragma unroll
                    for (int p = 0; p < RP; p++) rv[p] = (p >= b0 / RP && p * RP < b0 + NB) ? sR[p * 64 + lane] : 0.0;
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int e = 0; e < NB; e++) asm volatile("" : "+s"(g[e]));
#pragma unroll
                    for (int e = 0; e < NB; e++) {
                        if (b0 + e < NE) {
                            const int p = (b0 + e) / RP, q = (b0 + e) % RP;
                            c[q] = fma(g[e], rv[p], c[q]);
                            a[p] = fma(lv[q], g[e], a[p]);
                        }
                    }
                    // the products are not ordered against the next batch's loads by themselves: left floating they all sink
                    // behind the last batch and the 200 SGPRs of the matrix are parked in VGPR lanes meanwhile
#pragma unroll
                    for (int i = 0; i < RP; i++) asm volatile("" : "+v"(c[i]), "+v"(a[i]));
                }
#pragma unroll
                for (int i = 0; i < RP; i++) v = fma(sL[i * 64 + lane], c[i], v);
#pragma unroll
                for (int g = 0; g < NVL; g++) Vt[g] = dot_reg<RP>(Wf[g], c);
#pragma unroll
                for (int g = NVL; g < NR; g++) Vt[g] = dot_reg<RP>(a, Wf[g]);
                if constexpr (PKD > 0) { // the parked vectors last: their home rows are read under the register dots above
                    typedef double v2d __attribute__((ext_vector_type(2)));
#pragma unroll
                    for (int p = 0; p < PKD; p++) {
                        double w[RP];
#pragma unroll
                        for (int i = 0; i < RH; i++) {
                            const v2d t = *reinterpret_cast<const v2d *>(HM + ((p * RH + i) * 64 + lane) * 2);
                            w[2 * i] = t.x;
                            w[2 * i + 1] = t.y;
                        }
                        Vt[NR + p] = dot_reg<RP>(a, w);
                    }
                }
            }
            Vt[NV] = v;
        };
        // Only v[j] crosses: wavefront h writes row 2h + (t & 1) of the exchange block before the barrier of iteration t and its
        // partner reads it behind that barrier; the row is written again two EXECUTED trips (two barriers) later -- the trips an
        // absorbed tile leaves out (end of the loop) are cut so that the parity of t still alternates from one executed trip to
        // the next.
        double *VX = B0;
        double vwrap = 0.0; // value of node N-2 (left neighbour of node 0 under a periodic boundary): both wavefronts compute it
        if (bck == C3SC_PERIODIC) {
            double Vw[NP];
            stencil(N - 2, Vw);
            vwrap = Vw[NV];
        }
        double vone = 0.0;             // v[1]
        double v_m2 = 0.0, v_m1 = 0.0; // v[2t-2], v[2t-1]
        double Vd[NP];                 // wave 1: stencil of node 2t-1 waiting for v[2t]
#pragma unroll
        for (int g = 0; g < NP; g++) Vd[g] = 0.0;
        const int T = N / 2 + 1;
        for (int t = 0; t < T; t++) {
            const int j0 = 2 * t, j1 = 2 * t + 1;
            const bool has0 = j0 < N, has1 = j1 < N;
            double *vx = VX + (t & 1) * 64;
            double v0 = 0.0, v1 = 0.0; // v[j0], v[j1]
            double Pn[NP];
#pragma unroll
            for (int g = 0; g < NP; g++) Pn[g] = 0.0;
            if constexpr (H == 0) {
                if (has0) {
                    stencil(j0, Pn);
                    v0 = Pn[NV];
                    vx[lane] = v0;
                }
                FPP_STAMP(3) // stencil
                pair_barrier();
                FPP_STAMP(4) // the barrier
                if (has1) v1 = vx[2 * 64 + lane];
                if (has0) {
                    double vlo, vhi;
                    dimk_values(j0, N, bck, v_m1, v0, v1, vwrap, (j0 == 0 ? v1 : vone), vlo, vhi);
                    finalize(j0, Pn, vlo, vhi);
                }
            } else {
                if (has1) {
                    stencil(j1, Pn);
                    v1 = Pn[NV];
                    vx[2 * 64 + lane] = v1;
                }
                FPP_STAMP(3)
                pair_barrier();
                FPP_STAMP(4)
                if (has0) v0 = vx[lane];
                if (t >= 1) { // node 2t-1
                    const int jn = j0 - 1;
                    double vlo, vhi;
                    dimk_values(jn, N, bck, v_m2, Vd[NV], v0, vwrap, (jn == 1 ? Vd[NV] : vone), vlo, vhi);
                    finalize(jn, Vd, vlo, vhi);
                }
                if (has1) {
#pragma unroll
                    for (int g = 0; g < NP; g++) Vd[g] = Pn[g];
                }
            }
            if (t == 0) vone = v1;
            v_m2 = v0;
            v_m1 = v1;
            FPP_STAMP(5) // finalize
            // an absorbed tile under literal ends: the ends need the node pairs (0, 1) and (N-2, N-1) only, i.e. the trips 0,
            // T-2 and T-1; the interior nodes those trips finalise are absorbed and get boundcost once more.  The trip behind
            // trip 0 must be an odd one (it writes the other exchange rows: trip 0's are still being read, one barrier back):
            // T-2 where T is odd, T-3 where it is even.
            if (PART && dead_tile && t == 0 && T > 4) t = ((T - 3) | 1) - 1;
        }
        pair_barrier(); // the parked rows and L, R are read until the last node is finalised; the next tile overwrites them
        } else {
        // value of node N-2 (left neighbour of node 0 under a periodic boundary)
        double vwrap = 0.0;
        if (bck == C3SC_PERIODIC) {
            const double pv = partials(N - 2, [](int, double) __attribute__((always_inline)) {});
            if constexpr (H == 0) B0[NP * 64 + lane] = pv; // each wave writes the spare row of its own exchange block
            else B1[NP * 64 + lane] = pv;
            pair_barrier();
            vwrap = pv + (H == 0 ? B1[NP * 64 + lane] : B0[NP * 64 + lane]);
            pair_barrier();
        }
        double vone = 0.0;             // v[1]
        double v_m2 = 0.0, v_m1 = 0.0; // v[2t-2], v[2t-1]
        double Vd[NP];                 // wave 1: stencil of node 2t-1 waiting for v[2t]
#pragma unroll
        for (int g = 0; g < NP; g++) Vd[g] = 0.0;

        const int T = N / 2 + 1;
        for (int t = 0; t < T; t++) {
            const int j0 = 2 * t, j1 = 2 * t + 1;
            const bool has0 = j0 < N, has1 = j1 < N;
            double pv0 = 0.0, pv1 = 0.0;
            double Pown[NP]; // wave 0: its partial sums of the node it finalises stay in registers
#pragma unroll
            for (int g = 0; g < NP; g++) Pown[g] = 0.0;
            auto own_sink = [&](int g, double v) __attribute__((always_inline)) { Pown[g] = v; };
            if constexpr (K > 0 && K < D - 1 && FPP_PIPE2) {
                if (has0 && has1) { // both nodes: (c, a) of the second before the dots of the first
                    double chA[RH], ahA[RH], chB[RH], ahB[RH];
                    auto nofill = [](int) __attribute__((always_inline)) {};
                    auto value_of = [&](const double (&ch)[RH]) __attribute__((always_inline)) -> double {
                        double v = 0.0;
#pragma unroll
                        for (int i = 0; i < RH; i++) v = fma(sL[(H * RH + i) * 64 + lane], ch[i], v);
                        return v;
                    };
                    if constexpr (H == 0) {
                        auto sinkA = to_lds(B0);
                        ca_part(j1, chA, ahA, nofill);
                        ca_part(j0, chB, ahB, [&](int q) __attribute__((always_inline)) { dots_quarter(q, chA, ahA, sinkA); });
                        pv1 = value_of(chA);
                        sinkA(NV, pv1);
                        pv0 = dots_part(chB, ahB, own_sink);
                        B0[NP * 64 + lane] = pv0;
                    } else {
                        auto sinkA = to_lds(B1);
                        ca_part(j0, chA, ahA, nofill);
                        ca_part(j1, chB, ahB, [&](int q) __attribute__((always_inline)) { dots_quarter(q, chA, ahA, sinkA); });
                        pv0 = value_of(chA);
                        sinkA(NV, pv0);
                        pv1 = dots_part(chB, ahB, to_lds(B2));
                        B1[NP * 64 + lane] = pv1;
                    }
                } else if (has0) { // the last, unpaired node
                    if constexpr (H == 0) { pv0 = partials(j0, own_sink); B0[NP * 64 + lane] = pv0; }
                    else pv0 = partials(j0, to_lds(B1));
                }
            } else if constexpr (H == 0) { // the other wave's node first, the own node last
                if (has1) pv1 = partials(j1, to_lds(B0));
                if (has0) {
                    pv0 = partials(j0, own_sink);
                    B0[NP * 64 + lane] = pv0;
                }
            } else {
                if (has0) pv0 = partials(j0, to_lds(B1));
                if (has1) {
                    pv1 = partials(j1, to_lds(B2));
                    B1[NP * 64 + lane] = pv1;
                }
            }
            FPP_STAMP(3) // partials + LDS writes
            pair_barrier();
            FPP_STAMP(4) // barrier 1
            double v0 = 0.0, v1 = 0.0; // totals v[j0], v[j1]
            if constexpr (H == 0) {
                if (has1) v1 = pv1 + B1[NP * 64 + lane];
                if (has0) {
                    double P0[NP];
#pragma unroll
                    for (int g = 0; g < NP; g++) P0[g] = Pown[g] + B1[g * 64 + lane];
                    v0 = P0[NV];
                    double vlo, vhi;
                    dimk_values(j0, N, bck, v_m1, v0, v1, vwrap, (j0 == 0 ? v1 : vone), vlo, vhi);
                    finalize(j0, P0, vlo, vhi);
                }
            } else {
                if (has0) v0 = pv0 + B0[NP * 64 + lane];
                if (t >= 1) { // node 2t-1
                    const int jn = j0 - 1;
                    double vlo, vhi;
                    dimk_values(jn, N, bck, v_m2, Vd[NV], v0, vwrap, (jn == 1 ? Vd[NV] : vone), vlo, vhi);
                    finalize(jn, Vd, vlo, vhi);
                }
                if (has1) {
#pragma unroll
                    for (int g = 0; g < NP; g++) Vd[g] = B0[g * 64 + lane] + B2[g * 64 + lane];
                    v1 = Vd[NV];
                }
            }
            if (t == 0) vone = v1;
            v_m2 = v0;
            v_m1 = v1;
            FPP_STAMP(5) // LDS reads + finalize
            pair_barrier();
            FPP_STAMP(6) // barrier 2
            // an absorbed tile under literal ends: the trips 0, T-2, T-1 as in the node split; with two barriers per trip and
            // no row toggled by t, any trip may follow trip 0
            if (PART && dead_tile && t == 0 && T > 3) t = T - 3;
        }
        } // rank split
    }
    if (C3SC_STAMPS_ON && (A.dbg & 128) && lane == 0) {
        const size_t w = ((size_t)blockIdx.x * 2 + H) * 12;
        if (w < 65536 * 8)
            for (int i = 0; i < 12; i++) A.dbgbuf[w + i] = seg[i];
    }
}

// registers: two wavefronts per SIMD in general (256 VGPRs); the direct-fold kernels at ranks <= 6 sit at 122-137 and are asked to stay
// within 128 (four per SIMD: their LDS footprint allows it)
#ifndef FPP_WPS_LOW
#define FPP_WPS_LOW 4
#endif
#ifndef FPP_WPS_HIGH
#define FPP_WPS_HIGH 2 // wavefronts per SIMD of the staged (rank > 6) instantiations; 1 was measured (512 registers per wavefront, spills in AGPRs)
#endif
template <class Model, int RP>
__host__ __device__ constexpr int fpp_waves_per_simd() { return (fpp_direct<Model, RP>() && RP <= 6) ? FPP_WPS_LOW : (FPP_WPS_HIGH); }

template <class Model, int RP, int K, bool FORCED>
__global__ void __launch_bounds__(FPP_THREADS, (fpp_waves_per_simd<Model, RP>()))
    k_fiber_pair(const KArgs A, const double *__restrict__ ro, const int32_t *__restrict__ idx, double *__restrict__ outv,
                 int32_t *__restrict__ uidx, int32_t *__restrict__ absorbed)
{
    extern __shared__ double sKp[];
    unsigned st = 0;
    const int h = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (h == 0) fiber_pair_body<Model, RP, K, 0, FORCED, false>(A, ro, idx, outv, uidx, absorbed, nullptr, nullptr, sKp, st);
    else fiber_pair_body<Model, RP, K, 1, FORCED, false>(A, ro, idx, outv, uidx, absorbed, nullptr, nullptr, sKp, st);
    if (st) atomicOr(A.status, st);
}

// the same kernel behind a partition of its batch (fiber_partition.hpp): tiles read their fibers through perm, tiles of absorbed
// fibers leave the work out.  A kernel of its own, so that every launch without a partition runs the code it ran before.
template <class Model, int RP, int K, bool FORCED>
__global__ void __launch_bounds__(FPP_THREADS, (fpp_waves_per_simd<Model, RP>()))
    k_fiber_pair_part(const KArgs A, const double *__restrict__ ro, const int32_t *__restrict__ idx, double *__restrict__ outv,
                      int32_t *__restrict__ uidx, int32_t *__restrict__ absorbed, const int32_t *__restrict__ perm,
                      const int32_t *__restrict__ nlive_p)
{
    extern __shared__ double sKp[];
    unsigned st = 0;
    const int h = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (h == 0) fiber_pair_body<Model, RP, K, 0, FORCED, true>(A, ro, idx, outv, uidx, absorbed, perm, nlive_p, sKp, st);
    else fiber_pair_body<Model, RP, K, 1, FORCED, true>(A, ro, idx, outv, uidx, absorbed, perm, nlive_p, sKp, st);
    if (st) atomicOr(A.status, st);
}

// the partitioned kernel with the three-core tables (PairMap::Side::td() == 3); a kernel of its own again: the launcher picks it
// where the tables are built and the K is not on fpp_table3_optout, everything else runs the kernels above unchanged
template <class Model, int RP, int K, bool FORCED>
__global__ void __launch_bounds__(FPP_THREADS, (fpp_waves_per_simd<Model, RP>()))
    k_fiber_pair_part3(const KArgs A, const double *__restrict__ ro, const int32_t *__restrict__ idx, double *__restrict__ outv,
                       int32_t *__restrict__ uidx, int32_t *__restrict__ absorbed, const int32_t *__restrict__ perm,
                       const int32_t *__restrict__ nlive_p)
{
    extern __shared__ double sKp[];
    unsigned st = 0;
    const int h = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (h == 0) fiber_pair_body<Model, RP, K, 0, FORCED, true, true>(A, ro, idx, outv, uidx, absorbed, perm, nlive_p, sKp, st);
    else fiber_pair_body<Model, RP, K, 1, FORCED, true, true>(A, ro, idx, outv, uidx, absorbed, perm, nlive_p, sKp, st);
    if (st) atomicOr(A.status, st);
}

// the two kernels above under the parked node split (fpp_parked > 0): kernels of their own once more, with the argument lists of
// the ones they stand in for; the launcher picks them unless LaunchIO::parked is off
template <class Model, int RP, int K, bool FORCED>
__global__ void __launch_bounds__(FPP_THREADS, (fpp_waves_per_simd<Model, RP>()))
    k_fiber_pair_pk(const KArgs A, const double *__restrict__ ro, const int32_t *__restrict__ idx, double *__restrict__ outv,
                    int32_t *__restrict__ uidx, int32_t *__restrict__ absorbed)
{
    extern __shared__ double sKp[];
    constexpr int P = fpp_parked<Model, RP, K>();
    static_assert(P > 0, "no parked node split for this instantiation");
    unsigned st = 0;
    const int h = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (h == 0) fiber_pair_body<Model, RP, K, 0, FORCED, false, false, P>(A, ro, idx, outv, uidx, absorbed, nullptr, nullptr, sKp, st);
    else fiber_pair_body<Model, RP, K, 1, FORCED, false, false, P>(A, ro, idx, outv, uidx, absorbed, nullptr, nullptr, sKp, st);
    if (st) atomicOr(A.status, st);
}

template <class Model, int RP, int K, bool FORCED>
__global__ void __launch_bounds__(FPP_THREADS, (fpp_waves_per_simd<Model, RP>()))
    k_fiber_pair_part_pk(const KArgs A, const double *__restrict__ ro, const int32_t *__restrict__ idx, double *__restrict__ outv,
                         int32_t *__restrict__ uidx, int32_t *__restrict__ absorbed, const int32_t *__restrict__ perm,
                         const int32_t *__restrict__ nlive_p)
{
    extern __shared__ double sKp[];
    constexpr int P = fpp_parked<Model, RP, K>();
    static_assert(P > 0, "no parked node split for this instantiation");
    unsigned st = 0;
    const int h = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (h == 0) fiber_pair_body<Model, RP, K, 0, FORCED, true, false, P>(A, ro, idx, outv, uidx, absorbed, perm, nlive_p, sKp, st);
    else fiber_pair_body<Model, RP, K, 1, FORCED, true, false, P>(A, ro, idx, outv, uidx, absorbed, perm, nlive_p, sKp, st);
    if (st) atomicOr(A.status, st);
}

} // namespace c3sc
