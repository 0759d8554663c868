// kernel_chain_walk.hpp -- the approximating Markov chain itself (c3sc_hip_chain_transitions, c3sc_hip_simulate_chain).
// DESIGN.md 4.18.
//
// Every Bellman kernel applies the Kushner-Dupuis chain: at the node xi under the control u it moves to the 2d index-rule
// neighbours with the probabilities p_k / C, C = sum p_k, after the interpolation interval dt = h^2 / C.  The kernels here walk
// it.  k_chain_transitions is the deterministic half -- per node the greedy decision of the uploaded value function (node_backup
// in the plain form over the candidate list), its value, the stage cost, dt and the 2d probabilities -- and k_chain_walk samples
// trajectories of that chain, one lane each: J += D g dt, T += dt, D *= exp(-beta dt), then one uniform picks the neighbour.
//
// Outcome order = stencil order: k = 2m is the lo neighbour of dimension m, k = 2m + 1 its hi neighbour; the neighbours are
// fixed_neighbors' in EVERY dimension (a reflecting end names the node itself, so a self-loop that still costs its dt; the
// periodic seam is n - 2 / 1).  Sampling rule: with c_k = p_0 + .. + p_k summed in that order and C = c_{2d-1}, the outcome is
// the first k with v C < c_k; where rounding leaves none, the last k with p_k > 0.
//
// End points.  A node is absorbed (flag 1) on an absorbing face of ANY absorbing dimension -- index 0 or N - 1 -- else an
// obstacle node (flag -1) inside an obstacle, else live (0); the face wins over the obstacle, as in the fiber kernels.  This is
// the consistent end-point rule: a walk has no fiber direction, so there is no varying dimension whose end points could be
// treated differently, and the rule does NOT depend on c3sc_hip_set_consistent_ends.
//
// Lanes are independent; tail lanes repeat the last trajectory / node (k_rollout's lane rule, kernel_rollout.hpp) but store
// nothing: the walk's state is read at the start of a launch and written at its end, and a tail lane that wrote it could do so
// before another wave of its workgroup had read it.  Exits, freezes and the move are selects.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#include "kernel_common.hpp"
#include "kernel_rollout.hpp"
#include "philox.hpp"
#include "registry.hpp"

namespace c3sc {

// argument block of one chain launch (by value: kernarg space, wave-uniform)
struct ChainK {
    long n;                 // trajectories (walk) / nodes (transitions)
    long long traj_offset;  // global index of trajectory 0 (Philox counter)
    int s0, s1;             // steps [s0, s1) of this launch
    int nsteps;             // steps of the call: the launch with s1 == nsteps also tests xi_nsteps and writes V_end
    int save_every;         // 0: nothing saved
    unsigned long long seed;
    const int32_t *node0;   // [n][D] start nodes (walk, read when s0 == 0) / the nodes (transitions)
    const double *uniform;  // [n][nsteps] uniforms in [0, 1), or null: Philox (philox_jump_uniforms' u0); a jump form's walk
                            // reads [n][nsteps][2] = (v, u1)
    // walk: the state between launches ...
    int32_t *node;          // [n][D]
    double *cost, *disc, *time; // [n] J, D, T
    long long *exit_step;   // [n] -1 running, s >= 0: absorbed / obstacle at step s, -(s + 2): stuck at step s,
                            // -(s + 2) - 2^32: stopped at step s (the forms with the stop action)
    // ... and what it saves
    int32_t *traj;          // [n][nsteps / save_every + 1][D] or null
    int32_t *uidx;          // walk: [n][ceil(nsteps / save_every)] or null; transitions: [n] or null
    double *vend;           // [n] or null
    // transitions: each may be null
    double *value, *stage, *dt, *P; // [n], [n], [n], [n][2D]
    int32_t *flag;          // [n]
    // outcomes (k_chain_outcomes_form): each may be null
    double *pself, *pmark, *markval; // [n], [n][NJUMP], [n][NJUMP]
};

// The function train at the node ix and at its 2D index-rule neighbours: V[2m] = lo, V[2m + 1] = hi, V[2D] = the node.  The
// on-grid sibling of offgrid_stencil (kernel_rollout.hpp) with its prefix / suffix algebra: neighbour m differs from the node
// in index m only, V(y) = L_m G_m[y_m] R_{m+1}; the suffixes R[m] are formed once, the prefix L is carried forward, the row loops
// stay rolled and L is read by rotation (unrolled, every core load of an r x r product stays in flight: hundreds of VGPRs).
// One entry per core element and lane where core_at gathers two; global loads only.  The caller keeps 0 <= ix[m] < A.ngrid[m];
// fixed_neighbors then returns indices in the same range, so every address lies inside core m.
template <int D, int RP>
__device__ inline void node_stencil(const KArgs &A, const double *__restrict__ ro, const int (&ix)[D], double (&V)[2 * D + 1])
{
    static_assert(D >= 2, "dimension");
    double R[D][RP]; // R[m] = suffix from core m on (m = 1 .. D-1)
    {
        const double *G = ro + A.core_off[D - 1] + (size_t)ix[D - 1] * RP;
#pragma unroll
        for (int a = 0; a < RP; a++) R[D - 1][a] = G[a];
    }
    static_for<1, D - 1>([&](auto mc) { // m = D-2 .. 1 (compile-time indices: R stays in registers)
        constexpr int m = D - 1 - decltype(mc)::value;
        const double *G = ro + A.core_off[m] + (size_t)ix[m] * (RP * RP);
#pragma unroll
        for (int a = 0; a < RP; a++) R[m][a] = 0.0;
#pragma unroll 1
        for (int a = 0; a < RP; a++) { // row a of G_m[ix_m] R_{m+1}, shifted in at the end: R[m][a] after RP rounds
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < RP; b++) s += G[a + b * RP] * R[m + 1][b];
            (void)rot_left<RP>(R[m]);
            R[m][RP - 1] = s;
        }
    });
    double L[RP];
    static_for<0, D>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        int lo, hi;
        (void)fixed_neighbors(ix[m], A.ngrid[m], A.bctype[m], lo, hi);
        double vl = 0.0, vr = 0.0;
        if constexpr (m == 0) {
            const double *G = ro + A.core_off[0];
            const double *Gl = G + (size_t)lo * RP, *Gr = G + (size_t)hi * RP, *Gc = G + (size_t)ix[0] * RP;
#pragma unroll
            for (int b = 0; b < RP; b++) {
                vl += Gl[b] * R[1][b];
                vr += Gr[b] * R[1][b];
                L[b] = Gc[b];
            }
        } else if constexpr (m == D - 1) {
            const double *G = ro + A.core_off[m];
            const double *Gl = G + (size_t)lo * RP, *Gr = G + (size_t)hi * RP, *Gc = G + (size_t)ix[m] * RP;
            double vx = 0.0;
#pragma unroll
            for (int a = 0; a < RP; a++) {
                vl += L[a] * Gl[a];
                vr += L[a] * Gr[a];
                vx += L[a] * Gc[a];
            }
            V[2 * D] = vx;
        } else {
            const double *G = ro + A.core_off[m];
            auto through = [&](int iy) { // L_m G_m[iy] R_{m+1}, row by row
                const double *Gy = G + (size_t)iy * (RP * RP);
                double v = 0.0;
#pragma unroll 1
                for (int a = 0; a < RP; a++) {
                    const double la = rot_left<RP>(L);
                    double t = 0.0;
#pragma unroll
                    for (int b = 0; b < RP; b++) t += Gy[a + b * RP] * R[m + 1][b];
                    v += la * t;
                }
                return v;
            };
            vl = through(lo);
            vr = through(hi);
            const double *Gc = G + (size_t)ix[m] * (RP * RP);
            double Ln[RP];
#pragma unroll
            for (int b = 0; b < RP; b++) Ln[b] = 0.0;
#pragma unroll 1
            for (int a = 0; a < RP; a++) {
                const double la = rot_left<RP>(L);
#pragma unroll
                for (int b = 0; b < RP; b++) Ln[b] += la * Gc[a + b * RP];
            }
#pragma unroll
            for (int b = 0; b < RP; b++) L[b] = Ln[b];
        }
        V[2 * m] = vl;
        V[2 * m + 1] = vr;
    });
}

// a node's coordinates and its flag: 1 on an absorbing face, else -1 inside an obstacle, else 0 (the face wins)
template <int D>
__device__ inline int chain_flag(const KArgs &A, const double *__restrict__ ro, const int (&ix)[D], double (&x)[D])
{
    bool face = false;
#pragma unroll
    for (int m = 0; m < D; m++) {
        x[m] = ro[A.xg_off[m] + ix[m]];
        face = face || ((A.bctype[m] == C3SC_ABSORB) && ((ix[m] == 0) || (ix[m] == A.ngrid[m] - 1)));
    }
    const bool inobs = in_obstacle<D>(A, ro, x);
    return face ? 1 : (inobs ? -1 : 0);
}

// an index vector from memory, clamped into the grid: a caller's bad index never becomes an address outside a core (the host
// entry points reject such a call before anything is launched)
template <int D>
__device__ inline void chain_load_node(const KArgs &A, const int32_t *__restrict__ src, int (&ix)[D])
{
#pragma unroll
    for (int m = 0; m < D; m++) ix[m] = max(0, min((int)src[m], A.ngrid[m] - 1));
}

// What the chain does at one node: the block k_chain_transitions and k_chain_walk share.
template <int D>
struct ChainNode {
    int flag;      // chain_flag
    int ui;        // the greedy candidate; -1 on an absorbed, obstacle or stuck node
    bool stuck;    // live, and no valid candidate or a winner with C < 1e-14
    double value;  // the backup's value; the bound / obstacle cost on a flagged node
    double stage;  // g(x, u); the bound / obstacle cost on a flagged node
    double C, dt;  // C = sum p_k in stencil order, dt = h^2 / C; 0 where the chain does not move
    double p[2 * D]; // the winner's un-normalised rates, stencil order; 0 where the chain does not move
    double vnode;  // the function train at the node
};

template <int MID, class Model, int RP>
__device__ inline void chain_node(const KArgs &A, const double *__restrict__ ro, const CandLds<Model> &cr, const int (&ix)[Model::D],
                                  ChainNode<Model::D> &o, unsigned &st)
{
    constexpr int D = Model::D, DU = Model::DU, NT = Model::NTAB > 0 ? Model::NTAB : 1, NCFa = Model::NCF > 0 ? Model::NCF : 1;
    double x[D], V[2 * D + 1];
    node_stencil<D, RP>(A, ro, ix, V);
    o.vnode = V[2 * D];
    o.flag = chain_flag<D>(A, ro, ix, x); // after the stencil: the obstacle loop's scalars do not live across it
    double tv[NT];
    table_values<Model>(A, ro, ix, tv);
    int ui;
    unsigned stb = 0; // node_backup flags a live node with ANY candidate below the rate floor; the chain reports stuck nodes only
    o.value = node_backup<Model, 1, 1, CandLds<Model>, true, NoPre, 0u>(A, ro, x, tv, cr, V, o.flag, ui, stb);
    // the winner's rates, by the statements of the backup's own dimensions
    const int uc = ui < 0 ? 0 : ui;
    double u[DU], cf[NCFa];
    cf[0] = 0.0;
#pragma unroll
    for (int k = 0; k < DU; k++) u[k] = ro[A.cands_off + uc * DU + k];
#pragma unroll
    for (int q = 0; q < Model::NCF; q++) cf[q] = ro[A.cfeat_off + uc * Model::NCF + q];
    typename Model::Node nd;
    Model::prep(A.prm, x, tv, nd);
    double b[D], sg[D];
    Model::drift(A.prm, nd, x, u, cf, b);
    Model::sigma(A.prm, x, u, sg);
    double C = 0.0;
#pragma unroll
    for (int m = 0; m < D; m++) {
        upwind_rates(A.t[2 * m], A.t[2 * m + 1], b[m], sg[m], o.p[2 * m], o.p[2 * m + 1]);
        C += o.p[2 * m];
        C += o.p[2 * m + 1];
    }
    const bool live = o.flag == 0;
    o.stuck = live && ((ui < 0) || (C < 1e-14));
    const bool moves = live && !o.stuck;
    st |= o.stuck ? (unsigned)C3SC_STATUS_STATIONARY : 0u;
    const double g = Model::stage(A.prm, x, u);
    o.ui = moves ? ui : -1;
    o.stage = live ? g : o.value;
    o.C = moves ? C : 0.0;
    o.dt = moves ? A.h2 / (moves ? C : 1.0) : 0.0;
#pragma unroll
    for (int k = 0; k < 2 * D; k++) o.p[k] = moves ? o.p[k] : 0.0;
}

// one lane per node
template <int MID, class Model, int RP>
__global__ void __launch_bounds__(256) k_chain_transitions(const KArgs A, const ChainK S, const double *__restrict__ ro)
{
    constexpr int D = Model::D;
    extern __shared__ double smem[];
    CandLds<Model> cr;
    rollout_cands<Model>(A, ro, smem, cr);
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i = min(gid, S.n - 1); // tail lanes repeat the last node ...
    int ix[D];
    chain_load_node<D>(A, S.node0 + (size_t)i * D, ix);
    ChainNode<D> o;
    unsigned st = 0;
    chain_node<MID, Model, RP>(A, ro, cr, ix, o, st);
    if (gid >= S.n) return; // ... and store nothing
    if (S.uidx) S.uidx[i] = o.ui;
    if (S.value) S.value[i] = o.value;
    if (S.stage) S.stage[i] = o.stage;
    if (S.dt) S.dt[i] = o.dt;
    if (S.flag) S.flag[i] = o.flag;
    if (S.P) {
        const double inv = o.C > 0.0 ? o.C : 1.0;
#pragma unroll
        for (int k = 0; k < 2 * D; k++) S.P[(size_t)i * (2 * D) + k] = o.p[k] / inv;
    }
    if (st) atomicOr(A.status, st);
}

// one lane per trajectory
template <int MID, class Model, int RP>
__global__ void __launch_bounds__(256) k_chain_walk(const KArgs A, const ChainK S, const double *__restrict__ ro)
{
    constexpr int D = Model::D;
    extern __shared__ double smem[];
    CandLds<Model> cr;
    rollout_cands<Model>(A, ro, smem, cr);
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i = min(gid, S.n - 1); // tail lanes repeat the last trajectory ...
    const bool own = gid < S.n;       // ... and store nothing
    const int se = S.save_every;
    const long nrow = se > 0 ? S.nsteps / se + 1 : 0, nurow = se > 0 ? (S.nsteps + se - 1) / se : 0;
    int ix[D];
    double J, Dc, T;
    long long ex;
    if (S.s0 == 0) {
        chain_load_node<D>(A, S.node0 + (size_t)i * D, ix);
        J = 0.0;
        Dc = 1.0;
        T = 0.0;
        ex = -1;
        if (S.traj && own)
#pragma unroll
            for (int m = 0; m < D; m++) S.traj[(size_t)i * nrow * D + m] = ix[m];
    } else {
        chain_load_node<D>(A, S.node + (size_t)i * D, ix);
        J = S.cost[i];
        Dc = S.disc[i];
        T = S.time[i];
        ex = S.exit_step[i];
    }
    const double beta = A.discount;
    unsigned st = 0;
    // The launch that ends the call makes one more trip, at xi_nsteps (fin, wave-uniform): the flag test and V_end only -- no
    // stuck test, no cost, no move.  One trip body serves both, so the kernel holds one copy of the stencil.
    const int send = S.s1 == S.nsteps ? S.s1 + 1 : S.s1;
    for (int s = S.s0; s < send; s++) {
        const bool fin = s == S.nsteps;
        ChainNode<D> o;
        unsigned stn = 0;
        chain_node<MID, Model, RP>(A, ro, cr, ix, o, stn);
        const bool running = ex == -1;
        st |= (running && !fin) ? stn : 0u; // a frozen lane raises nothing more
        // 1. the flag test: an absorbed node pays the bound cost, an obstacle node the obstacle cost (o.value is that cost)
        const bool exits = running && (o.flag != 0);
        J = exits ? J + Dc * o.value : J;
        ex = exits ? (long long)s : ex;
        if (fin && S.vend && own) S.vend[i] = o.vnode;
        // 2. a stuck node freezes the lane where it is
        const bool sticks = running && o.stuck && !fin;
        ex = sticks ? -((long long)s + 2) : ex;
        const bool alive = running && !exits && !sticks && !fin;
        if (S.uidx && se > 0 && s % se == 0 && !fin && own) S.uidx[(size_t)i * nurow + s / se] = alive ? o.ui : -1;
        // 3. the interval's cost, the clock and the discount, in this order: the stage cost is discounted from the interval's start
        J = alive ? J + Dc * o.stage * o.dt : J;
        T = alive ? T + o.dt : T;
        Dc = alive ? Dc * exp(-beta * o.dt) : Dc;
        // 4. the outcome: the first k with v C < c_k, else the last k with p_k > 0
        double v = 0.0;
        if (fin) { // no draw: row s of the uniforms does not exist
        } else if (S.uniform) v = S.uniform[(size_t)i * S.nsteps + s];
        else {
            double u1;
            philox_jump_uniforms(S.seed, (unsigned long long)(S.traj_offset + i), (unsigned)s, v, u1);
        }
        const double vC = v * o.C;
        double cum = 0.0;
        int pick = -1, lastpos = -1;
#pragma unroll
        for (int k = 0; k < 2 * D; k++) {
            cum += o.p[k];
            pick = ((pick < 0) && (vC < cum)) ? k : pick;
            lastpos = (o.p[k] > 0.0) ? k : lastpos;
        }
        pick = (pick < 0) ? lastpos : pick;
#pragma unroll
        for (int m = 0; m < D; m++) {
            int lo, hi;
            (void)fixed_neighbors(ix[m], A.ngrid[m], A.bctype[m], lo, hi);
            const int nx = (pick == 2 * m) ? lo : ((pick == 2 * m + 1) ? hi : ix[m]);
            ix[m] = alive ? nx : ix[m];
        }
        // 5. the node after the step
        if (S.traj && se > 0 && (s + 1) % se == 0 && !fin && own)
#pragma unroll
            for (int m = 0; m < D; m++) S.traj[((size_t)i * nrow + (s + 1) / se) * D + m] = ix[m];
    }
    if (!own) return;
#pragma unroll
    for (int m = 0; m < D; m++) S.node[(size_t)i * D + m] = ix[m];
    S.cost[i] = J;
    S.disc[i] = Dc;
    S.time[i] = T;
    S.exit_step[i] = ex;
    if (st) atomicOr(A.status, st);
}

// ------------------------------------------------------------------------------------------------ the chain of a form
// The chain of the backup node_backup<.., FORM> applies, FORM a subset of {horizon, stop, jump} (form_offered, FORM_CHAIN); built
// by hipRTC only, for models compiled with the chain flag (rtc.hip).  The kernels above keep their own chain_node: sharing it
// would move their registers.
//
// Outcome order: the 2D axis neighbours (stencil order), then the marks m ascending with the weight rJ pi_m, rJ = h^2 lambda(x),
// then -- in horizon mode only -- the self-loop with the weight W - C, C = sum p_k + rJ.  The total is W = C without the horizon
// and W = h^2 / delta with it; the interval is h^2 / C, and delta with the horizon.  Sampling: the first outcome with v W < c_k
// (cumulative sums in outcome order), else the last one with a positive weight -- so a negative self-loop is never drawn.
// A mark outcome lands on a node of offgrid_cell's cell of the wrapped target: with whi the weight of the upper node of
// dimension m, m ascending and t = u1 at the start, the upper node is taken iff t < whi, and t becomes t / whi if it was taken,
// else (t - whi) / (1 - whi).  Under set_interp(ctx, 1) whi is 0 or 1, so the same rule names the nearer node.  A target inside
// an obstacle or outside an absorbing dimension's range ends the walk where it stands: it pays D_{s+1} times jump_target_value's
// cost and its exit word is s + 1.
template <int D>
struct ChainNodeForm {
    int flag;      // chain_flag
    int ui;        // the greedy candidate; ncand where the stop action wins; -1 on an absorbed, obstacle or stuck node
    bool stuck;    // live, no horizon, no stop, and no valid candidate or a winner with C < 1e-14
    bool stops;    // live, and the decision is the stop action
    double value;  // the backup's value; the bound / obstacle cost on a flagged node
    double stage;  // g(x, u); psi on a stopping node; the bound / obstacle cost on a flagged node
    double W, dt;  // the total weight and the interval; 0 where the chain does not move
    double rJ;     // the jump rate h^2 lambda(x); 0 where the chain does not move
    double pself;  // the self-loop's weight W - C (horizon mode); 0 otherwise
    double p[2 * D]; // the winner's un-normalised rates, stencil order; 0 where the chain does not move
    double vnode;  // the function train at the node
    double x[D];   // the node's coordinates
};

constexpr long long CHAIN_STOPPED_BIAS = (long long)1 << 32; // C3SC_CHAIN_STOPPED(s) = -(s + 2) - 2^32

template <int MID, class Model, int RP, unsigned FORM>
__device__ inline void chain_node_form(const KArgs &A, const double *__restrict__ ro, const CandLds<Model> &cr, const int (&ix)[Model::D],
                                       ChainNodeForm<Model::D> &o, unsigned &st)
{
    static_assert(form_offered(FORM, FORM_CHAIN), "the chain has no such form (form_offered, FORM_CHAIN)");
    constexpr bool HORIZON = (FORM & FORM_HORIZON) != 0, STOP = (FORM & FORM_STOP) != 0, JUMP = (FORM & FORM_JUMP) != 0;
    constexpr int D = Model::D, DU = Model::DU, NT = Model::NTAB > 0 ? Model::NTAB : 1, NCFa = Model::NCF > 0 ? Model::NCF : 1;
    double V[2 * D + 1];
    node_stencil<D, RP>(A, ro, ix, V);
    o.vnode = V[2 * D];
    o.flag = chain_flag<D>(A, ro, ix, o.x);
    double tv[NT];
    table_values<Model>(A, ro, ix, tv);
    double jrate = 0.0, jval = 0.0;
    if constexpr (JUMP) jump_term<Model, RP>(A, ro, o.x, jump_constelm<Model>(A, ro), jrate, jval);
    int ui;
    unsigned stb = 0; // of the backup's bits the chain passes on the CFL bit only; it reports stuck nodes itself
    o.value = node_backup<Model, 1, 1, CandLds<Model>, true, NoPre, FORM>(A, ro, o.x, tv, cr, V, o.flag, ui, stb, false, -1, NoPre(), jrate, jval);
    const bool live = o.flag == 0;
    bool stops = false;
    if constexpr (STOP) stops = live && (ui == A.ncand);
    // the winner's rates, by the statements of the backup's own dimensions
    const int uc = ((ui < 0) || (ui >= A.ncand)) ? 0 : ui;
    double u[DU], cf[NCFa];
    cf[0] = 0.0;
#pragma unroll
    for (int k = 0; k < DU; k++) u[k] = ro[A.cands_off + uc * DU + k];
#pragma unroll
    for (int q = 0; q < Model::NCF; q++) cf[q] = ro[A.cfeat_off + uc * Model::NCF + q];
    typename Model::Node nd;
    Model::prep(A.prm, o.x, tv, nd);
    double b[D], sg[D];
    Model::drift(A.prm, nd, o.x, u, cf, b);
    Model::sigma(A.prm, o.x, u, sg);
    double C = 0.0;
#pragma unroll
    for (int m = 0; m < D; m++) {
        upwind_rates(A.t[2 * m], A.t[2 * m + 1], b[m], sg[m], o.p[2 * m], o.p[2 * m + 1]);
        C += o.p[2 * m];
        C += o.p[2 * m + 1];
    }
    C += jrate;
    o.stuck = HORIZON ? false : (live && !stops && ((ui < 0) || (C < 1e-14)));
    const bool moves = live && !stops && !o.stuck;
    st |= o.stuck ? (unsigned)C3SC_STATUS_STATIONARY : 0u;
    st |= live ? (stb & (unsigned)C3SC_STATUS_CFL) : 0u;
    const double g = Model::stage(A.prm, o.x, u);
    o.stops = stops;
    o.ui = moves ? ui : (stops ? A.ncand : -1);
    o.stage = (live && !stops) ? g : o.value;
    double W = C, dt = A.h2 / (moves ? C : 1.0);
    if constexpr (HORIZON) {
        dt = ro[A.hz_off];
        W = A.h2 / dt;
    }
    o.W = moves ? W : 0.0;
    o.dt = moves ? dt : 0.0;
    o.rJ = moves ? jrate : 0.0;
    o.pself = (HORIZON && moves) ? W - C : 0.0;
#pragma unroll
    for (int k = 0; k < 2 * D; k++) o.p[k] = moves ? o.p[k] : 0.0;
}

// one lane per node: chain_transitions' outputs, and with them the self-loop's and the marks' probabilities and the marks' values
template <int MID, class Model, int RP, unsigned FORM>
__global__ void __launch_bounds__(256) k_chain_outcomes_form(const KArgs A, const ChainK S, const double *__restrict__ ro)
{
    constexpr int D = Model::D;
    extern __shared__ double smem[];
    CandLds<Model> cr;
    rollout_cands<Model>(A, ro, smem, cr);
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i = min(gid, S.n - 1); // tail lanes repeat the last node ...
    const bool own = gid < S.n;       // ... and store nothing
    int ix[D];
    chain_load_node<D>(A, S.node0 + (size_t)i * D, ix);
    ChainNodeForm<D> o;
    unsigned st = 0;
    chain_node_form<MID, Model, RP, FORM>(A, ro, cr, ix, o, st);
    const double inv = o.W > 0.0 ? o.W : 1.0;
    if constexpr ((FORM & FORM_JUMP) != 0) {
        const int ce = jump_constelm<Model>(A, ro);
#pragma unroll 1
        for (int m = 0; m < Model::NJUMP; m++) {
            double y[D];
            const double pi = Model::jump(A.prm, o.x, m, y);
            const double vj = jump_target_value<Model, RP>(A, ro, y, ce);
            if (S.pmark && own) S.pmark[(size_t)i * Model::NJUMP + m] = (o.rJ * pi) / inv;
            if (S.markval && own) S.markval[(size_t)i * Model::NJUMP + m] = vj;
        }
    }
    if (!own) return;
    if (S.uidx) S.uidx[i] = o.ui;
    if (S.value) S.value[i] = o.value;
    if (S.stage) S.stage[i] = o.stage;
    if (S.dt) S.dt[i] = o.dt;
    if (S.flag) S.flag[i] = o.flag;
    if (S.pself) S.pself[i] = o.pself / inv;
    if (S.P) {
#pragma unroll
        for (int k = 0; k < 2 * D; k++) S.P[(size_t)i * (2 * D) + k] = o.p[k] / inv;
    }
    if (st) atomicOr(A.status, st);
}

// one lane per trajectory
template <int MID, class Model, int RP, unsigned FORM>
__global__ void __launch_bounds__(256) k_chain_walk_form(const KArgs A, const ChainK S, const double *__restrict__ ro)
{
    constexpr bool HORIZON = (FORM & FORM_HORIZON) != 0, STOP = (FORM & FORM_STOP) != 0, JUMP = (FORM & FORM_JUMP) != 0;
    constexpr int D = Model::D;
    extern __shared__ double smem[];
    CandLds<Model> cr;
    rollout_cands<Model>(A, ro, smem, cr);
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i = min(gid, S.n - 1); // tail lanes repeat the last trajectory ...
    const bool own = gid < S.n;       // ... and store nothing
    const int se = S.save_every;
    const long nrow = se > 0 ? S.nsteps / se + 1 : 0, nurow = se > 0 ? (S.nsteps + se - 1) / se : 0;
    int ix[D];
    double J, Dc, T;
    long long ex;
    if (S.s0 == 0) {
        chain_load_node<D>(A, S.node0 + (size_t)i * D, ix);
        J = 0.0;
        Dc = 1.0;
        T = 0.0;
        ex = -1;
        if (S.traj && own)
#pragma unroll
            for (int m = 0; m < D; m++) S.traj[(size_t)i * nrow * D + m] = ix[m];
    } else {
        chain_load_node<D>(A, S.node + (size_t)i * D, ix);
        J = S.cost[i];
        Dc = S.disc[i];
        T = S.time[i];
        ex = S.exit_step[i];
    }
    const double beta = A.discount;
    unsigned st = 0;
    // the launch that ends the call makes one more trip, at xi_nsteps (fin, wave-uniform): the flag test and V_end only
    const int send = S.s1 == S.nsteps ? S.s1 + 1 : S.s1;
    for (int s = S.s0; s < send; s++) {
        const bool fin = s == S.nsteps;
        ChainNodeForm<D> o;
        unsigned stn = 0;
        chain_node_form<MID, Model, RP, FORM>(A, ro, cr, ix, o, stn);
        const bool running = ex == -1;
        st |= (running && !fin) ? stn : 0u; // a frozen lane raises nothing more
        // 1. the flag test
        const bool exits = running && (o.flag != 0);
        J = exits ? J + Dc * o.value : J;
        ex = exits ? (long long)s : ex;
        if (fin && S.vend && own) S.vend[i] = o.vnode;
        // 2. a stuck node freezes the lane where it is; so does the stop action, which pays psi (o.value there)
        const bool sticks = running && o.stuck && !fin;
        ex = sticks ? -((long long)s + 2) : ex;
        bool halts = false;
        if constexpr (STOP) {
            halts = running && !exits && o.stops && !fin;
            J = halts ? J + Dc * o.value : J;
            ex = halts ? -((long long)s + 2) - CHAIN_STOPPED_BIAS : ex;
        }
        const bool alive = running && !exits && !sticks && !halts && !fin;
        if (S.uidx && se > 0 && s % se == 0 && !fin && own) S.uidx[(size_t)i * nurow + s / se] = (alive || halts) ? o.ui : -1;
        // 3. the interval's cost, the clock and the discount, in this order
        J = alive ? J + Dc * o.stage * o.dt : J;
        T = alive ? T + o.dt : T;
        Dc = alive ? Dc * exp(-beta * o.dt) : Dc;
        // 4. the outcome: the first k with v W < c_k, else the last k with a positive weight
        double v = 0.0, u1 = 0.0;
        if (fin) { // no draw: row s of the uniforms does not exist
        } else if (S.uniform) {
            if constexpr (JUMP) {
                v = S.uniform[((size_t)i * S.nsteps + s) * 2];
                u1 = S.uniform[((size_t)i * S.nsteps + s) * 2 + 1];
            } else v = S.uniform[(size_t)i * S.nsteps + s];
        } else philox_jump_uniforms(S.seed, (unsigned long long)(S.traj_offset + i), (unsigned)s, v, u1);
        const double vW = v * o.W;
        double cum = 0.0;
        int pick = -1, lastpos = -1;
#pragma unroll
        for (int k = 0; k < 2 * D; k++) {
            cum += o.p[k];
            pick = ((pick < 0) && (vW < cum)) ? k : pick;
            lastpos = (o.p[k] > 0.0) ? k : lastpos;
        }
        int nmark = 0;
        double ysel[D], ylast[D];
#pragma unroll
        for (int m = 0; m < D; m++) ysel[m] = ylast[m] = o.x[m];
        if constexpr (JUMP) {
            nmark = Model::NJUMP;
#pragma unroll 1
            for (int mk = 0; mk < Model::NJUMP; mk++) {
                double y[D];
                const double w = o.rJ * Model::jump(A.prm, o.x, mk, y);
                cum += w;
                const bool take = (pick < 0) && (vW < cum), pos = w > 0.0;
                pick = take ? 2 * D + mk : pick;
                lastpos = pos ? 2 * D + mk : lastpos;
#pragma unroll
                for (int m = 0; m < D; m++) {
                    ysel[m] = take ? y[m] : ysel[m];
                    ylast[m] = pos ? y[m] : ylast[m];
                }
            }
        }
        if constexpr (HORIZON) {
            cum += o.pself;
            pick = ((pick < 0) && (vW < cum)) ? 2 * D + nmark : pick;
            lastpos = (o.pself > 0.0) ? 2 * D + nmark : lastpos;
        }
        const bool fell = pick < 0;
        pick = fell ? lastpos : pick;
        // a mark outcome: the wrapped target, its exit test (jump_target_value's) and its cell
        bool lands = false;
        int land[D];
#pragma unroll
        for (int m = 0; m < D; m++) land[m] = ix[m];
        if constexpr (JUMP) {
            const bool ismark = alive && (pick >= 2 * D) && (pick < 2 * D + nmark);
            double yin[D], y[D];
#pragma unroll
            for (int m = 0; m < D; m++) yin[m] = fell ? ylast[m] : ysel[m];
            wrap_periodic<D>(A, ro, yin, y);
            const bool inobs = in_obstacle<D>(A, ro, y);
            bool out = false;
#pragma unroll
            for (int m = 0; m < D; m++) {
                const double *g = ro + A.xg_off[m];
                out = out || ((A.bctype[m] == C3SC_ABSORB) && ((y[m] < g[0]) || (y[m] > g[A.ngrid[m] - 1])));
            }
            const double term = inobs ? Model::obscost(A.prm, y) : Model::boundcost(A.prm, y);
            const bool leaves = ismark && (inobs || out);
            J = leaves ? J + Dc * term : J; // Dc is D_{s+1} here
            ex = leaves ? (long long)s + 1 : ex;
            lands = ismark && !leaves;
            const int ce = jump_constelm<Model>(A, ro);
            double t = u1;
#pragma unroll
            for (int m = 0; m < D; m++) {
                int ic;
                double whi;
                offgrid_cell(ro + A.xg_off[m], A.ngrid[m], y[m], ce, ic, whi);
                const bool up = t < whi;
                t = up ? t / whi : (t - whi) / (1.0 - whi);
                land[m] = up ? ic + 1 : ic;
            }
        }
#pragma unroll
        for (int m = 0; m < D; m++) {
            int lo, hi;
            (void)fixed_neighbors(ix[m], A.ngrid[m], A.bctype[m], lo, hi);
            const int nx = (pick == 2 * m) ? lo : ((pick == 2 * m + 1) ? hi : ix[m]);
            ix[m] = alive ? (lands ? land[m] : nx) : ix[m];
        }
        // 5. the node after the step
        if (S.traj && se > 0 && (s + 1) % se == 0 && !fin && own)
#pragma unroll
            for (int m = 0; m < D; m++) S.traj[((size_t)i * nrow + (s + 1) / se) * D + m] = ix[m];
    }
    if (!own) return;
#pragma unroll
    for (int m = 0; m < D; m++) S.node[(size_t)i * D + m] = ix[m];
    S.cost[i] = J;
    S.disc[i] = Dc;
    S.time[i] = T;
    S.exit_step[i] = ex;
    if (st) atomicOr(A.status, st);
}


#ifndef __HIPCC_RTC__
// the launcher of both kernels (rollout geometry: one lane per trajectory / node, the candidate table in dynamic LDS)
template <class Model, auto KERN>
hipError_t launch_chain(const KArgs &A, const LaunchIO &io)
{
    if (A.cmode != 0) return hipErrorNotSupported; // candidate list only
    const ChainK &S = *(const ChainK *)io.sim;
    const size_t shmem = rollout_shmem(0, (size_t)CandLds<Model>::doubles(A.ncand));
    static LaunchCache cache;
    int blocks_per_cu = 1, num_cu = 256;
    hipError_t e = cache.prepare((const void *)KERN, 256, shmem, blocks_per_cu, num_cu);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(KERN, dim3(rollout_grid(S.n)), dim3(256), shmem, io.stream, A, S, io.ro);
    return hipGetLastError();
}

// one walk and one transitions kernel per (model, padded rank): the pairs that have a rollout kernel
#define C3SC_CHAIN_KERNELS(MODEL_ID, RP, ...)                                                                  \
    static Registrar C3SC_CAT(reg_cwalk_, __COUNTER__)(KernelEntry{                                           \
        MODEL_ID, __VA_ARGS__::D, RP, 0, VARIANT_CHAIN_WALK, 0, -1,                                             \
        &launch_chain<__VA_ARGS__, k_chain_walk<MODEL_ID, __VA_ARGS__, RP>>, "k_chain_walk<" #__VA_ARGS__ "," #RP ">"}); \
    static Registrar C3SC_CAT(reg_ctrans_, __COUNTER__)(KernelEntry{                                          \
        MODEL_ID, __VA_ARGS__::D, RP, 0, VARIANT_CHAIN_TRANSITIONS, 0, -1,                                      \
        &launch_chain<__VA_ARGS__, k_chain_transitions<MODEL_ID, __VA_ARGS__, RP>>,                            \
        "k_chain_transitions<" #__VA_ARGS__ "," #RP ">"});
#endif

} // namespace c3sc
