// kernel_rollout.hpp -- batched closed-loop rollouts of the implicit policy (c3sc_hip_simulate) and the off-grid stencil
// they are built on (c3sc_hip_stencil_points).  DESIGN.md 4.8.
//
// One lane per trajectory.  A step of a lane is c3control_simulate's step (c3sc_bellman.c) with the host callbacks
// replaced by the device model: the off-grid stencil of mca_get_neighbor_node_costs at the controller's input, the
// per-lane minimiser the Bellman kernels use (node_backup over the candidate list, node_backup_box in a control box), then
// one Euler-Maruyama step with the model's diagonal diffusion.  Trajectory state stays in registers for the steps of a
// launch and goes to device memory between launches (a call is cut into launches of a bounded number of steps).
//
// Lanes are independent trajectories.  The kernels' own boundary branches, exit freeze and workgroup tail are selects (tail
// lanes repeat the last trajectory and store the same bits to the same addresses); the device libm (cos / sin / tan of the
// models' tables at an off-grid state) and the box minimiser do branch per lane.  That is harmless because nothing here is
// lane-distributed: the candidate table lives in LDS (CandLds, wave-uniform addresses), not in VGPR lanes read by v_readlane.
// The candidate-table fill, the wrap of the final state and the launcher are shared with the deterministic integrator,
// k_rollout_ode (kernel_rollout_ode.hpp).  The controller block is not: k_rollout keeps it in its step loop and k_rollout_ode has
// ode_policy, the same statements as a function.  Calling that function from k_rollout changes the register allocation of the
// instantiations that spill (car7d at ranks 16 and 20, cothrust6d at 20).
// tests/test_rollout_isa.py checks the ISA (global loads only; no scratch at the benchmark's ranks).
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>

#include <type_traits>
#endif

#include "kernel_common.hpp"
#include "model_tables.hpp"
#include "philox.hpp"
#include "registry.hpp"

namespace c3sc {

// argument block of one rollout / stencil-points launch (by value: kernarg space, wave-uniform)
struct SimK {
    long n;                 // trajectories (points) of the call
    long long traj_offset;  // global index of trajectory 0 (Philox counter)
    int s0, s1;             // steps [s0, s1) of this launch
    int nsteps;             // steps of the call: the launch with s1 == nsteps also tests x_nsteps and writes V_end
    int save_every;         // 0: nothing saved
    int wrap;               // map periodic dimensions into [lb, ub) before the controller sees the state
    int constelm;           // off-grid interpolation of a CONSTELM value function
    unsigned long long seed;
    double dt, sqdt;
    const double *x0;       // [n][D]: initial states (rollouts, read when s0 == 0) / the points (stencil_points)
    const double *noise;    // [n][nsteps][D] standard normals, or null: Philox (philox.hpp)
    double *x;              // [n][D] state between launches
    double *cost;           // [n] discounted cost so far
    long long *exit_step;   // [n] -1 while running
    double *traj;           // [n][nsteps / save_every + 1][D] or null
    double *u;              // [n][ceil(nsteps / save_every)][DU] or null
    double *vend;           // [n] or null
    double *out;            // stencil_points: [n][2D + 1]
    int32_t *absorbed;      // stencil_points: [n] or null
};

template <int B, int E, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// valuef_eval's cell of coordinate x on the grid g[0..N) (c3sc_cross.c: clamp, then the bisection): node i and the weight
// of node i + 1.  The bisection runs a wave-uniform number of rounds (enough for N), each a select: the same cell as the
// host's `while (hi - lo > 1)` without a lane-dependent trip count.
__device__ inline void offgrid_cell(const double *__restrict__ g, int N, double x, int constelm, int &i, double &w)
{
    int nit = 0;
    while ((1 << nit) < N - 1) nit++; // wave-uniform
    int lo = 0, hi = N - 1;
    for (int it = 0; it < nit; it++) {
        const int mid = (lo + hi) >> 1;
        const bool go = hi - lo > 1, le = g[mid] <= x;
        lo = (go && le) ? mid : lo;
        hi = (go && !le) ? mid : hi;
    }
    const double g0 = g[0], gn = g[N - 1], gl = g[lo], gr = g[lo + 1];
    const double wi = (x - gl) / (gr - gl);
    i = (x <= g0) ? 0 : ((x >= gn) ? N - 2 : lo);
    w = (x <= g0) ? 0.0 : ((x >= gn) ? 1.0 : wi);
    w = constelm ? ((w < 0.5) ? 0.0 : 1.0) : w; // the nearer node's value holds on its cell
}

// entry e of core m interpolated between nodes i and i + 1 (padded layout of k_pad_core)
template <int RP>
__device__ __forceinline__ double core_at(const double *__restrict__ G, int per, int i, double w, int e)
{
    return (1.0 - w) * G[(size_t)i * per + e] + w * G[(size_t)(i + 1) * per + e];
}

// v[0], with v rotated left by one (v[k] = v[k+1], v[RP-1] = the old v[0]): a rolled loop over a reads "v[a]" this way --
// indexing the register vector with the loop counter would move it to scratch
template <int RP>
__device__ __forceinline__ double rot_left(double (&v)[RP])
{
    const double h = v[0];
#pragma unroll
    for (int k = 0; k + 1 < RP; k++) v[k] = v[k + 1];
    v[RP - 1] = h;
    return h;
}

// mca_get_neighbor_node_costs (c3sc_bellman.c; nodeutil.c:718-816) at an arbitrary state x: V[2m], V[2m+1] = the
// interpolant at the (-, +) neighbour one grid spacing away in dim m (boundary rules of the host code), V[2D] = the
// interpolant at x.  Inside an obstacle every entry is the value at x and ab = -1.
// Neighbour m differs from x in coordinate m only: V(y) = L_m G_m(y_m) R_{m+1} with the prefix L_m = G_0(x_0) ... G_{m-1}
// (x_{m-1}) and the suffix R_{m+1} = G_{m+1}(x_{m+1}) ... G_{D-1}(x_{D-1}).  The suffixes are formed once (D-1 vectors in
// registers), the prefix is carried along the forward sweep: about 3 D r^2 multiply-adds per point instead of (2D+1) D r^2.
template <int D, int RP>
__device__ inline void offgrid_stencil(const KArgs &A, const double *__restrict__ ro, const double (&x)[D], int constelm,
                                       double (&V)[2 * D + 1], int &ab)
{
    static_assert(D >= 2, "dimension");
    ab = in_obstacle<D>(A, ro, x) ? -1 : 0;
    int ic[D];
    double wc[D];
#pragma unroll
    for (int m = 0; m < D; m++) offgrid_cell(ro + A.xg_off[m], A.ngrid[m], x[m], constelm, ic[m], wc[m]);
    double R[D][RP]; // R[m] = suffix from core m on (m = 1 .. D-1)
    {
        const double *G = ro + A.core_off[D - 1];
#pragma unroll
        for (int a = 0; a < RP; a++) R[D - 1][a] = core_at<RP>(G, RP, ic[D - 1], wc[D - 1], a);
    }
    static_for<1, D - 1>([&](auto mc) { // m = D-2 .. 1 (compile-time indices: R stays in registers)
        constexpr int m = D - 1 - decltype(mc)::value;
        const double *G = ro + A.core_off[m];
#pragma unroll
        for (int a = 0; a < RP; a++) R[m][a] = 0.0;
#pragma unroll 1
        for (int a = 0; a < RP; a++) { // row a of G_m(x_m) R_{m+1}, shifted in at the end: R[m][a] after RP rounds
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < RP; b++) s += core_at<RP>(G, RP * RP, ic[m], wc[m], a + b * RP) * R[m + 1][b];
            (void)rot_left<RP>(R[m]);
            R[m][RP - 1] = s;
        }
    });
    double L[RP];
    static_for<0, D>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const double *g = ro + A.xg_off[m];
        const int N = A.ngrid[m];
        const double xm = x[m], lb = g[0], ub = g[N - 1], h = g[1] - g[0];
        const int bc = A.bctype[m];
        const bool interior = ((xm + h) < ub) && (xm - h > lb);
        const bool left = !interior && ((xm - h) <= lb), right = !interior && !left;
        double yl = xm - h, yr = xm + h;
        const double yl_per = (xm > lb) ? ub - (h - (xm - lb)) : (ub - (lb - xm)) - h;
        const double yr_per = (xm < ub) ? lb + (h - (ub - xm)) : (lb + (xm - ub)) + h;
        yl = left ? ((bc == C3SC_PERIODIC) ? yl_per : lb) : yl;
        yr = right ? ((bc == C3SC_PERIODIC) ? yr_per : ub) : yr;
        int il, ir;
        double wl, wr;
        offgrid_cell(g, N, yl, constelm, il, wl);
        offgrid_cell(g, N, yr, constelm, ir, wr);
        const double *G = ro + A.core_off[m];
        double vl = 0.0, vr = 0.0;
        {
            if constexpr (m == 0) {
#pragma unroll
                for (int b = 0; b < RP; b++) {
                    vl += core_at<RP>(G, RP, il, wl, b) * R[1][b];
                    vr += core_at<RP>(G, RP, ir, wr, b) * R[1][b];
                    L[b] = core_at<RP>(G, RP, ic[0], wc[0], b);
                }
            } else if constexpr (m == D - 1) {
                double vx = 0.0;
#pragma unroll
                for (int a = 0; a < RP; a++) {
                    vl += L[a] * core_at<RP>(G, RP, il, wl, a);
                    vr += L[a] * core_at<RP>(G, RP, ir, wr, a);
                    vx += L[a] * core_at<RP>(G, RP, ic[m], wc[m], a);
                }
                V[2 * D] = vx;
            } else {
                // L_m G_m(y) R_{m+1} row by row; the row loops stay rolled (a fully unrolled r x r product keeps all its
                // loads in flight: hundreds of VGPRs), and L is read by rotating it instead of indexing it with the row
                auto through = [&](int iy, double wy) {
                    double v = 0.0;
#pragma unroll 1
                    for (int a = 0; a < RP; a++) {
                        const double la = rot_left<RP>(L);
                        double t = 0.0;
#pragma unroll
                        for (int b = 0; b < RP; b++) t += core_at<RP>(G, RP * RP, iy, wy, a + b * RP) * R[m + 1][b];
                        v += la * t;
                    }
                    return v;
                };
                vl = through(il, wl);
                vr = through(ir, wr);
                double Ln[RP];
#pragma unroll
                for (int b = 0; b < RP; b++) Ln[b] = 0.0;
#pragma unroll 1
                for (int a = 0; a < RP; a++) {
                    const double la = rot_left<RP>(L);
#pragma unroll
                    for (int b = 0; b < RP; b++) Ln[b] += la * core_at<RP>(G, RP * RP, ic[m], wc[m], a + b * RP);
                }
#pragma unroll
                for (int b = 0; b < RP; b++) L[b] = Ln[b];
            }
        }
        V[2 * m] = vl;
        V[2 * m + 1] = vr;
    });
#pragma unroll
    for (int e = 0; e < 2 * D; e++) V[e] = (ab != 0) ? V[2 * D] : V[e];
}

// x with its periodic dimensions mapped into [lb, ub) (the examples' state_transform, e.g. dubinscar.c:168)
template <int D>
__device__ inline void wrap_periodic(const KArgs &A, const double *__restrict__ ro, const double (&x)[D], double (&y)[D])
{
#pragma unroll
    for (int m = 0; m < D; m++) {
        const double *g = ro + A.xg_off[m];
        const double lb = g[0], ub = g[A.ngrid[m] - 1], len = ub - lb;
        double v = x[m] - floor((x[m] - lb) / len) * len;
        v = (v >= ub) ? v - len : v;
        v = (v < lb) ? v + len : v;
        y[m] = (A.bctype[m] == C3SC_PERIODIC) ? v : x[m];
    }
}

// The interpolant valuef_eval and the rollouts use at one arbitrary point y per lane (the V[2D] of offgrid_stencil alone):
// L = G_0(y_0) G_1(y_1) ... G_{D-1}(y_{D-1}), one offgrid_cell per dimension and D - 1 vector-matrix products.  Every core entry
// is gathered per lane from the padded cores in the arena, so there is no SGPR matrix operand and no LDS table here.  The row
// loops stay rolled and L is read by rotation, as in offgrid_stencil: unrolled, every core load stays in flight.
//
// Cell indices are in range for EVERY double y.  offgrid_cell keeps 0 <= lo < hi <= N - 1 through the bisection whatever the
// comparisons return, so lo is in [0, N - 2]; the result is 0, N - 2 or lo, and core_at reads nodes i and i + 1 <= N - 1.  A NaN
// fails every comparison (lo stays 0, neither clamp fires: cell 0 with a NaN weight), +-inf take the clamps (cells N - 2 and 0
// with weights 1 and 0).  A non-finite y therefore gives a non-finite or clamped VALUE and never an address outside core m.
template <int D, int RP>
__device__ inline double offgrid_value(const KArgs &A, const double *__restrict__ ro, const double (&y)[D], int constelm)
{
    static_assert(D >= 2, "dimension");
    int ic[D];
    double wc[D];
#pragma unroll
    for (int m = 0; m < D; m++) offgrid_cell(ro + A.xg_off[m], A.ngrid[m], y[m], constelm, ic[m], wc[m]);
    double L[RP];
    {
        const double *G = ro + A.core_off[0];
#pragma unroll
        for (int b = 0; b < RP; b++) L[b] = core_at<RP>(G, RP, ic[0], wc[0], b);
    }
    static_for<1, D - 1>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        const double *G = ro + A.core_off[m];
        double Ln[RP];
#pragma unroll
        for (int b = 0; b < RP; b++) Ln[b] = 0.0;
#pragma unroll 1
        for (int a = 0; a < RP; a++) {
            const double la = rot_left<RP>(L);
#pragma unroll
            for (int b = 0; b < RP; b++) Ln[b] += la * core_at<RP>(G, RP * RP, ic[m], wc[m], a + b * RP);
        }
#pragma unroll
        for (int b = 0; b < RP; b++) L[b] = Ln[b];
    });
    const double *G = ro + A.core_off[D - 1];
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < RP; a++) v += L[a] * core_at<RP>(G, RP, ic[D - 1], wc[D - 1], a);
    return v;
}

// The value a jump or an intervention to the state yin pays (jump_term and impulse_term call it):
// periodic dimensions are wrapped; a target the rollouts' exit_test
// calls exited -- inside an obstacle, or outside [lb, ub] on an absorbing dimension -- pays obscost or boundcost there, by
// exit_test's choice; any other target pays the interpolant, which clamps to the grid hull (reflecting dimensions clamp).
// Selects only: an exited lane evaluates the interpolant at its clamped cell as well.
template <class Model, int RP>
__device__ inline double jump_target_value(const KArgs &A, const double *__restrict__ ro, const double (&yin)[Model::D], int constelm)
{
    constexpr int D = Model::D;
    double y[D];
    wrap_periodic<D>(A, ro, yin, y);
    const bool inobs = in_obstacle<D>(A, ro, y);
    bool out = false;
#pragma unroll
    for (int m = 0; m < D; m++) {
        const double *g = ro + A.xg_off[m];
        out = out || ((A.bctype[m] == C3SC_ABSORB) && ((y[m] < g[0]) || (y[m] > g[A.ngrid[m] - 1])));
    }
    const double term = inobs ? Model::obscost(A.prm, y) : Model::boundcost(A.prm, y);
    const double v = offgrid_value<D, RP>(A, ro, y, constelm);
    return (inobs || out) ? term : v;
}

// The jump term of the node (or off-grid state) x: rate = h^2 lambda(x) and J = sum_m pi_m(x) Vjump(y_m), m ascending, one fma
// chain from 0.0.  The marks stay a rolled loop: one point evaluation's registers, not NJUMP of them.
template <class Model, int RP>
__device__ inline void jump_term(const KArgs &A, const double *__restrict__ ro, const double (&x)[Model::D], int constelm, double &rate,
                                 double &J)
{
    static_assert(Model::NJUMP >= 1 && Model::NJUMP <= C3SC_JUMP_MAX, "number of marks");
    rate = A.h2 * Model::jumprate(A.prm, x);
    J = 0.0;
#pragma unroll 1
    for (int m = 0; m < Model::NJUMP; m++) {
        double y[Model::D];
        const double pi = Model::jump(A.prm, x, m, y);
        J = fma(pi, jump_target_value<Model, RP>(A, ro, y, constelm), J);
    }
}

// The best intervention at the node (or off-grid state) x: c_m = k_m(x) + Vt(y_m), m ascending, Vt exactly the
// value a jump to y_m pays (jump_target_value).  The running minimum starts at +inf and is taken by the first strict '<', so
// imark = -1 where no c_m is finite (k_m = +inf or NaN: "not admissible at x").  On the forced path a lane whose fu names an
// intervention takes exactly that mark, by a select in the same loop: the trip count is NIMPULSE on every lane.  The marks stay
// a rolled loop: one point evaluation's registers, not NIMPULSE of them.
template <class Model, int RP>
__device__ inline void impulse_term(const KArgs &A, const double *__restrict__ ro, const double (&x)[Model::D], int constelm, bool forced,
                                    int fu, double &ival, int &imark)
{
    static_assert(Model::NIMPULSE >= 1 && Model::NIMPULSE <= C3SC_IMPULSE_MAX, "number of interventions");
    ival = __builtin_inf();
    imark = -1;
    const int fm = fu - A.ncand - 1;
#pragma unroll 1
    for (int m = 0; m < Model::NIMPULSE; m++) {
        double y[Model::D];
        const double k = Model::impulse(A.prm, x, m, y);
        const double c = k + jump_target_value<Model, RP>(A, ro, y, constelm);
        const bool take = forced ? (m == fm) : ((__builtin_fabs(k) < __builtin_inf()) & (c < ival)); // -inf is not a cost either
        ival = take ? c : ival;
        imark = take ? m : imark;
    }
}

// The function train at one GRID NODE per lane: L = G_0[idx_0] G_1[idx_1] ... G_{D-1}[idx_{D-1}], gathered from
// the padded cores in the arena.  offgrid_value's shape -- rolled row loops, L read by rotation, global loads only -- without
// offgrid_cell and without weights: one entry per core element and lane where core_at gathers two.  The caller keeps
// 0 <= idx[m] < A.ngrid[m].
// node_value_sub is the same at the node idx with the indices of the (wave-uniform) dimensions i and j replaced by ni and nj:
// the substitution is a select per dimension, so a caller inside a rolled loop (corr_term) builds no index vector -- a vector
// built there and handed on by reference is left behind as a stack object in three dimensions.
template <int D, int RP>
__device__ __forceinline__ double node_value_sub(const KArgs &A, const double *__restrict__ ro, const int (&idx)[D], int i, int ni, int j,
                                                 int nj)
{
    static_assert(D >= 2, "dimension");
    double L[RP];
    {
        const int n0 = (i == 0) ? ni : ((j == 0) ? nj : idx[0]);
        const double *G = ro + A.core_off[0] + (size_t)n0 * RP;
#pragma unroll
        for (int b = 0; b < RP; b++) L[b] = G[b];
    }
#pragma unroll
    for (int m = 1; m < D - 1; m++) {
        const int nm = (i == m) ? ni : ((j == m) ? nj : idx[m]);
        const double *G = ro + A.core_off[m] + (size_t)nm * (RP * RP);
        double Ln[RP];
#pragma unroll
        for (int b = 0; b < RP; b++) Ln[b] = 0.0;
#pragma unroll 1
        for (int a = 0; a < RP; a++) {
            const double la = rot_left<RP>(L);
#pragma unroll
            for (int b = 0; b < RP; b++) Ln[b] += la * G[a + b * RP];
        }
#pragma unroll
        for (int b = 0; b < RP; b++) L[b] = Ln[b];
    }
    const int nl = (i == D - 1) ? ni : ((j == D - 1) ? nj : idx[D - 1]);
    const double *G = ro + A.core_off[D - 1] + (size_t)nl * RP;
    double v = 0.0;
#pragma unroll
    for (int a = 0; a < RP; a++) v += L[a] * G[a];
    return v;
}
template <int D, int RP>
__device__ inline double node_value(const KArgs &A, const double *__restrict__ ro, const int (&idx)[D])
{
    return node_value_sub<D, RP>(A, ro, idx, -1, 0, -1, 0);
}

// The cross-diffusion correction of the node x with the multi-index ix (Kushner and Dupuis 5.3).  For each pair
// p = (i, j) of the model's compile-time list, p ascending, with a_p = covar(x, p) and t_m = A.t[2m]:
//     r_p = (t_i t_j / h^2) |a_p| / 2        the un-normalised rate to each of two diagonal neighbours,
// (+,+) and (-,-) where a_p > 0, (+,-) and (-,+) otherwise -- a per-lane select of indices -- and the same r_p off each of the
// four axis rates of i and j:
//     cq = sum_p (-2 r_p),   cpv = sum_p r_p [(V_d1 + V_d2) - ((V[2i] + V[2i+1]) + (V[2j] + V[2j+1]))]   (one fma chain from 0.0).
// A diagonal neighbour is a grid node: in both dimensions its index is fixed_neighbors' lo / hi of ix -- for the varying
// dimension too -- so a reflecting end names the node itself, the periodic seam n - 2 / 1, and a live node on an absorbing
// face of a fixed dimension itself.  Its value is the function train's there (node_value_sub): no exit test, no obstacle cost,
// no interpolation.  Dominance: the axis probability of dimension m stays non-negative iff t2_m sigma_m^2 / 2 >= sum_{p with m}
// r_p, sigma at the first candidate's control as in node_backup's Q0 block (the diffusion of a paired dimension must not read
// the control); a live lane that violates it raises C3SC_STATUS_DOMINANCE and keeps the algebra's value.
// The loop over the pairs is unrolled: the list is a compile-time constant, so i and j are, and everything that belongs to them
// (node index, size, boundary type, t, the axis values) is read directly.  Rolled, with i and j wave-uniform run-time values
// picked by selects, the three-dimensional forms were left with a 36-byte stack object of scalar spill slots that no instruction
// addressed.  The two point evaluations of a pair stay a rolled loop, and the pairs' evaluations are independent of each other
// only through cpv's chain, so the kernel holds little more than one evaluation's registers (DESIGN.md 4.16 has the counts).
template <class Model, int RP>
__device__ inline void corr_term(const KArgs &A, const double *__restrict__ ro, const double (&x)[Model::D], const int (&ix)[Model::D],
                                 const double (&V)[2 * Model::D + 1], int ab, double &cq, double &cpv, unsigned &st)
{
    constexpr int D = Model::D, P = Model::NCORR;
    static_assert(P >= 1 && P <= C3SC_CORR_MAX, "number of pairs");
    double used[D];
#pragma unroll
    for (int m = 0; m < D; m++) used[m] = 0.0;
    cq = 0.0;
    cpv = 0.0;
#pragma unroll
    for (int p = 0; p < P; p++) {
        const int i = Model::CORR_I[p], j = Model::CORR_J[p]; // constants of the unrolled trip
        const double a = Model::covar(A.prm, x, p);
        const double r = (A.t[2 * i] * A.t[2 * j] / A.h2) * __builtin_fabs(a) / 2.0;
        const bool pos = a > 0.0;
        int li, hi_i, lj, hj;
        (void)fixed_neighbors(ix[i], A.ngrid[i], A.bctype[i], li, hi_i);
        (void)fixed_neighbors(ix[j], A.ngrid[j], A.bctype[j], lj, hj);
        double vd = 0.0;
#pragma unroll 1
        for (int e = 0; e < 2; e++) { // e = 0: the neighbour on i's + side, e = 1: on its - side
            const int ni = e ? li : hi_i, nj = ((e != 0) == pos) ? lj : hj;
            vd += node_value_sub<D, RP>(A, ro, ix, i, ni, j, nj);
        }
        cq += -2.0 * r;
        cpv = fma(r, vd - ((V[2 * i] + V[2 * i + 1]) + (V[2 * j] + V[2 * j + 1])), cpv);
        used[i] += r;
        used[j] += r;
    }
    bool viol = false;
    {
        double u[Model::DU], s[D];
#pragma unroll
        for (int c = 0; c < Model::DU; c++) u[c] = ro[A.cands_off + c];
        Model::sigma(A.prm, x, u, s);
#pragma unroll
        for (int m = 0; m < D; m++) viol |= A.t[2 * m + 1] * (s[m] * s[m]) / 2.0 < used[m];
    }
    if (viol & (ab == 0)) st |= C3SC_STATUS_DOMINANCE;
}

template <int MID, class Model>
__device__ inline void offgrid_tables(const double (&x)[Model::D], double (&tv)[Model::NTAB > 0 ? Model::NTAB : 1])
{
    tv[0] = 0.0;
#pragma unroll
    for (int t = 0; t < Model::NTAB; t++) tv[t] = model_table_value(MID, t, x[Model::tab_dim(t)]);
}

template <int D, int RP>
__global__ void __launch_bounds__(256) k_stencil_points(const KArgs A, const SimK S, const double *__restrict__ ro)
{
    const long i = min((long)blockIdx.x * blockDim.x + threadIdx.x, S.n - 1); // tail lanes repeat the last point
    double x[D], V[2 * D + 1];
#pragma unroll
    for (int m = 0; m < D; m++) x[m] = S.x0[(size_t)i * D + m];
    int ab;
    offgrid_stencil<D, RP>(A, ro, x, S.constelm, V, ab);
#pragma unroll
    for (int e = 0; e < 2 * D + 1; e++) S.out[(size_t)i * (2 * D + 1) + e] = V[e];
    if (S.absorbed) S.absorbed[i] = ab;
}

// ---- the blocks k_rollout and k_rollout_ode (kernel_rollout_ode.hpp) share

// the candidate table of the list minimiser in dynamic LDS (the box minimiser, A.cmode == 1, reads none)
template <class Model>
__device__ inline void rollout_cands(const KArgs &A, const double *__restrict__ ro, double *smem, CandLds<Model> &cr)
{
    cr.tb = smem;
    if (A.cmode == 0) {
        for (int c0 = 0; c0 < A.ncand; c0 += 64) { // every wave writes the same rows
            CandRegs<Model> cr0;
            cr0.load(A, ro, c0);
            cr.fill(smem, cr0, A.ncand, c0);
        }
        __syncthreads();
    }
}

// the state the value function is read at for V_end: x, wrapped into the periodic dimensions when the call asks for it
template <int D>
__device__ inline void rollout_input(const KArgs &A, const double *__restrict__ ro, int wrap, const double (&x)[D], double (&xin)[D])
{
    if (wrap) wrap_periodic<D>(A, ro, x, xin);
    else
#pragma unroll
        for (int m = 0; m < D; m++) xin[m] = x[m];
}

// impulse models: the intervention of one step of one lane; empty for every other model, whose kernels keep
// their registers
template <int D, bool ON>
struct ImpulseStep {
};
template <int D>
struct ImpulseStep<D, true> {
    bool now = false;
    double y[D] = {};
};

// state in, controller, Euler-Maruyama step, exit test, state out
// BOX: the instantiation also serves the control-box minimiser (A.cmode == 1, a wave-uniform switch)
template <int MID, class Model, int RP, bool BOX>
__global__ void __launch_bounds__(256) k_rollout(const KArgs A, const SimK S, const double *__restrict__ ro)
{
    constexpr int D = Model::D, DU = Model::DU, NT = Model::NTAB > 0 ? Model::NTAB : 1, NCFa = Model::NCF > 0 ? Model::NCF : 1;
    extern __shared__ double smem[];
    CandLds<Model> cr;
    rollout_cands<Model>(A, ro, smem, cr);
    const long i = min((long)blockIdx.x * blockDim.x + threadIdx.x, S.n - 1); // tail lanes repeat the last trajectory
    const int se = S.save_every;
    const long nrow = se > 0 ? S.nsteps / se + 1 : 0, nurow = se > 0 ? (S.nsteps + se - 1) / se : 0;
    double x[D], J;
    long long ex;
    if (S.s0 == 0) {
#pragma unroll
        for (int m = 0; m < D; m++) x[m] = S.x0[(size_t)i * D + m];
        J = 0.0;
        ex = -1;
        if (S.traj)
#pragma unroll
            for (int m = 0; m < D; m++) S.traj[(size_t)i * nrow * D + m] = x[m];
    } else {
#pragma unroll
        for (int m = 0; m < D; m++) x[m] = S.x[(size_t)i * D + m];
        J = S.cost[i];
        ex = S.exit_step[i];
    }
    const double beta = A.discount, dt = S.dt;
    unsigned st = 0;
    // stop models: a voluntary stop at step k is kept as -(k + 2), so "still running" is -1 alone there
    auto running = [&]() {
        if constexpr (model_stop<Model>()) return ex == -1;
        else return ex < 0;
    };
    // exit at x_s: outside [lb, ub] on an absorbing dimension or inside an obstacle; the exit cost is charged once
    auto exit_test = [&](int s, double disc) {
        const bool inobs = in_obstacle<D>(A, ro, x);
        bool out = false;
#pragma unroll
        for (int m = 0; m < D; m++) {
            const double *g = ro + A.xg_off[m];
            out = out || ((A.bctype[m] == C3SC_ABSORB) && ((x[m] < g[0]) || (x[m] > g[A.ngrid[m] - 1])));
        }
        const bool now = running() && (inobs || out);
        const double term = inobs ? Model::obscost(A.prm, x) : Model::boundcost(A.prm, x);
        J = now ? J + disc * term : J;
        ex = now ? (long long)s : ex;
    };
    for (int s = S.s0; s < S.s1; s++) {
        const double disc = exp(-beta * ((double)s * dt));
        exit_test(s, disc);
        bool alive = running();
        double xin[D];
        if (S.wrap) wrap_periodic<D>(A, ro, x, xin);
        else
#pragma unroll
            for (int m = 0; m < D; m++) xin[m] = x[m];
        double V[2 * D + 1];
        int ab;
        offgrid_stencil<D, RP>(A, ro, xin, S.constelm, V, ab);
        double tv[NT];
        offgrid_tables<MID, Model>(xin, tv);
        double u[DU], cf[NCFa];
#pragma unroll
        for (int q = 0; q < NCFa; q++) cf[q] = 0.0;
        bool boxed = false;
        if constexpr (BOX) {
            if (A.cmode == 1) {
                boxed = true;
                double uo[DU];
                (void)node_backup_box<Model>(A, xin, tv, V, ab, uo, st, false, nullptr);
#pragma unroll
                for (int k = 0; k < DU; k++) u[k] = uo[k];
                if constexpr (requires { Model::CF_FROM_U; }) Model::features(u, cf);
            }
        }
        ImpulseStep<D, model_impulse<Model>()> iv; // impulse models: whether this lane's controller intervenes at this step, and where to
        if (!boxed) {
            int ui;
            // jump models: the controller's backup gets the jump term at the state it sees
            double jrate = 0.0, jval = 0.0;
            if constexpr (model_jump<Model>()) jump_term<Model, RP>(A, ro, xin, S.constelm, jrate, jval);
            // impulse models: ... and the best intervention there, after the jump term's registers are dead
            double ival = 0.0;
            int imark = -1;
            if constexpr (model_impulse<Model>()) impulse_term<Model, RP>(A, ro, xin, S.constelm, false, -1, ival, imark);
            // no rollout has a corr form (form_offered, FORM_ROLLOUT): the bit is masked off
            (void)node_backup<Model, 1, 1, CandLds<Model>, true, NoPre, (model_form<Model>() & ~FORM_CORR)>(
                A, ro, xin, tv, cr, V, ab, ui, st, false, -1, NoPre(), jrate, jval, ival, imark);
            if constexpr (model_impulse<Model>()) { // the controller intervenes here: the lane pays k_m at the state the controller saw
                                                    // and moves there to y_m; the step slot carries no stage cost and no increment
                iv.now = alive && (ui > A.ncand);
                const double kc = Model::impulse(A.prm, xin, iv.now ? ui - A.ncand - 1 : 0, iv.y);
                J = iv.now ? J + disc * kc : J;
                ui = (ui > A.ncand) ? -1 : ui; // the candidate table has no row >= ncand: u = 0
            }
            if constexpr (model_stop<Model>()) { // the controller stops here: the lane pays psi and is frozen like an exited one.  psi is
                                                 // taken at the state the controller saw (wrapped, with S.wrap): the amount that won
                const bool stopnow = alive && (ui == A.ncand);
                J = stopnow ? J + disc * Model::stopcost(A.prm, xin) : J;
                ex = stopnow ? -((long long)s + 2) : ex;
                alive = alive && !stopnow;
                ui = (ui == A.ncand) ? -1 : ui; // the candidate table has no row ncand: u = 0
            }
            const int uc = ui < 0 ? 0 : (model_game<Model>() ? game_pair_to_list(A, ui) : ui); // game: the saddle pair's list position
#pragma unroll
            for (int k = 0; k < DU; k++) u[k] = (ui >= 0) ? ro[A.cands_off + uc * DU + k] : 0.0; // obstacle: u = 0
#pragma unroll
            for (int q = 0; q < Model::NCF; q++) cf[q] = ro[A.cfeat_off + uc * Model::NCF + q];
        }
#pragma unroll
        for (int k = 0; k < DU; k++) u[k] = alive ? u[k] : 0.0;
        if (S.u && se > 0 && s % se == 0)
#pragma unroll
            for (int k = 0; k < DU; k++) S.u[((size_t)i * nurow + s / se) * DU + k] = u[k];
        const double stage = Model::stage(A.prm, x, u);
        if constexpr (model_impulse<Model>()) J = (alive && !iv.now) ? J + disc * stage * dt : J; // an intervention step pays no stage cost
        else J = alive ? J + disc * stage * dt : J;
        // the dynamics at x itself (the controller may have seen the wrapped state)
        double tvx[NT];
        if (S.wrap) offgrid_tables<MID, Model>(x, tvx);
        else
#pragma unroll
            for (int t = 0; t < NT; t++) tvx[t] = tv[t];
        typename Model::Node nd;
        Model::prep(A.prm, x, tvx, nd);
        double b[D], sg[D];
        Model::drift(A.prm, nd, x, u, cf, b);
        Model::sigma(A.prm, x, u, sg);
        double xi[D];
        if (S.noise)
#pragma unroll
            for (int m = 0; m < D; m++) xi[m] = S.noise[((size_t)i * S.nsteps + s) * D + m];
        else
#pragma unroll
            for (int m = 0; m < D; m++) xi[m] = philox_normal(S.seed, (unsigned long long)(S.traj_offset + i), (unsigned)s, (unsigned)m);
        // jump models: the compound-Poisson increment of the step, evaluated at x_k like the Euler-Maruyama increment.  An event
        // when u0 < min(lambda dt, 1) (no transcendental: the host twin takes the same branch); the mark is the first m with
        // u1 < pi_0 + .. + pi_m, and the last mark catches what rounding leaves.  Both uniforms are Philox's, with caller-supplied
        // normals too.  Selects only.
        double dj[D];
#pragma unroll
        for (int m = 0; m < D; m++) dj[m] = 0.0;
        if constexpr (model_jump<Model>()) {
            double u0, u1;
            philox_jump_uniforms(S.seed, (unsigned long long)(S.traj_offset + i), (unsigned)s, u0, u1);
            const bool event = u0 < fmin(Model::jumprate(A.prm, x) * dt, 1.0);
            double cum = 0.0;
            bool found = false;
            for (int mk = 0; mk < Model::NJUMP; mk++) {
                double y[D];
                cum += Model::jump(A.prm, x, mk, y);
                const bool take = event && !found && ((u1 < cum) || (mk == Model::NJUMP - 1));
#pragma unroll
                for (int m = 0; m < D; m++) dj[m] = take ? y[m] - x[m] : dj[m];
                found = found || take;
            }
        }
#pragma unroll
        for (int m = 0; m < D; m++) {
            double acc = x[m] + b[m] * dt; // c3control_simulate's order
            acc += sg[m] * S.sqdt * xi[m];
            if constexpr (model_jump<Model>()) acc += dj[m];
            if constexpr (model_impulse<Model>()) acc = iv.now ? iv.y[m] : acc;
            x[m] = alive ? acc : x[m];
        }
        if (S.traj && se > 0 && (s + 1) % se == 0)
#pragma unroll
            for (int m = 0; m < D; m++) S.traj[((size_t)i * nrow + (s + 1) / se) * D + m] = x[m];
    }
    if (S.s1 == S.nsteps) { // the final state: its exit test and the value there
        const double dend = exp(-beta * ((double)S.nsteps * dt));
        exit_test(S.nsteps, dend);
        // horizon mode: this launch carries the cores of V_nsteps, and a trajectory still alive at the end pays
        // the discounted interpolant there, so that the mean of J estimates V_0(x_0)
        if (S.vend || model_horizon<Model>()) {
            double xin[D], V[2 * D + 1];
            int ab;
            rollout_input<D>(A, ro, S.wrap, x, xin);
            offgrid_stencil<D, RP>(A, ro, xin, S.constelm, V, ab);
            if (S.vend) S.vend[i] = V[2 * D];
            if constexpr (model_horizon<Model>()) J = running() ? J + dend * V[2 * D] : J;
        }
    }
#pragma unroll
    for (int m = 0; m < D; m++) S.x[(size_t)i * D + m] = x[m];
    S.cost[i] = J;
    S.exit_step[i] = ex;
    if (st) atomicOr(A.status, st);
}

#ifndef __HIPCC_RTC__
// Launch geometry of k_rollout / k_rollout_ode (one lane per trajectory), shared with the module launcher of run-time compiled
// models (rtc.hip): dynamic LDS holds the candidate table (cand_doubles = CandLds<Model>::doubles(ncand)); the box minimiser
// reads none
inline size_t rollout_shmem(int cmode, size_t cand_doubles) { return (cmode == 0 ? cand_doubles : 1) * sizeof(double); }
inline unsigned rollout_grid(long n) { return (unsigned)((n + 255) / 256); }

// the launcher of k_rollout (K = SimK) and k_rollout_ode (K = OdeK): KERN is the kernel, so each has its own LaunchCache
template <class Model, bool BOX, class K, auto KERN>
hipError_t launch_closed_loop(const KArgs &A, const LaunchIO &io)
{
    if (A.cmode == 1 && !BOX) return hipErrorNotSupported;
    const K &S = *(const K *)io.sim;
    const size_t shmem = rollout_shmem(A.cmode, (size_t)CandLds<Model>::doubles(A.ncand));
    static LaunchCache cache;
    int blocks_per_cu = 1, num_cu = 256;
    hipError_t e = cache.prepare((const void *)KERN, 256, shmem, blocks_per_cu, num_cu);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(KERN, dim3(rollout_grid(S.n)), dim3(256), shmem, io.stream, A, S, io.ro);
    return hipGetLastError();
}

template <int D, int RP>
hipError_t launch_stencil_points(const KArgs &A, const LaunchIO &io)
{
    const SimK &S = *(const SimK *)io.sim;
    hipLaunchKernelGGL((k_stencil_points<D, RP>), dim3(rollout_grid(S.n)), dim3(256), 0, io.stream, A, S, io.ro);
    return hipGetLastError();
}

#ifndef C3SC_CAT
#define C3SC_CAT2(a, b) a##b
#define C3SC_CAT(a, b) C3SC_CAT2(a, b)
#endif

// one rollout kernel per (model, padded rank); BOX = 1 where the model's Bellman kernels serve the control box too
#define C3SC_REG_ROLLOUT(MODEL_ID, RP, BOX, ...)                                                               \
    static Registrar C3SC_CAT(reg_roll_, __COUNTER__)(KernelEntry{                                            \
        MODEL_ID, __VA_ARGS__::D, RP, 0, VARIANT_ROLLOUT, 0, -1,                                               \
        &launch_closed_loop<__VA_ARGS__, BOX, SimK, k_rollout<MODEL_ID, __VA_ARGS__, RP, BOX>>,                   \
        "k_rollout<" #__VA_ARGS__ "," #RP ">"});
#define C3SC_REG_STENCIL_POINTS(DIM, RP)                                                                       \
    static Registrar C3SC_CAT(reg_stp_, __COUNTER__)(KernelEntry{                                             \
        0, DIM, RP, 0, VARIANT_STENCIL_POINTS, 0, -1, &launch_stencil_points<DIM, RP>,                           \
        "k_stencil_points<" #DIM "," #RP ">"});
#endif

} // namespace c3sc
