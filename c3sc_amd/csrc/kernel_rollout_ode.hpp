// kernel_rollout_ode.hpp -- deterministic closed-loop integration of the implicit policy (c3sc_hip_integrate).  DESIGN.md 4.9.
//
// One lane per trajectory, as k_rollout (kernel_rollout.hpp).  The examples' tail (dubinscar.c:379-412, perch.c:447-480, ...)
// integrates x' = b(x, pi(x)) with cdyn's controlled integrators, the controller inside the right-hand side: this kernel takes
// nsub substeps of forward Euler or classical RK4 per outer step, evaluates the controller at every stage state and carries
// the discounted cost c' = e^{-beta t} stage(y, pi(y)) as one more ODE component.  Stops (exit, goal box, keep-in box) are
// tested at every outer step.  A launch covers a range of substeps; state, cost and stop fields go to device memory between
// launches, and every lane follows the same substep schedule, so the results do not depend on how a call is cut.
//
// The controller block is k_rollout's, restated here as the function ode_policy (off-grid stencil at the possibly wrapped state,
// node_backup over the candidates in LDS or node_backup_box, u = 0 inside an obstacle); k_rollout keeps its own copy inline,
// because calling ode_policy from it changes the register allocation of its spilling instantiations.  The candidate-table fill,
// the wrap of the final state and the launcher are kernel_rollout.hpp's.  The lane-uniformity rules are the same:
// frozen lanes and workgroup tail lanes are selects, nothing is lane-distributed.  The stage loop is rolled, so the controller is
// emitted once.
#pragma once
#include "kernel_rollout.hpp"

namespace c3sc {

// argument block of one integrate launch (by value: kernarg space, wave-uniform)
struct OdeK {
    long n;                 // trajectories of the call
    long long k0, k1;       // substeps [k0, k1) of this launch; substep k belongs to outer step k / nsub
    int nsub;               // substeps per outer step
    int nout;               // outer steps of the call: the launch with k1 == nout * nsub tests x_nout and writes V_end
    int nstage;             // 1 (forward Euler) or 4 (RK4)
    int save_every;         // 0: nothing saved
    int wrap;               // map periodic dimensions into [lb, ub) before the controller sees the state
    int constelm;           // off-grid interpolation of a CONSTELM value function
    int has_goal, has_keep; // stop boxes in use
    double h;               // integrator step
    double dt_out;          // outer step (time of the stop tests)
    double goal_lo[MAXD], goal_hi[MAXD], keep_lo[MAXD], keep_hi[MAXD];
    const double *x0;       // [n][D] initial states (read when k0 == 0)
    double *x;              // [n][D] state between launches
    double *cost;           // [n] integrated discounted cost
    long long *stop_step;   // [n] -1 while running
    int32_t *stop_reason;   // [n] 0 while running
    double *traj;           // [n][nout / save_every + 1][D] or null
    double *u;              // [n][ceil(nout / save_every)][DU] or null
    double *vend;           // [n] or null
};

// pi(y): k_rollout's controller block at y (wrapped when S.wrap); also returns the model tables at y itself for the drift
template <int MID, class Model, int RP, bool BOX>
__device__ inline void ode_policy(const KArgs &A, const double *__restrict__ ro, const CandLds<Model> &cr, int wrap, int constelm,
                                  const double (&y)[Model::D], double (&u)[Model::DU],
                                  double (&cf)[Model::NCF > 0 ? Model::NCF : 1],
                                  double (&tvy)[Model::NTAB > 0 ? Model::NTAB : 1], unsigned &st)
{
    constexpr int D = Model::D, DU = Model::DU, NT = Model::NTAB > 0 ? Model::NTAB : 1, NCFa = Model::NCF > 0 ? Model::NCF : 1;
    double xin[D];
    if (wrap) wrap_periodic<D>(A, ro, y, xin);
    else
#pragma unroll
        for (int m = 0; m < D; m++) xin[m] = y[m];
    double V[2 * D + 1];
    int ab;
    offgrid_stencil<D, RP>(A, ro, xin, constelm, V, ab);
    double tv[NT];
    offgrid_tables<MID, Model>(xin, tv);
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
    if (!boxed) {
        int ui;
        (void)node_backup<Model, 1, 1, CandLds<Model>, true, NoPre, model_form<Model>()>(A, ro, xin, tv, cr, V, ab, ui, st);
        const int uc = ui < 0 ? 0 : (model_game<Model>() ? game_pair_to_list(A, ui) : ui); // game: the saddle pair's list position
#pragma unroll
        for (int k = 0; k < DU; k++) u[k] = (ui >= 0) ? ro[A.cands_off + uc * DU + k] : 0.0; // obstacle: u = 0
#pragma unroll
        for (int q = 0; q < Model::NCF; q++) cf[q] = ro[A.cfeat_off + uc * Model::NCF + q];
    }
    // the dynamics at y itself (the controller may have seen the wrapped state)
    if (wrap) offgrid_tables<MID, Model>(y, tvy);
    else
#pragma unroll
        for (int t = 0; t < NT; t++) tvy[t] = tv[t];
}

// state in, controller at every stage state, RK4 / forward-Euler substep, stops, state out
template <int MID, class Model, int RP, bool BOX>
__global__ void __launch_bounds__(256) k_rollout_ode(const KArgs A, const OdeK S, const double *__restrict__ ro)
{
    constexpr int D = Model::D, DU = Model::DU, NT = Model::NTAB > 0 ? Model::NTAB : 1, NCFa = Model::NCF > 0 ? Model::NCF : 1;
    extern __shared__ double smem[];
    CandLds<Model> cr;
    rollout_cands<Model>(A, ro, smem, cr);
    const long i = min((long)blockIdx.x * blockDim.x + threadIdx.x, S.n - 1); // tail lanes repeat the last trajectory
    const int se = S.save_every, nsub = S.nsub;
    const long nrow = se > 0 ? S.nout / se + 1 : 0, nurow = se > 0 ? (S.nout + se - 1) / se : 0;
    const long long ktot = (long long)S.nout * nsub;
    double x[D], J;
    long long stp;
    int why;
    if (S.k0 == 0) {
#pragma unroll
        for (int m = 0; m < D; m++) x[m] = S.x0[(size_t)i * D + m];
        J = 0.0;
        stp = -1;
        why = 0;
        if (S.traj)
#pragma unroll
            for (int m = 0; m < D; m++) S.traj[(size_t)i * nrow * D + m] = x[m];
    } else {
#pragma unroll
        for (int m = 0; m < D; m++) x[m] = S.x[(size_t)i * D + m];
        J = S.cost[i];
        stp = S.stop_step[i];
        why = S.stop_reason[i];
    }
    const double beta = A.discount, h = S.h;
    unsigned st = 0;
    // the stops at x_j, in the contract's order: exit (1 face / 2 obstacle; its cost is charged once), goal (3), keep-in (4)
    auto stop_test = [&](long long j) {
        const bool inobs = in_obstacle<D>(A, ro, x);
        bool out = false, ingoal = S.has_goal != 0, outkeep = false;
#pragma unroll
        for (int m = 0; m < D; m++) {
            const double *g = ro + A.xg_off[m];
            out = out || ((A.bctype[m] == C3SC_ABSORB) && ((x[m] < g[0]) || (x[m] > g[A.ngrid[m] - 1])));
            ingoal = ingoal && (S.goal_lo[m] < x[m]) && (x[m] < S.goal_hi[m]);
            outkeep = outkeep || (x[m] < S.keep_lo[m]) || (x[m] > S.keep_hi[m]);
        }
        outkeep = outkeep && (S.has_keep != 0);
        const bool run = stp < 0, ex = inobs || out;
        const double disc = exp(-beta * ((double)j * S.dt_out));
        const double term = inobs ? Model::obscost(A.prm, x) : Model::boundcost(A.prm, x);
        J = (run && ex) ? J + disc * term : J;
        const int r = ex ? (inobs ? 2 : 1) : (ingoal ? 3 : (outkeep ? 4 : 0));
        stp = (run && r != 0) ? j : stp;
        why = (run && r != 0) ? r : why;
    };
    for (long long k = S.k0; k < S.k1; k++) {
        const long long j = k / nsub;
        const int sub = (int)(k - j * nsub);
        if (sub == 0) stop_test(j);
        const bool alive = stp < 0;
        const double t = (double)k * h;
        double y[D], ks[D], kq[D], cs = 0.0, cq = 0.0;
#pragma unroll
        for (int m = 0; m < D; m++) { y[m] = x[m]; ks[m] = 0.0; kq[m] = 0.0; }
#pragma unroll 1
        for (int q = 0; q < S.nstage; q++) { // wave-uniform: Euler one stage, RK4 four
            const double a = (q == 0) ? 0.0 : ((q == 3) ? h : h / 2);
#pragma unroll
            for (int m = 0; m < D; m++) y[m] = (q == 0) ? x[m] : x[m] + a * kq[m];
            double u[DU], cf[NCFa], tvy[NT];
            ode_policy<MID, Model, RP, BOX>(A, ro, cr, S.wrap, S.constelm, y, u, cf, tvy, st);
#pragma unroll
            for (int c = 0; c < DU; c++) u[c] = alive ? u[c] : 0.0;
            if (S.u && se > 0 && q == 0 && sub == 0 && j % se == 0)
#pragma unroll
                for (int c = 0; c < DU; c++) S.u[((size_t)i * nurow + j / se) * DU + c] = u[c];
            const double stage = Model::stage(A.prm, y, u);
            typename Model::Node nd;
            Model::prep(A.prm, y, tvy, nd);
            double b[D];
            Model::drift(A.prm, nd, y, u, cf, b);
            const double disc = exp(-beta * (t + a));
            const double wq = (q == 0 || q == 3) ? 1.0 : 2.0;
#pragma unroll
            for (int m = 0; m < D; m++) {
                kq[m] = b[m];
                ks[m] = (q == 0) ? b[m] : ks[m] + wq * b[m];
            }
            cq = disc * stage;
            cs = (q == 0) ? cq : cs + wq * cq;
        }
        if (S.nstage == 1) { // forward Euler in k_rollout's order: J + disc stage dt, x + b dt
            J = alive ? J + cs * h : J;
#pragma unroll
            for (int m = 0; m < D; m++) x[m] = alive ? x[m] + ks[m] * h : x[m];
        } else { // RK4: y + h/6 (k1 + 2 k2 + 2 k3 + k4)
            J = alive ? J + h / 6.0 * cs : J;
#pragma unroll
            for (int m = 0; m < D; m++) x[m] = alive ? x[m] + h / 6.0 * ks[m] : x[m];
        }
        if (S.traj && se > 0 && sub == nsub - 1 && (j + 1) % se == 0)
#pragma unroll
            for (int m = 0; m < D; m++) S.traj[((size_t)i * nrow + (j + 1) / se) * D + m] = x[m];
    }
    if (S.k1 == ktot) { // the final state: its stops and the value there
        stop_test(S.nout);
        if (S.vend) {
            double xin[D], V[2 * D + 1];
            int ab;
            rollout_input<D>(A, ro, S.wrap, x, xin);
            offgrid_stencil<D, RP>(A, ro, xin, S.constelm, V, ab);
            S.vend[i] = V[2 * D];
        }
    }
#pragma unroll
    for (int m = 0; m < D; m++) S.x[(size_t)i * D + m] = x[m];
    S.cost[i] = J;
    S.stop_step[i] = stp;
    S.stop_reason[i] = why;
    if (st) atomicOr(A.status, st);
}

#ifndef __HIPCC_RTC__
// one integrate kernel per (model, padded rank); BOX = 1 where the model's Bellman kernels serve the control box too
#define C3SC_REG_ROLLOUT_ODE(MODEL_ID, RP, BOX, ...)                                                                   \
    static Registrar C3SC_CAT(reg_rode_, __COUNTER__)(KernelEntry{                                                    \
        MODEL_ID, __VA_ARGS__::D, RP, 0, VARIANT_ROLLOUT_ODE, 0, -1,                                                   \
        &launch_closed_loop<__VA_ARGS__, BOX, OdeK, k_rollout_ode<MODEL_ID, __VA_ARGS__, RP, BOX>>,                       \
        "k_rollout_ode<" #__VA_ARGS__ "," #RP ">"});
#endif

} // namespace c3sc
