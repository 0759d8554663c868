"""Impulse control (c3sc_hip_set_impulses): device sources of a three-intervention LQR on the ragged 21 x 70
grid, of a two-intervention LQR in three dimensions, of a known-answer model and of the two-item inventory problem of
examples/inventory_impulse.c; a numpy restatement of the backup with interventions, dense value iteration of the inventory
problem on its whole 11 x 11 grid (dense_vi), the replay of a rollout with interventions and a restatement of the noisy
rollouts (inv_rollouts).  Shared by the CPU and GPU tests.  It shares no code with the kernels; the value at a target and the interpolants are jump_lib's.

The operator is the quasi-variational inequality V(x) = min(min_u backup_u(x), min_m [k_m(x) + Vt(y_m(x))]).  The candidates are
scanned first (backup_ref.candidate_values: the plain backup, with the Poisson term where jumps are on), then the interventions,
m ascending: c_m = k_m(x) + Vt(y_m); the running minimum of the c_m starts at +inf and is taken by the first strict '<', a cost
that is not finite never wins; the best intervention then beats the scan's winner where it is strictly smaller and where the
scan left no valid candidate (backup_ref.backup with c).  Intervention m has the index ncand + 1 + m (ncand is the stop
action's).  Vt is jump_lib.vjump:
periodic wrap, the obstacle or boundary cost at a target that left the domain, otherwise the interpolant clamped to the hull."""
import dataclasses

import numpy as np

import backup_ref as BR
import jump_lib as JL
import stop_lib as SL

IMPULSE_MAX = 8

# ---------------------------------------------------------------------------------------------------- the 2-D impulse LQR
# jump_lib's LQR (prm = {sig, q, r, s, K, kp, lam0, lam1}; the stop parameters' places hold the intervention costs) with three
# interventions whose displacements are no multiples of the grid spacings:
#   0: y = 0.3 x + (0.11, -0.07)   k = K (0.8 + kp |x - y|_1)   always interior
#   1: y = x + (0.53, 0)           k = K (1.0 + kp 0.53)        beyond the absorbing face of dim 0 from x0 > 1.47, into the
#                                                               obstacle from the nodes to its left
#   2: y = x + (0, 0.71)           k = K (0.9 + kp 0.71)        across the periodic seam of dim 1 from x1 > 1.29; not admissible
#                                                               (+inf) where x0 > 0.3
LQR_IMPULSES = r"""
__device__ double impulse(const double *prm, const double *x, int m, double *y)
{
    if (m == 0) {
        y[0] = 0.3 * x[0] + 0.11;
        y[1] = 0.3 * x[1] - 0.07;
        return prm[4] * (0.8 + prm[5] * (fabs(x[0] - y[0]) + fabs(x[1] - y[1])));
    }
    if (m == 1) {
        y[0] = x[0] + 0.53;
        y[1] = x[1];
        return prm[4] * (1.0 + prm[5] * 0.53);
    }
    y[0] = x[0];
    y[1] = x[1] + 0.71;
    return x[0] > 0.3 ? __builtin_inf() : prm[4] * (0.9 + prm[5] * 0.71);
}
"""
LQR = SL.LQR + LQR_IMPULSES
LQR_JUMP = SL.LQR + JL.LQR_JUMPS + LQR_IMPULSES
LQR_MASKS = JL.LQR_MASKS
LQR_NIMPULSE = 3
LQR_KP = 0.1


def lqr_prm(K, jumps=True):
    """K: the cost scale of the interventions (inf: none is admissible anywhere)"""
    return JL.LQR_PRM[:4] + (K, LQR_KP) + (JL.LQR_PRM[6:] if jumps else (0.0, 0.0))


def lqr_impulses(prm, x):
    """numpy twin of LQR_IMPULSES: (k [P, 3], y [P, 3, 2]) for x [P, 2]"""
    K, kp = prm[4], prm[5]
    y0 = 0.3 * x + np.array([0.11, -0.07])
    y = np.stack([y0, x + np.array([0.53, 0.0]), x + np.array([0.0, 0.71])], axis=1)
    k0 = K * (0.8 + kp * (np.abs(x[:, 0] - y0[:, 0]) + np.abs(x[:, 1] - y0[:, 1])))
    k1 = np.full(len(x), K * (1.0 + kp * 0.53))
    k2 = np.where(x[:, 0] > 0.3, np.inf, K * (0.9 + kp * 0.71))
    return np.stack([k0, k1, k2], axis=-1), y


def lqr_workload(mid, rank, discount, K, jumps=True):
    """the ragged 21 x 70 grid of the stop and jump tests"""
    return dataclasses.replace(JL.lqr_workload(mid, rank, discount, lqr_prm(K, jumps)), name="lqr_ic")


# the cost scale per rank: the seeded trains of the tests hold values of about 0.12 rank with a few per cent of node-to-node
# variation, so an intervention competes with the continuation value when its cost is a small fraction of that.
# tests/test_impulse_lib.py holds the preconditions of the GPU comparison (interventions win at 10 % .. 90 % of the live nodes,
# each of them somewhere, margins clear at 99.9 %) to these numbers
LQR_COST_SCALE = {4: 0.08, 8: 0.08, 12: 0.1}


def lqr_cost_scale(rank, discount=None):
    return LQR_COST_SCALE[rank]


# ---------------------------------------------------------------------------------------------------- the 3-D impulse LQR
# jump_lib's LQR3 on 5 x 128 x 5 (absorbing, periodic, reflecting) for the L2 form, two interventions:
#   0: y = 0.4 x                    k = K (1 + kp |x|_1)
#   1: y = x + (0, 0.61, 1.22)      k = K 0.9      across the seam; beyond the reflecting face: clamped
LQR3_IMPULSES = r"""
__device__ double impulse(const double *prm, const double *x, int m, double *y)
{
    if (m == 0) {
        y[0] = 0.4 * x[0];
        y[1] = 0.4 * x[1];
        y[2] = 0.4 * x[2];
        return prm[4] * (1.0 + prm[5] * (fabs(x[0]) + fabs(x[1]) + fabs(x[2])));
    }
    y[0] = x[0];
    y[1] = x[1] + 0.61;
    y[2] = x[2] + 1.22;
    return prm[4] * 0.9;
}
"""
LQR3 = JL.LQR3 + LQR3_IMPULSES
LQR3_MASKS = JL.LQR3_MASKS
LQR3_NIMPULSE = 2
LQR3_K = 0.06


def lqr3_prm(K=LQR3_K):
    return JL.LQR3_PRM[:4] + (K, LQR_KP) + JL.LQR3_PRM[6:]


def lqr3_impulses(prm, x):
    K, kp = prm[4], prm[5]
    y = np.stack([0.4 * x, x + np.array([0.0, 0.61, 1.22])], axis=1)
    k = np.stack([K * (1.0 + kp * np.abs(x).sum(-1)), np.full(len(x), K * 0.9)], axis=-1)
    return k, y


def lqr3_workload(mid, ranks=(1, 12, 9, 1), discount=0.3, K=LQR3_K):
    return dataclasses.replace(JL.lqr3_workload(mid, ranks, discount), name="lqr3_ic", params=lqr3_prm(K))


# ---------------------------------------------------------------------------------------------------- the known answer
# every target beyond the absorbing face of dim 0, which costs c, and constant k_m: V = min(continuation, min_m k_m + c)
# exactly.  prm = {sig, q, r, s, c, k0, k1, k2}
KNOWN = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = u[0]; b[1] = u[1]; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[0]; s[1] = prm[0]; }
__device__ double stage(const double *prm, const double *x, const double *u)
{
    return prm[1] * (x[0] * x[0] + x[1] * x[1]) + prm[2] * (u[0] * u[0] + u[1] * u[1]);
}
__device__ double boundcost(const double *prm, const double *x) { return prm[4]; }
__device__ double obscost(const double *prm, const double *x) { return -1.0; }
__device__ double impulse(const double *prm, const double *x, int m, double *y)
{
    y[0] = x[0] + 10.0 + m;
    y[1] = x[1];
    return prm[5 + m];
}
"""
KNOWN_MASKS = LQR_MASKS
KNOWN_NIMPULSE = 3
KNOWN_PRM = (0.3, 1.0, 1.0, 2.0, 0.25, 0.375, 0.3125, 0.3125)  # k1 = k2 < k0: mark 1 wins the tie, by the first strict '<'
KNOWN_TARGET = 0.25 + 0.3125  # exact in binary; near the median continuation value of the seeded rank-4 train on 9 x 13


def known_impulses(prm, x):
    y = np.stack([x + np.array([10.0 + m, 0.0]) for m in range(3)], axis=1)
    return np.broadcast_to(np.array(prm[5:8]), (len(x), 3)), y


def known_workload(mid, rank=4, discount=0.3):
    from c3sc_amd import workloads as wl

    return wl.Workload("known_ic", mid, KNOWN_PRM, 2, 2, (-1.0, -1.0), (1.0, 1.0), (9, 13), wl.uniform_ranks(2, rank), discount,
                       (wl.BC_ABSORB, wl.BC_REFLECT), [], JL.lqr_cands())


# ---------------------------------------------------------------------------------------------------- one node
def impulse_values(w, impulses, interp, x, bcost, ocost, constelm=False):
    """c [P, M] = k_m(x) + Vt(y_m) of every intervention at the states x [P, D]; +inf where k_m is not finite"""
    k, y = impulses(w.params, x)
    c = np.full(k.shape, np.inf)
    for m in range(k.shape[1]):
        adm = np.isfinite(k[:, m])
        ym = np.where(adm[:, None], y[:, m], x)  # the target of an inadmissible intervention is not used
        c[:, m] = np.where(adm, k[:, m] + JL.vjump(w, interp, ym, bcost, ocost, constelm), np.inf)
    return c


def impulse_fibers(w, host, impulses, interp, k, idx, costs, absorbed, bcost, ocost, forced=None, constelm=False, jumps=None,
                   with_impulses=True):
    """the backup with interventions of every node of fibers idx from their stencils (costs [F, N, 2D+1], absorbed [F, N]) and
    the interpolant `interp` of the same value function; jumps: a jump model of jump_lib to add the Poisson term (None: no
    jumps).  Returns (value, index, margin, stationary, c [F, N, M]) of shape [F, N]"""
    x = BR.node_states(w, k, idx).reshape(-1, w.dx)
    if jumps is not None:
        jrate, J = JL.jump_terms(w, jumps, interp, x, bcost, ocost, constelm)
    else:
        jrate, J = np.zeros(len(x)), np.zeros(len(x))
    c = impulse_values(w, impulses, interp, x, bcost, ocost, constelm)
    if not with_impulses:
        c = np.full(c.shape, np.inf)
    out, ui, mg, stat, _ = BR.fibers(w, host, k, idx, costs, absorbed, bcost, ocost, jrate, jrate * J, c=c, forced=forced)
    return out, ui, mg, stat, c.reshape(absorbed.shape + (c.shape[1],))


def point_decisions(w, host, impulses, interp, x, V, ab, bcost, ocost, constelm=False):
    """the controller's decision at arbitrary states x [n, D] from their off-grid stencils V [n, 2D+1] (ab: -1 inside an
    obstacle): (index [n], margin [n]) of the backup with interventions, -1 where absorbed"""
    h2, t = BR.mca_constants(w)
    vals, _, _ = BR.candidate_values(host, w.params, x, V, np.asarray(w.cands, dtype=np.float64), h2, t, w.discount)
    _, ui, mg = BR.backup(vals, c=impulse_values(w, impulses, interp, x, bcost, ocost, constelm))
    return np.where(ab != 0, -1, ui), mg


# ---------------------------------------------------------------------------------------------------- the inventory problem
# examples/inventory_impulse.c: the stock x = (x_0, x_1) of two items, x_i < 0 a backlog.  Demand is Brownian with the mean rate
# d, production at the rate u_i from a candidate list costs cu u_i^2: dx_i = (u_i - d) dt + sig dw_i.  Holding costs hold per
# unit and time, a backlog back.  Interventions: order q of item 1, q of item 2, q of both at a joint fixed cost below the sum of
# the two, 2 q of both; every order pays its fixed cost and cq per unit.  Both dimensions absorb: the boundary cost is the
# holding / backlog cost rate over the discount rate.  prm = {sig, d, hold, back, cu, q, K1, K12}
INV = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = u[0] - prm[1]; b[1] = u[1] - prm[1]; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[0]; s[1] = prm[0]; }
__device__ double inv_run(const double *prm, const double *x)
{
    return (x[0] > 0.0 ? prm[2] * x[0] : -prm[3] * x[0]) + (x[1] > 0.0 ? prm[2] * x[1] : -prm[3] * x[1]);
}
__device__ double stage(const double *prm, const double *x, const double *u) { return inv_run(prm, x) + prm[4] * (u[0] * u[0] + u[1] * u[1]); }
__device__ double boundcost(const double *prm, const double *x) { return inv_run(prm, x) / 0.5; }
__device__ double obscost(const double *prm, const double *x) { return 0.0; }
__device__ double impulse(const double *prm, const double *x, int m, double *y)
{
    const double q = prm[5], n0 = (m == 0 || m == 2) ? 1.0 : (m == 3 ? 2.0 : 0.0), n1 = (m == 1 || m == 2) ? 1.0 : (m == 3 ? 2.0 : 0.0);
    y[0] = x[0] + n0 * q;
    y[1] = x[1] + n1 * q;
    return (m < 2 ? prm[6] : prm[7]) + 0.2 * q * (n0 + n1);
}
"""
INV_MASKS = dict(udep_mask=0b11, uconst_mask=0b11, stage_udep=True)
INV_NIMPULSE = 4
INV_BETA = 0.5
INV_CQ = 0.2
INV_PRM = (0.4, 0.5, 1.0, 4.0, 0.5, 0.7, 0.5, 0.7)
INV_N = 11
INV_LB, INV_UB = -2.0, 2.0
INV_PLAIN_SWEEPS = 400  # sweeps without interventions from 0: the no-intervention solution, converged to the last bit
INV_SWEEPS = 200  # dense_vi from that solution meets its fixed point to 1e-10 within this many sweeps (152 when it was recorded)


def inv_cands():
    u = np.array([0.0, 0.5, 1.0])
    return np.array([(a, b) for a in u for b in u])


def inv_run(prm, x):
    return (np.where(x[..., 0] > 0, prm[2] * x[..., 0], -prm[3] * x[..., 0]) +
            np.where(x[..., 1] > 0, prm[2] * x[..., 1], -prm[3] * x[..., 1]))


def inv_host(prm, x, u):
    b = u - prm[1] + 0.0 * x
    return b, np.full(b.shape, prm[0]), inv_run(prm, x) + prm[4] * (u ** 2).sum(-1)


def inv_bcost(prm, x):
    return inv_run(prm, x) / INV_BETA


def inv_impulses(prm, x):
    q = prm[5]
    n = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, 2.0]])
    y = x[:, None, :] + q * n[None]
    k = np.array([prm[6], prm[6], prm[7], prm[7]]) + INV_CQ * q * n.sum(-1)
    return np.broadcast_to(k, (len(x), 4)), y


def inv_workload(mid, rank=INV_N):
    from c3sc_amd import workloads as wl

    return wl.Workload("inventory", mid, INV_PRM, 2, 2, (INV_LB, INV_LB), (INV_UB, INV_UB), (INV_N, INV_N), wl.uniform_ranks(2, rank),
                       INV_BETA, (wl.BC_ABSORB, wl.BC_ABSORB), [], inv_cands())


def dense_vi(w, host, impulses, bcost, V0, nsweeps, with_impulses=True, fault=None):
    """value iteration sweeps of the impulse operator on the whole grid of a 2-D workload whose dimensions both absorb: the
    boundary nodes keep their boundary cost, and the targets read the bilinear interpolant of the sweep's input V (a target
    beyond a face pays the boundary cost there).  Returns ([V_0, V_1, .. V_nsweeps], the indices of every sweep).
    fault = "stale": the obstacle k_m + V(y_m) is read from the continuation values of the sweep before instead of from V"""
    x, ab, sten = BR.grid2(w)
    h2, t = BR.mca_constants(w)
    ocost = lambda xx: np.zeros(len(xx))
    start = np.where(ab, bcost(x), np.asarray(V0).reshape(-1)).reshape(w.ngrid)
    before = [None]  # the input of the sweep before

    def terms(Vn):
        src = Vn
        if fault == "stale":
            src = start
            if before[0] is not None:
                vals, _, _ = BR.candidate_values(host, w.params, x, sten(before[0]), np.asarray(w.cands, dtype=np.float64), h2, t, w.discount)
                src = np.where(ab, bcost(x), np.nanmin(vals, axis=1)).reshape(w.ngrid)
            before[0] = Vn
        c = impulse_values(w, impulses, JL.Nodal(w, src), x, bcost, ocost)
        return None, None, c if with_impulses else np.full(c.shape, np.inf), None

    V, dec, _, _, _ = BR.sweeps(w, host, start, bcost(x), nsweeps, terms, fault=fault if fault in ("index", "le") else None)
    return V, dec


# ---------------------------------------------------------------------------------------------------- rollouts
def replay(w, impulses, drift_fn, stage_fn, bcost, ocost, traj, u, marks, dt, beta, wrap=False):
    """a rollout without noise replayed from its saved states traj [n, N + 1, D], controls u [n, N, du] and the intervention of
    every step, marks [n, N] (-1: none): every step's exit test at the state itself (obstacle first, then the absorbing faces),
    then either the stage cost and x + b dt, or -- an intervention -- k_m(xin) and y_m(xin) with no stage cost and no drift,
    xin the wrapped state if wrap.  Returns (next states [n, N, D] as predicted, exit step [n] (-1: never), cost [n])"""
    n, N1, D = traj.shape
    N = N1 - 1
    alive = np.ones(n, dtype=bool)
    ex = np.full(n, -1)
    J = np.zeros(n)
    nxt = np.zeros((n, N, D))
    nowrap = dataclasses.replace(w, bc=tuple(0 if b == 2 else b for b in w.bc))

    def exit_test(s, xs):
        nonlocal alive, J
        _, inobs, out, _ = JL.target_kinds(nowrap, xs)
        gone = alive & (inobs | out)
        J = J + np.where(gone, np.exp(-beta * (s * dt)) * np.where(inobs, ocost(xs), bcost(xs)), 0.0)
        ex[gone] = s
        alive = alive & ~gone

    for s in range(N):
        xs = traj[:, s]
        exit_test(s, xs)
        disc = np.exp(-beta * (s * dt))
        xin = JL.wrap(w, xs) if wrap else xs
        k, y = impulses(w.params, xin)
        mk = marks[:, s]
        iv = alive & (mk >= 0)
        ar = np.arange(n)
        J = J + np.where(iv, disc * k[ar, np.maximum(mk, 0)], 0.0)
        us = np.where((alive & ~iv)[:, None], u[:, s], 0.0)
        J = J + np.where(alive & ~iv, disc * stage_fn(xs, us) * dt, 0.0)
        acc = np.where(iv[:, None], y[ar, np.maximum(mk, 0)], xs + drift_fn(xs, us) * dt)
        nxt[:, s] = np.where(alive[:, None], acc, xs)
    exit_test(N, traj[:, N])
    return nxt, ex, J


# ---------------------------------------------------------------------------------------------------- the reference API
INV_VI_SWEEPS = 6
IMPULSE_MARKER = "impulse_lib.vi_child: first-fiber check done"


def impulse_callback(impulses, prm, d):
    """ctypes form of a numpy impulse model impulses(prm, x[P, d]) -> (k, y), for c3control_add_impulses"""
    import ctypes as C

    FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double))

    def _fn(x, m, y):
        k, yy = impulses(prm, np.array([[x[i] for i in range(d)]]))
        for i in range(d):
            y[i] = yy[0, m, i]
        return float(k[0, m])

    return FN(_fn)


def inv_callbacks(prm):
    import facade_lib as fl

    return fl.callbacks2d(lambda x, u: (u[0] - prm[1], u[1] - prm[1]), lambda x, u: (prm[0], prm[0]),
                          lambda x, u: float(inv_run(prm, np.asarray(x)[None])[0]) + prm[4] * (u[0] * u[0] + u[1] * u[1]),
                          lambda x: float(inv_bcost(prm, np.asarray(x)[None])[0]), lambda x: 0.0, lambda x: 0.0)[0]


def vi_child(out_path, nsweeps=INV_VI_SWEEPS):
    """the inventory problem through the reference API (run in a child process by tests/test_gpu_impulse.py):
    c3control_vi_solve one sweep at a time from V_0 = running cost / beta, the nodal values after every sweep saved.  The first
    sweep runs the first-fiber check of the device source against the host callbacks (a marker line on stderr after it), the
    later ones the device-resident cross"""
    import ctypes as C
    import os
    import sys

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(INV, 2, 2, ranks=(4, 8, 12), name="inventory_api", nimpulse=INV_NIMPULSE, **INV_MASKS)
    w = inv_workload(mid)
    L = fl.solver_lib()
    ctl = fl.Control(w, callbacks=inv_callbacks(INV_PRM), consistent_ends=None)
    cb = impulse_callback(inv_impulses, INV_PRM, 2)
    L.c3control_add_impulses.argtypes = [C.c_void_p, C.c_int, type(cb)]
    L.c3control_add_impulses(ctl.h, INV_NIMPULSE, cb)
    L.c3control_set_impulses.argtypes = [C.c_void_p, C.c_int]
    L.c3control_set_impulses(ctl.h, 1)
    aa = fl.approx_args(L)
    v, keep = fl.init_value(L, ctl, aa, lambda xx: inv_bcost(INV_PRM, xx))
    n0, n1 = w.ngrid
    out = [fl.nodal(L, v.value, n0, n1)]
    for s in range(nsweeps):
        v = C.c_void_p(L.c3control_vi_solve(ctl.h, C.c_size_t(1), C.c_double(0.0), v, aa, ctl.opt, C.c_int(0), None))
        out.append(fl.nodal(L, v.value, n0, n1))
        if s == 0:
            sys.stdout.flush()
            sys.stderr.flush()
            os.write(2, (IMPULSE_MARKER + "\n").encode())
    np.savez(out_path, V=np.array(out))


# ---------------------------------------------------------------------------------------------------- noisy rollouts
INV_SIM_DT, INV_SIM_STEPS = 0.05, 60
INV_X0 = ((0.0, 0.0), (-0.8, -0.4), (0.8, -0.8))  # nodes of the 11 x 11 grid: the policy steers at the first, orders at the others


# the discretisation gap at those states: a CPU run of inv_rollouts with 2^18 paths per state (numpy default_rng(2718), the three
# states in turn, dt = 0.05, 60 steps) under the dense fixed point gives means 2.147075, 3.091685, 2.924426 against
# V = 1.841576, 3.026121, 2.973785: gaps +0.305499, +0.065564, -0.049359 with standard errors 0.000881, 0.000807, 0.000804 and
# 0.98, 1.93, 1.77 interventions per path (the Euler step of the rollouts against a chain whose interpolation interval h^2 / Q
# is about 0.4 on the coarse grid; an intervention also delays the clock by dt).  The bound of the device test at a state is twice
# the gap there
INV_GAP = (0.305499, 0.065564, 0.049359)
INV_ALLOWANCE = tuple(2 * g for g in INV_GAP)


def inv_fixed_point(w=None):
    """the value function of the inventory problem on its 11 x 11 grid: dense_vi from the boundary cost, 200 sweeps (a
    contraction by about 0.8 per sweep: converged to rounding)"""
    w = inv_workload(0) if w is None else w
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    bc = lambda x: inv_bcost(w.params, x)
    V, dec = dense_vi(w, inv_host, inv_impulses, bc, bc(X), 200)
    return V[-1], dec[-1]


def inv_rollouts(w, V, x0, n, dt, nsteps, rng, chunk=1 << 16):
    """the rollout restatement for the inventory problem under the nodal value function V (both dimensions absorbing): n noisy
    paths from the state x0 with numpy's own normals.  A step is the device's: exit test (pay the discounted boundary cost,
    freeze); the controller's backup with interventions on the off-grid stencil of V (neighbours one spacing away, clamped to
    the faces); where it intervenes the path pays the discounted k_m and moves to y_m, with no stage cost and no increment --
    the step slot still takes dt --; otherwise the discounted stage cost times dt and x + b dt + sigma sqrt(dt) xi.  A path
    alive after the last step adds the discounted V(x_N).  Returns (costs [n], interventions per path [n])"""
    prm, beta = w.params, w.discount
    h2, t = BR.mca_constants(w)
    g = w.xgrid()[0]
    h, lb, ub = g[1] - g[0], g[0], g[-1]
    C = np.asarray(w.cands, dtype=np.float64)
    bc = lambda xx: inv_bcost(prm, xx)
    oc = lambda xx: np.zeros(len(xx))
    Vn = JL.Nodal(w, V)
    cl = lambda y: np.clip(y, lb, ub)
    out, cnt = [], []
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        x = np.tile(np.asarray(x0, dtype=np.float64), (m, 1))
        J, alive, niv = np.zeros(m), np.ones(m, dtype=bool), np.zeros(m, dtype=int)
        for s in range(nsteps + 1):
            disc = np.exp(-beta * (s * dt))
            gone = alive & ((x < lb) | (x > ub)).any(axis=1)
            J = J + np.where(gone, disc * bc(x), 0.0)
            alive = alive & ~gone
            if s == nsteps:
                J = J + np.where(alive, disc * Vn.value(cl(x)), 0.0)
                break
            xc = cl(x)  # exited paths are frozen outside: their controller's result is not used
            S = np.stack([Vn.value(cl(xc - [h, 0])), Vn.value(cl(xc + [h, 0])), Vn.value(cl(xc - [0, h])), Vn.value(cl(xc + [0, h])),
                          Vn.value(xc)], axis=-1)
            vals, _, _ = BR.candidate_values(inv_host, prm, xc, S, C, h2, t, beta)
            _, ui, _ = BR.backup(vals, c=impulse_values(w, inv_impulses, Vn, xc, bc, oc))
            iv = alive & (ui > len(C))
            mk = np.where(iv, ui - len(C) - 1, 0)
            k, y = inv_impulses(prm, x)
            ar = np.arange(m)
            J = J + np.where(iv, disc * k[ar, mk], 0.0)
            u = C[np.clip(ui, 0, len(C) - 1)]
            b, sg, st = inv_host(prm, x, u)
            J = J + np.where(alive & ~iv, disc * st * dt, 0.0)
            xn = x + b * dt + sg * np.sqrt(dt) * rng.standard_normal((m, 2))
            xn = np.where(iv[:, None], y[ar, mk], xn)
            x = np.where(alive[:, None], xn, x)
            niv += iv
        out.append(J)
        cnt.append(niv)
    return np.concatenate(out), np.concatenate(cnt)
