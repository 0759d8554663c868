"""Optimal stopping (c3sc_hip_set_stopping): device sources of a stopping LQR and of an American put on the
mean of two assets, the stopping backup of the nodes of fibers, and the dense explicit chain of the put and value iteration of
the LQR on a whole small grid.  Shared by the CPU and GPU tests and tools/stop_bench.py.

The backup is backup_ref's with the stop action psi: it comes after the candidates, wins where it is strictly smaller than the
scan's winner and where the scan left no valid candidate, and its index is ncand.  The margin the stop tests choose their
compared indices by is the stop decision's own (backup_ref.stop_margin), not the margin over every action."""
import dataclasses

import numpy as np

import backup_ref as BR
import horizon_lib as H

STOPCOST_LQR = r"""
__device__ double stopcost(const double *prm, const double *x) { return prm[4] + prm[5] * (x[0] * x[0] + x[1] * x[1]); }
"""
# the decoupled 2-D LQR of horizon_lib with a stopping cost psi = c0 + c1 |x|^2: prm = {sig, q, r, s, c0, c1}
LQR = H.LQR + STOPCOST_LQR
LQR_MASKS = H.LQR_MASKS
LQR_PRM = (0.3, 1.0, 1.0, 2.0, 0.6, 0.5)
LQR_NEVER_PRM = (0.3, 1.0, 1.0, 2.0, 1.0e30, 0.0)  # a psi so large that stop never wins


def lqr_cands():
    u = np.linspace(-1.5, 1.5, 5)
    return np.array([(a, b) for a in u for b in u])


def lqr_psi(prm, x):
    return prm[4] + prm[5] * (x ** 2).sum(-1)


# the same LQR in three dimensions (x_i' = u_i), for a fiber-per-wave launch whose middle core does not fit the CU's LDS:
# prm as LQR_PRM
LQR3 = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = u[0]; b[1] = u[1]; b[2] = u[2]; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[0]; s[1] = prm[0]; s[2] = prm[0]; }
__device__ double stage(const double *prm, const double *x, const double *u)
{
    return prm[1] * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) + prm[2] * (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
}
__device__ double boundcost(const double *prm, const double *x) { return prm[3] * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]); }
__device__ double obscost(const double *prm, const double *x) { return 5.0; }
__device__ double stopcost(const double *prm, const double *x) { return prm[4] + prm[5] * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]); }
"""
LQR3_MASKS = dict(udep_mask=0b111, uconst_mask=0b111, stage_udep=True)


def lqr3_cands():
    u = np.linspace(-1.5, 1.5, 5)
    return np.array([(a, b, c) for a in u for b in u for c in u])


def lqrn_host(prm, x, u):
    """numpy twin of the LQR in any dimension: (drift, sigma, stage) for x[..., D], u[..., D]"""
    b = u + 0.0 * x
    return b, np.full(b.shape, prm[0]), prm[1] * (x ** 2).sum(-1) + prm[2] * (u ** 2).sum(-1)


def lqrn_terminal(prm, x):
    return prm[3] * (x ** 2).sum(-1)


# American put on the mean of two assets: dS_i = r S_i dt + v S_i dW_i, one dummy candidate, no running cost; exercising pays
# psi = -max(K - mean S, 0) (a cost: the payoff with a minus sign), and so do the absorbing faces, the obstacles and the
# terminal time.  prm = {r, v, K}; the discount is beta = r
PUT = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = prm[0] * x[0]; b[1] = prm[0] * x[1]; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[1] * x[0]; s[1] = prm[1] * x[1]; }
__device__ double stage(const double *prm, const double *x, const double *u) { return 0.0; }
__device__ double stopcost(const double *prm, const double *x)
{
    const double p = prm[2] - 0.5 * (x[0] + x[1]);
    return p > 0.0 ? -p : 0.0;
}
__device__ double boundcost(const double *prm, const double *x) { return stopcost(prm, x); }
__device__ double obscost(const double *prm, const double *x) { return stopcost(prm, x); }
"""
PUT_MASKS = dict(udep_mask=0, uconst_mask=0, stage_udep=False)
PUT_R, PUT_V, PUT_K = 0.1, 0.3, 1.0
PUT_PRM = (PUT_R, PUT_V, PUT_K)
PUT_NEVER = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = prm[0] * x[0]; b[1] = prm[0] * x[1]; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[1] * x[0]; s[1] = prm[1] * x[1]; }
__device__ double stage(const double *prm, const double *x, const double *u) { return 0.0; }
__device__ double stopcost(const double *prm, const double *x) { return 1.0e30; }
__device__ double boundcost(const double *prm, const double *x)
{
    const double p = prm[2] - 0.5 * (x[0] + x[1]);
    return p > 0.0 ? -p : 0.0;
}
__device__ double obscost(const double *prm, const double *x) { return boundcost(prm, x); }
"""
PUT_CANDS = np.array([[0.0]])
PUT_LB, PUT_UB = 0.2, 1.8
PUT_N = 11
PUT_DELTA = 0.025      # Q delta / h^2 <= 0.64 * 0.025 / 0.0256 < 1 on the 11 x 11 grid: no CFL bit
PUT_STAGES = 20        # T = 0.5


def put_host(prm, x, u):
    r, v = prm[0], prm[1]
    b = r * x + 0.0 * u[..., :1]
    s = v * x + 0.0 * u[..., :1]
    return b, s, np.zeros(b.shape[:-1])


def put_psi(prm, x):
    return -np.maximum(prm[2] - 0.5 * (x[..., 0] + x[..., 1]), 0.0)


def put_workload(mid, rank=11, n=PUT_N, discount=PUT_R):
    from c3sc_amd import workloads as wl

    return wl.Workload("put", mid, PUT_PRM, 2, 1, (PUT_LB, PUT_LB), (PUT_UB, PUT_UB), (n, n), wl.uniform_ranks(2, rank), discount,
                       (wl.BC_ABSORB, wl.BC_ABSORB), [], PUT_CANDS)


# ---------------------------------------------------------------------------------------------------- one node
def stop_backup(vals, psi, forced=None):
    """backup_ref.backup with the stop action psi [P], and the stop decision's own margin in place of the one over every action
    (inf on the forced path)"""
    out, ui, mg = BR.backup(vals, psi, forced=forced)
    return out, ui, mg if forced is not None else BR.stop_margin(vals, psi)


def stop_fibers(w, host, psi_fn, k, idx, costs, absorbed, bcost, ocost, delta=None, forced=None):
    """the stopping backup of every node of fibers idx from their stencils (costs [F, N, 2D+1], absorbed [F, N]); psi_fn, bcost,
    ocost: callables of x[P, D]; delta: the horizon step (None: infinite horizon).  Returns (value, index, margin, stationary,
    cfl) of shape [F, N]; the flags are the scanned candidates' alone (of the forced candidate on the forced path)"""
    x = BR.node_states(w, k, idx).reshape(-1, w.dx)
    return BR.fibers(w, host, k, idx, costs, absorbed, bcost, ocost, delta=delta, forced=forced,
                     decide=lambda vals: stop_backup(vals, psi_fn(x), forced))


# ---------------------------------------------------------------------------------------------------- the put on a whole grid
def dense_chain(w, host, psi_fn, delta, nstages, stopping=True):
    """the explicit chain of a 2-D workload whose dimensions both absorb, with the stop action (stopping=False: without, the
    European value): V[s] for s = 0 .. nstages with V[nstages] = psi at every node, the boundary nodes keep psi;
    returns (V [nstages + 1, n0, n1], stop [nstages, n0, n1] -- the decision of stage s at the interior nodes, cfl seen)"""
    psi = psi_fn(BR.grid2(w)[0])
    V, ui, _, anycfl, _ = BR.sweeps(w, host, psi, psi, nstages, psi=psi if stopping else None, delta=delta)
    return V[::-1].copy(), ui[::-1] == w.ncand, anycfl


# the states the noisy rollouts start from (nodes of the 11 x 11 grid) and the discretisation bound of the dense chain there:
# |V_0 on 11 x 11 at PUT_DELTA - V_0 on 21 x 21 at PUT_DELTA / 4| at those states is 0.00069, 0.00035, 0.00079
# (tests/test_stop_host.py measures it and holds it under PUT_DISC); times two -- one factor for the rollouts' Euler step, one
# for the interpolation of V between the nodes
PUT_X0 = [(1.0, 1.0), (0.84, 1.0), (1.16, 1.0)]
PUT_DISC = 0.0008
PUT_BOUND = 2 * PUT_DISC


# ---------------------------------------------------------------------------------------------------- the reference API
LQR_VI_BETA = 0.5
LQR_VI_SWEEPS = 6


def lqr_vi_workload(mid, rank=11):
    return dataclasses.replace(H.lqr_workload(mid, rank=rank, discount=LQR_VI_BETA), params=LQR_PRM, cands=lqr_cands())


def dense_vi(w, host, psi_fn, bcost, V0, nsweeps):
    """value iteration sweeps of the stopping operator on the whole grid of a 2-D workload whose dimensions both absorb (the
    boundary nodes keep their boundary cost): [V_0, V_1, .. V_nsweeps] and the decisions of the last sweep"""
    x, ab, _ = BR.grid2(w)
    V, ui, _, _, _ = BR.sweeps(w, host, np.where(ab, bcost(x), V0.reshape(-1)), bcost(x), nsweeps, psi=psi_fn(x))
    return V, ui[-1]


def lqr_callbacks(prm=LQR_PRM):
    import facade_lib as fl

    sig, q, r, s = prm[:4]
    return fl.callbacks2d(lambda x, u: (u[0], u[1]), lambda x, u: (sig, sig),
                          lambda x, u: q * (x[0] * x[0] + x[1] * x[1]) + r * (u[0] * u[0] + u[1] * u[1]),
                          lambda x: s * (x[0] * x[0] + x[1] * x[1]), lambda x: 5.0, lambda x: float(lqr_psi(prm, x)))


def put_callbacks(prm=PUT_PRM):
    import facade_lib as fl

    r, v = prm[0], prm[1]
    psi = lambda x: float(put_psi(prm, x))
    return fl.callbacks2d(lambda x, u: (r * x[0], r * x[1]), lambda x, u: (v * x[0], v * x[1]), lambda x, u: 0.0, psi, psi, psi)


def vi_child(out_path, nsweeps=LQR_VI_SWEEPS):
    """the stopping LQR through the reference API (run in a child process by tests/test_gpu_stop.py): c3control_vi_solve one
    sweep at a time from V_0 = s |x|^2, the nodal values after every sweep saved"""
    import ctypes as C

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(LQR, 2, 2, ranks=(4, 8, 12), name="lqr_os_api", stop=True, **LQR_MASKS)
    w = lqr_vi_workload(mid)
    cbs, stop_cb = lqr_callbacks()
    L, ctl, aa = fl.stop_control(w, cbs, stop_cb)
    v, keep = fl.init_value(L, ctl, aa, lambda xx: H.lqr_terminal(LQR_PRM, xx))
    n0, n1 = w.ngrid
    out = [fl.nodal(L, v.value, n0, n1)]
    for _ in range(nsweeps):
        v = C.c_void_p(L.c3control_vi_solve(ctl.h, C.c_size_t(1), C.c_double(0.0), v, aa, ctl.opt, C.c_int(0), None))
        out.append(fl.nodal(L, v.value, n0, n1))
    np.savez(out_path, V=np.array(out))


def fh_child(out_path, delta=PUT_DELTA, nstages=PUT_STAGES):
    """the American put through the reference API (run in a child process): c3control_fh_solve in stop mode from the terminal
    value psi, V_s at every node of every stage saved"""
    import ctypes as C

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(PUT, 2, 1, ranks=(4, 8, 12), name="put_os_api", horizon=True, stop=True, **PUT_MASKS)
    w = put_workload(mid, rank=11)
    cbs, stop_cb = put_callbacks()
    L, ctl, aa = fl.stop_control(w, cbs, stop_cb)
    vt, keep = fl.init_value(L, ctl, aa, lambda xx: put_psi(PUT_PRM, xx))
    V = L.c3control_fh_solve(ctl.h, C.c_size_t(nstages), C.c_double(delta), vt, aa, ctl.opt, C.c_int(0))
    fl.save_stages(out_path, L, V, nstages, *w.ngrid)
