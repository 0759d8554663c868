"""Optimal stopping (c3sc_hip_set_stopping): device sources of a stopping LQR and of an American put on the
mean of two assets, a numpy restatement of the stopping backup of one node, and the dense explicit chain of the put on a whole
small grid.  Shared by the CPU and GPU tests and tools/stop_bench.py.

The restatement is built on horizon_lib.candidate_values / horizon_lib.backup for the horizon form and on the plain
per-candidate formulas (as game_lib restates them) for the infinite-horizon form: upwind rates with the +-1e-14 dead zone,
Q = sum of the rates, a candidate with Q < 1e-14 skipped, dt = h2 / Q, value = dt stage + exp(-beta dt) (PV / Q + (1 - Q / Q)
V_node).  The stop action comes last: psi wins where it is strictly smaller than the scan's winner and where the scan left no
valid candidate; its index is ncand."""
import dataclasses

import numpy as np

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
def plain_candidate_values(host, prm, x, V, C, h2, t, beta):
    """infinite-horizon values [P, nc] of every candidate (NaN = skipped, Q < 1e-14) and the per-node stationary flag"""
    D = x.shape[1]
    xx = np.broadcast_to(x[:, None, :], (x.shape[0], len(C), D))
    uu = np.broadcast_to(C[None], (x.shape[0],) + C.shape)
    b, s, st = host(prm, xx, uu)
    Q = np.zeros(b.shape[:-1])
    PV = np.zeros(b.shape[:-1])
    for m in range(D):
        half = t[2 * m + 1] * (s[..., m] * s[..., m]) / 2.0
        tb = t[2 * m] * b[..., m]
        pm = np.where(b[..., m] < -1e-14, half - tb, half)
        pp = np.where(b[..., m] > 1e-14, half + tb, half)
        Q += pm + pp
        PV += pm * V[:, None, 2 * m] + pp * V[:, None, 2 * m + 1]
    bad = Q < 1e-14
    Qs = np.where(bad, 1.0, Q)
    dt = h2 / Qs
    val = dt * st + np.exp(-beta * dt) * (PV / Qs + (1.0 - Qs / Qs) * V[:, None, 2 * D])
    return np.where(bad, np.nan, val), bad.any(axis=1)


def stop_backup(vals, psi, forced=None):
    """(value, index, margin) per node: the scan over vals[P, nc] (NaN = skipped; the first strict minimum of the others), then
    the stop action psi[P] with the index nc -- it wins where strictly smaller and where no candidate was valid.  forced: nc
    yields psi, another index applies that candidate without the comparison (0 and -1 if it is skipped or out of range).
    margin: |psi - continuation| relative to max(1, |continuation|), inf where there is no continuation value"""
    P, nc = vals.shape
    if forced is not None:
        fi = np.asarray(forced).reshape(-1)
        inr = (fi >= 0) & (fi < nc)
        v = vals[np.arange(P), np.clip(fi, 0, nc - 1)]
        ok = inr & ~np.isnan(v)
        out = np.where(fi == nc, psi, np.where(ok, v, 0.0))
        return out, np.where(fi == nc, nc, np.where(ok, fi, -1)), np.full(P, np.inf)
    any_ok = ~np.isnan(vals).all(axis=1)
    filled = np.where(np.isnan(vals), np.inf, vals)
    ci = np.argmin(filled, axis=1)  # the first of equal minima
    cont = filled[np.arange(P), ci]
    stop = ~any_ok | (psi < cont)
    out = np.where(stop, psi, cont)
    ui = np.where(stop, nc, ci)
    margin = np.where(any_ok, np.abs(psi - cont) / np.maximum(1.0, np.abs(np.where(any_ok, cont, 0.0))), np.inf)
    return out, ui, margin


def loop_backup(host, prm, x, V, C, h2, t, beta, psi, delta=None):
    """the same decision by a per-candidate Python loop over one node at a time (the check of the vectorised restatement):
    (value, index) per node; delta: the horizon step (None: the infinite-horizon form)"""
    P, D = x.shape
    out, idx = np.zeros(P), np.full(P, -1)
    for p in range(P):
        best, bi = 0.0, -1
        for c in range(len(C)):
            b, s, st = host(prm, x[p], C[c])
            Q = PV = 0.0
            for m in range(D):
                half = t[2 * m + 1] * (s[m] * s[m]) / 2.0
                tb = t[2 * m] * b[m]
                pm = half - tb if b[m] < -1e-14 else half
                pp = half + tb if b[m] > 1e-14 else half
                Q += pm + pp
                PV += pm * V[p, 2 * m] + pp * V[p, 2 * m + 1]
            if delta is None:
                if Q < 1e-14:
                    continue
                dt = h2 / Q
                val = dt * st + np.exp(-beta * dt) * (PV / Q + (1.0 - Q / Q) * V[p, 2 * D])
            else:
                val = st * delta + np.exp(-beta * delta) * (V[p, 2 * D] + (delta / h2) * (PV - Q * V[p, 2 * D]))
            if bi < 0 or val < best:
                best, bi = val, c
        if bi < 0 or psi[p] < best:
            best, bi = psi[p], len(C)
        out[p], idx[p] = best, bi
    return out, idx


def node_values(host, prm, x, V, C, h2, t, beta, delta=None):
    """per-candidate values (NaN = skipped), stationary flag and CFL flags [P, nc] of either form"""
    if delta is None:
        vals, stat = plain_candidate_values(host, prm, x, V, C, h2, t, beta)
        return vals, stat, np.zeros(vals.shape, dtype=bool)
    vals, cfl = H.candidate_values(host, prm, x, V, C, h2, t, beta, delta)
    return vals, np.zeros(len(x), dtype=bool), cfl


def stop_fibers(w, host, psi_fn, k, idx, costs, absorbed, bcost, ocost, delta=None, forced=None):
    """the stopping backup of every node of fibers idx from their stencils (costs [F, N, 2D+1], absorbed [F, N]); psi_fn, bcost,
    ocost: callables of x[P, D]; delta: the horizon step (None: infinite horizon).  Returns (value, index, margin, stationary,
    cfl) of shape [F, N]; the flags are the scanned candidates' alone (of the forced candidate on the forced path)"""
    h2, t = H.mca_constants(w)
    x = H.node_states(w, k, idx).reshape(-1, w.dx)
    V = costs.reshape(-1, 2 * w.dx + 1)
    C = np.asarray(w.cands, dtype=np.float64)
    vals, stat, cfl = node_values(host, w.params, x, V, C, h2, t, w.discount, delta)
    out, ui, mg = stop_backup(vals, psi_fn(x), forced)
    if forced is not None:
        fi = np.asarray(forced).reshape(-1)
        cfl = cfl[np.arange(len(fi)), np.clip(fi, 0, len(C) - 1)] & (fi >= 0) & (fi < len(C))
    else:
        cfl = cfl.any(axis=1)
    ab = absorbed.reshape(-1)
    out = np.where(ab == 1, bcost(x), np.where(ab == -1, ocost(x), out))
    ui = np.where(ab != 0, -1, ui)
    sh = absorbed.shape
    return out.reshape(sh), ui.reshape(sh), mg.reshape(sh), (stat & (ab == 0)).reshape(sh), (cfl & (ab == 0)).reshape(sh)


# ---------------------------------------------------------------------------------------------------- the put on a whole grid
def dense_chain(w, host, psi_fn, delta, nstages, stopping=True):
    """the explicit chain of a 2-D workload whose dimensions both absorb, with the stop action (stopping=False: without, the
    European value): V[s] for s = 0 .. nstages with V[nstages] = psi at every node, the boundary nodes keep psi;
    returns (V [nstages + 1, n0, n1], stop [nstages, n0, n1] -- the decision of stage s at the interior nodes, cfl seen)"""
    n0, n1 = w.ngrid
    xg = w.xgrid()
    i0, i1 = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
    x = np.stack([xg[0][i0], xg[1][i1]], axis=-1).reshape(-1, 2)
    ab = ((i0 == 0) | (i0 == n0 - 1) | (i1 == 0) | (i1 == n1 - 1)).reshape(-1)
    h2, t = H.mca_constants(w)
    C = np.asarray(w.cands, dtype=np.float64)
    psi = psi_fn(x)
    Vn = psi.reshape(n0, n1)
    out, dec = [Vn], []
    anycfl = False
    lo0, hi0 = np.clip(i0 - 1, 0, n0 - 1), np.clip(i0 + 1, 0, n0 - 1)
    lo1, hi1 = np.clip(i1 - 1, 0, n1 - 1), np.clip(i1 + 1, 0, n1 - 1)
    for _ in range(nstages):
        S = np.stack([Vn[lo0, i1], Vn[hi0, i1], Vn[i0, lo1], Vn[i0, hi1], Vn], axis=-1).reshape(-1, 5)
        vals, cfl = H.candidate_values(host, w.params, x, S, C, h2, t, w.discount, delta)
        if stopping:
            v, ui, _ = stop_backup(vals, psi)
        else:
            v, ui, _ = H.backup(vals)
        anycfl |= bool((cfl.any(axis=1) & ~ab).any())
        Vn = np.where(ab, psi, v).reshape(n0, n1)
        out.append(Vn)
        dec.append(((ui == len(C)) & ~ab).reshape(n0, n1))
    return np.array(out[::-1]), np.array(dec[::-1]), anycfl


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
    n0, n1 = w.ngrid
    xg = w.xgrid()
    i0, i1 = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
    x = np.stack([xg[0][i0], xg[1][i1]], axis=-1).reshape(-1, 2)
    ab = ((i0 == 0) | (i0 == n0 - 1) | (i1 == 0) | (i1 == n1 - 1)).reshape(-1)
    h2, t = H.mca_constants(w)
    C = np.asarray(w.cands, dtype=np.float64)
    psi = psi_fn(x)
    Vn = np.where(ab, bcost(x), V0.reshape(-1)).reshape(n0, n1)
    out = [Vn]
    lo0, hi0 = np.clip(i0 - 1, 0, n0 - 1), np.clip(i0 + 1, 0, n0 - 1)
    lo1, hi1 = np.clip(i1 - 1, 0, n1 - 1), np.clip(i1 + 1, 0, n1 - 1)
    ui = None
    for _ in range(nsweeps):
        S = np.stack([Vn[lo0, i1], Vn[hi0, i1], Vn[i0, lo1], Vn[i0, hi1], Vn], axis=-1).reshape(-1, 5)
        vals, _ = plain_candidate_values(host, w.params, x, S, C, h2, t, w.discount)
        v, ui, _ = stop_backup(vals, psi)
        Vn = np.where(ab, bcost(x), v).reshape(n0, n1)
        out.append(Vn)
    return np.array(out), np.where(ab, -1, ui).reshape(n0, n1)


def _callbacks(drift_fn, diag_fn, stage_fn, psi_like_b, psi_like_o, psi_fn):
    """ctypes callbacks (drift, diff, stage, boundcost, obscost) and the stopping cost, from functions of numpy (x[2], u)"""
    import facade_lib as fl

    def _x(p):
        return np.array([p[0], p[1]])

    def drift(t, x, u, out, jac, args):
        out[0], out[1] = drift_fn(_x(x), u)
        return 0

    def diff(t, x, u, out, grad, args):
        s = diag_fn(_x(x), u)
        out[0], out[1], out[2], out[3] = s[0], 0.0, 0.0, s[1]
        return 0

    def stage(t, x, u, out, grad):
        out[0] = stage_fn(_x(x), u)
        return 0

    def bcost(t, x, out):
        out[0] = psi_like_b(_x(x))
        return 0

    def ocost(x, out):
        out[0] = psi_like_o(_x(x))
        return 0

    def stop(t, x, out):
        out[0] = psi_fn(_x(x))
        return 0

    return (fl.DYN_FN(drift), fl.DYN_FN(diff), fl.STAGE_FN(stage), fl.BOUND_FN(bcost), fl.OBS_FN(ocost)), fl.BOUND_FN(stop)


def lqr_callbacks(prm=LQR_PRM):
    sig, q, r, s = prm[:4]
    return _callbacks(lambda x, u: (u[0], u[1]), lambda x, u: (sig, sig),
                      lambda x, u: q * (x[0] * x[0] + x[1] * x[1]) + r * (u[0] * u[0] + u[1] * u[1]),
                      lambda x: s * (x[0] * x[0] + x[1] * x[1]), lambda x: 5.0, lambda x: float(lqr_psi(prm, x)))


def put_callbacks(prm=PUT_PRM):
    r, v = prm[0], prm[1]
    psi = lambda x: float(put_psi(prm, x))
    return _callbacks(lambda x, u: (r * x[0], r * x[1]), lambda x, u: (v * x[0], v * x[1]), lambda x, u: 0.0, psi, psi, psi)


def _api_setup(w, callbacks, stop_cb, rank=11):
    """a C3Control in stop mode over workload w with its host callbacks, and rank-`rank` interpolation arguments"""
    import ctypes as C

    import facade_lib as fl

    L = fl.lib()
    for n in ("c3control_init_value", "c3control_vi_solve"):
        getattr(L, n).restype = C.c_void_p
    L.c3control_fh_solve.restype = C.POINTER(C.c_void_p)
    L.valuef_eval_ind.restype = C.c_double
    ctl = fl.Control(w, callbacks=callbacks, consistent_ends=None)
    L.c3control_add_stopcost(ctl.h, stop_cb)
    L.c3control_set_stopping.argtypes = [C.c_void_p, C.c_int]
    L.c3control_set_stopping(ctl.h, 1)
    aa = C.c_void_p(L.approx_args_init())
    L.approx_args_set_cross_tol(aa, C.c_double(1e-12))
    L.approx_args_set_round_tol(aa, C.c_double(1e-15))
    L.approx_args_set_kickrank(aa, C.c_size_t(0))
    L.approx_args_set_adapt(aa, C.c_int(0))
    L.approx_args_set_startrank(aa, C.c_size_t(rank))
    L.approx_args_set_maxrank(aa, C.c_size_t(rank))
    return L, ctl, aa


def _nodal(L, vf, n0, n1):
    import ctypes as C

    import facade_lib as fl

    out = np.empty((n0, n1))
    ind = np.zeros(2, dtype=np.uintp)
    for a in range(n0):
        for b in range(n1):
            ind[:] = (a, b)
            out[a, b] = L.valuef_eval_ind(C.c_void_p(vf), fl.sp(ind))
    return out


def _init_value(L, ctl, aa, fn):
    import ctypes as C

    import facade_lib as fl

    def _term(n, x, out, a):
        xx = np.ctypeslib.as_array(x, shape=(n, 2))
        np.ctypeslib.as_array(out, shape=(n,))[:] = fn(xx)
        return 0

    term = fl.FIBER_FN(_term)
    return C.c_void_p(L.c3control_init_value(ctl.h, term, None, aa, 0)), term


def vi_child(out_path, nsweeps=LQR_VI_SWEEPS):
    """the stopping LQR through the reference API (run in a child process by tests/test_gpu_stop.py): c3control_vi_solve one
    sweep at a time from V_0 = s |x|^2, the nodal values after every sweep saved"""
    import ctypes as C

    from c3sc_amd import engine as E

    mid = E.compile_model(LQR, 2, 2, ranks=(4, 8, 12), name="lqr_os_api", stop=True, **LQR_MASKS)
    w = lqr_vi_workload(mid)
    cbs, stop_cb = lqr_callbacks()
    L, ctl, aa = _api_setup(w, cbs, stop_cb)
    v, keep = _init_value(L, ctl, aa, lambda xx: H.lqr_terminal(LQR_PRM, xx))
    n0, n1 = w.ngrid
    out = [_nodal(L, v.value, n0, n1)]
    for _ in range(nsweeps):
        v = C.c_void_p(L.c3control_vi_solve(ctl.h, C.c_size_t(1), C.c_double(0.0), v, aa, ctl.opt, C.c_int(0), None))
        out.append(_nodal(L, v.value, n0, n1))
    np.savez(out_path, V=np.array(out))


def fh_child(out_path, delta=PUT_DELTA, nstages=PUT_STAGES):
    """the American put through the reference API (run in a child process): c3control_fh_solve in stop mode from the terminal
    value psi, V_s at every node of every stage saved"""
    import ctypes as C

    from c3sc_amd import engine as E

    mid = E.compile_model(PUT, 2, 1, ranks=(4, 8, 12), name="put_os_api", horizon=True, stop=True, **PUT_MASKS)
    w = put_workload(mid, rank=11)
    cbs, stop_cb = put_callbacks()
    L, ctl, aa = _api_setup(w, cbs, stop_cb)
    vt, keep = _init_value(L, ctl, aa, lambda xx: put_psi(PUT_PRM, xx))
    V = L.c3control_fh_solve(ctl.h, C.c_size_t(nstages), C.c_double(delta), vt, aa, ctl.opt, C.c_int(0))
    n0, n1 = w.ngrid
    if not V:
        np.savez(out_path, V=np.zeros(0))
        return
    np.savez(out_path, V=np.array([_nodal(L, V[s], n0, n1) for s in range(nstages + 1)]))
