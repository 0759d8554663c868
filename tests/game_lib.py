"""Zero-sum games (c3sc_hip_set_game): device sources of two game models and the game backup of one node, shared
by the CPU and GPU tests and tools/game_bench.py.

The values of the pairs are backup_ref.candidate_values over the candidate list product(U, W); then the min-max over the
(nu, nw) matrix of values: first strict '<' / '>' in both reductions, skipped candidates and emptied groups out."""
import numpy as np

import backup_ref as BR

# 2-D linear-quadratic game: x0' = x1, x1' = u + w; stage x'x + r u^2 - g2 w^2.  prm = {sig0, sig1, r, g2}
LQGAME = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = x[1]; b[1] = u[0] + u[1]; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[0]; s[1] = prm[1]; }
__device__ double stage(const double *prm, const double *x, const double *u)
{
    return x[0] * x[0] + x[1] * x[1] + prm[2] * u[0] * u[0] - prm[3] * u[1] * u[1];
}
__device__ double boundcost(const double *prm, const double *x) { return 100.0; }
__device__ double obscost(const double *prm, const double *x) { return 0.0; }
"""
LQGAME_MASKS = dict(udep_mask=1 << 1, uconst_mask=1 << 1, stage_udep=True)
LQGAME_PRM = (0.5, 0.5, 1.0, 4.0)


def lqgame_host(prm, x, u):
    """numpy twin of LQGAME: (drift[..., 2], sigma[..., 2], stage[...]) for x[..., 2], u[..., 2]"""
    s0, s1, r, g2 = prm[:4]
    b = np.stack([x[..., 1], u[..., 0] + u[..., 1]], axis=-1)
    s = np.broadcast_to(np.array([s0, s1]), b.shape).copy()
    st = x[..., 0] ** 2 + x[..., 1] ** 2 + r * u[..., 0] ** 2 - g2 * u[..., 1] ** 2
    return b, s, st


# two cars in the pursuer's frame (examples/pursuit_game.c): state (x, y, theta), pursuer turn rate u, evader turn rate w.
# prm = {v_e, v_p, om_p, om_e, sig}; stage 1 (time to capture), capture box = obstacle of cost 0, escape penalty 20
PURSUIT = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b)
{
    b[0] = prm[0] * cos(x[2]) - prm[1] + prm[2] * u[0] * x[1];
    b[1] = prm[0] * sin(x[2]) - prm[2] * u[0] * x[0];
    b[2] = prm[3] * u[1] - prm[2] * u[0];
}
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[4]; s[1] = prm[4]; s[2] = prm[4]; }
__device__ double stage(const double *prm, const double *x, const double *u) { return 1.0; }
__device__ double boundcost(const double *prm, const double *x) { return 20.0; }
__device__ double obscost(const double *prm, const double *x) { return 0.0; }
"""
PURSUIT_MASKS = dict(udep_mask=0b111, uconst_mask=0b100, stage_udep=False)
PURSUIT_PRM = (0.6, 1.0, 1.0, 1.0, 0.05)


def pursuit_host(prm, x, u):
    ve, vp, op, oe, sg = prm[:5]
    b = np.stack([ve * np.cos(x[..., 2]) - vp + op * u[..., 0] * x[..., 1],
                  ve * np.sin(x[..., 2]) - op * u[..., 0] * x[..., 0],
                  oe * u[..., 1] - op * u[..., 0]], axis=-1)
    s = np.full(b.shape, sg)
    return b, s, np.ones(b.shape[:-1])


def product(U, W):
    """pair list (nu * nw, du_min + du_max) in pair order iu * nw + iw"""
    U, W = np.atleast_2d(U), np.atleast_2d(W)
    return np.concatenate([np.repeat(U, len(W), axis=0), np.tile(W, (len(U), 1))], axis=1)


def candidate_values(host, prm, x, V, U, W, h2, t, beta):
    """values [P, nu, nw] of every pair at P nodes x[P, D] with stencils V[P, 2D+1]; NaN = skipped (Q < 1e-14); and the
    per-node stationary flag"""
    vals, stat, _ = BR.candidate_values(host, prm, x, V, product(U, W), h2, t, beta)
    return vals.reshape(-1, len(np.atleast_2d(U)), len(np.atleast_2d(W))), stat


def minmax(vals, order="minmax"):
    """(value, pair index, margin) per node of vals[P, nu, nw] (NaN = skipped).  margin: the smaller relative gap between the
    winner and the runner-up of the inner reduction in the winning group and of the outer reduction (inf if unique)"""
    P, nu, nw = vals.shape
    a = vals if order == "minmax" else np.swapaxes(vals, 1, 2)  # [P, groups, members]
    imax = order == "minmax"
    out, idx, margin = np.zeros(P), np.full(P, -1), np.full(P, np.inf)
    for p in range(P):
        gv, gi = [], []
        for g in range(a.shape[1]):
            row = a[p, g]
            ok = ~np.isnan(row)
            if not ok.any():
                continue
            j = int(np.nanargmax(row) if imax else np.nanargmin(row))  # first occurrence of the extreme
            gv.append(row[j])
            gi.append((g, j, np.sort(row[ok])))
        if not gv:
            continue
        gv = np.array(gv)
        q = int(np.argmin(gv) if imax else np.argmax(gv))
        g, j, srt = gi[q]
        out[p] = gv[q]
        iu, iw = (g, j) if order == "minmax" else (j, g)
        idx[p] = iu * nw + iw
        sc = max(1.0, abs(gv[q]))
        if len(srt) > 1:
            margin[p] = min(margin[p], (srt[-1] - srt[-2] if imax else srt[1] - srt[0]) / sc)
        if len(gv) > 1:
            sg = np.sort(gv)
            margin[p] = min(margin[p], (sg[1] - sg[0] if imax else sg[-1] - sg[-2]) / sc)
    return out, idx, margin


def game_backup(w, host, k, idx, costs, absorbed, U, W, order, bcost, ocost):
    """the game backup of every node of fibers idx from their stencils (costs [F, N, 2D+1], absorbed [F, N]); bcost, ocost: the
    constant boundary and obstacle costs.  Returns (value, pair index, margin, stationary) of shape [F, N]"""
    nu, nw = len(np.atleast_2d(U)), len(np.atleast_2d(W))
    return BR.fibers(w, host, k, idx, costs, absorbed, lambda x: bcost, lambda x: ocost, cands=product(U, W),
                     decide=lambda vals: minmax(vals.reshape(-1, nu, nw), order))[:4]


# ---------------------------------------------------------------------------------------------------- the reference API
def lq_callbacks(prm=LQGAME_PRM):
    """the host callbacks of LQGAME (what a C program passes to c3control_add_*), as ctypes function pointers"""
    import facade_lib as fl

    s0, s1, r, g2 = prm[:4]

    def drift(t, x, u, out, jac, args):
        out[0], out[1] = x[1], u[0] + u[1]
        return 0

    def diff(t, x, u, out, grad, args):
        out[0], out[1], out[2], out[3] = s0, 0.0, 0.0, s1
        return 0

    def stage(t, x, u, out, grad):
        out[0] = x[0] * x[0] + x[1] * x[1] + r * u[0] * u[0] - g2 * u[1] * u[1]
        return 0

    def bcost(t, x, out):
        out[0] = 100.0
        return 0

    def ocost(x, out):
        out[0] = 0.0
        return 0

    return (fl.DYN_FN(drift), fl.DYN_FN(diff), fl.STAGE_FN(stage), fl.BOUND_FN(bcost), fl.OBS_FN(ocost))


def lq_vi_workload(mid, n=11, rank=11, discount=0.1):
    from c3sc_amd import workloads as wl

    U, W = np.linspace(-1.0, 1.0, 9).reshape(-1, 1), np.linspace(-0.5, 0.5, 5).reshape(-1, 1)
    return wl.Workload("lqgame", mid, LQGAME_PRM, 2, 2, (-2.0, -2.0), (2.0, 2.0), (n, n), wl.uniform_ranks(2, rank), discount,
                       (wl.BC_ABSORB, wl.BC_REFLECT), [], product(U, W)), U, W


def dense_sweep(w, V, U, W, order, bcost=100.0):
    """one sweep of the game's Markov chain on the whole grid of a 2-D workload with dim 0 absorbing and dim 1 reflecting
    (the library's neighbour rules, nodeutil.c:513-624 with consistent ends): V[n0, n1] -> (T V, saddle pair index, margin)"""
    nu, nw = len(np.atleast_2d(U)), len(np.atleast_2d(W))
    out, ui, mg, _, _ = BR.sweeps(w, lqgame_host, V, bcost, 1, cands=product(U, W),
                                  decide=lambda vals: minmax(vals.reshape(-1, nu, nw), order))
    return out[1], ui[0], mg[0]


def vi_child(order, sweeps, out_path):
    """value iteration of the LQ game through the reference API (run in a child process by tests/test_gpu_game.py): a run-time
    compiled game model beside the host callbacks, a game c3Opt, c3control_vi_solve one sweep at a time; saves the value at
    every node after every sweep and the host c3control_policy_eval at every node of the last value function"""
    import ctypes as C

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(LQGAME, 2, 2, ranks=(12,), name="lqgame_vi", game=True, **LQGAME_MASKS)
    w, U, W = lq_vi_workload(mid)
    L = fl.solver_lib()
    ctl = fl.Control(w, callbacks=lq_callbacks(), consistent_ends=None)
    u, ww = fl.f64(U), fl.f64(W)
    L.c3opt_set_brute_force_game(ctl.opt, C.c_size_t(1), C.c_size_t(len(u)), fl.dp(u), C.c_size_t(len(ww)), fl.dp(ww),
                                 C.c_int(GAME_ORDERS[order]))
    aa = fl.approx_args(L)
    cur, keep = fl.init_value(L, ctl, aa, lambda xx: 1.0 + 0.3 * xx[:, 0] ** 2 + 0.2 * xx[:, 0] * xx[:, 1] + 0.1 * np.sin(xx[:, 1]))
    n0, n1 = w.ngrid
    nodes = lambda vf: fl.nodal(L, vf.value, n0, n1)
    hist = [nodes(cur)]
    for _ in range(sweeps):
        nxt = C.c_void_p(L.c3control_vi_solve(ctl.h, C.c_size_t(1), C.c_double(0.0), cur, aa, ctl.opt, C.c_int(0), None))
        cur = nxt
        hist.append(nodes(cur))
    # the host twin: c3control_policy_eval (bellman_optimal over the callbacks) at every node of the last value function
    L.c3control_add_policy_sim(ctl.h, cur, ctl.opt, None)
    xg = w.xgrid()
    pol = np.zeros((n0, n1, 2))
    for a in range(n0):
        for b in range(n1):
            uu = np.zeros(2)
            assert L.c3control_policy_eval(ctl.h, C.c_double(0.0), fl.dp(fl.f64([xg[0][a], xg[1][b]])), fl.dp(uu)) == 0
            pol[a, b] = uu
    np.savez(out_path, V=np.array(hist), pol=pol)


GAME_ORDERS = {"minmax": 0, "maxmin": 1}
