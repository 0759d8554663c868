"""Correlated noise (c3sc_hip_set_correlation): device sources of a correlated LQR in two dimensions (one pair)
and three (pairs (0,1) and (1,2) of opposite sign), of a known-answer model and of an American put under Heston, and a numpy
restatement of the backup with the cross-diffusion terms on the full value array; the dense explicit chain of the Heston put and
dense value iteration of the correlated LQR on a whole small grid, and the child processes that drive the reference API.  Shared
by the CPU and GPU tests and tools/corr_bench.py.  It shares no code with the kernels.

The chain is Kushner and Dupuis, section 5.3.  Pair p = (i, j) with a_p(x) = (sigma sigma^T)_{ij}(x) sends the un-normalised
rate r_p = (h2 / (h_i h_j)) |a_p| / 2 to each of two diagonal neighbours -- (+,+) and (-,-) where a_p > 0, (+,-) and (-,+) where
a_p < 0 -- and takes the same r_p off each of the four axis rates of i and j.  Everything is linear in the rates, so Q and PV of
every candidate gain
    cq = sum_p (-2 r_p),   cpv = sum_p r_p [(V_d1 + V_d2) - (V[2i] + V[2i+1] + V[2j] + V[2j+1])]
and everything downstream is the backup without the term (backup_ref states it; the two numbers go into its q0 and pv0).  A diagonal neighbour is a grid node and pays the value array's entry there.  Its index in
each of the two dimensions, stated here on its own (neighbour_indices): one node down / up in the interior; at a reflecting end
the node itself on the outer side; across the periodic seam (node 0 and node n - 1 are one point) n - 2 below and 1 above; on an
absorbing face the node itself on both sides.  The axis probabilities of dimension m stay non-negative iff
(h2 / h_m^2) sigma_m^2 / 2 >= sum_{p with m} r_p (the dominance condition), sigma at the first candidate."""
import dataclasses

import numpy as np

import backup_ref as BR
import horizon_lib as H
import jump_lib as JL
import stop_lib as SL

CORR_MAX = 8
STATUS_DOMINANCE = 4

# ---------------------------------------------------------------------------------------------------- the 2-D correlated LQR
# stop_lib's decoupled LQR with one pair (0, 1): a(x) = amp sig^2 sin(1.7 x0 - 2.3 x1 + 0.4), both signs on every grid used.
# prm = {sig, q, r, s, c0, c1, amp}.  On the ragged 21 x 70 grid h0 / h1 = 3.45: dominance holds iff |amp sin| <= 0.29
LQR_COVAR = r"""
__device__ double covar(const double *prm, const double *x, int p) { return prm[6] * prm[0] * prm[0] * sin(1.7 * x[0] - 2.3 * x[1] + 0.4); }
"""
LQR = SL.LQR + LQR_COVAR
LQR_MASKS = SL.LQR_MASKS
LQR_PAIRS = ((0, 1),)
LQR_AMP, LQR_DOM_AMP = 0.25, 0.8
LQR_PRM = SL.LQR_PRM + (LQR_AMP,)
LQR_ZERO_PRM = SL.LQR_PRM + (0.0,)
LQR_DOM_PRM = SL.LQR_PRM + (LQR_DOM_AMP,)  # violates dominance where |sin| > 0.29 / 0.8
# with jump_lib's three marks (prm[6], prm[7] are the jump rate's there): the amplitude is a constant of the source
LQR_JUMP = JL.LQR + r"""
__device__ double covar(const double *prm, const double *x, int p) { return 0.25 * prm[0] * prm[0] * sin(1.7 * x[0] - 2.3 * x[1] + 0.4); }
"""


def lqr_covar(prm, x, amp=None):
    """numpy twin of LQR_COVAR: a [P, 1] for x [P, 2]"""
    amp = prm[6] if amp is None else amp
    return (amp * prm[0] * prm[0] * np.sin(1.7 * x[:, 0] - 2.3 * x[:, 1] + 0.4))[:, None]


def lqr_jump_covar(prm, x):
    return lqr_covar(prm, x, 0.25)


def lqr_workload(mid, rank, discount, prm=LQR_PRM):
    """jump_lib's ragged 21 x 70 grid: dim 0 absorbs (NPL 1), dim 1 is periodic (N = 70: NPL 2), one obstacle"""
    return dataclasses.replace(JL.lqr_workload(mid, rank, discount), name="lqr_cd", params=tuple(prm))


# ---------------------------------------------------------------------------------------------------- the 3-D correlated LQR
# stop_lib's LQR3 with the pairs (0,1) and (1,2): a_01 = prm[6] (1 + 0.3 x2) > 0, a_12 = prm[7] (1 + 0.3 x0) < 0
LQR3 = SL.LQR3 + r"""
__device__ double covar(const double *prm, const double *x, int p) { return p == 0 ? prm[6] * (1.0 + 0.3 * x[2]) : prm[7] * (1.0 + 0.3 * x[0]); }
"""
LQR3_MASKS = SL.LQR3_MASKS
LQR3_PAIRS = ((0, 1), (1, 2))
LQR3_OBSTACLE = JL.LQR3_OBSTACLE


def lqr3_covar(prm, x):
    return np.stack([prm[6] * (1.0 + 0.3 * x[:, 2]), prm[7] * (1.0 + 0.3 * x[:, 0])], axis=-1)


def lqr3_workload(mid, ngrid=(5, 128, 5), ranks=(1, 12, 9, 1), discount=0.3):
    """absorbing, periodic, reflecting.  On 5 x 128 x 5 (bond ranks 12 and 9: a launch along the middle dimension takes the L2
    form) h = (1, 4/127, 1); on 9 x 12 x 7 h = (0.5, 4/11, 2/3).  The covariances are sized to the grid: 80 % of what dominance
    allows at the largest factor 1.6 of either pair, split evenly over the two pairs of dimension 1"""
    from c3sc_amd import workloads as wl

    h = [4.0 / (n - 1) for n in ngrid]
    s2 = SL.LQR_PRM[0] ** 2
    a01 = 0.8 * s2 * min(h[1] / h[0], 0.5 * h[0] / h[1]) / 1.6
    a12 = -0.8 * s2 * min(h[1] / h[2], 0.5 * h[2] / h[1]) / 1.6
    return wl.Workload("lqr3_cd", mid, SL.LQR_PRM + (a01, a12), 3, 3, (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), tuple(ngrid), tuple(ranks), discount,
                       (wl.BC_ABSORB, wl.BC_PERIODIC, wl.BC_REFLECT), [LQR3_OBSTACLE], JL.lqr3_cands())


# ---------------------------------------------------------------------------------------------------- the known answer
# b = 0, g = 0, beta = 0, constant sigma and covariance a, V = x0 x1: the axis second differences of V vanish and the two
# diagonal neighbours give 2 r h0 h1 sign(a) = h2 a, so one explicit step of length delta gives x0 x1 + delta a at every node whose
# neighbours are one node away.  prm = {sigma, a}
KNOWN = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = 0.0; b[1] = 0.0; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[0]; s[1] = prm[0]; }
__device__ double stage(const double *prm, const double *x, const double *u) { return 0.0; }
__device__ double boundcost(const double *prm, const double *x) { return 0.0; }
__device__ double obscost(const double *prm, const double *x) { return 0.0; }
__device__ double covar(const double *prm, const double *x, int p) { return prm[1]; }
"""
KNOWN_MASKS = dict(udep_mask=0, uconst_mask=0, stage_udep=False)
KNOWN_PAIRS = ((0, 1),)
KNOWN_SIGMA, KNOWN_A, KNOWN_DELTA = 0.9, 0.35, 0.004


def known_host(prm, x, u):
    b = 0.0 * x + 0.0 * u[..., :1]
    return b, np.full(b.shape, prm[0]), np.zeros(b.shape[:-1])


def known_covar(prm, x):
    return np.full((len(x), 1), prm[1])


def known_workload(mid, a=KNOWN_A):
    """9 x 13 on [-1, 1]^2, absorbing x reflecting; V = x0 x1 as a train of rank 1"""
    from c3sc_amd import workloads as wl

    return wl.Workload("known_cd", mid, (KNOWN_SIGMA, a), 2, 1, (-1.0, -1.0), (1.0, 1.0), (9, 13), (1, 1, 1), 0.0,
                       (wl.BC_ABSORB, wl.BC_REFLECT), [], np.array([[0.0]]))


def known_cores(w):
    xg = w.xgrid()
    return [np.asarray(xg[0], dtype=np.float64).reshape(-1, 1), np.asarray(xg[1], dtype=np.float64).reshape(-1, 1)]


# ---------------------------------------------------------------------------------------------------- the Heston put
# American put under Heston in x = (log S, v): dx0 = (r - v / 2) dt + sqrt(v) dW1, dv = kappa (theta - v) dt + xi sqrt(v) dW2,
# d<W1, W2> = rho dt, so sigma = (sqrt(v), xi sqrt(v)) and a = rho xi v.  One dummy candidate; exercising, the faces and the
# terminal time pay psi = -max(K - exp(x0), 0).  prm = {r, kappa, theta, xi, rho, K}.  In log-price dominance is the grid-ratio
# condition |rho| xi <= h_v / h_x <= xi / |rho|: 0.12 <= 0.02 / 0.16 = 0.125 <= 0.75 on the 11 x 11 grid
HESTON = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = prm[0] - 0.5 * x[1]; b[1] = prm[1] * (prm[2] - x[1]); }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = sqrt(x[1]); s[1] = prm[3] * sqrt(x[1]); }
__device__ double stage(const double *prm, const double *x, const double *u) { return 0.0; }
__device__ double stopcost(const double *prm, const double *x)
{
    const double p = prm[5] - exp(x[0]);
    return p > 0.0 ? -p : 0.0;
}
__device__ double boundcost(const double *prm, const double *x) { return stopcost(prm, x); }
__device__ double obscost(const double *prm, const double *x) { return stopcost(prm, x); }
__device__ double covar(const double *prm, const double *x, int p) { return prm[4] * prm[3] * x[1]; }
"""
HESTON_MASKS = dict(udep_mask=0, uconst_mask=0, stage_udep=False)
HESTON_PAIRS = ((0, 1),)
HESTON_PRM = (0.05, 1.5, 0.1, 0.3, -0.4, 1.0)
HESTON_RHO0_PRM = HESTON_PRM[:4] + (0.0,) + HESTON_PRM[5:]
HESTON_LB, HESTON_UB, HESTON_N = (-0.8, 0.02), (0.8, 0.22), 11
# Q delta / h^2 < 1: h2 = 0.0004 and Q <= (h2 / h0^2) v + xi^2 v + (h2 / h0) |b0| + (h2 / h1) |b1| < 0.028 at v = 0.22
HESTON_DELTA, HESTON_STAGES = 0.0125, 20


def heston_host(prm, x, u):
    v = x[..., 1]
    b = np.stack([prm[0] - 0.5 * v, prm[1] * (prm[2] - v)], axis=-1) + 0.0 * u[..., :1]
    s = np.stack([np.sqrt(v), prm[3] * np.sqrt(v)], axis=-1) + 0.0 * u[..., :1]
    return b, s, np.zeros(b.shape[:-1])


def heston_covar(prm, x):
    return (prm[4] * prm[3] * x[:, 1])[:, None]


def heston_psi(prm, x):
    return -np.maximum(prm[5] - np.exp(x[..., 0]), 0.0)


def heston_workload(mid, rank=11, prm=HESTON_PRM):
    from c3sc_amd import workloads as wl

    return wl.Workload("heston_put", mid, tuple(prm), 2, 1, HESTON_LB, HESTON_UB, (HESTON_N, HESTON_N), wl.uniform_ranks(2, rank), prm[0],
                       (wl.BC_ABSORB, wl.BC_ABSORB), [], np.array([[0.0]]))


# ---------------------------------------------------------------------------------------------------- the operator
def neighbour_indices(i, n, bc):
    """(lo, hi) node indices of the neighbours of node i [..] along a dimension of n nodes with boundary type bc"""
    from c3sc_amd import workloads as wl

    i = np.asarray(i)
    lo, hi = i - 1, i + 1
    first, last = i == 0, i == n - 1
    if bc == wl.BC_ABSORB:
        lo, hi = np.where(first | last, i, lo), np.where(first | last, i, hi)
    elif bc == wl.BC_REFLECT:
        lo, hi = np.where(first, i, lo), np.where(last, i, hi)
    else:  # periodic: node 0 and node n - 1 are the same point
        lo, hi = np.where(first, n - 2, lo), np.where(last, 1, hi)
    return lo, hi


def full_values(w, cores):
    """the function train on the whole grid: V[n_0, .., n_{D-1}]"""
    G = JL.Train(w, cores).G
    v = G[0][:, 0, :]
    for m in range(1, w.dx):
        v = np.tensordot(v, G[m], axes=([-1], [1]))
    return v[..., 0]


def pair_rates(w, covar, pairs, x):
    """(r [P, npairs], a [P, npairs]): r_p = (h2 / (h_i h_j)) |a_p| / 2"""
    h2, t = BR.mca_constants(w)
    a = covar(w.params, x)
    r = np.stack([(t[2 * i] * t[2 * j] / h2) * np.abs(a[:, p]) / 2.0 for p, (i, j) in enumerate(pairs)], axis=-1)
    return r, a


def corr_terms(w, covar, pairs, Vfull, ix, x, V):
    """(cq [P], cpv [P], r [P, npairs]) at the nodes with multi-indices ix [P, D], states x [P, D] and axis stencils V [P, 2D+1]"""
    r, a = pair_rates(w, covar, pairs, x)
    cq, cpv = np.zeros(len(x)), np.zeros(len(x))
    nb = [neighbour_indices(ix[:, m], w.ngrid[m], w.bc[m]) for m in range(w.dx)]
    for p, (i, j) in enumerate(pairs):
        pos = a[:, p] > 0.0
        d1, d2 = [ix[:, m] for m in range(w.dx)], [ix[:, m] for m in range(w.dx)]
        d1[i], d1[j] = nb[i][1], np.where(pos, nb[j][1], nb[j][0])
        d2[i], d2[j] = nb[i][0], np.where(pos, nb[j][0], nb[j][1])
        vd = Vfull[tuple(d1)] + Vfull[tuple(d2)]
        cq = cq + (-2.0 * r[:, p])
        cpv = cpv + r[:, p] * (vd - ((V[:, 2 * i] + V[:, 2 * i + 1]) + (V[:, 2 * j] + V[:, 2 * j + 1])))
    return cq, cpv, r


def dominance(w, host, pairs, x, r):
    """[P] True where some paired dimension's axis rate would go negative: (h2 / h_m^2) sigma_m^2 / 2 < sum_{p with m} r_p"""
    h2, t = BR.mca_constants(w)
    C = np.asarray(w.cands, dtype=np.float64)
    _, s, _ = host(w.params, x, np.broadcast_to(C[0], (len(x), C.shape[1])))
    bad = np.zeros(len(x), dtype=bool)
    for m in range(w.dx):
        used = sum((r[:, p] for p, ij in enumerate(pairs) if m in ij), np.zeros(len(x)))
        bad |= t[2 * m + 1] * (s[:, m] * s[:, m]) / 2.0 < used
    return bad


def corr_fibers(w, host, covar, pairs, Vfull, k, idx, costs, absorbed, bcost, ocost, delta=None, psi_fn=None, forced=None,
                jumps=None, interp=None, with_corr=True):
    """the backup with the cross terms of every node of fibers idx from their axis stencils (costs [F, N, 2D+1], absorbed
    [F, N]) and the full value array Vfull of the same value function; jumps / interp: a jump model and the interpolant of the
    value function for the jump term as well.  Returns (value, index, margin, stationary, cfl, dominance) of shape [F, N]"""
    x = BR.node_states(w, k, idx).reshape(-1, w.dx)
    q0, pv0 = np.zeros(len(x)), np.zeros(len(x))
    if jumps is not None:
        jrate, J = JL.jump_terms(w, jumps, interp, x, bcost, ocost)
        q0, pv0 = q0 + jrate, pv0 + jrate * J
    dom = np.zeros(len(x), dtype=bool)
    if with_corr:
        cq, cpv, r = corr_terms(w, covar, pairs, Vfull, BR.node_indices(w, k, idx), x, costs.reshape(-1, 2 * w.dx + 1))
        q0, pv0 = q0 + cq, pv0 + cpv
        dom = dominance(w, host, pairs, x, r)
    res = BR.fibers(w, host, k, idx, costs, absorbed, bcost, ocost, q0, pv0, None if psi_fn is None else psi_fn(x), delta=delta,
                    forced=forced)
    return res + ((dom & (absorbed.reshape(-1) == 0)).reshape(absorbed.shape),)


# ---------------------------------------------------------------------------------------------------- the chain itself
def chain_rows(w, host, covar, pairs, x, ix, u):
    """the un-normalised transition rates of the node x [D] (multi-index ix) under the control u: a dict {neighbour multi-index
    tuple: rate} over the 2D axis neighbours and the 2 npairs diagonal ones (rates to one node are summed), and Q"""
    h2, t = BR.mca_constants(w)
    x1, ix1 = np.asarray(x, dtype=np.float64)[None], np.asarray(ix)[None]
    b, s, _ = host(w.params, x1, np.asarray(u, dtype=np.float64)[None])
    r, a = pair_rates(w, covar, pairs, x1)
    rows = {}

    def add(node, rate):
        node = tuple(int(v) for v in node)
        rows[node] = rows.get(node, 0.0) + float(rate)

    nb = [neighbour_indices(ix1[:, m], w.ngrid[m], w.bc[m]) for m in range(w.dx)]
    for m in range(w.dx):
        half = t[2 * m + 1] * s[0, m] ** 2 / 2.0
        tb = t[2 * m] * b[0, m]
        pm = half - tb if b[0, m] < -1e-14 else half
        pp = half + tb if b[0, m] > 1e-14 else half
        used = sum(r[0, p] for p, ij in enumerate(pairs) if m in ij)
        for side, rate in ((0, pm - used), (1, pp - used)):
            node = list(ix)
            node[m] = nb[m][side][0]
            add(node, rate)
    for p, (i, j) in enumerate(pairs):
        pos = a[0, p] > 0.0
        for si, sj in (((1, 1), (0, 0)) if pos else ((1, 0), (0, 1))):
            node = list(ix)
            node[i], node[j] = nb[i][si][0], nb[j][sj][0]
            add(node, r[0, p])
    return rows, sum(rows.values())


# ---------------------------------------------------------------------------------------------------- dense chains
def dense_terms(w, host, covar, pairs):
    """the per-sweep callable of backup_ref.sweeps: the pairs' correction on the nodal array the sweep reads, and the dominance
    flag"""
    x, _, sten = BR.grid2(w)
    ix = np.stack([a.reshape(-1) for a in np.meshgrid(np.arange(w.ngrid[0]), np.arange(w.ngrid[1]), indexing="ij")], axis=-1)

    def terms(Vn):
        cq, cpv, r = corr_terms(w, covar, pairs, Vn, ix, x, sten(Vn))
        return cq, cpv, None, dominance(w, host, pairs, x, r)

    return terms


def dense_chain(w, host, covar, pairs, psi_fn, delta, nstages, stopping=True, with_corr=True):
    """the explicit chain with the cross terms of a 2-D workload whose dimensions both absorb: V[s] for s = 0 .. nstages with
    V[nstages] = psi, the boundary nodes keep psi.  Returns (V [nstages + 1, n0, n1], index [nstages, n0, n1], cfl seen,
    dominance violated)"""
    psi = psi_fn(BR.grid2(w)[0])
    V, ui, _, anycfl, anydom = BR.sweeps(w, host, psi, psi, nstages, dense_terms(w, host, covar, pairs) if with_corr else None,
                                         psi if stopping else None, delta)
    return V[::-1].copy(), ui[::-1].copy(), anycfl, anydom


LQR_VI_BETA, LQR_VI_SWEEPS, LQR_VI_AMP = 0.5, 6, 0.8


def lqr_vi_workload(mid, rank=11):
    """the correlated LQR on horizon_lib's 11 x 11 grid (both dimensions absorb, no obstacle, h0 = h1: dominance iff |amp| <= 1)"""
    return dataclasses.replace(H.lqr_workload(mid, rank=rank, discount=LQR_VI_BETA), params=SL.LQR_PRM + (LQR_VI_AMP,), cands=JL.lqr_cands())


def dense_vi(w, host, covar, pairs, bcost, V0, nsweeps, with_corr=True):
    """value iteration sweeps of the correlated operator on the whole grid of a 2-D workload whose dimensions both absorb (the
    boundary nodes keep their boundary cost): [V_0, V_1, .. V_nsweeps]"""
    x, ab, _ = BR.grid2(w)
    return BR.sweeps(w, host, np.where(ab, bcost(x), V0.reshape(-1)), bcost(x), nsweeps,
                     dense_terms(w, host, covar, pairs) if with_corr else None)[0]


# ---------------------------------------------------------------------------------------------------- the reference API
def covar_callback(covar, prm, d):
    """ctypes form of a numpy covariance model covar(prm, x[P, d]) -> a [P, npairs], for c3control_add_covariance"""
    import ctypes as C

    FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_int)

    def _cov(x, p):
        return float(covar(prm, np.array([[x[i] for i in range(d)]]))[0, p])

    return FN(_cov)


def add_covariance(L, ctl, covar, prm, d, pairs):
    """c3control_add_covariance + c3control_set_correlation(1) on the facade control ctl; returns what must stay alive"""
    import ctypes as C

    cb = covar_callback(covar, prm, d)
    dims = (C.c_size_t * (2 * len(pairs)))(*[v for ij in pairs for v in ij])
    L.c3control_add_covariance.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), type(cb)]
    L.c3control_add_covariance(ctl.h, len(pairs), dims, cb)
    L.c3control_set_correlation.argtypes = [C.c_void_p, C.c_int]
    L.c3control_set_correlation(ctl.h, 1)
    return cb, dims


def heston_callbacks(prm=HESTON_PRM):
    """(callbacks, stop callback) of the Heston put for facade_lib.Control, built like stop_lib.put_callbacks"""
    import facade_lib as fl

    psi = lambda x: float(heston_psi(prm, np.asarray(x)))
    return fl.callbacks2d(lambda x, u: [prm[0] - 0.5 * x[1], prm[1] * (prm[2] - x[1])],
                          lambda x, u: [np.sqrt(x[1]), prm[3] * np.sqrt(x[1])], lambda x, u: 0.0, psi, psi, psi)


def fh_child(out_path, delta=HESTON_DELTA, nstages=HESTON_STAGES):
    """the Heston put through the reference API (run in a child process): c3control_fh_solve in stop and correlation mode from
    the terminal value psi, V_s at every node of every stage saved"""
    import ctypes as C

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(HESTON, 2, 1, ranks=(4, 8, 12), name="heston_api", horizon=True, stop=True, corr_pairs=HESTON_PAIRS, **HESTON_MASKS)
    w = heston_workload(mid, rank=11)
    cbs, stop_cb = heston_callbacks(HESTON_PRM)
    L, ctl, aa = fl.stop_control(w, cbs, stop_cb)
    keep = add_covariance(L, ctl, heston_covar, HESTON_PRM, 2, HESTON_PAIRS)
    vt, keep2 = fl.init_value(L, ctl, aa, lambda xx: heston_psi(HESTON_PRM, xx))
    V = L.c3control_fh_solve(ctl.h, C.c_size_t(nstages), C.c_double(delta), vt, aa, ctl.opt, C.c_int(0))
    fl.save_stages(out_path, L, V, nstages, *w.ngrid)


def vi_child(out_path, nsweeps=LQR_VI_SWEEPS):
    """the correlated LQR through the reference API (run in a child process): c3control_vi_solve one sweep at a time from
    V_0 = s |x|^2, the nodal values after every sweep saved"""
    import ctypes as C

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(LQR, 2, 2, ranks=(4, 8, 12), name="lqr_cd_api", corr_pairs=LQR_PAIRS, **LQR_MASKS)
    w = lqr_vi_workload(mid)
    L = fl.solver_lib()
    ctl = fl.Control(w, callbacks=H.lqr_callbacks(w.params), consistent_ends=None)
    keep = add_covariance(L, ctl, lqr_covar, w.params, 2, LQR_PAIRS)
    aa = fl.approx_args(L)
    v, keep2 = fl.init_value(L, ctl, aa, lambda xx: H.lqr_terminal(w.params, xx))
    n0, n1 = w.ngrid
    out = [fl.nodal(L, v.value, n0, n1)]
    for _ in range(nsweeps):
        v = C.c_void_p(L.c3control_vi_solve(ctl.h, C.c_size_t(1), C.c_double(0.0), v, aa, ctl.opt, C.c_int(0), None))
        out.append(fl.nodal(L, v.value, n0, n1))
    np.savez(out_path, V=np.array(out))
