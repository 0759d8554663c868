"""Jump diffusions (c3sc_hip_set_jumps): device sources of a jump LQR in two and three dimensions, of a
known-answer model and of Merton's American put, and a numpy restatement of the backup with the Poisson jump term; dense value
and policy iteration of the jump LQR on a whole small grid (dense_vi, dense_pi) and the child processes that drive the
reference API (vi_child, pi_child, fh_child).  Shared by the CPU and GPU tests and tools/jump_bench.py.  It shares no code with
the kernels.

The chain is the rate form of Kushner and Dupuis, section 5.6: a jump is one more transition with the un-normalised rate
h2 lambda(x) to the mark average J(x) = sum_m pi_m(x) Vjump(y_m), so Q and PV of every candidate gain h2 lambda and h2 lambda J
and everything downstream is the backup without jumps (backup_ref states it; the two terms are its q0 and pv0).  Vjump(y): periodic dimensions are wrapped into [lb, ub); a target inside an obstacle pays the obstacle
cost, one outside [lb, ub] on an absorbing dimension the boundary cost (the obstacle first, as the rollouts' exit test chooses);
any other target pays the interpolant of the function train -- multilinear, or the nearer node with constelm -- clamped to
the grid hull."""
import dataclasses
import os

import numpy as np

import backup_ref as BR
import horizon_lib as H
import stop_lib as SL

JUMP_MAX = 8

# ---------------------------------------------------------------------------------------------------- the 2-D jump LQR
# horizon_lib's decoupled LQR with stop_lib's stopping cost and three marks.  prm = {sig, q, r, s, c0, c1, lam0, lam1}
# (C3SC_MAX_PARAMS = 8; the displacements d0 = 0.53 and d1 = 0.71 are constants of the source):
#   lambda(x) = lam0 + lam1 x0^2
#   mark 0: y = x + (d0, 0)      weight 0.5 - a   beyond the absorbing face of dim 0 from the nodes with x0 > ub - d0
#   mark 1: y = x + (0, d1)      weight 0.3 + a   across the periodic seam of dim 1 from the nodes with x1 > ub - d1
#   mark 2: y = (x + centre) / 2 weight 0.2       into the obstacle from the nodes around it (centre = its centre)
# with a = 0.05 x1 / 2; d0 and d1 are no multiples of the grid spacings, so the targets are off-node
LQR_JUMPS = r"""
__device__ double jumprate(const double *prm, const double *x) { return prm[6] + prm[7] * x[0] * x[0]; }
__device__ double jump(const double *prm, const double *x, int m, double *y)
{
    const double a = 0.05 * x[1] / 2.0;
    if (m == 0) { y[0] = x[0] + 0.53; y[1] = x[1]; return 0.5 - a; }
    if (m == 1) { y[0] = x[0]; y[1] = x[1] + 0.71; return 0.3 + a; }
    y[0] = (x[0] + 0.9) / 2.0;
    y[1] = (x[1] - 0.9) / 2.0;
    return 0.2;
}
"""
LQR = SL.LQR + LQR_JUMPS
LQR_MASKS = H.LQR_MASKS
LQR_NJUMP = 3
LQR_PRM = (0.3, 1.0, 1.0, 2.0, 0.6, 0.5, 1.5, 0.8)
LQR_D0, LQR_D1 = 0.53, 0.71
LQR_ZERO_RATE_PRM = LQR_PRM[:6] + (0.0, 0.0)
LQR_OBSTACLE = ((0.9, -0.9), (0.5, 0.6))


def lqr_cands():
    """5 x 5 candidates without a pair +-a in either component: where a node's two neighbours in a dimension hold the same
    value (the live end nodes of a periodic fiber on an absorbing face, quirk Q3), candidates +a and -a would tie exactly, and
    the index-margin precondition of the tests counts ties"""
    u = np.linspace(-1.5, 1.2, 5)
    return np.array([(a, b) for a in u for b in u])


def lqr3_cands():
    u = np.linspace(-1.5, 1.2, 5)
    return np.array([(a, b, c) for a in u for b in u for c in u])


def lqr_workload(mid, rank, discount, prm=LQR_PRM):
    """the ragged 21 x 70 grid of the stop tests: dim 0 absorbs (NPL 1), dim 1 is periodic (N = 70: NPL 2), one obstacle"""
    from c3sc_amd import workloads as wl

    return wl.Workload("lqr_jd", mid, tuple(prm), 2, 2, (-2.0, -2.0), (2.0, 2.0), (21, 70), wl.uniform_ranks(2, rank), discount,
                       (wl.BC_ABSORB, wl.BC_PERIODIC), [LQR_OBSTACLE], lqr_cands())


def lqr_jumps(prm, x):
    """numpy twin of LQR_JUMPS: (lambda [P], pi [P, 3], y [P, 3, 2]) for x [P, 2]"""
    lam = prm[6] + prm[7] * x[:, 0] * x[:, 0]
    a = 0.05 * x[:, 1] / 2.0
    pi = np.stack([0.5 - a, 0.3 + a, np.full(len(x), 0.2)], axis=-1)
    y = np.stack([x + np.array([LQR_D0, 0.0]), x + np.array([0.0, LQR_D1]), (x + np.array([0.9, -0.9])) / 2.0], axis=1)
    return lam, pi, y


# ---------------------------------------------------------------------------------------------------- the 3-D jump LQR
# stop_lib's LQR3 on 5 x 128 x 5 (absorbing, periodic, reflecting) for the L2 form: prm = LQR_PRM[:6] + {lam0, lam1}, d = 0.61
#   mark 0: y = x + (d, 0, 0) (beyond the absorbing face from the last nodes), weight 0.6
#   mark 1: y = x + (0, d, 2 d) (across the seam; beyond the reflecting face: clamped), weight 0.4
LQR3 = SL.LQR3 + r"""
__device__ double jumprate(const double *prm, const double *x) { return prm[6] + prm[7] * x[2] * x[2]; }
__device__ double jump(const double *prm, const double *x, int m, double *y)
{
    y[0] = x[0] + (m == 0 ? 0.61 : 0.0);
    y[1] = x[1] + (m == 0 ? 0.0 : 0.61);
    y[2] = x[2] + (m == 0 ? 0.0 : 1.22);
    return m == 0 ? 0.6 : 0.4;
}
"""
LQR3_MASKS = SL.LQR3_MASKS
LQR3_NJUMP = 2
LQR3_PRM = (0.3, 1.0, 1.0, 2.0, 0.6, 0.5, 1.2, 0.5)
LQR3_D = 0.61
LQR3_OBSTACLE = ((0.5, -0.9, 0.0), (1.2, 0.6, 1.2))


def lqr3_workload(mid, ranks=(1, 12, 9, 1), discount=0.3):
    """unequal bond ranks, padded to 12; a launch along the 128-node middle dimension takes the L2 form (tests/test_gpu_stop.py)"""
    from c3sc_amd import workloads as wl

    return wl.Workload("lqr3_jd", mid, LQR3_PRM, 3, 3, (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (5, 128, 5), tuple(ranks), discount,
                       (wl.BC_ABSORB, wl.BC_PERIODIC, wl.BC_REFLECT), [LQR3_OBSTACLE], lqr3_cands())


def lqr3_jumps(prm, x):
    d = LQR3_D
    lam = prm[6] + prm[7] * x[:, 2] * x[:, 2]
    pi = np.broadcast_to(np.array([0.6, 0.4]), (len(x), 2))
    y = np.stack([x + np.array([d, 0.0, 0.0]), x + np.array([0.0, d, 2.0 * d])], axis=1)
    return lam, pi, y


# ---------------------------------------------------------------------------------------------------- the known answer
# b = sigma = 0, constant stage cost g and rate lambda, every mark beyond the absorbing face of dim 0, which costs c:
# dt = h2 / (h2 lambda) and V = g / lambda + exp(-beta / lambda) c at every live node.  prm = {g, lambda, c}
KNOWN = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = 0.0; b[1] = 0.0; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = 0.0; s[1] = 0.0; }
__device__ double stage(const double *prm, const double *x, const double *u) { return prm[0]; }
__device__ double boundcost(const double *prm, const double *x) { return prm[2]; }
__device__ double obscost(const double *prm, const double *x) { return -1.0; }
__device__ double jumprate(const double *prm, const double *x) { return prm[1]; }
__device__ double jump(const double *prm, const double *x, int m, double *y)
{
    y[0] = x[0] + 10.0 + m;
    y[1] = x[1];
    return m == 2 ? 0.5 : 0.25;
}
"""
KNOWN_MASKS = dict(udep_mask=0, uconst_mask=0, stage_udep=False)
KNOWN_NJUMP = 3
KNOWN_PRM = (0.7, 2.0, 3.0)
KNOWN_BETA = 0.3


def known_answer(prm=KNOWN_PRM, beta=KNOWN_BETA):
    return prm[0] / prm[1] + np.exp(-beta / prm[1]) * prm[2]


def known_workload(mid, rank=4, discount=KNOWN_BETA):
    from c3sc_amd import workloads as wl

    return wl.Workload("known_jd", mid, KNOWN_PRM, 2, 1, (-1.0, -1.0), (1.0, 1.0), (9, 13), wl.uniform_ranks(2, rank), discount,
                       (wl.BC_ABSORB, wl.BC_REFLECT), [], np.array([[0.0]]))


# ---------------------------------------------------------------------------------------------------- Merton's American put
# stop_lib's put on the mean of two assets with a common lognormal jump: S -> S exp(z_m), three atoms of z ~ N(mu, s^2) (the
# three-point Gauss-Hermite rule: z = mu, mu -+ sqrt(3) s with weights 2/3, 1/6, 1/6) at the intensity prm[3].
# prm = {r, v, K, lambda, mu, s}.  The drift keeps r (no compensator): the test compares chains, not prices
PUT = SL.PUT + r"""
__device__ double jumprate(const double *prm, const double *x) { return prm[3]; }
__device__ double jump(const double *prm, const double *x, int m, double *y)
{
    const double z = prm[4] + (m == 0 ? 0.0 : (m == 1 ? -1.7320508075688772 : 1.7320508075688772)) * prm[5];
    const double f = exp(z);
    y[0] = x[0] * f;
    y[1] = x[1] * f;
    return m == 0 ? 2.0 / 3.0 : 1.0 / 6.0;
}
"""
PUT_MASKS = SL.PUT_MASKS
PUT_NJUMP = 3
PUT_PRM = (SL.PUT_R, SL.PUT_V, SL.PUT_K, 0.8, -0.1, 0.25)
# (Q + h2 lambda) delta / h^2 < 1 on the 11 x 11 grid: Q delta / h^2 <= 0.64 as in stop_lib, and lambda delta = 0.02
PUT_DELTA, PUT_STAGES = SL.PUT_DELTA, SL.PUT_STAGES


def put_jumps(prm, x):
    z = prm[4] + np.array([0.0, -1.7320508075688772, 1.7320508075688772]) * prm[5]
    f = np.exp(z)
    y = x[:, None, :] * f[None, :, None]
    pi = np.broadcast_to(np.array([2.0 / 3.0, 1.0 / 6.0, 1.0 / 6.0]), (len(x), 3))
    return np.full(len(x), prm[3]), pi, y


def put_workload(mid, rank=11, n=SL.PUT_N):
    return dataclasses.replace(SL.put_workload(mid, rank=rank, n=n), name="put_jd", params=PUT_PRM)


# ---------------------------------------------------------------------------------------------------- Vjump
class Train:
    """the interpolant of a function train at arbitrary points, in float64: cores[m][j, a + b r_m] as the engine takes them"""

    def __init__(self, w, cores):
        self.w = w
        self.g = [np.asarray(g, dtype=np.float64) for g in w.xgrid()]
        self.G = [np.asarray(cores[m], dtype=np.float64).reshape(w.ngrid[m], w.ranks[m + 1], w.ranks[m]).transpose(0, 2, 1)
                  for m in range(w.dx)]

    @staticmethod
    def cell(g, y, constelm):
        """valuef_eval's cell per coordinate: closed clamps, otherwise the last node with g[i] <= y; the weight of node i + 1"""
        N = len(g)
        i = np.clip(np.searchsorted(g, y, side="right") - 1, 0, N - 2)
        wt = (y - g[i]) / (g[i + 1] - g[i])
        lo, hi = y <= g[0], y >= g[N - 1]
        i = np.where(lo, 0, np.where(hi, N - 2, i))
        wt = np.where(lo, 0.0, np.where(hi, 1.0, wt))
        if constelm:
            wt = np.where(wt < 0.5, 0.0, 1.0)
        return i, wt

    def value(self, y, constelm=False):
        y = np.asarray(y, dtype=np.float64)
        v = np.ones((len(y), 1))
        for m in range(self.w.dx):
            i, wt = self.cell(self.g[m], y[:, m], constelm)
            Gm = (1.0 - wt)[:, None, None] * self.G[m][i] + wt[:, None, None] * self.G[m][i + 1]
            v = np.einsum("pa,pab->pb", v, Gm)
        return v[:, 0]


class Nodal:
    """the same interpolant of a 2-D nodal matrix V[n0, n1] (a train of full rank): bilinear, or the nearer node"""

    def __init__(self, w, V):
        self.w, self.V = w, np.asarray(V, dtype=np.float64)
        self.g = [np.asarray(g, dtype=np.float64) for g in w.xgrid()]

    def value(self, y, constelm=False):
        i, a = Train.cell(self.g[0], y[:, 0], constelm)
        j, b = Train.cell(self.g[1], y[:, 1], constelm)
        V = self.V
        return (1 - a) * ((1 - b) * V[i, j] + b * V[i, j + 1]) + a * ((1 - b) * V[i + 1, j] + b * V[i + 1, j + 1])


def wrap(w, y):
    """the periodic dimensions of y [P, D] mapped into [lb, ub) by the formulas of the rollouts' wrap"""
    from c3sc_amd import workloads as wl

    out = np.array(y, dtype=np.float64)
    for m, g in enumerate(w.xgrid()):
        if w.bc[m] != wl.BC_PERIODIC:
            continue
        lb, ub = g[0], g[-1]
        ln = ub - lb
        v = y[:, m] - np.floor((y[:, m] - lb) / ln) * ln
        v = np.where(v >= ub, v - ln, v)
        v = np.where(v < lb, v + ln, v)
        out[:, m] = v
    return out


def target_kinds(w, y):
    """per target y [P, D]: (wrapped y, inside an obstacle, beyond an absorbing face, moved by the wrap)"""
    from c3sc_amd import workloads as wl

    yw = wrap(w, y)
    inobs = np.zeros(len(y), dtype=bool)
    for c, wd in w.obstacles:
        lo, hi = np.array(c) - np.array(wd) / 2.0, np.array(c) + np.array(wd) / 2.0
        inobs |= np.all((yw >= lo) & (yw <= hi), axis=1)  # closed boxes
    out = np.zeros(len(y), dtype=bool)
    for m, g in enumerate(w.xgrid()):
        if w.bc[m] == wl.BC_ABSORB:
            out |= (yw[:, m] < g[0]) | (yw[:, m] > g[-1])
    return yw, inobs, out, np.any(yw != y, axis=1)


def vjump(w, interp, y, bcost, ocost, constelm=False):
    """the value a jump to y [P, D] pays; interp: a Train or Nodal of the value function the backup reads"""
    yw, inobs, out, _ = target_kinds(w, y)
    return np.where(inobs, ocost(yw), np.where(out, bcost(yw), interp.value(yw, constelm)))


def jump_terms(w, jumps, interp, x, bcost, ocost, constelm=False):
    """(h2 lambda [P], J [P]) at the states x [P, D]; J sums the marks in ascending order"""
    h2, _ = BR.mca_constants(w)
    lam, pi, y = jumps(w.params, x)
    J = np.zeros(len(x))
    for m in range(pi.shape[1]):
        J = J + pi[:, m] * vjump(w, interp, y[:, m], bcost, ocost, constelm)
    return h2 * lam, J


# ---------------------------------------------------------------------------------------------------- one node
def jump_fibers(w, host, jumps, interp, k, idx, costs, absorbed, bcost, ocost, delta=None, psi_fn=None, forced=None, constelm=False,
                with_jumps=True):
    """the backup with jumps of every node of fibers idx from their stencils (costs [F, N, 2D+1], absorbed [F, N]) and the
    interpolant `interp` of the same value function.  Returns (value, index, margin, stationary, cfl, rate, J) of shape [F, N]"""
    x = BR.node_states(w, k, idx).reshape(-1, w.dx)
    if with_jumps:
        jrate, J = jump_terms(w, jumps, interp, x, bcost, ocost, constelm)
    else:
        jrate, J = np.zeros(len(x)), np.zeros(len(x))
    res = BR.fibers(w, host, k, idx, costs, absorbed, bcost, ocost, jrate, jrate * J, None if psi_fn is None else psi_fn(x),
                    delta=delta, forced=forced)
    return res + (jrate.reshape(absorbed.shape), J.reshape(absorbed.shape))


# ---------------------------------------------------------------------------------------------------- dense chains
def dense_terms(w, jumps, bcost, ocost):
    """the per-sweep callable of backup_ref.sweeps: the jump terms read from the bilinear interpolant of the sweep's input"""
    x = BR.grid2(w)[0]

    def terms(Vn):
        jrate, J = jump_terms(w, jumps, Nodal(w, Vn), x, bcost, ocost)
        return jrate, jrate * J, None, None

    return terms


def dense_chain(w, host, jumps, psi_fn, delta, nstages, stopping=True):
    """the explicit chain with jumps of a 2-D workload whose dimensions both absorb: V[s] for s = 0 .. nstages with
    V[nstages] = psi, the boundary nodes keep psi (the boundary cost of the put); the jump targets read the bilinear
    interpolant of V[s + 1].  Returns (V [nstages + 1, n0, n1], index [nstages, n0, n1], cfl seen)"""
    psi = psi_fn(BR.grid2(w)[0])
    V, ui, _, anycfl, _ = BR.sweeps(w, host, psi, psi, nstages, dense_terms(w, jumps, psi_fn, psi_fn), psi if stopping else None, delta)
    return V[::-1].copy(), ui[::-1].copy(), anycfl


# ---------------------------------------------------------------------------------------------------- rollouts
def jump_uniforms(seed, traj, step):
    """(u0, u1) of one rollout step: the host twin of the device's Philox draw (c3sc_hip_jump_uniforms)"""
    from c3sc_amd import engine as E

    return E.jump_uniforms(seed, traj, step)


def step_jumps(w, jumps, x, seed, trajs, step, dt):
    """the compound-Poisson increment of one step at the states x [n, D] of the trajectories trajs [n] (global indices):
    (event [n], mark [n] (-1: none), increment [n, D]).  Event when u0 < min(lambda dt, 1); the mark is the first m with
    u1 < pi_0 + .. + pi_m, the last mark catches rounding; the increment is y_m(x) - x"""
    lam, pi, y = jumps(w.params, x)
    n, M = pi.shape
    uu = np.array([jump_uniforms(seed, int(t), step) for t in trajs])
    event = uu[:, 0] < np.minimum(lam * dt, 1.0)
    cum = np.zeros(n)
    mark = np.full(n, -1)
    for m in range(M):
        cum = cum + pi[:, m]
        take = (mark < 0) & ((uu[:, 1] < cum) | (m == M - 1))
        mark = np.where(take, m, mark)
    mark = np.where(event, mark, -1)
    inc = np.where(event[:, None], y[np.arange(n), np.maximum(mark, 0)] - x, 0.0)
    return event, mark, inc


def replay(w, jumps, drift_fn, stage_fn, bcost, ocost, traj, u, seed, dt, beta, push=None, traj_offset=0):
    """a rollout without diffusion noise replayed from its saved states traj [n, N + 1, D] and controls u [n, N, du]: every
    step's exit test (obstacle first, then the absorbing faces, at the state itself), stage cost and next state
    x + b dt + push + jump increment, all formed at the device's own x_k.  push [n, N, D]: sigma sqrt(dt) xi of given normals.
    Returns (next states [n, N, D] as predicted, events [n, N], marks [n, N], exit step [n] (-1: never), cost [n])"""
    n, N1, D = traj.shape
    N = N1 - 1
    alive = np.ones(n, dtype=bool)
    ex = np.full(n, -1)
    J = np.zeros(n)
    nxt = np.zeros((n, N, D))
    events, marks = np.zeros((n, N), dtype=bool), np.full((n, N), -1)
    trajs = traj_offset + np.arange(n)

    def exit_test(k, xk):
        nonlocal alive, J
        _, inobs, out, _ = target_kinds(dataclasses.replace(w, bc=tuple(0 if b == 2 else b for b in w.bc)), xk)  # no wrap here
        gone = alive & (inobs | out)
        J = J + np.where(gone, np.exp(-beta * (k * dt)) * np.where(inobs, ocost(xk), bcost(xk)), 0.0)
        ex[gone] = k
        alive = alive & ~gone

    for k in range(N):
        xk = traj[:, k]
        exit_test(k, xk)
        uk = np.where(alive[:, None], u[:, k], 0.0)
        J = J + np.where(alive, np.exp(-beta * (k * dt)) * stage_fn(xk, uk) * dt, 0.0)
        ev, mk, inc = step_jumps(w, jumps, xk, seed, trajs, k, dt)
        acc = xk + drift_fn(xk, uk) * dt
        if push is not None:
            acc = acc + push[:, k]
        acc = acc + inc
        nxt[:, k] = np.where(alive[:, None], acc, xk)
        events[:, k], marks[:, k] = ev & alive, np.where(alive, mk, -1)
    exit_test(N, traj[:, N])
    return nxt, events, marks, ex, J


def put_rollouts(w, stack, x0, n, dt, rng, chunk=1 << 16):
    """the rollout restatement for Merton's put under the value stack `stack` (nodal V_0 .. V_N of the explicit chain, both
    dimensions absorbing, one candidate): n noisy paths from the state x0 with numpy's own normals and uniforms.  A step is the
    device's: exit test (pay the discounted boundary cost, freeze), the controller's backup with the jump term on the off-grid
    stencil of V_{k+1} (neighbours one spacing away, clamped to the faces) -- a lane stops where psi wins and pays the
    discounted psi --, then x + b dt + sigma sqrt(dt) xi + the compound-Poisson increment, all at x_k.  A path alive after the
    last step adds the discounted V_N(x_N).  Returns the costs [n]"""
    N = len(stack) - 1
    prm, beta = w.params, w.discount
    h2, t = BR.mca_constants(w)
    g = w.xgrid()[0]
    h, lb, ub = g[1] - g[0], g[0], g[-1]
    C = np.asarray(w.cands, dtype=np.float64)
    psi_fn = lambda xx: SL.put_psi(prm, xx)
    out = []
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        x = np.tile(np.asarray(x0, dtype=np.float64), (m, 1))
        J, alive = np.zeros(m), np.ones(m, dtype=bool)
        for k in range(N + 1):
            disc = np.exp(-beta * (k * dt))
            gone = alive & ((x < lb) | (x > ub)).any(axis=1)
            J = J + np.where(gone, disc * psi_fn(x), 0.0)
            alive = alive & ~gone
            if k == N:
                J = J + np.where(alive, disc * Nodal(w, stack[N]).value(x), 0.0)
                break
            V = Nodal(w, stack[k + 1])
            cl = lambda y: np.clip(y, lb, ub)
            S = np.stack([V.value(cl(x - [h, 0])), V.value(cl(x + [h, 0])), V.value(cl(x - [0, h])), V.value(cl(x + [0, h])),
                          V.value(x)], axis=-1)
            jrate, Jv = jump_terms(w, put_jumps, V, x, psi_fn, psi_fn)
            vals, _, _ = BR.candidate_values(SL.put_host, prm, x, S, C, h2, t, beta, jrate, jrate * Jv, dt)
            _, ui, _ = BR.backup(vals, psi_fn(x))
            stop = alive & (ui == len(C))
            J = J + np.where(stop, disc * psi_fn(x), 0.0)
            alive = alive & ~stop
            b, s, _ = SL.put_host(prm, x, np.zeros((m, 1)))
            lam, pi, y = put_jumps(prm, x)
            u0, u1 = rng.random(m), rng.random(m)
            mark = np.minimum((u1[:, None] >= np.cumsum(pi, axis=1)).sum(axis=1), pi.shape[1] - 1)
            inc = np.where((u0 < np.minimum(lam * dt, 1.0))[:, None], y[np.arange(m), mark] - x, 0.0)
            xn = x + b * dt + s * np.sqrt(dt) * rng.standard_normal((m, 2)) + inc
            x = np.where(alive[:, None], xn, x)
        out.append(J)
    return np.concatenate(out)


# the states the noisy rollouts of the put start from (nodes of the 11 x 11 grid) and the discretisation gap there: a CPU run of
# put_rollouts with 2^18 paths per state (numpy default_rng(2718), the three states in turn) under the dense chain's own stack
# gives means -0.070433, -0.109889, -0.045848 against V_0 = -0.073635, -0.113049, -0.047845: gaps 0.003202, 0.003160, 0.001997
# with standard errors 0.000209, 0.000226, 0.000184 (Euler step of the rollouts against the chain's interpolated jump targets
# on a coarse grid).  PUT_GAP is the largest; the bound of the device test is twice it
PUT_X0 = SL.PUT_X0
PUT_GAP = 0.003202
PUT_BOUND = 2 * PUT_GAP


# ---------------------------------------------------------------------------------------------------- the reference API
LQR_VI_BETA = 0.5
LQR_VI_SWEEPS = 6


def jump_callbacks(jumps, prm, d):
    """ctypes forms (rate, mark) of a numpy jump model jumps(prm, x[P, d]) -> (lambda, pi, y), for c3control_add_jumps"""
    import ctypes as C

    RATE_FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double))
    MARK_FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double))

    def _rate(x):
        return float(jumps(prm, np.array([[x[i] for i in range(d)]]))[0][0])

    def _mark(x, m, y):
        _, pi, yy = jumps(prm, np.array([[x[i] for i in range(d)]]))
        for i in range(d):
            y[i] = yy[0, m, i]
        return float(pi[0, m])

    return RATE_FN(_rate), MARK_FN(_mark)


def add_jumps(L, ctl, jumps, prm, d, njump):
    """c3control_add_jumps + c3control_set_jumps(1) on the facade control ctl; returns the callbacks (keep them alive)"""
    import ctypes as C

    rate, mark = jump_callbacks(jumps, prm, d)
    L.c3control_add_jumps.argtypes = [C.c_void_p, C.c_int, type(rate), type(mark)]
    L.c3control_add_jumps(ctl.h, njump, rate, mark)
    L.c3control_set_jumps.argtypes = [C.c_void_p, C.c_int]
    L.c3control_set_jumps(ctl.h, 1)
    return rate, mark


def lqr_vi_workload(mid, rank=11):
    """the jump LQR on horizon_lib's 11 x 11 grid (both dimensions absorb, no obstacle)"""
    return dataclasses.replace(H.lqr_workload(mid, rank=rank, discount=LQR_VI_BETA), params=LQR_PRM, cands=lqr_cands())


def dense_vi(w, host, jumps, bcost, V0, nsweeps):
    """value iteration sweeps of the jump operator on the whole grid of a 2-D workload whose dimensions both absorb (the
    boundary nodes keep their boundary cost; the jump targets read the bilinear interpolant of the sweep's input):
    [V_0, V_1, .. V_nsweeps]"""
    x, ab, _ = BR.grid2(w)
    terms = dense_terms(w, jumps, bcost, lambda xx: np.full(len(xx), 5.0))
    return BR.sweeps(w, host, np.where(ab, bcost(x), V0.reshape(-1)), bcost(x), nsweeps, terms)[0]


def dense_pi(w, host, jumps, bcost, P, nsweeps, mu=None):
    """policy iteration sweeps of the jump operator on the whole grid of the same class of workload: the greedy policy of P
    (candidate index per node and its margin, jump terms from the bilinear interpolant of P), then V_0 = P and V_{s+1} = that
    policy's backup of V_s at the live nodes (jump terms from the interpolant of V_s), the boundary cost at the absorbed ones --
    what c3control_pi_solve(maxiter = s, policy = P) applies.  mu [n0, n1]: a policy to evaluate in place of the greedy one.
    Returns (mu [n0, n1] (-1: absorbed), margin [n0, n1] (inf: absorbed), [V_0, V_1, .. V_nsweeps])"""
    x, ab, _ = BR.grid2(w)
    terms = dense_terms(w, jumps, bcost, lambda xx: np.full(len(xx), 5.0))
    _, greedy, margin, _, _ = BR.sweeps(w, host, P, bcost(x), 1, terms)
    pol = greedy[0] if mu is None else np.where(ab.reshape(w.ngrid), -1, np.asarray(mu).reshape(w.ngrid))
    V = BR.sweeps(w, host, P, bcost(x), nsweeps, terms, forced=pol)[0]
    return pol, np.where(ab.reshape(w.ngrid), np.inf, margin[0]), V


def vi_child(out_path, nsweeps=LQR_VI_SWEEPS):
    """the jump LQR through the reference API (run in a child process by tests/test_gpu_jump.py): c3control_vi_solve one sweep
    at a time from V_0 = s |x|^2, the nodal values after every sweep saved; then c3control_simulate_batch of the last sweep's
    policy without diffusion noise, its states, controls, costs and exit steps saved"""
    import ctypes as C

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(LQR, 2, 2, ranks=(4, 8, 12), name="lqr_jd_api", njump=LQR_NJUMP, **LQR_MASKS)
    w = lqr_vi_workload(mid)
    L = fl.solver_lib()
    ctl = fl.Control(w, callbacks=H.lqr_callbacks(LQR_PRM), consistent_ends=None)
    keep = add_jumps(L, ctl, lqr_jumps, LQR_PRM, 2, LQR_NJUMP)
    aa = fl.approx_args(L)
    v, keep2 = fl.init_value(L, ctl, aa, lambda xx: H.lqr_terminal(LQR_PRM, xx))
    n0, n1 = w.ngrid
    out = [fl.nodal(L, v.value, n0, n1)]
    for _ in range(nsweeps):
        v = C.c_void_p(L.c3control_vi_solve(ctl.h, C.c_size_t(1), C.c_double(0.0), v, aa, ctl.opt, C.c_int(0), None))
        out.append(fl.nodal(L, v.value, n0, n1))
    L.c3control_add_policy_sim(ctl.h, v, ctl.opt, None)
    n, N = SIM_N, SIM_STEPS
    x0 = np.ascontiguousarray(np.random.default_rng(9).uniform(-1.6, 1.6, size=(n, 2)))
    x0[:8, 0] = 1.9  # a mark-0 jump from here leaves through the absorbing face
    noise = np.zeros((n, N, 2))
    traj, ut, cost, ex = np.zeros((n, N + 1, 2)), np.zeros((n, N, 2)), np.zeros(n), np.zeros(n, dtype=np.int64)
    rc = L.c3control_simulate_batch(ctl.h, C.c_size_t(n), fl.dp(x0), C.c_double(SIM_DT), C.c_size_t(N), C.c_uint64(SIM_SEED), fl.dp(noise),
                                    C.c_int(0), C.c_size_t(1), fl.dp(traj), fl.dp(ut), fl.dp(cost), ex.ctypes.data_as(C.c_void_p), None)
    np.savez(out_path, V=np.array(out), rc=rc, traj=traj, u=ut, cost=cost, exit=ex)


SIM_N, SIM_STEPS, SIM_DT, SIM_SEED = 48, 32, 0.02, 77


PI_BEFORE, PI_AFTER = (1, 3), (1, 3, 6)  # evaluation sweeps asked of c3control_pi_solve before and after the vi step
PI_MARKERS = ("jump_lib.pi_child: host-driven policy iteration done", "jump_lib.pi_child: first-fiber check done")


def pi_child(out_path):
    """policy iteration on the jump LQR through the reference API (run in a child process by tests/test_gpu_jump_policy.py):
    c3control_pi_solve(K, policy = V_0 = s |x|^2) for K in PI_BEFORE while the device model is not yet checked against the host
    callbacks (the host-driven pi_core whatever the environment), one c3control_vi_solve step from V_0 (the first-fiber check),
    then K in PI_AFTER (the device-resident cross_iteration_pi unless C3SC_HOST_CROSS is set).  A marker line on stderr after
    each of the first two parts; the nodal values of every result saved"""
    import ctypes as C
    import sys

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(LQR, 2, 2, ranks=(12,), name="lqr_jd_pi_api", njump=LQR_NJUMP, **LQR_MASKS)
    w = lqr_vi_workload(mid)
    L = fl.solver_lib()
    ctl = fl.Control(w, callbacks=H.lqr_callbacks(LQR_PRM), consistent_ends=None)
    keep = add_jumps(L, ctl, lqr_jumps, LQR_PRM, 2, LQR_NJUMP)
    aa = fl.approx_args(L)
    v0, keep2 = fl.init_value(L, ctl, aa, lambda xx: H.lqr_terminal(LQR_PRM, xx))
    n0, n1 = w.ngrid

    def pi(K):
        v = C.c_void_p(L.c3control_pi_solve(ctl.h, C.c_size_t(K), C.c_double(0.0), v0, aa, ctl.opt, C.c_int(0), None))
        return fl.nodal(L, v.value, n0, n1)

    def mark(line):
        sys.stdout.flush()
        sys.stderr.flush()
        os.write(2, (line + "\n").encode())  # unbuffered, in order with the library's own fprintf(stderr)

    before = [pi(K) for K in PI_BEFORE]
    mark(PI_MARKERS[0])
    v1 = C.c_void_p(L.c3control_vi_solve(ctl.h, C.c_size_t(1), C.c_double(0.0), v0, aa, ctl.opt, C.c_int(0), None))
    vi = fl.nodal(L, v1.value, n0, n1)
    mark(PI_MARKERS[1])
    after = [pi(K) for K in PI_AFTER]
    np.savez(out_path, V0=fl.nodal(L, v0.value, n0, n1), before=np.array(before), vi=vi, after=np.array(after))


def fh_child(out_path, delta=PUT_DELTA, nstages=PUT_STAGES):
    """Merton's American put through the reference API (run in a child process): c3control_fh_solve in stop and jump mode from
    the terminal value psi, V_s at every node of every stage saved"""
    import ctypes as C

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(PUT, 2, 1, ranks=(4, 8, 12), name="put_jd_api", horizon=True, stop=True, njump=PUT_NJUMP, **PUT_MASKS)
    w = put_workload(mid, rank=11)
    cbs, stop_cb = SL.put_callbacks(PUT_PRM)
    L, ctl, aa = fl.stop_control(w, cbs, stop_cb)
    keep = add_jumps(L, ctl, put_jumps, PUT_PRM, 2, PUT_NJUMP)
    vt, keep2 = fl.init_value(L, ctl, aa, lambda xx: SL.put_psi(PUT_PRM, xx))
    V = L.c3control_fh_solve(ctl.h, C.c_size_t(nstages), C.c_double(delta), vt, aa, ctl.opt, C.c_int(0))
    fl.save_stages(out_path, L, V, nstages, *w.ngrid)
