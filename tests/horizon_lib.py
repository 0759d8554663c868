"""Finite-horizon problems (c3sc_hip_set_horizon_step): device sources of a decoupled 2-D LQR and a nonlinear
model, the explicit backup of the nodes of fibers and the dense explicit-chain recursion over a whole small grid (both
backup_ref's, with the horizon step delta) and the Riccati solution of the LQR.  Shared by the CPU and GPU tests and
tools/horizon_bench.py."""
import numpy as np

import backup_ref as BR

# decoupled 2-D LQR: x_i' = u_i, diffusion sig per dimension, stage q |x|^2 + r |u|^2, boundary (terminal) cost s |x|^2.
# prm = {sig, q, r, s}; s != q, so that P(t) and with it the optimal feedback change from stage to stage
LQR = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = u[0]; b[1] = u[1]; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[0]; s[1] = prm[0]; }
__device__ double stage(const double *prm, const double *x, const double *u)
{
    return prm[1] * (x[0] * x[0] + x[1] * x[1]) + prm[2] * (u[0] * u[0] + u[1] * u[1]);
}
__device__ double boundcost(const double *prm, const double *x) { return prm[3] * (x[0] * x[0] + x[1] * x[1]); }
__device__ double obscost(const double *prm, const double *x) { return 5.0; }
"""
LQR_MASKS = dict(udep_mask=0b11, uconst_mask=0b11, stage_udep=True)
LQR_PRM = (0.3, 1.0, 1.0, 2.0)


def lqr_host(prm, x, u):
    """numpy twin of LQR: (drift[..., 2], sigma[..., 2], stage[...]) for x[..., 2], u[..., 2]"""
    sig, q, r = prm[0], prm[1], prm[2]
    b = np.stack([u[..., 0], u[..., 1]], axis=-1) + 0.0 * x
    s = np.full(b.shape, sig)
    st = q * (x[..., 0] ** 2 + x[..., 1] ** 2) + r * (u[..., 0] ** 2 + u[..., 1] ** 2)
    return b, s, st


def lqr_terminal(prm, x):
    return prm[3] * (x[..., 0] ** 2 + x[..., 1] ** 2)


# nonlinear pendulum with a damping control: x0' = x1, x1' = -sin(x0) + u0 - c x1 u1, control-dependent diffusion in dim 1.
# prm = {sig0, sig1, c, r}; periodic in x0
PENDULUM = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = x[1]; b[1] = -sin(x[0]) + u[0] - prm[2] * x[1] * u[1]; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[0]; s[1] = prm[1] * (1.0 + 0.5 * u[1]); }
__device__ double stage(const double *prm, const double *x, const double *u)
{
    return (1.0 - cos(x[0])) + 0.1 * x[1] * x[1] + prm[3] * (u[0] * u[0] + u[1]);
}
__device__ double boundcost(const double *prm, const double *x) { return 10.0; }
__device__ double obscost(const double *prm, const double *x) { return 3.0; }
"""
PENDULUM_MASKS = dict(udep_mask=0b10, uconst_mask=0, stage_udep=True)
PENDULUM_PRM = (0.2, 0.3, 0.5, 0.2)


def pendulum_host(prm, x, u):
    s0, s1, c, r = prm[:4]
    b = np.stack([x[..., 1], -np.sin(x[..., 0]) + u[..., 0] - c * x[..., 1] * u[..., 1]], axis=-1)
    s = np.stack([np.full(b.shape[:-1], s0), s1 * (1.0 + 0.5 * u[..., 1])], axis=-1)
    st = (1.0 - np.cos(x[..., 0])) + 0.1 * x[..., 1] ** 2 + r * (u[..., 0] ** 2 + u[..., 1])
    return b, s, st


def horizon_backup(w, host, k, idx, costs, absorbed, delta, bcost, ocost, forced=None):
    """the explicit backup of every node of fibers idx from their stencils (costs [F, N, 2D+1], absorbed [F, N]); bcost, ocost:
    callables of x[P, D] (the model's boundary and obstacle costs).  Returns (value, index, margin, cfl) of shape [F, N]"""
    out, ui, mg, _, cfl = BR.fibers(w, host, k, idx, costs, absorbed, bcost, ocost, delta=delta, forced=forced)
    return out, ui, mg, cfl


# ---------------------------------------------------------------------------------------------------- the LQR problem
LQR_N = 11             # nodes per dimension of the solve (each stage uploaded as its exact train: SVD, numerical rank <= 8)
LQR_LB, LQR_UB = -2.0, 2.0
LQR_DELTA = 0.05       # horizon step; T = LQR_STAGES * LQR_DELTA
LQR_STAGES = 10
LQR_U = np.linspace(-1.5, 1.5, 13)
# bound on |V_0 - Riccati| at the interior nodes |x_i| <= LQR_INNER of the 11 x 11 dense chain (0.48 at beta = 0), pinned on the CPU
# (tests/test_horizon_host.py): the discretisation bound the GPU rollouts are held to as well
LQR_INNER = 0.8
LQR_BOUND = 0.6


def lqr_cands():
    return np.array([(a, b) for a in LQR_U for b in LQR_U])


def lqr_workload(mid, rank=11, discount=0.0, n=LQR_N):
    from c3sc_amd import workloads as wl

    return wl.Workload("lqr_fh", mid, LQR_PRM, 2, 2, (LQR_LB, LQR_LB), (LQR_UB, LQR_UB), (n, n), wl.uniform_ranks(2, rank),
                       discount, (wl.BC_ABSORB, wl.BC_ABSORB), [], lqr_cands())


def dense_chain(w, host, terminal, bcost, delta, nstages):
    """the explicit chain on the whole grid of a 2-D workload whose dimensions both absorb (the boundary nodes are absorbed and
    keep their boundary cost, every interior node's neighbours are grid nodes): V[s] for s = 0 .. nstages, V[nstages] =
    terminal at the nodes (bcost on the boundary); returns (V [nstages + 1, n0, n1], cfl seen)"""
    x, ab, _ = BR.grid2(w)
    V, _, _, anycfl, _ = BR.sweeps(w, host, np.where(ab, bcost(x), terminal(x)), bcost(x), nstages, delta=delta)
    return V[::-1].copy(), anycfl


def riccati(prm, T, beta=0.0, nsub=20000):
    """(P(0), c(0)) of the scalar LQR per dimension: -P' = q - P^2 / r - beta P, -c' = sig^2 P - beta c, P(T) = s, c(T) = 0
    (RK4 backward in time); V(0, x) = P |x|^2 + 2 c in 2-D"""
    sig, q, r, s = prm[:4]

    def f(y):
        P, c = y
        return np.array([q - P * P / r - beta * P, sig * sig * P - beta * c])

    y = np.array([s, 0.0])
    h = T / nsub
    for _ in range(nsub):
        k1 = f(y)
        k2 = f(y + 0.5 * h * k1)
        k3 = f(y + 0.5 * h * k2)
        k4 = f(y + h * k3)
        y = y + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return y[0], y[1]


def full_rank_train(V):
    """an exact 2-D train of the matrix V[n0, n1] (SVD, every singular value kept): (ranks, [core0 (n0, 1, r), core1 (n1, r, 1)])
    in upload_value's layout"""
    U, S, Vt = np.linalg.svd(V)
    r = len(S)
    c0 = (U[:, :r] * S[None, :r]).reshape(V.shape[0], 1, r)
    c1 = np.ascontiguousarray(Vt[:r, :].T).reshape(V.shape[1], r, 1)
    return [1, r, 1], [c0, c1]


# ---------------------------------------------------------------------------------------------------- the reference API
def lqr_callbacks(prm=LQR_PRM):
    """the host callbacks of LQR (what a C program passes to c3control_add_*), as ctypes function pointers"""
    import facade_lib as fl

    sig, q, r, s = prm[:4]

    def drift(t, x, u, out, jac, args):
        out[0], out[1] = u[0], u[1]
        return 0

    def diff(t, x, u, out, grad, args):
        out[0], out[1], out[2], out[3] = sig, 0.0, 0.0, sig
        return 0

    def stage(t, x, u, out, grad):
        out[0] = q * (x[0] * x[0] + x[1] * x[1]) + r * (u[0] * u[0] + u[1] * u[1])
        return 0

    def bcost(t, x, out):
        out[0] = s * (x[0] * x[0] + x[1] * x[1])
        return 0

    def ocost(x, out):
        out[0] = 5.0
        return 0

    return (fl.DYN_FN(drift), fl.DYN_FN(diff), fl.STAGE_FN(stage), fl.BOUND_FN(bcost), fl.OBS_FN(ocost))


def fh_child(out_path, delta=LQR_DELTA, nstages=LQR_STAGES):
    """the LQR through the reference API (run in a child process by tests/test_gpu_horizon.py): a run-time compiled horizon model
    beside the host callbacks, c3control_fh_solve from the terminal value s |x|^2 (an exact train), V_s at every node of every
    stage saved; None from the solve (a CFL stop) saves an empty array"""
    import ctypes as C

    import facade_lib as fl
    from c3sc_amd import engine as E

    mid = E.compile_model(LQR, 2, 2, ranks=(4, 8, 12), name="lqr_fh_api", horizon=True, **LQR_MASKS)
    w = lqr_workload(mid, rank=11)
    L = fl.solver_lib()
    ctl = fl.Control(w, callbacks=lqr_callbacks(), consistent_ends=None)
    aa = fl.approx_args(L)
    vt, keep = fl.init_value(L, ctl, aa, lambda xx: lqr_terminal(LQR_PRM, xx))
    V = L.c3control_fh_solve(ctl.h, C.c_size_t(nstages), C.c_double(delta), vt, aa, ctl.opt, C.c_int(0))
    fl.save_stages(out_path, L, V, nstages, *w.ngrid)
