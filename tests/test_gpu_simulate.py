"""Batched closed-loop rollouts on the device (c3sc_hip_stencil_points, c3sc_hip_simulate; kernel_rollout.hpp) against the
oracle's restatement of the host tail: mca_get_neighbor_node_costs at off-grid states (nodeutil.c:718-816),
c3control_policy_eval (bellman.c:2105-2158) and the models' drift / diffusion / cost callbacks."""
import ctypes as C
import math

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _setup(w, cores, box=None):
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    if box is not None:
        eng.set_control_box(*box)
    return eng


def _oracle_fns(oracle, w):
    L = oracle.lib()
    prm = oracle.f64(list(w.params) if len(w.params) else [0.0])

    def call(name, x, u=None, n=1):
        out = np.zeros(n)
        xx = oracle.f64(x)
        if u is None:
            rc = getattr(L, name)(C.c_int(w.model), oracle.dp(prm), oracle.dp(xx), oracle.dp(out))
        else:
            rc = getattr(L, name)(C.c_int(w.model), oracle.dp(prm), oracle.dp(xx), oracle.dp(oracle.f64(u)), oracle.dp(out))
        assert rc == 0
        return out

    return dict(drift=lambda x, u: call("orc_model_drift", x, u, w.dx), diff=lambda x, u: call("orc_model_diff_diag", x, u, w.dx),
                stage=lambda x, u: call("orc_model_stage", x, u)[0], bound=lambda x: call("orc_model_boundcost", x)[0],
                obs=lambda x: call("orc_model_obscost", x)[0])


def _oracle_stencil(oracle, P, w, x):
    L = oracle.lib()
    gs = [oracle.f64(P.xgrid(m)) for m in range(w.dx)]
    out, ab = np.full(2 * w.dx + 1, np.nan), C.c_int(9)
    rc = L.orc_mca_get_neighbor_node_costs(C.c_size_t(w.dx), oracle.dp(oracle.f64(x)), P.boundary_handle(), P.vf.h,
                                           oracle.sp(oracle.usz(w.ngrid)), oracle.ptr_array(gs), C.byref(ab), oracle.dp(out))
    assert rc == 0
    return out, ab.value


def _oracle_value(oracle, P, w, x):
    L = oracle.lib()
    L.orc_valuef_eval.restype = C.c_double
    gs = [oracle.f64(P.xgrid(m)) for m in range(w.dx)]
    return float(L.orc_valuef_eval(P.vf.h, oracle.ptr_array(gs), oracle.dp(oracle.f64(x))))


def _oracle_policy(oracle, P, x):
    ui, val = C.c_int(-5), C.c_double(0.0)
    assert oracle.lib().orc_policy_eval(P.h, oracle.dp(oracle.f64(x)), C.byref(ui), C.byref(val)) == 0
    return ui.value


def _margins(oracle, w, cores):
    """best-to-second-best gap of the host controller at a state: the oracle's policy evaluation over each candidate alone"""
    Ps = [oracle.Problem(wl.Workload(w.name, w.model, w.params, w.dx, w.du, w.lb, w.ub, w.ngrid, w.ranks, w.discount, w.bc,
                                     list(w.obstacles), w.cands[c:c + 1]), cores) for c in range(w.ncand)]
    lib = oracle.lib()

    def margin(x):
        xx = oracle.f64(x)
        vals = []
        for P in Ps:
            ui, val = C.c_int(-5), C.c_double(0.0)
            assert lib.orc_policy_eval(P.h, oracle.dp(xx), C.byref(ui), C.byref(val)) == 0
            vals.append(val.value)
        v = np.sort(vals)
        return float(v[1] - v[0]) if len(v) > 1 else np.inf

    margin.problems = Ps
    return margin


def _wrap(w, x):
    y = np.array(x, dtype=np.float64)
    for m, b in enumerate(w.bc):
        if b == wl.BC_PERIODIC:
            lb, ub = w.lb[m], w.ub[m]
            L = ub - lb
            v = y[..., m] - np.floor((y[..., m] - lb) / L) * L
            v = np.where(v >= ub, v - L, v)
            y[..., m] = np.where(v < lb, v + L, v)
    return y


def _points(w, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(w.lb), np.array(w.ub)
    span = hi - lo
    pts = [lo + span * rng.uniform(-0.05, 1.05, w.dx) for _ in range(n)]  # some outside the domain
    h = span / (np.array(w.ngrid) - 1)
    for m in range(w.dx):  # near each face, on it, across it (periodic seam)
        for off in (-1.5, -0.5, -1e-9, 0.0, 0.3, 0.999, 1.0, 2.5):
            p = lo + span * rng.uniform(0.2, 0.8, w.dx)
            q = p.copy()
            p[m] = lo[m] + off * h[m]
            q[m] = hi[m] - off * h[m]
            pts += [p, q]
    for c, wd in w.obstacles:  # inside obstacles, on their faces
        c, wd = np.array(c), np.array(wd)
        pts += [c, c + wd / 2, c - wd / 2 * 0.999, c + wd / 2 * 1.001]
    return np.ascontiguousarray(pts, dtype=np.float64)


STENCIL_CASES = [("dubins3d", dict(ngrid=(21, 17, 16), rank=6)), ("car7d", dict(ngrid=(41,) * 7, rank=10)),
                 ("lqg2d", dict(ngrid=(51, 51), rank=4))]


@pytest.mark.parametrize("name,kw", STENCIL_CASES, ids=[c[0] for c in STENCIL_CASES])
def test_stencil_points_vs_oracle(oracle, name, kw):
    torch = _torch()
    w = wl.WORKLOADS[name]().scaled(**kw)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _setup(w, cores)
    X = _points(w, 300, 17)
    out, ab = eng.stencil_points(torch.from_numpy(X).cuda())
    torch.cuda.synchronize()
    out, ab = out.cpu().numpy(), ab.cpu().numpy()
    assert "k_stencil_points" in eng.last_kernel()
    for i, x in enumerate(X):
        want, wab = _oracle_stencil(oracle, P, w, x)
        assert ab[i] == wab, (i, x)
        if wab == 0:  # the host routine leaves entry 2d to its caller: the value at x itself
            want[2 * w.dx] = _oracle_value(oracle, P, w, x)
        scale = max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(out[i], want, rtol=1e-12, atol=1e-12 * scale, err_msg=f"point {i}: {x}")


def test_stencil_points_constelm_vs_host_rule(oracle):
    """CONSTELM: valuef_eval takes the nearer node of each cell (the oracle has no CONSTELM; restated here)"""
    torch = _torch()
    w = wl.c1_lqg2d().scaled(ngrid=(21, 21), rank=4)
    cores = wl.synth_cores(w)
    eng = _setup(w, cores)
    eng.set_interp(True)
    xg = w.xgrid()

    def veval(x):
        v = np.ones(1)
        for m in range(w.dx):
            g = xg[m]
            N = len(g)
            if x[m] <= g[0]:
                i, wt = 0, 0.0
            elif x[m] >= g[-1]:
                i, wt = N - 2, 1.0
            else:
                i = int(np.searchsorted(g, x[m], side="right") - 1)
                wt = (x[m] - g[i]) / (g[i + 1] - g[i])
            wt = 0.0 if wt < 0.5 else 1.0
            r0, r1 = w.ranks[m], w.ranks[m + 1]
            G = cores[m].reshape(N, r1, r0)
            v = v @ ((1 - wt) * G[i].T + wt * G[i + 1].T)
        return float(v[0])

    X = _points(w, 100, 3)
    out, ab = eng.stencil_points(torch.from_numpy(X).cuda())
    out = out.cpu().numpy()
    for i, x in enumerate(X):
        assert out[i, 2 * w.dx] == pytest.approx(veval(x), rel=1e-12, abs=1e-12)
        h = xg[0][1] - xg[0][0]
        if x[0] - h > w.lb[0] and x[0] + h < w.ub[0]:
            y = x.copy()
            y[0] -= h
            assert out[i, 0] == pytest.approx(veval(y), rel=1e-12, abs=1e-12)


def _x0(w, n, seed, frac=0.8):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(w.lb), np.array(w.ub)
    c, half = (lo + hi) / 2, (hi - lo) / 2 * frac
    return np.ascontiguousarray(c + half * rng.uniform(-1, 1, (n, w.dx)))


LOCKSTEP = [("dubins3d", dict(ngrid=(21, 17, 16), rank=6), True, 0.05), ("car7d", dict(ngrid=(21,) * 7, rank=10), False, 0.02),
            ("cothrust6d", dict(ngrid=(12,) * 6, rank=8), False, 0.01)]


@pytest.mark.parametrize("name,kw,wrap,dt", LOCKSTEP, ids=[c[0] for c in LOCKSTEP])
def test_lockstep_controller_and_dynamics(oracle, name, kw, wrap, dt):
    torch = _torch()
    w = wl.WORKLOADS[name]().scaled(**kw)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    fn = _oracle_fns(oracle, w)
    eng = _setup(w, cores)
    n, K = 256, 50
    x0 = _x0(w, n, 5)
    noise = np.random.default_rng(6).standard_normal((n, K, w.dx))
    r = eng.simulate(torch.from_numpy(x0).cuda(), dt, K, noise_t=torch.from_numpy(noise).cuda(), wrap_periodic=wrap, save_every=1)
    traj, U, ex = r["traj"].cpu().numpy(), r["u"].cpu().numpy(), r["exit"].cpu().numpy()
    assert "k_rollout" in eng.last_kernel()
    margin = _margins(oracle, w, cores)
    checked = ties = 0
    for i in range(n):
        last = K if ex[i] < 0 else ex[i]
        for k in range(last):
            x = traj[i, k]
            xin = _wrap(w, x) if wrap else x
            ui = _oracle_policy(oracle, P, xin)
            u_want = w.cands[ui] if ui >= 0 else np.zeros(w.du)
            checked += 1
            if not np.array_equal(U[i, k], u_want):
                # only where the host's best and second-best candidates are within 1e-9 of each other
                assert ui >= 0 and margin(xin) <= 1e-9, (i, k, x, U[i, k], u_want)
                ties += 1
                u_want = U[i, k]  # a tie: follow the device's choice for the dynamics check
            b, s = fn["drift"](x, u_want), fn["diff"](x, u_want)
            xn = (x + b * dt) + s * math.sqrt(dt) * noise[i, k]
            np.testing.assert_allclose(traj[i, k + 1], xn, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(xn).max())))
        for k in range(last, K):  # frozen after the exit
            assert np.array_equal(traj[i, k + 1], traj[i, last]) and not U[i, k].any()
    assert checked > n * 5


def test_lqg2d_deterministic_closed_loop_candidate_list(oracle):
    """zero noise: the lqg2d closed loop (examples/lqg2d_pi.c's set-up) against a host loop over the oracle's controller"""
    torch = _torch()
    w = wl.c1_lqg2d()
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    fn = _oracle_fns(oracle, w)
    n, K, dt = 8, 100, 1e-2
    x0 = _x0(w, n, 9, 0.7)
    zero = torch.zeros((n, K, w.dx), dtype=torch.float64).cuda()
    eng = _setup(w, cores)
    r = eng.simulate(torch.from_numpy(x0).cuda(), dt, K, noise_t=zero, save_every=1)
    traj, U = r["traj"].cpu().numpy(), r["u"].cpu().numpy()
    for i in range(n):
        x = x0[i].copy()
        for k in range(K):
            ui = _oracle_policy(oracle, P, x)
            u = w.cands[ui] if ui >= 0 else np.zeros(w.du)
            assert np.array_equal(U[i, k], u)
            x = x + fn["drift"](x, u) * dt
            np.testing.assert_allclose(traj[i, k + 1], x, rtol=1e-10, atol=1e-10)


def test_seed_mode_reproducible_split_and_matches_host_twin():
    torch = _torch()
    w = wl.c2_dubins().scaled(ngrid=(21, 17, 16), rank=6)
    cores = wl.synth_cores(w)
    eng = _setup(w, cores)
    n, K, dt = 300, 50, 0.02
    x0 = torch.from_numpy(_x0(w, n, 12)).cuda()
    a = eng.simulate(x0, dt, K, seed=77, wrap_periodic=True, save_every=1, steps_per_launch=16)
    b = eng.simulate(x0, dt, K, seed=77, wrap_periodic=True, save_every=1)
    for key in ("traj", "u", "cost", "exit", "vend", "xfinal"):
        assert torch.equal(a[key], b[key]), key
    lo = eng.simulate(x0[:100].contiguous(), dt, K, seed=77, wrap_periodic=True, save_every=1)
    hi = eng.simulate(x0[100:].contiguous(), dt, K, seed=77, wrap_periodic=True, save_every=1, traj_offset=100)
    for key in ("traj", "u", "cost", "exit", "vend"):
        assert torch.equal(torch.cat([lo[key], hi[key]]), a[key]), key
    z = torch.from_numpy(E.normals(77, 0, n, 0, K, w.dx)).cuda()
    c = eng.simulate(x0, dt, K, noise_t=z, wrap_periodic=True, save_every=1)
    np.testing.assert_allclose(c["traj"].cpu().numpy(), a["traj"].cpu().numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name,kw,wrap", [("dubins3d", dict(ngrid=(21, 17, 16), rank=6), True),
                                          ("lqg2d", dict(ngrid=(21, 21), rank=4), False)])
def test_cost_exit_and_value_recomputed(oracle, name, kw, wrap):
    torch = _torch()
    w = wl.WORKLOADS[name]().scaled(**kw)
    if name == "lqg2d":  # absorbing faces so that trajectories exit
        w.bc = (wl.BC_ABSORB, wl.BC_ABSORB)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    fn = _oracle_fns(oracle, w)
    eng = _setup(w, cores)
    n, K, dt = 256, 60, 0.05
    x0 = _x0(w, n, 21, 0.98)
    if w.obstacles:  # a few start inside the obstacle, a few just outside it
        c, wd = np.array(w.obstacles[0][0]), np.array(w.obstacles[0][1])
        x0[:8] = c + wd / 2 * np.random.default_rng(1).uniform(-0.9, 0.9, (8, w.dx))
        x0[8:16, 0] = c[0] + wd[0] / 2 + 0.02
    noise = 3.0 * np.random.default_rng(22).standard_normal((n, K, w.dx))  # strong noise: many exits
    r = eng.simulate(torch.from_numpy(x0).cuda(), dt, K, noise_t=torch.from_numpy(noise).cuda(), wrap_periodic=wrap, save_every=1)
    traj, U = r["traj"].cpu().numpy(), r["u"].cpu().numpy()
    J, ex, vend, xf = r["cost"].cpu().numpy(), r["exit"].cpu().numpy(), r["vend"].cpu().numpy(), r["xfinal"].cpu().numpy()
    lo, hi = np.array(w.lb), np.array(w.ub)
    absorb = np.array([b == wl.BC_ABSORB for b in w.bc])
    beta = w.discount
    n_exit_face = n_exit_obs = 0
    for i in range(n):
        e, Jw = -1, 0.0
        for k in range(K + 1):
            x = traj[i, k]
            inobs = P.bound.in_obstacle(x) == 1
            out = bool(np.any(absorb & ((x < lo) | (x > hi))))
            if inobs or out:
                e = k
                Jw += math.exp(-beta * k * dt) * (fn["obs"](x) if inobs else fn["bound"](x))
                n_exit_obs += inobs
                n_exit_face += (not inobs)
                break
            if k < K:
                Jw += math.exp(-beta * k * dt) * fn["stage"](x, U[i, k]) * dt
        assert ex[i] == e, i
        assert J[i] == pytest.approx(Jw, rel=1e-12, abs=1e-12)
        if e >= 0:
            assert (traj[i, e:] == traj[i, e]).all()
        xe = _wrap(w, xf[i]) if wrap else xf[i]
        np.testing.assert_array_equal(xf[i], traj[i, K])
        assert vend[i] == pytest.approx(_oracle_value(oracle, P, w, xe), rel=1e-12, abs=1e-12)
    assert n_exit_face > 0
    if w.obstacles:
        assert n_exit_obs > 0


def test_last_kernel_and_unsupported_requests():
    torch = _torch()
    w = wl.rossler3d().scaled(ngrid=(12, 12, 12), rank=4)  # Bellman kernels exist, no rollout instantiation
    eng = _setup(w, wl.synth_cores(w))
    x0 = torch.zeros((4, 3), dtype=torch.float64).cuda()
    with pytest.raises(E.C3scHipError, match="code 3"):
        eng.simulate(x0, 0.01, 10)
    # a model with rollouts, at a padded rank that only its Bellman kernels serve (cothrust6d: the fiber-pair kernel at 10)
    w = wl.cothrust6d().scaled(ngrid=(8,) * 6, rank=10)
    eng = _setup(w, wl.synth_cores(w))
    with pytest.raises(E.C3scHipError, match="code 3"):
        eng.simulate(torch.zeros((4, 6), dtype=torch.float64).cuda(), 0.01, 10)
    w = wl.c1_lqg2d().scaled(ngrid=(21, 21), rank=4)
    eng = _setup(w, wl.synth_cores(w))
    x0 = torch.zeros((4, 2), dtype=torch.float64).cuda()
    with pytest.raises(E.C3scHipError, match="code 1"):
        eng.simulate(x0, 0.0, 10)
    with pytest.raises(E.C3scHipError, match="code 1"):
        eng.simulate(x0, 0.01, 10, box=True)  # no control box set
    r = eng.simulate(x0, 0.01, 10, seed=3)
    torch.cuda.synchronize()
    assert eng.last_kernel().startswith("k_rollout<LqgNd<2>")
    assert torch.isfinite(r["cost"]).all()


# ---------------------------------------------------------------- the reference API: c3control_simulate_batch (libc3sc.so)
def _facade():
    import facade_lib

    L = facade_lib.lib()
    dpp = C.POINTER(C.c_double)
    L.c3control_simulate_batch.argtypes = [C.c_void_p, C.c_size_t, dpp, C.c_double, C.c_size_t, C.c_uint64, dpp, C.c_int, C.c_size_t,
                                           dpp, dpp, dpp, C.POINTER(C.c_long), dpp]
    L.c3control_simulate_batch.restype = C.c_int
    return L, facade_lib


def _cothrust_callbacks():
    """examples/cothrust2/copterposethrust.c:40-222 with the reference's signatures (features from u with libm)"""
    import facade_lib

    def drift(t, x, u, out, jac, args):
        m, g = 1.227, 9.81
        mg = m * g
        cphi, sphi, cth, sth = math.cos(u[1]), math.sin(u[1]), math.cos(u[2]), math.sin(u[2])
        out[0], out[1], out[2] = x[3], x[4], x[5]
        out[3] = cphi * sth * (u[0] - mg) / m
        out[4] = -sphi * (u[0] - mg) / m
        out[5] = g + cth * cphi * (u[0] - mg) / m
        return 0

    def diff(t, x, u, out, grad, args):
        for i in range(36):
            out[i] = 0.0
        for i, v in enumerate((1e-1, 1e-1, 2e-1, 12e-1, 12e-1, 12e-1)):
            out[7 * i] = v
        return 0

    def stage(t, x, u, out, grad):
        o = 0.0
        o = o + 60.0 + 2.0 * (u[0] * u[0]) + 1.0 * (u[1] * u[1]) + 6.0 * (u[2] * u[2])
        o = o + 8.0 * (x[2] * x[2])
        o = o + 6.0 * (x[1] * x[1])
        o = o + 8.0 * (x[0] * x[0])
        out[0] = o
        return 0

    def bcost(t, x, out):
        out[0] = 10.0
        return 0

    def ocost(x, out):
        out[0] = 0.0
        return 0

    return (facade_lib.DYN_FN(drift), facade_lib.DYN_FN(diff), facade_lib.STAGE_FN(stage), facade_lib.BOUND_FN(bcost),
            facade_lib.OBS_FN(ocost))


def _batch(L, fl, ctl, x0, dt, K, noise):
    n, d, du = x0.shape[0], ctl.w.dx, ctl.w.du
    traj, U = np.zeros((n, K + 1, d)), np.zeros((n, K, du))
    cost, vend = np.zeros(n), np.zeros(n)
    ex = np.zeros(n, dtype=np.int64)
    nz = fl.f64(noise) if noise is not None else None
    rc = L.c3control_simulate_batch(ctl.h, n, fl.dp(fl.f64(x0)), dt, K, 5, fl.dp(nz) if nz is not None else None, 0, 1, fl.dp(traj),
                                    fl.dp(U), fl.dp(cost), ex.ctypes.data_as(C.POINTER(C.c_long)), fl.dp(vend))
    assert rc == 0
    return traj, U, ex


BOX_CASES = [("lqg2d", dict(ngrid=(25, 23), rank=4), ([-1.0], [1.0]), 0.01),
             ("cothrust6d", dict(ngrid=(10,) * 6, rank=8), ([-1.5, -0.4, -0.4], [1.5, 0.4, 0.4]), 0.01)]


@pytest.mark.parametrize("name,kw,box,dt", BOX_CASES, ids=[c[0] for c in BOX_CASES])
def test_reference_api_box_minimiser_lockstep(name, kw, box, dt):
    """c3control_simulate_batch with a box opt_sim (the examples' BFGS set-up): every device control against the host
    c3control_policy_eval (host box minimiser over the user's callbacks) at the same state, every step against the host
    callbacks.  cothrust6d runs the box path whose candidate features are formed from u on the device."""
    from test_policy_tail import _lqg2d_callbacks

    L, fl = _facade()
    w = wl.WORKLOADS[name]().scaled(**kw)
    cbs = _lqg2d_callbacks() if name == "lqg2d" else _cothrust_callbacks()
    ctl = fl.Control(w, cbs, box=box, consistent_ends=None)
    cores = wl.synth_cores(w)
    vf = ctl.valuef(cores)
    L.valuef_attach_grid(vf, fl.ptrs([fl.f64(g) for g in ctl.xgrid()]))
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    n, K = 24, 12
    x0 = _x0(w, n, 31, 0.6)
    noise = np.random.default_rng(32).standard_normal((n, K, w.dx))
    traj, U, ex = _batch(L, fl, ctl, x0, dt, K, noise)
    width = (np.array(box[1]) - np.array(box[0]))
    checked, worst = 0, 0.0
    b_, s_, *_ = cbs
    for i in range(n):
        last = K if ex[i] < 0 else ex[i]
        for k in range(last):
            x = fl.f64(traj[i, k])
            u = np.zeros(w.du)
            assert L.c3control_policy_eval(ctl.h, C.c_double(0.0), fl.dp(x), fl.dp(u)) == 0
            checked += 1
            # the same grid cell and the same golden-section point up to the resolution of a minimum of a smooth objective: near
            # the optimum the objective is flat to O(du^2), so rounding-level differences of the device and host objectives
            # (device libm, FMA contraction) move the 40-step bracket by ~sqrt(eps) of the control range
            d = float((np.abs(U[i, k] - u) / width).max())
            worst = max(worst, d)
            assert d <= 1e-5, (i, k, x, U[i, k], u)
            b, sg = np.zeros(w.dx), np.zeros(w.dx * w.dx)
            uu = fl.f64(U[i, k])
            b_(0.0, fl.dp(x), fl.dp(uu), fl.dp(b), None, None)
            s_(0.0, fl.dp(x), fl.dp(uu), fl.dp(sg), None, None)
            xn = (x + b * dt) + np.diag(sg.reshape(w.dx, w.dx)) * math.sqrt(dt) * noise[i, k]
            np.testing.assert_allclose(traj[i, k + 1], xn, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(xn).max())))
    assert checked >= n * 4
    print(f"{name}: {checked} box controls, worst difference {worst:.2e} of the box width")
    L.valuef_destroy(vf)
    ctl.close()


def test_reference_api_matches_host_simulate_both_minimisers():
    """issue test 3: with zero noise, c3control_simulate_batch reproduces the host c3control_simulate (noise = NULL) of the
    lqg2d closed loop over 100 steps, under the candidate list and under the box minimiser"""
    from test_policy_tail import _lqg2d_callbacks

    L, fl = _facade()
    w = wl.c1_lqg2d()
    cores = wl.synth_cores(w)
    n, K, dt = 6, 100, 1e-2
    x0 = _x0(w, n, 9, 0.7)
    for box in (None, ([-1.0], [1.0])):
        ctl = fl.Control(w, _lqg2d_callbacks(), box=box, consistent_ends=None)
        vf = ctl.valuef(cores)
        L.valuef_attach_grid(vf, fl.ptrs([fl.f64(g) for g in ctl.xgrid()]))
        L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
        traj, U, ex = _batch(L, fl, ctl, x0, dt, K, np.zeros((n, K, w.dx)))
        for i in range(n):
            ht, hu = np.zeros((K + 1, w.dx)), np.zeros((K, w.du))
            assert L.c3control_simulate(ctl.h, fl.dp(fl.f64(x0[i])), C.c_double(dt), C.c_size_t(K), None, fl.dp(ht), fl.dp(hu)) == 0
            if box is None:  # the candidate list: the same candidates, the same states to rounding
                np.testing.assert_allclose(traj[i], ht, rtol=1e-10, atol=1e-10)
                np.testing.assert_array_equal(U[i], hu)
            else:  # the box minimiser resolves u to ~sqrt(eps) of its range (see the lock-step test above)
                np.testing.assert_allclose(traj[i], ht, rtol=1e-7, atol=1e-7)
                np.testing.assert_allclose(U[i], hu, rtol=0, atol=2e-5)
        L.valuef_destroy(vf)
        ctl.close()
