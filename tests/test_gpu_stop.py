"""Optimal stopping on the GPU (c3sc_hip_set_stopping).

- The L2 form of the rank-12 stop kernels, in both forms, on a 3-D grid whose 128-node middle core does not fit the LDS.
- The stop forms of the per-wave kernel against the numpy restatement of stop_lib on a ragged 21 x 70 grid (both NPL forms) with
  boundary, obstacle and periodic nodes: the stopping LQR and the put, ranks 4 and 8 (12 once: the rank that also has an L2 form), beta > 0 and
  beta = 0, infinite horizon and horizon.  Values to 1e-12 of the value scale; indices exactly, except where the reference's own
  margin |psi - continuation| is below 1e-9 relative (at most 2 % of the nodes); both decisions occur in every case.
- A psi that never wins: the stop kernel equals the plain kernel of the same model bit for bit, status included.
- The forced path reproduces the minimising run from its own indices, and a forced ncand gives psi.
- A node whose candidates are all stationary returns psi with the index ncand, and STATIONARY stays raised; in horizon mode CFL
  is raised exactly when a candidate violates the rule, whether or not stop wins.
- Rollouts: without noise a lane stops at the first step where stop_lib says stop on the off-grid stencil, pays the discounted
  stage costs plus the discounted psi there and decodes as (step, stopped = 1); lanes that start outside or leave through a
  face in mid-run decode as exits and pay the discounted boundary cost; in the
  infinite-horizon form and under a value stack.  With noise the mean cost of the put from three states estimates the dense
  chain's V_0 within 4 standard errors plus the discretisation bound pinned on the CPU.
- The stage-by-stage device solve of the put equals the dense chain to 1e-9.
- Through libc3sc.so in child processes: c3control_vi_solve of the stopping LQR sweep by sweep and c3control_fh_solve of the put
  equal the dense chains to 1e-9 (first-fiber check against the host twin, then the device-resident cross).
- Errors: built-in models, a model without stop kernels (also one set after the switch), the pair variant, the box and TABLE
  calls, cross_iteration_pi, integrate, set_game in either order."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import backup_ref as BR
import gpu_case_lib as GC
import horizon_lib as H
import stop_lib as SL

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 3
STATUS_STATIONARY, STATUS_CFL = 1, 2


@pytest.fixture(scope="module")
def ids():
    return {
        "lqr": E.compile_model(SL.LQR, 2, 2, ranks=(4, 8, 12), name="lqr_os", horizon=True, stop=True, **SL.LQR_MASKS),
        "put": E.compile_model(SL.PUT, 2, 1, ranks=(4, 8, 12), name="put_os", horizon=True, stop=True, **SL.PUT_MASKS),
        "put_never": E.compile_model(SL.PUT_NEVER, 2, 1, ranks=(4,), name="put_never", horizon=True, stop=True, **SL.PUT_MASKS),
        "lqr_nostop": E.compile_model(H.LQR, 2, 2, ranks=(4,), name="lqr_nostop", horizon=True, **H.LQR_MASKS),
        "lqr3": E.compile_model(SL.LQR3, 3, 3, ranks=(12,), name="lqr3_os", horizon=True, stop=True, **SL.LQR3_MASKS),
        "lqr_stop_only": E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_stop_only", stop=True, **SL.LQR_MASKS),
    }


def lqr_workload(mid, rank, discount, prm=SL.LQR_PRM):
    return wl.Workload("lqr_os", mid, tuple(prm), 2, 2, (-2.0, -2.0), (2.0, 2.0), (21, 70), wl.uniform_ranks(2, rank), discount,
                       (wl.BC_ABSORB, wl.BC_PERIODIC), [((0.9, -0.9), (0.5, 0.6))], SL.lqr_cands())


def lqr3_workload(mid, rank, discount):
    """three dimensions with a middle fiber of 128 nodes: at rank 12 its core (128 x 145 doubles) with the per-wave scratch and the
    table of 125 candidates exceeds the 160 KB of LDS, so a launch along dim 1 takes the L2 form of the per-wave kernel"""
    return wl.Workload("lqr3_os", mid, SL.LQR_PRM, 3, 3, (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (5, 128, 5), wl.uniform_ranks(3, rank),
                       discount, (wl.BC_ABSORB, wl.BC_PERIODIC, wl.BC_REFLECT), [((0.5, -0.9, 0.0), (1.2, 0.6, 1.2))], SL.lqr3_cands())


def put_workload(mid, rank, discount):
    return wl.Workload("put_os", mid, SL.PUT_PRM, 2, 1, (0.2, 0.2), (1.8, 1.8), (21, 70), wl.uniform_ranks(2, rank), discount,
                       (wl.BC_ABSORB, wl.BC_PERIODIC), [((1.3, 0.7), (0.3, 0.3))], SL.PUT_CANDS)


LQR_DELTA, PUT_DELTA_RAGGED, LQR3_DELTA = 0.01, 0.001, 0.004  # within the CFL rule of the ragged grids (Q delta / h^2 < 0.7)


def _lqr_bcost(x):
    return H.lqr_terminal(SL.LQR_PRM, x)


def _case(ids, model, rank, discount, horizon):
    """(engine with stopping on, workload, host twin, psi, boundary cost, obstacle cost, delta) of one case.  The inputs are
    chosen from the reference so that both decisions occur: the LQR's psi gets the constant c0 that puts it at the median of
    the continuation values; the put's value function (positive synthetic cores) is scaled to a mean of -0.4, inside psi's range"""
    delta = None
    if model in ("lqr", "lqr3"):
        w = lqr_workload(ids["lqr"], rank, discount) if model == "lqr" else lqr3_workload(ids["lqr3"], rank, discount)
        cores = wl.synth_cores(w)
        host, bcost, ocost = SL.lqrn_host, (lambda x: SL.lqrn_terminal(SL.LQR_PRM, x)), (lambda x: np.full(len(x), 5.0))
        if horizon:
            delta = LQR_DELTA if model == "lqr" else LQR3_DELTA
    else:
        w = put_workload(ids["put"], rank, discount)
        cores = wl.synth_cores(w)
        host = SL.put_host
        bcost = ocost = lambda x: SL.put_psi(SL.PUT_PRM, x)
        if horizon:
            delta = PUT_DELTA_RAGGED
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    k0 = 0 if model != "lqr3" else 1
    idx = wl.synth_fibers(w, k0, 64)
    costs, ab = eng.stencil_fibers_host(k0, idx)
    if model != "put":
        h2, t = BR.mca_constants(w)
        x = BR.node_states(w, k0, idx).reshape(-1, w.dx)
        vals, _, _ = BR.candidate_values(host, w.params, x, costs.reshape(-1, 2 * w.dx + 1), np.asarray(w.cands), h2, t, discount, delta=delta)
        cont = np.nanmin(vals, axis=1)[ab.reshape(-1) == 0]
        c1 = SL.LQR_PRM[5]
        c0 = float(np.median(cont - c1 * (x[ab.reshape(-1) == 0] ** 2).sum(-1)))
        w = dataclasses.replace(w, params=SL.LQR_PRM[:4] + (c0, c1))
        eng.set_model(w.model, w.params)
        eng.w = w
        psi = lambda xx: SL.lqr_psi(w.params, xx)
    else:
        scale = -0.4 / costs[..., 4].mean()
        cores = [cores[0] * scale, cores[1]]
        eng.upload_value(w.ranks, cores)
        psi = lambda xx: SL.put_psi(SL.PUT_PRM, xx)
    if delta is not None:
        eng.set_horizon_step(delta)
    eng.set_stopping(True)
    return eng, w, host, psi, bcost, ocost, delta


def _check_case(ids, model, rank, discount, horizon, ks=(0, 1)):
    eng, w, host, psi, bcost, ocost, delta = _case(ids, model, rank, discount, horizon)
    nc = w.ncand
    eng.status(clear=True)
    kernels = set()
    for k in ks:
        idx = wl.synth_fibers(w, k, 257)
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        kernels.add(eng.last_kernel())
        assert eng.last_kernel().startswith("k_fiber_per_wave<rtc:")
        costs, sab = eng.stencil_fibers_host(k, idx)
        np.testing.assert_array_equal(ab, sab)
        assert (ab == 1).any() and (ab == -1).any() and (ab == 0).any(), "fibers must include boundary, obstacle and live nodes"
        r_out, r_ui, mg, _, _ = SL.stop_fibers(w, host, psi, k, idx, costs, ab, bcost, ocost, delta)
        scale = np.maximum(1.0, np.abs(r_out))
        print(model, rank, discount, horizon, k, "max err", np.abs(out - r_out).max(), "stop share", (r_ui == nc).mean(),
              "unsure share", (mg <= 1e-9).mean())
        assert np.all(np.abs(out - r_out) <= 1e-12 * scale), (k, np.abs(out - r_out).max())
        sure = mg > 1e-9
        assert (~sure).mean() <= 0.02, "the reference's own decisions must be clear at 98 % of the nodes"
        np.testing.assert_array_equal(ui[sure], r_ui[sure])
        live = ab == 0
        assert (ui[live] == nc).any() and (ui[live] < nc).any(), "both decisions occur"
        assert (ui[live] >= 0).all() and (ui[~live] == -1).all()
        # the forced path: the minimising run's own indices reproduce its values; a forced ncand gives psi
        f_out, f_ab = eng.policy_fibers_host(k, idx, ui)
        np.testing.assert_array_equal(f_ab, ab)
        assert np.all(np.abs(f_out - out) <= 1e-12 * scale), (k, np.abs(f_out - out).max())
        s_out, _ = eng.policy_fibers_host(k, idx, np.full(ab.shape, nc, dtype=np.int32))
        x = BR.node_states(w, k, idx).reshape(-1, w.dx)
        p_ref = np.where(live.reshape(-1), psi(x), r_out.reshape(-1)).reshape(ab.shape)
        assert np.all(np.abs(s_out - p_ref) <= 1e-12 * np.maximum(1.0, np.abs(p_ref)))
        # a random forced candidate applies it and does not compare with psi
        rng = np.random.default_rng(rank + k)
        pol = rng.integers(0, nc, size=ab.shape).astype(np.int32)
        q_out, _ = eng.policy_fibers_host(k, idx, pol)
        q_ref, _, _, _, _ = SL.stop_fibers(w, host, psi, k, idx, costs, ab, bcost, ocost, delta, forced=pol)
        assert np.all(np.abs(q_out - q_ref) <= 1e-12 * np.maximum(1.0, np.abs(q_ref))), (k, np.abs(q_out - q_ref).max())
    if horizon:
        assert eng.status() & STATUS_CFL == 0
    return kernels


@pytest.mark.parametrize("model", ["lqr", "put"])
@pytest.mark.parametrize("rank", [4, 8])
@pytest.mark.parametrize("discount", [0.3, 0.0])
@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
def test_per_wave_stop_vs_numpy(ids, model, rank, discount, horizon):
    kernels = _check_case(ids, model, rank, discount, horizon)
    assert any(",1>" in k for k in kernels) and any(",2>" in k for k in kernels), kernels  # N = 21 and N = 70: both NPL forms


@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
def test_per_wave_stop_rank_12(ids, horizon):
    # the rank-12 stop forms.  Which of the two runs is the launcher's choice by LDS size (launch_fpw.hpp): in two dimensions both
    # cores are edge cores of N x 13 doubles, which always fit, so this is the staged form; the L2 form is compiled beside it
    # (tests/test_stop_build.py) for grids whose middle core does not fit
    kernels = _check_case(ids, "lqr", 12, 0.3, horizon)
    assert all(",12," in k for k in kernels), kernels


@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
def test_per_wave_stop_rank_12_l2_form(ids, horizon):
    """the L2 form of the rank-12 stop kernels: a launch along the 128-node middle dimension of a 3-D grid, whose staged layout
    needs more than the 160 KB the launcher stages in, so the kernel that reads the varying core from global memory runs"""
    w = lqr3_workload(ids["lqr3"], 12, 0.3)
    cw = 3 + 1 + 2 * 3 + 1  # CandLds row: u, one feature slot, the constant rates of three dimensions, their sum
    assert GC.fpw_lds_bytes(w, 1, 12, 2, cw) > 160 * 1024, "the staged form would fit: this case would not run the L2 form"
    assert GC.fpw_lds_bytes(w, 1, 12, 2, cw) - 8 * 128 * 145 < 160 * 1024  # ... and the L2 form's own layout fits
    kernels = _check_case(ids, "lqr3", 12, 0.3, horizon, ks=(1,))
    assert kernels == {"k_fiber_per_wave<rtc:lqr3_os,12,2>"}, kernels


@pytest.mark.parametrize("model", ["lqr", "put_never"])
@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
@pytest.mark.parametrize("discount", [0.3, 0.0])
def test_never_stopping_psi_equals_the_plain_kernel_bit_for_bit(ids, model, horizon, discount):
    if model == "lqr":
        w = lqr_workload(ids["lqr"], 4, discount, SL.LQR_NEVER_PRM)
        delta = LQR_DELTA
    else:
        w = put_workload(ids["put_never"], 4, discount)
        delta = PUT_DELTA_RAGGED
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    if horizon:
        eng.set_horizon_step(delta)
    for k in (0, 1):
        idx = wl.synth_fibers(w, k, 129)
        eng.set_stopping(False)
        eng.status(clear=True)
        p_out, p_ui, p_ab = eng.bellman_fibers_host(k, idx)
        p_kernel, p_st = eng.last_kernel(), eng.status(clear=True)
        eng.set_stopping(True)
        s_out, s_ui, s_ab = eng.bellman_fibers_host(k, idx)
        assert eng.last_kernel() == p_kernel  # the entry is the same; the launcher takes its stop form
        np.testing.assert_array_equal(s_out, p_out)
        np.testing.assert_array_equal(s_ui, p_ui)
        np.testing.assert_array_equal(s_ab, p_ab)
        assert eng.status(clear=True) == p_st


def test_all_stationary_node_returns_psi_and_keeps_the_bit(ids):
    """the put at S = (0, 0) on a reflecting grid: no drift and no diffusion, the one candidate is skipped"""
    w = wl.Workload("put_os", ids["put"], SL.PUT_PRM, 2, 1, (0.0, 0.0), (1.6, 1.6), (9, 9), wl.uniform_ranks(2, 4), 0.1,
                    (wl.BC_REFLECT, wl.BC_REFLECT), [], SL.PUT_CANDS)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    idx = np.zeros((1, 2), dtype=np.int32)
    eng.status(clear=True)
    out, ui, ab = eng.bellman_fibers_host(0, idx)  # plain: the node has no valid candidate, value 0 and index -1
    assert ab[0, 0] == 0 and ui[0, 0] == -1 and out[0, 0] == 0.0
    assert eng.status(clear=True) & STATUS_STATIONARY
    eng.set_stopping(True)
    out, ui, ab = eng.bellman_fibers_host(0, idx)
    assert ab[0, 0] == 0 and ui[0, 0] == w.ncand and out[0, 0] == -SL.PUT_K
    assert eng.status(clear=True) & STATUS_STATIONARY
    # a fiber without such a node raises nothing
    idx[0, 1] = 3
    out, ui, ab = eng.bellman_fibers_host(0, idx)
    assert eng.status(clear=True) & STATUS_STATIONARY == 0


def test_cfl_bit_is_the_scanned_candidates_alone(ids):
    for delta, flagged in ((LQR_DELTA, False), (2.0, True)):
        w = lqr_workload(ids["lqr"], 4, 0.1)
        eng = E.BellmanEngine(0)
        eng.configure(w, wl.synth_cores(w))
        eng.set_horizon_step(delta)
        eng.set_stopping(True)
        eng.status(clear=True)
        idx = wl.synth_fibers(w, 0, 64)
        out, ui, ab = eng.bellman_fibers_host(0, idx)
        costs, _ = eng.stencil_fibers_host(0, idx)
        psi = lambda xx: SL.lqr_psi(w.params, xx)
        r_out, r_ui, _, _, cfl = SL.stop_fibers(w, H.lqr_host, psi, 0, idx, costs, ab, _lqr_bcost, lambda x: np.full(len(x), 5.0), delta)
        assert bool(cfl.any()) == flagged
        assert bool(eng.status() & STATUS_CFL) == flagged
        if flagged:
            assert (cfl & (r_ui == w.ncand)).any(), "stop wins at nodes whose candidates violate the rule, and the bit stays"
        assert np.all(np.abs(out - r_out) <= 1e-12 * np.maximum(1.0, np.abs(r_out)))
    # stop alone raises nothing: with every candidate inside the rule a forced stop leaves the status clear
    eng.set_horizon_step(LQR_DELTA)
    eng.status(clear=True)
    eng.policy_fibers_host(0, idx, np.full(ab.shape, w.ncand, dtype=np.int32))
    assert eng.status() == 0


# ---------------------------------------------------------------------------------------------------- rollouts
def _stencil(G, xg, x):
    """the off-grid stencil on a grid whose dimensions both absorb (mca_get_neighbor_node_costs): the neighbours one spacing away,
    the face itself where that would leave the grid; every point is read inside the grid (the interpolant clamps)"""
    h = xg[1] - xg[0]
    c = lambda y: np.clip(y, xg[0], xg[-1])
    return np.stack([GC.interp(G, xg, c(x - [h, 0])), GC.interp(G, xg, c(x + [h, 0])), GC.interp(G, xg, c(x - [0, h])),
                     GC.interp(G, xg, c(x + [0, h])), GC.interp(G, xg, c(x))], axis=-1)


def _check_noise_free(r, n_inside, w, host, psi, stage_fn, drift_fn, stacks, xg, beta, dt, N, horizon, bcost, push=None):
    """every step of a run without random noise against stop_lib on the off-grid stencil.  stacks[k]: the nodal value the
    controller of step k reads (V_{k+1} under a stack, V itself otherwise); lanes n_inside.. start outside the grid; bcost: the
    cost of leaving through an absorbing face; push[n, N, 2]: a given displacement per step (sigma sqrt(dt) xi of the noise
    array handed to the device) that carries a lane out of the grid in mid-run.  Returns (step, stopped, sure decisions)"""
    traj, u, J = r["traj"].cpu().numpy(), r["u"].cpu().numpy(), r["cost"].cpu().numpy()
    step, stopped = E.decode_exit(r["exit"].cpu().numpy())
    assert (stopped[n_inside:] == 0).all() and (step[n_inside:] == 0).all(), "lanes that start outside decode as exits at step 0"
    h2, t = BR.mca_constants(w)
    Cn = np.asarray(w.cands, dtype=np.float64)
    nc = len(Cn)
    n = n_inside
    alive = np.ones(n, dtype=bool)
    exited = np.full(n, -1)
    Jref = np.zeros(n)
    sure_n = 0
    outside = lambda y: ((y < xg[0]) | (y > xg[-1])).any(axis=1)
    for k in range(N):
        xk = traj[:n, k]
        gone = alive & outside(xk)  # the exit test comes first: the lane pays the boundary cost there and is frozen
        Jref += np.where(gone, np.exp(-beta * k * dt) * bcost(xk), 0.0)
        exited[gone] = k
        alive = alive & ~gone
        S = _stencil(stacks[k], xg, xk)
        vals, _, _ = BR.candidate_values(host, w.params, xk, S, Cn, h2, t, beta, delta=dt if horizon else None)
        _, ui, mg = SL.stop_backup(vals, psi(xk))
        _, ci, cmg = BR.backup(np.where(np.isnan(vals), np.inf, vals))
        disc = np.exp(-beta * k * dt)
        dev_stop = alive & (stopped[:n] == 1) & (step[:n] == k)
        sure = alive & (mg > 1e-9)
        np.testing.assert_array_equal(dev_stop[sure], (ui == nc)[sure])
        sure_n += sure.sum()
        cont = alive & ~dev_stop
        okc = cont & (cmg > 1e-9)
        np.testing.assert_array_equal(u[:n][okc, k], Cn[ci[okc]])
        assert (u[:n][~cont, k] == 0.0).all(), "the saved controls of a stopped lane are 0"
        Jref += np.where(dev_stop, disc * psi(xk), 0.0) + np.where(cont, disc * stage_fn(xk, u[:n, k]) * dt, 0.0)
        xn = xk + drift_fn(xk, u[:n, k]) * dt
        if push is not None:
            xn = xn + push[:n, k]
        xn = np.where(cont[:, None], xn, xk)
        np.testing.assert_allclose(traj[:n, k + 1], xn, rtol=0, atol=1e-14)
        alive = cont
    gone = alive & outside(traj[:n, N])  # the final state is tested too
    Jref += np.where(gone, np.exp(-beta * N * dt) * bcost(traj[:n, N]), 0.0)
    exited[gone] = N
    alive = alive & ~gone
    left = exited >= 0
    np.testing.assert_array_equal(step[:n][left], exited[left])
    assert (stopped[:n][left] == 0).all(), "a lane that leaves through an absorbing face decodes as an exit"
    assert (step[:n][~alive & ~left] >= 0).all() and (stopped[:n][~alive & ~left] == 1).all()
    assert (step[:n][alive] == -1).all() and (stopped[:n][alive] == 0).all()
    if horizon:
        Jref += np.where(alive, np.exp(-beta * N * dt) * GC.interp(stacks[N], xg, traj[:n, N]), 0.0)
    np.testing.assert_allclose(J[:n], Jref, rtol=1e-12, atol=1e-12)
    return step[:n], stopped[:n], sure_n


def test_noise_free_rollouts_infinite_horizon(ids):
    """the stopping LQR under V = 0.8 |x|^2 + 0.3 with psi = 0.15 + 2.2 |x|^2: the controller steers towards the origin and stops
    once psi falls below the continuation value (about 0.36 + 1.6 |x|^2: inside |x| < 0.6 or so)"""
    import torch

    prm = SL.LQR_PRM[:4] + (0.15, 2.2)
    beta = 0.2
    w = dataclasses.replace(H.lqr_workload(ids["lqr"], rank=4, discount=beta), params=prm, cands=SL.lqr_cands())
    xg = w.xgrid()[0]
    X = np.stack(np.meshgrid(xg, xg, indexing="ij"), axis=-1)
    V = 0.8 * (X ** 2).sum(-1) + 0.3
    ranks, cores = GC.train(V, 4)
    eng = E.BellmanEngine(0)
    eng.configure(dataclasses.replace(w, ranks=tuple(ranks)), cores)
    eng.set_stopping(True)
    # lane 6 is carried towards the face x_0 = 2 by a given noise of +4 per step in dimension 0 (0.27 a step against a control of
    # 0.075 at most): it leaves the grid after a few steps and must decode as an exit there, charged the boundary cost
    x0 = np.array([[0.9, -0.5], [0.45, 0.8], [-0.7, 0.3], [0.1, 0.05], [-1.1, -1.0], [0.62, 0.0], [1.5, 0.1], [2.3, 0.0], [0.0, -2.4]])
    n_inside, N, dt = 7, 40, 0.05
    x0_t = torch.tensor(x0, dtype=torch.float64, device="cuda")
    xi = np.zeros((len(x0), N, 2))
    xi[6, :, 0] = 4.0
    noise = torch.tensor(xi, dtype=torch.float64, device="cuda")
    push = prm[0] * np.sqrt(dt) * xi
    r = eng.simulate(x0_t, dt, N, noise_t=noise, save_every=1)
    torch.cuda.synchronize()
    psi = lambda xx: SL.lqr_psi(prm, xx)
    stage = lambda xx, uu: prm[1] * (xx ** 2).sum(-1) + prm[2] * (uu ** 2).sum(-1)
    bcost = lambda xx: H.lqr_terminal(prm, xx)
    step, stopped, sure_n = _check_noise_free(r, n_inside, w, H.lqr_host, psi, stage, lambda xx, uu: uu, [V] * (N + 1), xg, beta, dt, N,
                                              False, bcost, push)
    print("stop steps", step, stopped)
    assert stopped[6] == 0 and 0 < step[6] < N, "the pushed lane leaves through the face in mid-run"
    assert bcost(r["traj"].cpu().numpy()[6:7, step[6]])[0] > 1.0  # ... where leaving costs something: J carries it
    assert stopped.sum() >= 3 and (step[stopped == 1] > 0).sum() >= 2 and (step[stopped == 1] == 0).any()
    assert sure_n >= 0.8 * stopped.size


@pytest.fixture(scope="module")
def put_solve(ids):
    """the put solved stage by stage on the device (stop and horizon forms, each stage uploaded as its exact train) and by the
    dense chain: (engine, device stages, dense stages, trains, workload)"""
    w = SL.put_workload(ids["put"], rank=11)
    psi = lambda x: SL.put_psi(SL.PUT_PRM, x)
    dense, dec, cfl = SL.dense_chain(w, SL.put_host, psi, SL.PUT_DELTA, SL.PUT_STAGES)
    assert not cfl
    eng = E.BellmanEngine(0)
    n = SL.PUT_N
    Vn = dense[-1]
    ranks, cores = GC.train(Vn, 12)
    eng.configure(dataclasses.replace(w, ranks=tuple(ranks)), cores)
    eng.set_horizon_step(SL.PUT_DELTA)
    eng.set_stopping(True)
    idx = np.zeros((n, 2), dtype=np.int32)
    idx[:, 1] = np.arange(n)
    dev, trains, uis = [Vn], [(ranks, cores)], []
    for _ in range(SL.PUT_STAGES):
        eng.upload_value(ranks, cores)
        out, ui, ab = eng.bellman_fibers_host(0, idx)  # fiber j along dim 0: out[j, i] = V_n(x_i, x_j)
        Vn = np.ascontiguousarray(out.T)
        dev.append(Vn)
        uis.append(np.ascontiguousarray(ui.T))
        ranks, cores = GC.train(Vn, 12)
        trains.append((ranks, cores))
    assert eng.status() == 0
    return eng, np.array(dev[::-1]), dense, trains[::-1], w, np.array(uis[::-1]), dec


def test_stage_by_stage_put_equals_the_dense_chain(put_solve):
    _, dev, dense, _, w, uis, dec = put_solve
    assert dev.shape == dense.shape
    for s in range(dev.shape[0]):
        err = np.abs(dev[s] - dense[s]).max() / max(1.0, np.abs(dense[s]).max())
        assert err <= 1e-9, (s, err)
    inner = (slice(1, -1), slice(1, -1))
    agree = ((uis[0] == w.ncand) == dec[0])[inner].mean()
    assert agree >= 0.98, agree
    assert (uis[0][inner] == w.ncand).mean() >= 0.10 and (uis[0][inner] == 0).mean() >= 0.10


def test_noise_free_rollouts_under_the_stack(put_solve):
    import torch

    eng, dev, dense, trains, w, _, _ = put_solve
    eng.upload_value_stack([t[0] for t in trains], [t[1] for t in trains])
    xg = w.xgrid()[0]
    m = np.array([0.62, 0.78, 0.86, 0.88, 0.90, 0.92, 0.94, 0.96, 1.0, 1.1])
    # the last inside lane starts just below the upper face of S_1 and drifts out of the grid after a few steps (r S dt a step)
    x0 = np.concatenate([np.stack([m + 0.03, m - 0.03], axis=-1), [[1.79, 0.5]], [[1.9, 1.0], [1.0, 0.1]]])
    n_inside, N, dt = len(m) + 1, SL.PUT_STAGES, SL.PUT_DELTA
    x0_t = torch.tensor(x0, dtype=torch.float64, device="cuda")
    noise = torch.zeros((len(x0), N, 2), dtype=torch.float64, device="cuda")
    r = eng.simulate(x0_t, dt, N, noise_t=noise, save_every=1)
    torch.cuda.synchronize()
    psi = lambda xx: SL.put_psi(SL.PUT_PRM, xx)
    stacks = [dev[k + 1] for k in range(N)] + [dev[N]]
    step, stopped, sure_n = _check_noise_free(r, n_inside, w, SL.put_host, psi, lambda xx, uu: np.zeros(len(xx)),
                                              lambda xx, uu: SL.PUT_R * xx, stacks, xg, SL.PUT_R, dt, N, True, psi)
    print("stop steps", step, stopped)
    assert (stopped == 1).any() and (stopped == 0).any() and (step[stopped == 1] == 0).any()
    assert stopped[-1] == 0 and 0 < step[-1] < N, "the lane near the upper face drifts out in mid-run and decodes as an exit"
    assert sure_n >= 0.8 * stopped.size
    assert eng.status() & STATUS_CFL == 0


def test_noisy_put_rollouts_estimate_v0(put_solve):
    import torch

    eng, dev, dense, trains, w, _, _ = put_solve
    eng.upload_value_stack([t[0] for t in trains], [t[1] for t in trains])
    xg = w.xgrid()[0]
    n = 8192
    for x0 in SL.PUT_X0:
        i, j = (int(np.argmin(np.abs(xg - v))) for v in x0)
        v0 = dense[0][i, j]
        x0_t = torch.tensor([x0] * n, dtype=torch.float64, device="cuda")
        r = eng.simulate(x0_t, SL.PUT_DELTA, SL.PUT_STAGES, seed=11)
        torch.cuda.synchronize()
        J = r["cost"].cpu().numpy()
        step, stopped = E.decode_exit(r["exit"].cpu().numpy())
        se = J.std() / np.sqrt(n)
        print("put rollouts", x0, "mean", J.mean(), "v0", v0, "se", se, "stopped", stopped.mean(), "exited", ((step >= 0) & (stopped == 0)).mean())
        assert abs(J.mean() - v0) <= 4 * se + SL.PUT_BOUND, (x0, J.mean(), v0, se)
    assert eng.status() & STATUS_CFL == 0


# ---------------------------------------------------------------------------------------------------- errors
def test_errors(ids):
    import torch

    L = E.load_library()
    # built-in model
    w = wl.c4_car7d().scaled(ngrid=(7,) * 7, rank=4)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    assert L.c3sc_hip_set_stopping(eng.h, 1) == ERR_UNSUPPORTED
    assert L.c3sc_hip_set_stopping(eng.h, 0) == 0
    # a run-time model compiled without stop kernels
    wp = lqr_workload(ids["lqr_nostop"], 4, 0.1)
    eng = E.BellmanEngine(0)
    eng.configure(wp, wl.synth_cores(wp))
    assert L.c3sc_hip_set_stopping(eng.h, 1) == ERR_UNSUPPORTED
    assert "stop kernels" in L.c3sc_hip_last_error(eng.h).decode()
    # the pair variant, integrate, the box and TABLE calls, policy iteration on the device, a game on top
    wr = lqr_workload(ids["lqr"], 4, 0.1)
    eng = E.BellmanEngine(0)
    eng.configure(wr, wl.synth_cores(wr))
    eng.set_stopping(True)
    eng.set_variant(E.VARIANT_FIBER_PAIR)
    idx = np.ascontiguousarray(wl.synth_fibers(wr, 0, 8), dtype=np.int32)
    out = np.empty((8, wr.ngrid[0]))
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    eng.set_variant(E.VARIANT_AUTO)
    x0 = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(E.C3scHipError, match="not offered for stopping problems"):
        eng.integrate(x0, 0.1, 3, method="rk4")
    tables = np.zeros((8, wr.ngrid[0], wr.ncand, 5))
    costs2 = np.zeros((8, wr.ngrid[0], 2))
    assert L.c3sc_hip_bellman_fibers_tables_host(eng.h, 0, 8, idx.ctypes.data, tables.ctypes.data, costs2.ctypes.data,
                                                 out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "stop" in L.c3sc_hip_last_error(eng.h).decode()
    L.c3sc_hip_bellman_fibers_box_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 4
    lb, ub = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    L.c3sc_hip_set_control_box.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    assert L.c3sc_hip_set_control_box(eng.h, 2, lb.ctypes.data, ub.ctypes.data, 5, 1) == 0
    assert L.c3sc_hip_bellman_fibers_box_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "stopping" in L.c3sc_hip_last_error(eng.h).decode()
    assert L.c3sc_hip_cross_iteration_pi(eng.h, eng.h, 1, None) == ERR_UNSUPPORTED
    assert "stopping" in L.c3sc_hip_last_error(eng.h).decode()
    U, W = np.array([[0.0]]), np.array([[1.0]])
    up, wp_ = U.ctypes.data_as(C.POINTER(C.c_double)), W.ctypes.data_as(C.POINTER(C.c_double))
    assert L.c3sc_hip_set_game(eng.h, 1, 1, up, 1, wp_, 0) == ERR_UNSUPPORTED
    assert "stopping" in L.c3sc_hip_last_error(eng.h).decode()
    # the horizon step on top needs a model compiled with both flags
    wo = lqr_workload(ids["lqr_stop_only"], 4, 0.1)
    eng2 = E.BellmanEngine(0)
    eng2.configure(wo, wl.synth_cores(wo))
    eng2.set_stopping(True)
    assert L.c3sc_hip_set_horizon_step(eng2.h, C.c_double(0.01)) == ERR_UNSUPPORTED
    # a model without stop kernels set after the switch: caught at launch
    eng.set_model(ids["lqr_nostop"], H.LQR_PRM)
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "stop kernels" in L.c3sc_hip_last_error(eng.h).decode()
    with pytest.raises(E.C3scHipError, match="stop kernels"):
        eng.simulate(x0, 0.02, 3)
    # game first, stopping second
    gid = E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_game_os", game=True, **SL.LQR_MASKS)
    wg = lqr_workload(gid, 4, 0.1)
    eng3 = E.BellmanEngine(0)
    eng3.configure(wg, wl.synth_cores(wg))
    eng3.set_game(np.array([[0.0], [1.0]]), np.array([[0.0], [0.5]]))
    assert L.c3sc_hip_set_stopping(eng3.h, 1) == ERR_UNSUPPORTED
    # switching it off restores the plain operator
    eng.set_model(ids["lqr"], SL.LQR_PRM)
    eng.set_stopping(False)
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == 0


# ---------------------------------------------------------------------------------------------------- the reference API
def test_vi_solve_through_the_reference_api(tmp_path):
    """the stopping LQR through libc3sc.so in a child process: c3control_vi_solve sweep by sweep (11 x 11, rank 11, host
    callbacks beside the stop model).  The first sweep passes the first-fiber check against the host twin, the next ones take the
    device-resident cross; every sweep equals the dense Markov-chain value iteration to 1e-9"""
    out = tmp_path / "vi.npz"
    r = GC.child(f"import stop_lib; stop_lib.vi_child({str(out)!r})")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "c3sc cross trace: speculate" in r.stderr  # the device-resident cross iterations ran
    V = np.load(out)["V"]
    w = SL.lqr_vi_workload(0)
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    dense, ui = SL.dense_vi(w, H.lqr_host, lambda x: SL.lqr_psi(SL.LQR_PRM, x), _lqr_bcost, H.lqr_terminal(SL.LQR_PRM, X),
                            SL.LQR_VI_SWEEPS)
    inner = ui[1:-1, 1:-1]
    assert (inner == w.ncand).any() and (inner < w.ncand).any(), "both decisions occur in the last sweep"
    assert V.shape == dense.shape
    for s in range(len(V)):
        err = np.abs(V[s] - dense[s]) / np.maximum(1.0, np.abs(dense[s]))
        assert err.max() <= 1e-9, (s, err.max())


def test_fh_solve_of_the_put_through_the_reference_api(tmp_path):
    """the American put through libc3sc.so in a child process: c3control_fh_solve in stop mode equals the dense chain stage by
    stage to 1e-9"""
    out = tmp_path / "fh.npz"
    r = GC.child(f"import stop_lib; stop_lib.fh_child({str(out)!r})")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "c3sc cross trace: speculate" in r.stderr
    V = np.load(out)["V"]
    w = SL.put_workload(0)
    dense, _, _ = SL.dense_chain(w, SL.put_host, lambda x: SL.put_psi(SL.PUT_PRM, x), SL.PUT_DELTA, SL.PUT_STAGES)
    assert V.shape == dense.shape
    for s in range(len(V)):
        err = np.abs(V[s] - dense[s]) / np.maximum(1.0, np.abs(dense[s]))
        assert err.max() <= 1e-9, (s, err.max())
