"""Finite-horizon problems on the GPU (c3sc_hip_set_horizon_step, c3sc_hip_upload_value_stack).

- The horizon per-wave kernel against the numpy restatement of horizon_lib on random fibers with boundary, obstacle and periodic
  nodes: the 2-D LQR and the nonlinear pendulum, ranks 4 and 8, beta > 0 and beta = 0.  Values to 1e-12 relative, indices
  wherever the winning margin exceeds 1e-9 relative.  The forced path (policy evaluation) applies the given index.
- A candidate that violates the CFL rule raises C3SC_STATUS_CFL; at a step within the rule the bit stays clear.
- A stage-by-stage solve of the LQR on the 11 x 11 grid (the uploaded value is the exact train of V_{n+1}) equals the dense
  explicit chain stage by stage to 1e-9.
- Rollouts under the stack V_0 .. V_N from several start states: with nsteps = 0 the cost is V_0(x_0); over the whole horizon the
  mean J matches V_0(x_0) within 4 standard errors plus the discretisation bound pinned on the CPU.
- Errors: built-in models, a model without horizon kernels, the pair variant, integrate, simulate without a stack, with another
  dt or with too many steps."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import backup_ref as BR
import gpu_case_lib as GC
import horizon_lib as H

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 3
STATUS_CFL = 2


@pytest.fixture(scope="module")
def ids():
    return {
        "lqr": E.compile_model(H.LQR, 2, 2, ranks=(4, 8), name="lqr_fh", horizon=True, **H.LQR_MASKS),
        "pendulum": E.compile_model(H.PENDULUM, 2, 2, ranks=(4, 8), name="pendulum_fh", horizon=True, **H.PENDULUM_MASKS),
        "lqr_plain": E.compile_model(H.LQR, 2, 2, ranks=(4,), name="lqr_nofh", **H.LQR_MASKS),
    }


PEND_U = np.array([(a, b) for a in np.linspace(-1.0, 1.0, 7) for b in (0.0, 0.5, 1.0)])


def lqr_random_workload(mid, rank, discount):
    return wl.Workload("lqr_fh", mid, H.LQR_PRM, 2, 2, (-2.0, -2.0), (2.0, 2.0), (21, 19), wl.uniform_ranks(2, rank), discount,
                       (wl.BC_ABSORB, wl.BC_PERIODIC), [((0.9, -0.9), (0.5, 0.6))], H.lqr_cands())


def pendulum_workload(mid, rank, discount):
    return wl.Workload("pendulum_fh", mid, H.PENDULUM_PRM, 2, 2, (-np.pi, -3.0), (np.pi, 3.0), (23, 21), wl.uniform_ranks(2, rank),
                       discount, (wl.BC_PERIODIC, wl.BC_ABSORB), [((0.5, 1.0), (0.6, 0.8))], PEND_U)


def _lqr_bcost(x):
    return H.lqr_terminal(H.LQR_PRM, x)


CASES = [("lqr", lqr_random_workload, H.lqr_host, _lqr_bcost, lambda x: np.full(len(x), 5.0), 0.02),
         ("pendulum", pendulum_workload, H.pendulum_host, lambda x: np.full(len(x), 10.0), lambda x: np.full(len(x), 3.0), 0.02)]


def _engine(w, delta):
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    eng.set_horizon_step(delta)
    return eng


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("rank", [4, 8])
@pytest.mark.parametrize("discount", [0.3, 0.0])
def test_per_wave_horizon_vs_numpy(ids, case, rank, discount):
    name, mk, host, bcost, ocost, delta = case
    w = mk(ids[name], rank, discount)
    eng = _engine(w, delta)
    rng = np.random.default_rng(rank)
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, 257)
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        assert eng.last_kernel().startswith("k_fiber_per_wave<rtc:")
        costs, sab = eng.stencil_fibers_host(k, idx)
        np.testing.assert_array_equal(ab, sab)
        assert (ab == 1).any() and (ab == -1).any() and (ab == 0).any(), "fibers must include boundary, obstacle and live nodes"
        r_out, r_ui, mg, _ = H.horizon_backup(w, host, k, idx, costs, ab, delta, bcost, ocost)
        scale = np.maximum(1.0, np.abs(r_out))
        assert np.all(np.abs(out - r_out) <= 1e-12 * scale), (k, np.abs(out - r_out).max())
        sure = mg > 1e-9
        assert sure.mean() > 0.5
        np.testing.assert_array_equal(ui[sure], r_ui[sure])
        # the forced path: a random candidate per node
        pol = rng.integers(0, w.ncand, size=ab.shape).astype(np.int32)
        f_out, f_ab = eng.policy_fibers_host(k, idx, pol)
        np.testing.assert_array_equal(f_ab, ab)
        p_out, _, _, _ = H.horizon_backup(w, host, k, idx, costs, ab, delta, bcost, ocost, forced=pol)
        assert np.all(np.abs(f_out - p_out) <= 1e-12 * np.maximum(1.0, np.abs(p_out))), (k, np.abs(f_out - p_out).max())
    assert eng.status() & STATUS_CFL == 0


def test_cfl_violation_raises_the_status_bit(ids):
    w = lqr_random_workload(ids["lqr"], 4, 0.1)
    h2, t = BR.mca_constants(w)
    for delta, flagged in ((0.02, False), (2.0, True)):
        eng = _engine(w, delta)
        eng.status(clear=True)
        idx = wl.synth_fibers(w, 0, 64)
        out, ui, ab = eng.bellman_fibers_host(0, idx)
        costs, _ = eng.stencil_fibers_host(0, idx)
        r_out, _, _, cfl = H.horizon_backup(w, H.lqr_host, 0, idx, costs, ab, delta, _lqr_bcost, lambda x: np.full(len(x), 5.0))
        assert bool(cfl.any()) == flagged
        assert bool(eng.status() & STATUS_CFL) == flagged
        # the violating candidates still took part: the values are the formula's
        assert np.all(np.abs(out - r_out) <= 1e-12 * np.maximum(1.0, np.abs(r_out)))


@pytest.fixture(scope="module")
def lqr_solve(ids):
    """the LQR solved stage by stage on the device and by the dense chain: (engine, device stages, dense stages, trains)"""
    w = H.lqr_workload(ids["lqr"], rank=8)
    term = lambda x: H.lqr_terminal(H.LQR_PRM, x)
    dense, cfl = H.dense_chain(w, H.lqr_host, term, term, H.LQR_DELTA, H.LQR_STAGES)
    assert not cfl
    eng = E.BellmanEngine(0)
    n = H.LQR_N
    Vn = dense[-1]
    ranks, cores = GC.train(Vn, 8)
    eng.configure(dataclasses.replace(w, ranks=tuple(ranks)), cores)
    eng.set_horizon_step(H.LQR_DELTA)
    idx = np.zeros((n, 2), dtype=np.int32)
    idx[:, 1] = np.arange(n)
    dev = [Vn]
    trains = [(ranks, cores)]
    for _ in range(H.LQR_STAGES):
        eng.upload_value(ranks, cores)
        out, ui, ab = eng.bellman_fibers_host(0, idx)  # fiber j along dim 0: out[j, i] = V_n(x_i, x_j)
        Vn = np.ascontiguousarray(out.T)
        dev.append(Vn)
        ranks, cores = GC.train(Vn, 8)
        trains.append((ranks, cores))
    assert eng.status() == 0
    return eng, np.array(dev[::-1]), dense, trains[::-1]


def test_stage_by_stage_solve_equals_the_dense_chain(lqr_solve):
    _, dev, dense, _ = lqr_solve
    assert dev.shape == dense.shape
    for s in range(dev.shape[0]):
        err = np.abs(dev[s] - dense[s]).max() / max(1.0, np.abs(dense[s]).max())
        assert err <= 1e-9, (s, err)


X0S = [(0.0, 0.0), (0.4, -0.4), (0.8, 0.0)]


def test_rollouts_under_the_stack_estimate_v0(lqr_solve):
    import torch

    eng, dev, dense, trains = lqr_solve
    eng.upload_value_stack([t[0] for t in trains], [t[1] for t in trains])
    xg = H.lqr_workload(0).xgrid()[0]
    n = 8192
    for x0 in X0S:
        i, j = (int(np.argmin(np.abs(xg - v))) for v in x0)
        v0 = dense[0][i, j]
        x0_t = torch.tensor([x0] * n, dtype=torch.float64, device="cuda")
        # no step: the cost is the terminal interpolant of V_0 at x_0 (a node: the device stage's value there)
        r0 = eng.simulate(x0_t, H.LQR_DELTA, 0, seed=3)
        torch.cuda.synchronize()
        assert np.allclose(r0["cost"].cpu().numpy(), dev[0][i, j], rtol=1e-10, atol=1e-10)
        assert np.allclose(r0["vend"].cpu().numpy(), dev[0][i, j], rtol=1e-10, atol=1e-10)
        r = eng.simulate(x0_t, H.LQR_DELTA, H.LQR_STAGES, seed=11)
        torch.cuda.synchronize()
        J = r["cost"].cpu().numpy()
        ex = r["exit"].cpu().numpy()
        assert (ex < 0).mean() > 0.99, "trajectories should stay inside the domain"
        se = J.std() / np.sqrt(n)
        assert abs(J.mean() - v0) <= 4 * se + H.LQR_BOUND, (x0, J.mean(), v0, se)
    assert eng.status() & STATUS_CFL == 0


def test_errors(ids, lqr_solve):
    import torch

    L = E.load_library()
    # built-in model
    w = wl.c4_car7d().scaled(ngrid=(7,) * 7, rank=4)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    assert L.c3sc_hip_set_horizon_step(eng.h, C.c_double(0.1)) == ERR_UNSUPPORTED
    # a run-time model compiled without horizon kernels
    wp = lqr_random_workload(ids["lqr_plain"], 4, 0.1)
    eng = E.BellmanEngine(0)
    eng.configure(wp, wl.synth_cores(wp))
    assert L.c3sc_hip_set_horizon_step(eng.h, C.c_double(0.1)) == ERR_UNSUPPORTED
    assert L.c3sc_hip_set_horizon_step(eng.h, C.c_double(-1.0)) == ERR_ARG
    assert L.c3sc_hip_set_horizon_step(eng.h, C.c_double(0.0)) == 0
    # the pair variant and integrate in horizon mode
    wr = lqr_random_workload(ids["lqr"], 4, 0.1)
    eng = _engine(wr, 0.02)
    eng.set_variant(E.VARIANT_FIBER_PAIR)
    idx = np.ascontiguousarray(wl.synth_fibers(wr, 0, 8), dtype=np.int32)
    out = np.empty((8, wr.ngrid[0]))
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    eng.set_variant(E.VARIANT_AUTO)
    x0 = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(E.C3scHipError, match="not offered in horizon mode"):
        eng.integrate(x0, 0.1, 3, method="rk4")
    # the box calls, the TABLE path, policy iteration on the device, a game on top, a model without horizon kernels set later
    out8 = np.empty((8, wr.ngrid[0]))
    tables = np.zeros((8, wr.ngrid[0], wr.ncand, 5))
    costs2 = np.zeros((8, wr.ngrid[0], 2))
    assert L.c3sc_hip_bellman_fibers_tables_host(eng.h, 0, 8, idx.ctypes.data, tables.ctypes.data, costs2.ctypes.data,
                                                 out8.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "horizon" in L.c3sc_hip_last_error(eng.h).decode()
    L.c3sc_hip_bellman_fibers_box_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 4
    lb, ub = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    L.c3sc_hip_set_control_box.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    assert L.c3sc_hip_set_control_box(eng.h, 2, lb.ctypes.data, ub.ctypes.data, 5, 1) == 0
    assert L.c3sc_hip_bellman_fibers_box_host(eng.h, 0, 8, idx.ctypes.data, out8.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "horizon" in L.c3sc_hip_last_error(eng.h).decode()
    L.c3sc_hip_cross_iteration_pi.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    assert L.c3sc_hip_cross_iteration_pi(eng.h, eng.h, 1, None) == ERR_UNSUPPORTED
    assert "horizon" in L.c3sc_hip_last_error(eng.h).decode()
    U, W = np.array([[0.0]]), np.array([[1.0]])
    assert L.c3sc_hip_set_game(eng.h, 1, 1, U.ctypes.data_as(C.POINTER(C.c_double)), 1, W.ctypes.data_as(C.POINTER(C.c_double)),
                               0) == ERR_UNSUPPORTED
    # simulate: no stack, then another dt and too many steps
    with pytest.raises(E.C3scHipError, match="stack"):
        eng.simulate(x0, 0.02, 3)
    eng.set_model(ids["lqr_plain"], H.LQR_PRM)
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "horizon kernels" in L.c3sc_hip_last_error(eng.h).decode()
    seng, _, _, trains = lqr_solve
    seng.upload_value_stack([t[0] for t in trains], [t[1] for t in trains])
    with pytest.raises(E.C3scHipError, match="dt must equal"):
        seng.simulate(x0, 2 * H.LQR_DELTA, 3)
    with pytest.raises(E.C3scHipError, match="exceeds the value stack"):
        seng.simulate(x0, H.LQR_DELTA, H.LQR_STAGES + 1)
    # clearing horizon mode restores the plain operator
    seng.set_horizon_step(0.0)
    assert L.c3sc_hip_set_horizon_step(seng.h, C.c_double(H.LQR_DELTA)) == 0


def test_noise_free_rollouts_apply_the_stage_policy_and_pay_v_n(lqr_solve):
    """without noise every step is checkable: the control of step k is the explicit scheme's argmin over the stencil of V_{k+1}
    at x_k, and J is the discounted stage costs plus V_N(x_N).  LQR_PRM has s != q, so the stages' policies differ"""
    import torch

    eng, dev, dense, trains = lqr_solve
    eng.upload_value_stack([t[0] for t in trains], [t[1] for t in trains])
    w = H.lqr_workload(0)
    xg = w.xgrid()[0]
    h = xg[1] - xg[0]
    h2, t = BR.mca_constants(w)
    C2 = H.lqr_cands()
    x0 = np.array([[0.8, -0.4], [0.4, 0.75], [-0.7, 0.3], [0.55, 0.55]])
    n, N = len(x0), H.LQR_STAGES
    x0_t = torch.tensor(x0, dtype=torch.float64, device="cuda")
    noise = torch.zeros((n, N, 2), dtype=torch.float64, device="cuda")
    r = eng.simulate(x0_t, H.LQR_DELTA, N, noise_t=noise, save_every=1)
    torch.cuda.synchronize()
    traj, u, J = r["traj"].cpu().numpy(), r["u"].cpu().numpy(), r["cost"].cpu().numpy()
    assert (r["exit"].cpu().numpy() < 0).all()
    sure = differ = 0
    for k in range(N):
        xk = traj[:, k]
        S = np.stack([GC.interp(dev[k + 1], xg, xk - [h, 0]), GC.interp(dev[k + 1], xg, xk + [h, 0]),
                      GC.interp(dev[k + 1], xg, xk - [0, h]), GC.interp(dev[k + 1], xg, xk + [0, h]), GC.interp(dev[k + 1], xg, xk)], axis=-1)
        vals, _, _ = BR.candidate_values(H.lqr_host, H.LQR_PRM, xk, S, C2, h2, t, 0.0, delta=H.LQR_DELTA)
        _, ui, mg = BR.backup(vals)
        ok = mg > 1e-9
        np.testing.assert_array_equal(u[ok, k], C2[ui[ok]])
        sure += ok.sum()
        # the policy of another stage would have chosen differently somewhere: the stage index is tested
        S0 = np.stack([GC.interp(dev[0], xg, xk - [h, 0]), GC.interp(dev[0], xg, xk + [h, 0]), GC.interp(dev[0], xg, xk - [0, h]),
                       GC.interp(dev[0], xg, xk + [0, h]), GC.interp(dev[0], xg, xk)], axis=-1)
        v0, _, _ = BR.candidate_values(H.lqr_host, H.LQR_PRM, xk, S0, C2, h2, t, 0.0, delta=H.LQR_DELTA)
        differ += (BR.backup(v0)[1] != ui).sum()
        np.testing.assert_allclose(traj[:, k + 1], xk + u[:, k] * H.LQR_DELTA, rtol=0, atol=1e-14)
    assert sure >= 0.8 * n * N and differ > 0
    stage = H.LQR_PRM[1] * (traj[:, :N] ** 2).sum(-1) + H.LQR_PRM[2] * (u ** 2).sum(-1)
    ref = (stage * H.LQR_DELTA).sum(axis=1) + GC.interp(dev[N], xg, traj[:, N])
    np.testing.assert_allclose(J, ref, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["vend"].cpu().numpy(), GC.interp(dev[N], xg, traj[:, N]), rtol=1e-12, atol=1e-12)
    # and V_{N-1} at the end would be a different number: the terminal stage is tested
    assert np.abs(GC.interp(dev[N - 1], xg, traj[:, N]) - GC.interp(dev[N], xg, traj[:, N])).min() > 1e-6


def test_fh_solve_through_the_reference_api(tmp_path):
    """the LQR through libc3sc.so in a child process: c3control_fh_solve (11 x 11, rank 11, host callbacks beside the horizon
    model).  The first stage passes the first-fiber check against the host twin, the next ones take the device-resident cross
    (c3sc_hip_cross_iteration with its node memo); every stage equals the dense explicit chain to 1e-9"""
    out = tmp_path / "fh.npz"
    r = GC.child(f"import horizon_lib; horizon_lib.fh_child({str(out)!r})")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "c3sc cross trace: speculate" in r.stderr  # the device-resident cross iterations ran
    V = np.load(out)["V"]
    w = H.lqr_workload(0)
    term = lambda x: H.lqr_terminal(H.LQR_PRM, x)
    dense, _ = H.dense_chain(w, H.lqr_host, term, term, H.LQR_DELTA, H.LQR_STAGES)
    assert V.shape == dense.shape
    for s in range(len(V)):
        err = np.abs(V[s] - dense[s]) / np.maximum(1.0, np.abs(dense[s]))
        assert err.max() <= 1e-9, (s, err.max())


def test_fh_solve_stops_on_cfl(tmp_path):
    out = tmp_path / "fh_cfl.npz"
    r = GC.child(f"import horizon_lib; horizon_lib.fh_child({str(out)!r}, delta=2.0, nstages=2)")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert np.load(out)["V"].size == 0
    assert "C3SC_STATUS_CFL" in r.stderr
