"""Run-time compiled device models on the GPU (c3sc_hip_model_compile).

- A restatement of the built-in Chain<4> with its masks gives the built-in kernels' bits: per-wave Bellman outputs, argmins and
  absorbed flags, and closed-loop integration with forward Euler and RK4.
- Restated Dubins car (device sin / cos) and lqg2d agree with the oracle to 1e-12, one case with more than 64 KB of staged LDS;
  lqg2d's box minimiser agrees with the built-in box kernel and, through the reference API, with the host
  c3control_policy_eval; a box-compiled model's closed loops serve candidate lists too.
- A problem with no built-in functor (the damped pendulum) equals the TABLE path over the same physics evaluated in numpy, and
  its closed loops are consistent: forward Euler with one substep is c3sc_hip_simulate without noise, x1 = x0 + h b(x0, u0).
- Through the reference API (examples/pendulum_rtc.c over libc3sc.so): value iteration with the run-time id passes the
  first-fiber check, takes the device-resident cross and reaches the tolerance the TABLE path reaches; closed-loop batches
  accept the id; a source that disagrees with the host callbacks stops bellman_vi.
- Errors: an uncompiled rank, the pair / quad variants, an unknown id."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
from rtc_models import (CHAIN4, CHAIN4_MASKS, DUBINS3D, DUBINS3D_MASKS, LQG2D, LQG2D_MASKS, PENDULUM, PENDULUM_MASKS,
                        PENDULUM_PRM, build_example, pendulum_host)

pytestmark = pytest.mark.gpu
ERR_ARG = 1  # C3SC_ERR_ARG


@pytest.fixture(scope="module")
def ids():
    return {
        "chain4": E.compile_model(CHAIN4, 4, 1, ranks=(4,), name="chain4", **CHAIN4_MASKS),
        "dubins": E.compile_model(DUBINS3D, 3, 1, ranks=(4, 12), name="dubins", **DUBINS3D_MASKS),
        "lqg2d": E.compile_model(LQG2D, 2, 1, ranks=(4,), box=True, name="lqg2d", **LQG2D_MASKS),
        "pendulum": E.compile_model(PENDULUM, 2, 1, ranks=(4,), name="pendulum", **PENDULUM_MASKS),
    }


def _engine(w, cores, variant=E.VARIANT_FIBER_PER_WAVE):
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    eng.set_variant(variant)
    return eng


def chain4():
    return wl.Workload("chain4", wl.MODEL_CHAIN, (4.0, 1.0, 0.5, 1.0), 4, 1, (-2.0,) * 4, (2.0,) * 4, (9, 10, 11, 12),
                       wl.uniform_ranks(4, 4), 0.1, (wl.BC_REFLECT,) * 4, [], np.array([[-1.0], [0.0], [1.0]]))


def pendulum():
    return wl.Workload("pendulum", 0, PENDULUM_PRM, 2, 1, (-np.pi, -6.0), (np.pi, 6.0), (41, 37), wl.uniform_ranks(2, 4), 0.5,
                       (wl.BC_PERIODIC, wl.BC_ABSORB), [], np.linspace(-2.0, 2.0, 9).reshape(-1, 1))


def _x0(w, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.array(w.lb), np.array(w.ub)
    return lo + (hi - lo) * (0.1 + 0.8 * rng.random((n, w.dx)))


def test_chain4_bitwise_equal_to_the_builtin(ids):
    import torch

    w = chain4()
    cores = wl.synth_cores(w)
    ref = _engine(w, cores)
    rtc = _engine(dataclasses.replace(w, model=ids["chain4"]), cores)
    for k in range(4):
        idx = wl.synth_fibers(w, k, 300)
        a, b = ref.bellman_fibers_host(k, idx), rtc.bellman_fibers_host(k, idx)
        assert ref.last_kernel() == "k_fiber_per_wave<Chain<4>,4,1>"
        assert rtc.last_kernel() == "k_fiber_per_wave<rtc:chain4,4,1>"
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    x0 = torch.tensor(_x0(w, 1000, 1), device="cuda")
    for method in ("euler", "rk4"):
        ra = ref.integrate(x0, 0.05, 40, method=method, dt_int=0.025, save_every=4)
        rb = rtc.integrate(x0, 0.05, 40, method=method, dt_int=0.025, save_every=4)
        assert "Chain<4>" in ref.last_kernel() and rtc.last_kernel() == "k_rollout_ode<rtc:chain4,4>"
        for key in ra:
            assert torch.equal(ra[key], rb[key]), (method, key)


def _oracle_parity(oracle, w, rid, rank, ngrid, F=200):
    w = w.scaled(ngrid=ngrid, rank=rank)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _engine(dataclasses.replace(w, model=rid), cores, E.VARIANT_AUTO)
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, F)
        ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        assert eng.status() == 0
        assert "rtc:" in eng.last_kernel()
        np.testing.assert_array_equal(ab, ref_ab)
        scale = np.abs(ref).max()
        assert np.abs(out - ref).max() <= 1e-12 * scale, (w.name, k)
        bad = ui != ref_ui
        assert not bad.any() or np.abs(out - ref)[bad].max() <= 1e-12 * scale
    return eng


def test_dubins_vs_oracle(oracle, ids):
    _oracle_parity(oracle, wl.c2_dubins(), ids["dubins"], 4, (21, 17, 16))


def test_dubins_vs_oracle_staged_lds_above_64k(oracle, ids):
    w = wl.c2_dubins()
    # middle dimension: N = 70 nodes of 12 x 12 (stride 145) staged, two nodes per lane: 4 * 184 + 70 * 145 + 3 * 5 doubles
    lds = (4 * (4 * 12 + 2 * 3 * 12 + 64 * 2) + 70 * 145 + 3 * 5) * 8
    assert 64 * 1024 < lds <= 160 * 1024
    eng = _oracle_parity(oracle, w, ids["dubins"], 12, (20, 70, 16), F=150)
    assert eng.last_kernel() == "k_fiber_per_wave<rtc:dubins,12,1>"  # k = 2 ran last (N = 16)


def test_lqg2d_vs_oracle_and_box_vs_builtin(oracle, ids):
    _oracle_parity(oracle, wl.c1_lqg2d(), ids["lqg2d"], 4, (51, 47))
    w = wl.c1_lqg2d().scaled(ngrid=(51, 47), rank=4)
    cores = wl.synth_cores(w)
    ref = _engine(w, cores)
    rtc = _engine(dataclasses.replace(w, model=ids["lqg2d"]), cores)
    for e in (ref, rtc):
        e.set_control_box([-1.0], [1.0], grid=33, polish=2)
    for k in range(2):
        idx = wl.synth_fibers(w, k, 100)
        ov, uv, av = ref.bellman_fibers_box_host(k, idx)
        rv, ru, ra = rtc.bellman_fibers_box_host(k, idx)
        assert "rtc:lqg2d" in rtc.last_kernel()
        np.testing.assert_array_equal(av, ra)
        live = av == 0
        assert np.abs(ru - uv)[live].max() <= 1e-5 * 2.0
        assert np.abs(rv - ov).max() <= 1e-9 * np.abs(ov).max()


def _agree(a_u, b_u, a_x, b_x):
    """trajectories whose controls agree at every saved step have the same states: lanes differ only where a near-tie of two
    candidates (the built-in's stage cost is summed in another order) picks the other candidate"""
    same = (a_u == b_u).all(axis=(1, 2))
    assert same.mean() >= 0.9, same.mean()
    np.testing.assert_allclose(a_x[same], b_x[same], rtol=0, atol=1e-12)


def test_box_compiled_model_serves_candidate_lists_in_closed_loops(ids):
    """spec.box adds the box kernels: the rollout and integrate kernels it compiles (BOX = true) serve candidate lists too, as
    the built-in LqgNd<2>'s do.  Integrate (RK4) and zero-noise simulate of the box-compiled lqg2d with a candidate list against
    the built-in, then the box itself."""
    import torch

    w = wl.c1_lqg2d().scaled(ngrid=(51, 47), rank=4)
    cores = wl.synth_cores(w)
    ref = _engine(w, cores)
    rtc = _engine(dataclasses.replace(w, model=ids["lqg2d"]), cores)
    n, nout = 1000, 25
    x0 = torch.tensor(_x0(w, n, 11), device="cuda")
    ra = ref.integrate(x0, 0.02, nout, method="rk4", dt_int=0.01, save_every=1)
    rb = rtc.integrate(x0, 0.02, nout, method="rk4", dt_int=0.01, save_every=1)
    assert rtc.last_kernel() == "k_rollout_ode<rtc:lqg2d,4>"
    _agree(ra["u"].cpu().numpy(), rb["u"].cpu().numpy(), ra["traj"].cpu().numpy(), rb["traj"].cpu().numpy())
    zero = torch.zeros((n, nout, 2), dtype=torch.float64, device="cuda")
    sa = ref.simulate(x0, 0.02, nout, noise_t=zero, save_every=1)
    sb = rtc.simulate(x0, 0.02, nout, noise_t=zero, save_every=1)
    assert rtc.last_kernel() == "k_rollout<rtc:lqg2d,4>"
    _agree(sa["u"].cpu().numpy(), sb["u"].cpu().numpy(), sa["traj"].cpu().numpy(), sb["traj"].cpu().numpy())
    for e in (ref, rtc):
        e.set_control_box([-1.0], [1.0], grid=33, polish=2)
    ia = ref.integrate(x0, 0.02, 5, method="rk4", dt_int=0.01, box=True, save_every=1)
    ib = rtc.integrate(x0, 0.02, 5, method="rk4", dt_int=0.01, box=True, save_every=1)
    assert np.abs(ia["u"].cpu().numpy() - ib["u"].cpu().numpy()).max() <= 1e-5 * 2.0


def test_box_minimiser_vs_the_host_policy_eval(ids):
    """The box-compiled lqg2d through the reference API: c3control_simulate_batch with a box opt_sim, every device control
    against the host c3control_policy_eval (the host box minimiser over the user's callbacks) at the same state, to 1e-5 of the
    box width (tests/test_gpu_simulate.py's lock-step check, with the run-time model as the device model)."""
    import ctypes as C

    from test_gpu_simulate import _batch, _facade
    from test_gpu_simulate import _x0 as sim_x0
    from test_policy_tail import _lqg2d_callbacks

    L, fl = _facade()
    w = dataclasses.replace(wl.c1_lqg2d().scaled(ngrid=(25, 23), rank=4), model=ids["lqg2d"])
    box = ([-1.0], [1.0])
    ctl = fl.Control(w, _lqg2d_callbacks(), box=box, consistent_ends=None)
    vf = ctl.valuef(wl.synth_cores(w))
    L.valuef_attach_grid(vf, fl.ptrs([fl.f64(g) for g in ctl.xgrid()]))
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    n, K = 24, 12
    x0 = sim_x0(w, n, 31, 0.6)
    traj, U, ex = _batch(L, fl, ctl, x0, 0.01, K, np.random.default_rng(32).standard_normal((n, K, w.dx)))
    checked = 0
    for i in range(n):
        for k in range(K if ex[i] < 0 else ex[i]):
            x, u = fl.f64(traj[i, k]), np.zeros(w.du)
            assert L.c3control_policy_eval(ctl.h, C.c_double(0.0), fl.dp(x), fl.dp(u)) == 0
            assert float(np.abs(U[i, k] - u).max()) / 2.0 <= 1e-5, (i, k, U[i, k], u)
            checked += 1
    assert checked >= n * 4
    L.valuef_destroy(vf)
    ctl.close()


def _pendulum_tables(w, k, idx):
    xg = w.xgrid()
    F, N = idx.shape[0], w.ngrid[k]
    x = np.empty((F, N, 2))
    for m in range(2):
        x[:, :, m] = xg[m][np.arange(N)][None, :] if m == k else xg[m][idx[:, m]][:, None]
    U = w.cands.shape[0]
    xx = np.broadcast_to(x[:, :, None, :], (F, N, U, 2))
    uu = np.broadcast_to(w.cands[None, None, :, :], (F, N, U, 1))
    b, s, st = pendulum_host(w.params, xx, uu)
    tables = np.concatenate([b, s, st[..., None]], axis=-1)
    costs2 = np.stack([np.full((F, N), 50.0), np.zeros((F, N))], axis=-1)
    return tables, costs2


def test_pendulum_equals_the_table_path(ids):
    w = pendulum()
    cores = wl.synth_cores(w)
    tab = _engine(dataclasses.replace(w, model=wl.MODEL_LQGND), cores, E.VARIANT_AUTO)  # any model: the table path sets its own
    rtc = _engine(dataclasses.replace(w, model=ids["pendulum"]), cores, E.VARIANT_AUTO)
    for k in range(2):
        idx = wl.synth_fibers(w, k, 300)
        tables, costs2 = _pendulum_tables(w, k, idx)
        t_out, t_ui, t_ab = tab.bellman_fibers_tables_host(k, idx, tables, costs2)
        out, ui, ab = rtc.bellman_fibers_host(k, idx)
        assert rtc.last_kernel() == "k_fiber_per_wave<rtc:pendulum,4,1>"
        np.testing.assert_array_equal(ab, t_ab)
        scale = np.abs(t_out).max()
        assert np.abs(out - t_out).max() <= 1e-12 * scale, k
        bad = ui != t_ui
        assert not bad.any() or np.abs(out - t_out)[bad].max() <= 1e-12 * scale


def test_pendulum_closed_loops(ids):
    import torch

    w = pendulum()
    cores = wl.synth_cores(w)
    eng = _engine(dataclasses.replace(w, model=ids["pendulum"]), cores)
    n, h, nout = 2000, 0.01, 30
    x0 = torch.tensor(_x0(w, n, 7), device="cuda")
    ie = eng.integrate(x0, h, nout, method="euler", dt_int=h, save_every=1)
    assert eng.last_kernel() == "k_rollout_ode<rtc:pendulum,4>"
    sim = eng.simulate(x0, h, nout, noise_t=torch.zeros((n, nout, 2), dtype=torch.float64, device="cuda"), save_every=1)
    assert eng.last_kernel() == "k_rollout<rtc:pendulum,4>"
    assert torch.equal(ie["traj"], sim["traj"]) and torch.equal(ie["u"], sim["u"])
    assert torch.equal(ie["cost"], sim["cost"])
    # one forward-Euler step against numpy with the saved control
    traj, u = ie["traj"].cpu().numpy(), ie["u"].cpu().numpy()
    b, _, _ = pendulum_host(w.params, traj[:, 0, :], u[:, 0, :])
    run = ie["stop_step"].cpu().numpy()
    live = (run < 0) | (run >= 1)
    np.testing.assert_allclose(traj[live, 1, :], (traj[:, 0, :] + h * b)[live], rtol=1e-13, atol=1e-13)
    # stops at constructed states: beyond the absorbing rate bound (face), in the goal box, left the keep-in box, none
    xs = torch.tensor([[0.5, 6.5], [0.0, 0.05], [0.5, 0.0], [-1.0, 0.0]], dtype=torch.float64, device="cuda")
    st = eng.integrate(xs, h, 5, method="rk4", dt_int=h / 2, goal=([-0.1, -0.1], [0.1, 0.1]), keep_in=([-0.8, -7.0], [4.0, 7.0]))
    stop, why = st["stop_step"].cpu().numpy(), st["stop_reason"].cpu().numpy()
    assert list(stop) == [0, 0, -1, 0] and list(why) == [1, 3, 0, 4], (stop, why)


def test_errors(ids):
    import ctypes as C

    w = pendulum().scaled(rank=8)
    cores = wl.synth_cores(w)
    eng = E.BellmanEngine(0)
    eng.configure(dataclasses.replace(w, model=wl.MODEL_LQGND), cores)  # rank 8 exists for other d = 2 models
    eng.set_model(ids["pendulum"], PENDULUM_PRM)  # compiled at rank 4 only
    idx = wl.synth_fibers(w, 0, 10)
    with pytest.raises(E.C3scHipError, match=r"code 3"):
        eng.bellman_fibers_host(0, idx)
    w4 = pendulum()
    eng4 = _engine(dataclasses.replace(w4, model=ids["pendulum"]), wl.synth_cores(w4), E.VARIANT_FIBER_PAIR)
    with pytest.raises(E.C3scHipError, match=r"code 3"):
        eng4.bellman_fibers_host(0, wl.synth_fibers(w4, 0, 10))
    eng4.set_variant(E.VARIANT_FIBER_QUAD)
    with pytest.raises(E.C3scHipError, match=r"code 3"):
        eng4.bellman_fibers_host(0, wl.synth_fibers(w4, 0, 10))
    p = (C.c_double * 1)(0.0)
    assert eng4.L.c3sc_hip_set_model(eng4.h, 1999, p, 0) == ERR_ARG


def test_vi_solve_through_the_reference_api(tmp_path):
    exe = build_example(tmp_path)
    env = dict(os.environ, C3SC_CROSS_TRACE="1")
    runs = {}
    for mode in ("rtc", "table"):
        p = subprocess.run([exe, "41", "30", mode], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        print(mode, p.stdout[-1500:], p.stderr[-1500:])
        assert p.returncode == 0 and "PENDULUM_RTC_OK" in p.stdout, mode
        m = re.search(r"value iteration: (\d+) sweeps, relative change ([^,\s]+), \|V\| = ([^,\s]+)", p.stdout)
        runs[mode] = (int(m.group(1)), float(m.group(2)), float(m.group(3)), p.stderr)
    # the device-resident cross iterations (c3sc_interp_device) trace their speculation set-up; the TABLE path never runs them
    assert "c3sc cross trace: speculate" in runs["rtc"][3] and "c3sc cross trace: speculate" not in runs["table"][3]
    assert "does not reproduce" not in runs["rtc"][3]
    # the same sweeps reach the same value function and the same change per sweep (the tolerance of the solve)
    assert runs["rtc"][0] == runs["table"][0]
    assert abs(runs["rtc"][1] - runs["table"][1]) <= 0.05 * runs["table"][1] + 1e-12
    assert abs(runs["rtc"][2] - runs["table"][2]) <= 1e-6 * runs["table"][2]


def test_a_source_that_disagrees_with_the_callbacks_stops_bellman_vi(tmp_path):
    exe = build_example(tmp_path)
    p = subprocess.run([exe, "21", "3", "wrong"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert p.returncode == 1, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    assert "does not reproduce the host callbacks" in p.stderr
