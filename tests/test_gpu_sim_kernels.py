"""Every registered instantiation of the closed-loop kernels (k_stencil_points, k_rollout, k_rollout_ode; kernel_rollout.hpp,
kernel_rollout_ode.hpp) with full-rank cores.  The rows come from tests/sim_kernel_cases.py, which test_sim_kernel_cases.py
holds to the C3SC_REG_* lines; every test asserts the kernel name it expects, so a fall-through to another instantiation
cannot pass.

  a. k_stencil_points against the longdouble reference of tests/offgrid_ref.py (pinned to the oracle on the CPU): positive and
     signed full-rank cores, grids of unequal N from {2, 3, 5, 33, 128}, points on nodes, faces, seams and one spacing from the
     faces; D = 2, 3, 7 once more as a CONSTELM value function, all 2D+1 entries.  |device - ref| <= 1e-12 Vabs per entry, a
     bound derived in offgrid_ref.py; flags bit-exact.
  b. k_rollout in lock-step with the oracle's controller and dynamics (the body of
     test_gpu_simulate.py::test_lockstep_controller_and_dynamics), and at each model's top class bit-identical results across
     launch cuts and batch splits.
  c. k_rollout_ode in lock-step with the host loop over the oracle's controller (the body of
     test_gpu_integrate.py::test_lockstep_one_outer_step_both_methods), which gives the D = 4 and D = 5 instantiations of the
     off-grid stencil their full-rank data."""
import math

import numpy as np
import pytest

import offgrid_ref as R
import sim_kernel_cases as S
from c3sc_amd import workloads as wl
from test_gpu_simulate import _margins, _oracle_fns, _oracle_policy, _setup, _wrap, _x0

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


# ------------------------------------------------------------------------------------------------------ a. k_stencil_points
@pytest.mark.parametrize("signed", [False, True], ids=["synth", "signed"])
@pytest.mark.parametrize("case", S.STENCIL, ids=S.case_id)
def test_stencil_points_vs_longdouble_reference(case, signed):
    torch = _torch()
    w = S.workload(case)
    cs = S.cores(case, w, signed)
    ref = R.OffgridRef(w, cs)
    eng = _setup(w, cs)
    X = S.stencil_points(w)
    for constelm in ((False, True) if case.key in S.CONSTELM_DIMS else (False,)):
        eng.set_interp(constelm)
        out, ab = eng.stencil_points(torch.from_numpy(X).cuda())
        torch.cuda.synchronize()
        out, ab = out.cpu().numpy(), ab.cpu().numpy()
        assert eng.last_kernel() == case.kernel
        worst, bad = 0.0, []
        for i, x in enumerate(X):
            V, Vabs, flag = ref.stencil(x, constelm)
            assert ab[i] == flag, (i, x)
            err = R.rel_err(out[i], V, Vabs)
            worst = max(worst, float(err.max()))
            if not (err <= R.TOL).all():
                bad.append((i, x, out[i], V.astype(np.float64), float(err.max())))
        print(f"{eng.last_kernel()} {'signed' if signed else 'synth'}{' constelm' if constelm else ''}: {len(X)} points, "
              f"worst |device - ref| / Vabs = {worst:.2e}")
        assert not bad, bad[:3]


# --------------------------------------------------------------------------------------------------------------- b. k_rollout
def _rollout_x0(case, w):
    x0 = _x0(w, case.opts["n"], 5)
    if case.opts["wrap"]:  # a few trajectories start several periods outside the periodic dimension
        for m, b in enumerate(w.bc):
            if b == wl.BC_PERIODIC:
                x0[:6, m] += (w.ub[m] - w.lb[m]) * np.array([-3.0, -2.0, 2.0, 3.0, 5.0, -7.0])
    return x0


@pytest.mark.parametrize("case", S.ROLLOUT, ids=S.case_id)
def test_rollout_lockstep_controller_and_dynamics(oracle, case):
    torch = _torch()
    w = S.workload(case)
    cs = S.cores(case, w)
    P = oracle.Problem(w, cs)
    fn = _oracle_fns(oracle, w)
    eng = _setup(w, cs)
    n, K, dt, wrap = case.opts["n"], case.opts["K"], case.opts["dt"], case.opts["wrap"]
    x0 = _rollout_x0(case, w)
    noise = np.random.default_rng(6).standard_normal((n, K, w.dx))
    r = _np(eng.simulate(torch.from_numpy(x0).cuda(), dt, K, noise_t=torch.from_numpy(noise).cuda(), wrap_periodic=wrap, save_every=1))
    traj, U, ex = r["traj"], r["u"], r["exit"]
    assert eng.last_kernel() == case.kernel
    margin = _margins(oracle, w, cs)
    checked = ties = 0
    worst = 0.0
    for i in range(n):
        assert np.array_equal(traj[i, 0], x0[i])
        last = K if ex[i] < 0 else ex[i]
        for k in range(last):
            x = traj[i, k]
            xin = _wrap(w, x) if wrap else x  # the controller sees the wrapped state, the dynamics the unwrapped one
            ui = _oracle_policy(oracle, P, xin)
            u_want = w.cands[ui] if ui >= 0 else np.zeros(w.du)
            checked += 1
            if not np.array_equal(U[i, k], u_want):
                # only where the host's best and second-best candidates are within 1e-9 of each other
                assert ui >= 0 and margin(xin) <= S.MARGIN_TOL, (i, k, x, U[i, k], u_want)
                ties += 1
                u_want = U[i, k]  # a tie: follow the device's choice for the dynamics check
            b, s = fn["drift"](x, u_want), fn["diff"](x, u_want)
            xn = (x + b * dt) + s * math.sqrt(dt) * noise[i, k]
            scale = max(1.0, float(np.abs(xn).max()))
            worst = max(worst, float(np.abs(traj[i, k + 1] - xn).max()) / scale)
            np.testing.assert_allclose(traj[i, k + 1], xn, rtol=1e-12, atol=1e-12 * scale)
        for k in range(last, K):  # frozen after the exit
            assert np.array_equal(traj[i, k + 1], traj[i, last]) and not U[i, k].any()
    print(f"{eng.last_kernel()}: {checked} controls checked, {ties} at a margin <= 1e-9 ({100.0 * ties / max(checked, 1):.2f} %), "
          f"{int((ex >= 0).sum())} of {n} exited, worst step error {worst:.2e}")
    assert checked > n * 5
    assert ties <= 0.05 * checked


@pytest.mark.parametrize("case", [c for c in S.ROLLOUT if c.opts.get("top")], ids=S.case_id)
def test_rollout_top_class_launch_cut_and_batch_split_bit_identical(case):
    """state goes through device memory between launches: where a kernel that spills would first differ"""
    torch = _torch()
    w = S.workload(case)
    eng = _setup(w, S.cores(case, w))
    n, K, dt, wrap = case.opts["n"], case.opts["K"], case.opts["dt"], case.opts["wrap"]
    x0 = torch.from_numpy(_rollout_x0(case, w)).cuda()
    whole = eng.simulate(x0, dt, K, seed=77, wrap_periodic=wrap, save_every=1)
    assert eng.last_kernel() == case.kernel
    cut = eng.simulate(x0, dt, K, seed=77, wrap_periodic=wrap, save_every=1, steps_per_launch=7)
    for key in ("traj", "u", "cost", "exit", "vend", "xfinal"):
        assert torch.equal(whole[key], cut[key]), key
    lo = eng.simulate(x0[:50].contiguous(), dt, K, seed=77, wrap_periodic=wrap, save_every=1)
    hi = eng.simulate(x0[50:].contiguous(), dt, K, seed=77, wrap_periodic=wrap, save_every=1, traj_offset=50, steps_per_launch=5)
    torch.cuda.synchronize()
    assert eng.last_kernel() == case.kernel
    for key in ("traj", "u", "cost", "exit", "vend", "xfinal"):
        assert torch.equal(torch.cat([lo[key], hi[key]]), whole[key]), key
    assert torch.isfinite(whole["cost"]).all() and bool((whole["traj"][:, 1] != whole["traj"][:, 0]).any())


# ----------------------------------------------------------------------------------------------------------- c. k_rollout_ode
@pytest.mark.parametrize("case", S.ODE, ids=S.case_id)
def test_ode_lockstep_one_outer_step_both_methods_full_rank(oracle, case):
    torch = _torch()
    n = case.opts["n"]
    eng = None
    for method in S.ODE_METHODS:
        w, cs, x0, rows = S.ode_reference(oracle, case, method)
        if eng is None:
            eng = _setup(w, cs)
        wrap = any(b == wl.BC_PERIODIC for b in w.bc)
        r = _np(eng.integrate(torch.from_numpy(x0).cuda(), S.ODE_DT_OUT, 1, method=method, dt_int=S.ODE_DT_OUT / 2, wrap_periodic=wrap,
                              save_every=1))
        assert eng.last_kernel() == case.kernel
        dropped = checked = 0
        worst = 0.0
        for i in range(n):
            assert (r["stop_step"][i] == 0) == (rows[i] is None), i
            if rows[i] is None:  # stopped at x_0 (an obstacle): nothing integrated
                np.testing.assert_array_equal(r["xfinal"][i], x0[i])
                continue
            xs, u0, J, worst_margin = rows[i]
            if worst_margin <= S.MARGIN_TOL:
                dropped += 1
                continue
            checked += 1
            np.testing.assert_array_equal(r["u"][i, 0], u0)
            if r["stop_step"][i] < 0:
                scale = max(1.0, float(np.abs(xs).max()))
                worst = max(worst, float(np.abs(r["xfinal"][i] - xs).max()) / scale)
                np.testing.assert_allclose(r["xfinal"][i], xs, rtol=1e-12, atol=1e-12 * scale)
                assert r["cost"][i] == pytest.approx(J, rel=1e-12, abs=1e-14)
        print(f"{eng.last_kernel()} {method}: {checked} states checked, {dropped} dropped (a stage margin <= 1e-9), "
              f"worst end-state error {worst:.2e}")
        assert dropped <= S.ODE_MAX_DROPPED * n and checked >= S.ODE_MIN_CHECKED * n
