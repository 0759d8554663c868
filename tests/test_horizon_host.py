"""Finite-horizon problems, host side: no GPU is needed.

- horizon_lib's vectorised restatement of the explicit backup agrees with a plain per-candidate loop over the operator as the
  header states it, at beta > 0 and beta = 0, on every node of a grid of random stencils.
- Q = 0 ("stay") candidates are neither skipped nor flagged, and can win; Q delta > h^2 flags CFL and still takes part.
- libc3sc.so's host twin of the scan (c3control_set_horizon_step, then c3control_policy_eval over a nodal value function) picks
  the numpy argmin at every interior node of an 11 x 11 grid, at beta > 0 and beta = 0, and keeps a Q = 0 "stay" candidate.
- Policy iteration stops with a message in horizon mode (child processes).
- The dense explicit chain of the LQR on the 11 x 11 grid matches the Riccati solution V = P(t) |x|^2 + c(t) at the interior
  nodes within horizon_lib.LQR_BOUND: this pins the discretisation the GPU rollouts are held to."""
import dataclasses
import math
import os

import numpy as np
import pytest

import backup_ref as BR
import horizon_lib as H


@pytest.mark.parametrize("beta", [0.4, 0.0])
@pytest.mark.parametrize("case", ["lqr", "pendulum"])
def test_restatement_matches_the_operator_node_by_node(case, beta):
    rng = np.random.default_rng(7)
    if case == "lqr":
        host, prm, C = H.lqr_host, H.LQR_PRM, H.lqr_cands()
    else:
        host, prm = H.pendulum_host, H.PENDULUM_PRM
        C = np.array([(a, b) for a in np.linspace(-1.0, 1.0, 7) for b in (0.0, 0.5, 1.0)])
    P = 60
    x = rng.uniform(-2.0, 2.0, size=(P, 2))
    V = rng.uniform(0.0, 3.0, size=(P, 5))
    h2, t, delta = 0.04, [0.2, 1.0, 0.18, 0.81], 0.03
    vals, _, cfl = BR.candidate_values(host, prm, x, V, C, h2, t, beta, delta=delta)
    out, ui, _ = BR.backup(vals)
    l_out, l_ui, _, l_cfl = BR.loop_backup(host, prm, x, V, C, h2, t, beta, delta=delta)
    for p in range(P):
        assert abs(out[p] - l_out[p]) <= 1e-13 * max(1.0, abs(l_out[p]))
        assert ui[p] == l_ui[p]
        assert bool(cfl[p].any()) == l_cfl[p]


def test_stay_candidates_are_not_skipped():
    # no diffusion and u = 0: Q = 0 for the "stay" candidate, whose value is g delta + e^{-beta delta} V_self
    prm = (0.0, 1.0, 1.0, 1.0)
    C = np.array([(0.0, 0.0), (0.5, 0.0), (-0.5, 0.0)])
    x = np.array([[0.3, 0.2]])
    V = np.array([[9.0, 9.0, 9.0, 9.0, 1.0]])  # every neighbour costs more: staying is best
    vals, _, cfl = BR.candidate_values(H.lqr_host, prm, x, V, C, 0.04, [0.2, 1.0, 0.2, 1.0], 0.1, delta=0.02)
    out, ui, _ = BR.backup(vals)
    assert ui[0] == 0 and not cfl.any()
    assert out[0] == pytest.approx(0.13 * 0.02 + math.exp(-0.1 * 0.02) * 1.0, rel=1e-15)
    assert np.isfinite(vals).all()


def test_cfl_candidates_take_part():
    C = np.array([(0.0, 0.0), (1.5, 1.5)])
    x = np.array([[0.0, 0.0]])
    V = np.array([[0.0, -50.0, 0.0, -50.0, 0.0]])  # a negative self-loop makes the fast candidate's value very low
    vals, _, cfl = BR.candidate_values(H.lqr_host, H.LQR_PRM, x, V, C, 0.04, [0.2, 1.0, 0.2, 1.0], 0.0, delta=0.2)
    assert cfl[0, 1] and not cfl[0, 0]
    out, ui, _ = BR.backup(vals)
    assert ui[0] == 1 and out[0] == vals[0, 1]


@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_dense_chain_matches_riccati_at_the_interior_nodes(beta):
    w = dataclasses.replace(H.lqr_workload(0), discount=beta)
    term = lambda x: H.lqr_terminal(H.LQR_PRM, x)
    V, cfl = H.dense_chain(w, H.lqr_host, term, term, H.LQR_DELTA, H.LQR_STAGES)
    assert not cfl, "the LQR step must keep every self-loop non-negative"
    assert V.shape == (H.LQR_STAGES + 1, H.LQR_N, H.LQR_N)
    xg = w.xgrid()[0]
    X0, X1 = np.meshgrid(xg, xg, indexing="ij")
    inner = (np.abs(X0) <= H.LQR_INNER + 1e-9) & (np.abs(X1) <= H.LQR_INNER + 1e-9)
    for s in (0, H.LQR_STAGES // 2, H.LQR_STAGES):
        P, c = H.riccati(H.LQR_PRM, (H.LQR_STAGES - s) * H.LQR_DELTA, beta)
        R = P * (X0 ** 2 + X1 ** 2) + 2.0 * c
        err = np.abs(V[s] - R)[inner].max()
        assert err <= H.LQR_BOUND, (s, err)
    # the bound is not loose by an order of magnitude: the scheme's error at this grid is of its size
    P, c = H.riccati(H.LQR_PRM, H.LQR_STAGES * H.LQR_DELTA, beta)
    assert np.abs(V[0] - (P * (X0 ** 2 + X1 ** 2) + 2.0 * c))[inner].max() > 0.1 * H.LQR_BOUND


def test_riccati_reference():
    # q = r = 1, beta = 0: P(tau) = coth(tau + acoth(s)) and c(tau) = sig^2 log(sinh(tau + a) / sinh(a)), tau the time to go
    sig, s = H.LQR_PRM[0], H.LQR_PRM[3]
    a = math.atanh(1.0 / s)
    P, c = H.riccati(H.LQR_PRM, 0.5)
    assert P == pytest.approx(1.0 / math.tanh(0.5 + a), rel=1e-10)
    assert c == pytest.approx(sig * sig * math.log(math.sinh(0.5 + a) / math.sinh(a)), rel=1e-10)
    assert H.riccati(H.LQR_PRM, 0.0) == (s, 0.0)


def test_full_rank_train_is_exact():
    V = np.random.default_rng(1).normal(size=(11, 11))
    ranks, (c0, c1) = H.full_rank_train(V)
    assert ranks == [1, 11, 1]
    np.testing.assert_allclose(np.einsum("iab,jbc->ij", c0, c1), V, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- libc3sc.so's host twin
def _policy_control(V, prm, beta, delta):
    """a C3Control of the LQR with the host callbacks, its policy the nodal value function V[11, 11], horizon mode on"""
    import ctypes as C

    import facade_lib as fl

    w = dataclasses.replace(H.lqr_workload(0), discount=beta, params=tuple(prm))
    L = fl.lib()
    L.valuef_create_nodal.restype = C.c_void_p
    ctl = fl.Control(w, callbacks=H.lqr_callbacks(prm), device_model=False, consistent_ends=None)
    ranks, cores = H.full_rank_train(V)
    rk = fl.usz(ranks)
    cs = [np.ascontiguousarray(c, dtype=np.float64) for c in cores]
    vf = C.c_void_p(L.valuef_create_nodal(C.c_size_t(2), fl.sp(fl.usz(w.ngrid)), fl.sp(rk), fl.ptrs(cs)))
    xg = [fl.f64(g) for g in w.xgrid()]
    L.valuef_attach_grid(vf, fl.ptrs(xg))
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    L.c3control_set_horizon_step.argtypes = [C.c_void_p, C.c_double]
    L.c3control_get_horizon_step.restype = C.c_double
    L.c3control_set_horizon_step(ctl.h, delta)
    assert L.c3control_get_horizon_step(ctl.h) == delta
    return L, ctl, w, (vf, cs, xg, rk)


@pytest.mark.parametrize("beta", [0.4, 0.0])
def test_host_twin_picks_the_numpy_argmin_at_every_interior_node(beta):
    import ctypes as C

    import facade_lib as fl

    rng = np.random.default_rng(11)
    V = rng.uniform(0.0, 3.0, size=(11, 11))
    L, ctl, w, keep = _policy_control(V, H.LQR_PRM, beta, 0.05)
    h2, t = BR.mca_constants(w)
    xg = w.xgrid()
    C2 = np.asarray(w.cands, dtype=np.float64)
    checked = 0
    for a in range(1, 10):
        for b in range(1, 10):
            x = np.array([xg[0][a], xg[1][b]])
            S = np.array([[V[a - 1, b], V[a + 1, b], V[a, b - 1], V[a, b + 1], V[a, b]]])
            vals, _, _ = BR.candidate_values(H.lqr_host, w.params, x[None], S, C2, h2, t, beta, delta=0.05)
            _, ui, mg = BR.backup(vals)
            u = np.zeros(2)
            assert L.c3control_policy_eval(ctl.h, C.c_double(0.0), fl.dp(fl.f64(x)), fl.dp(u)) == 0
            if mg[0] > 1e-9:
                np.testing.assert_array_equal(u, C2[ui[0]])
                checked += 1
    assert checked > 60


def test_host_twin_keeps_the_stay_candidate():
    import ctypes as C

    import facade_lib as fl

    V = np.full((11, 11), 9.0)
    V[5, 5] = 1.0  # every neighbour of the centre costs more: with no diffusion, staying (u = 0, Q = 0) is best
    prm = (0.0, 1.0, 1.0, 2.0)
    L, ctl, w, keep = _policy_control(V, prm, 0.1, 0.05)
    u = np.full(2, 7.0)
    assert L.c3control_policy_eval(ctl.h, C.c_double(0.0), fl.dp(fl.f64([0.0, 0.0])), fl.dp(u)) == 0
    np.testing.assert_array_equal(u, [0.0, 0.0])


@pytest.mark.parametrize("call", ["c3control_pi_solve", "c3control_step_pi"])
def test_policy_iteration_is_refused_in_horizon_mode(call):
    import subprocess
    import sys
    import textwrap

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = textwrap.dedent(f"""
        import ctypes as C, numpy as np, sys
        sys.path[:0] = [{root!r}, {os.path.join(root, "tests")!r}]
        import facade_lib as fl, horizon_lib as H
        L = fl.lib()
        ctl = fl.Control(H.lqr_workload(0), callbacks=H.lqr_callbacks(), device_model=False)
        L.c3control_set_horizon_step.argtypes = [C.c_void_p, C.c_double]
        L.c3control_set_horizon_step(ctl.h, 0.05)
        if {call!r} == "c3control_pi_solve":
            L.c3control_pi_solve(ctl.h, C.c_size_t(3), C.c_double(1e-6), None, None, ctl.opt, 0, None)
        else:
            L.c3control_step_pi(ctl.h, None, None, None, ctl.opt, 0, None)
        print("NOT REFUSED")
    """)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NOT REFUSED" not in r.stdout
    assert "policy iteration is not offered in horizon mode" in r.stderr, r.stderr[-2000:]
