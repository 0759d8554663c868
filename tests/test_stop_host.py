"""Optimal stopping without a GPU: the numpy restatement (stop_lib) against a per-candidate Python loop in both
forms and discount regimes; a psi too large to win leaves the plain scan's values and indices bit for bit; the host twin
(c3control_policy_eval_stop) takes stop_lib's decision at the interior nodes; policy iteration is refused; and the dense explicit
chain of the American put on 11 x 11: V <= psi, V <= the European value, V_n non-increasing in the time to go, both regions
populated at stage 0, and the discretisation bound the GPU rollouts are held to."""
import dataclasses
import os

import numpy as np
import pytest

import backup_ref as BR
import horizon_lib as H
import stop_lib as SL


def _random_nodes(rng, P, lo, hi):
    x = rng.uniform(lo, hi, size=(P, 2))
    V = rng.uniform(0.0, 3.0, size=(P, 5))
    return x, V


H2, T = 0.04, [0.2, 1.0, 0.2, 1.0]  # h = 0.2 in both dimensions


@pytest.mark.parametrize("beta", [0.3, 0.0])
@pytest.mark.parametrize("delta", [None, 0.02])
def test_stop_lib_equals_a_per_candidate_loop(beta, delta):
    rng = np.random.default_rng(5)
    x, V = _random_nodes(rng, 200, -2.0, 2.0)
    C = SL.lqr_cands()
    psi = SL.lqr_psi(SL.LQR_PRM, x)
    vals, _, _ = BR.candidate_values(H.lqr_host, SL.LQR_PRM, x, V, C, H2, T, beta, delta=delta)
    out, ui, mg = SL.stop_backup(vals, psi)
    l_out, l_ui, _, _ = BR.loop_backup(H.lqr_host, SL.LQR_PRM, x, V, C, H2, T, beta, psi=psi, delta=delta)
    sure = mg > 1e-12
    assert sure.mean() > 0.99
    np.testing.assert_array_equal(ui[sure], l_ui[sure])
    np.testing.assert_allclose(out, l_out, rtol=1e-13, atol=1e-13)
    assert (ui == len(C)).any() and (ui < len(C)).any(), "both decisions occur"


def test_stop_wins_where_no_candidate_is_valid():
    # the put at S = 0: no drift, no diffusion, Q = 0 -- the infinite-horizon scan skips its one candidate
    x = np.array([[0.0, 0.0], [1.0, 1.2]])
    V = np.ones((2, 5))
    vals, stat, _ = BR.candidate_values(SL.put_host, SL.PUT_PRM, x, V, SL.PUT_CANDS, H2, T, 0.1)
    assert stat.tolist() == [True, False] and np.isnan(vals[0, 0])
    out, ui, mg = SL.stop_backup(vals, SL.put_psi(SL.PUT_PRM, x))
    assert ui[0] == 1 and out[0] == -1.0 and np.isinf(mg[0])
    # forced: ncand yields psi, a skipped candidate 0 and -1
    f_out, f_ui, _ = SL.stop_backup(vals, SL.put_psi(SL.PUT_PRM, x), forced=np.array([1, 1]))
    assert f_ui.tolist() == [1, 1] and f_out.tolist() == [-1.0, 0.0]
    f_out, f_ui, _ = SL.stop_backup(vals, SL.put_psi(SL.PUT_PRM, x), forced=np.array([0, 0]))
    assert f_ui.tolist() == [-1, 0] and f_out[0] == 0.0 and f_out[1] == vals[1, 0]


@pytest.mark.parametrize("delta", [None, 0.02])
def test_a_psi_that_never_wins_leaves_the_plain_scan_bit_for_bit(delta):
    rng = np.random.default_rng(7)
    x, V = _random_nodes(rng, 300, -2.0, 2.0)
    C = SL.lqr_cands()
    vals, _, _ = BR.candidate_values(H.lqr_host, SL.LQR_NEVER_PRM, x, V, C, H2, T, 0.2, delta=delta)
    out, ui, _ = SL.stop_backup(vals, SL.lqr_psi(SL.LQR_NEVER_PRM, x))
    p_out, p_ui, _ = BR.backup(vals)
    np.testing.assert_array_equal(out, p_out)
    np.testing.assert_array_equal(ui, p_ui)


# ---------------------------------------------------------------------------------------------------- the put on 11 x 11
@pytest.fixture(scope="module")
def put_chain():
    w = SL.put_workload(0)
    psi = lambda x: SL.put_psi(SL.PUT_PRM, x)
    V, dec, cfl = SL.dense_chain(w, SL.put_host, psi, SL.PUT_DELTA, SL.PUT_STAGES)
    E, _, _ = SL.dense_chain(w, SL.put_host, psi, SL.PUT_DELTA, SL.PUT_STAGES, stopping=False)
    return w, V, dec, cfl, E


def test_dense_put_chain(put_chain):
    w, V, dec, cfl, E = put_chain
    assert not cfl, "PUT_DELTA keeps every self-loop probability non-negative"
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    psi = SL.put_psi(SL.PUT_PRM, X)
    assert (V <= psi[None] + 1e-15).all()
    assert (V <= E + 1e-15).all(), "the right to stop early is worth something: the American value is below the European cost"
    assert (V[:-1] < E[:-1] - 1e-6).any()
    assert (np.diff(V, axis=0) >= -1e-15).all(), "V_n is non-increasing in the time to go"
    inner = dec[0][1:-1, 1:-1]
    assert inner.mean() >= 0.10 and (1.0 - inner.mean()) >= 0.10, inner.mean()


def test_put_discretisation_bound(put_chain):
    """|V_0 on 11 x 11 at PUT_DELTA - V_0 on 21 x 21 at PUT_DELTA / 4| at the rollouts' start states stays under PUT_DISC; the
    GPU rollouts are held to twice that (stop_lib.PUT_BOUND)"""
    w, V, _, _, _ = put_chain
    w2 = SL.put_workload(0, n=21)
    V2, _, cfl2 = SL.dense_chain(w2, SL.put_host, lambda x: SL.put_psi(SL.PUT_PRM, x), SL.PUT_DELTA / 4, SL.PUT_STAGES * 4)
    assert not cfl2
    xg, xg2 = w.xgrid()[0], w2.xgrid()[0]
    worst = 0.0
    for x0 in SL.PUT_X0:
        i, j = (int(np.argmin(np.abs(xg - v))) for v in x0)
        i2, j2 = (int(np.argmin(np.abs(xg2 - v))) for v in x0)
        assert abs(xg[i] - x0[0]) < 1e-12 and abs(xg2[i2] - x0[0]) < 1e-12 and abs(xg[j] - x0[1]) < 1e-12
        worst = max(worst, abs(V[0][i, j] - V2[0][i2, j2]))
    print("put discretisation:", worst)
    assert worst <= SL.PUT_DISC
    assert worst > 0.25 * SL.PUT_DISC, "the bound is of the size of what it bounds"
    assert SL.PUT_BOUND == 2 * SL.PUT_DISC


# ---------------------------------------------------------------------------------------------------- libc3sc.so's host twin
def _stop_control(V, prm, beta, delta):
    """a C3Control of the stopping LQR with the host callbacks, its policy the nodal value function V[11, 11], stopping on"""
    import ctypes as C

    import facade_lib as fl

    w = dataclasses.replace(H.lqr_workload(0), discount=beta, params=tuple(prm), cands=SL.lqr_cands())
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

    def _psi(t, x, out):
        out[0] = prm[4] + prm[5] * (x[0] * x[0] + x[1] * x[1])
        return 0

    psi = fl.BOUND_FN(_psi)
    L.c3control_add_stopcost(ctl.h, psi)
    L.c3control_set_stopping.argtypes = [C.c_void_p, C.c_int]
    L.c3control_set_stopping(ctl.h, 1)
    assert L.c3control_get_stopping(ctl.h) == 1
    if delta:
        L.c3control_set_horizon_step.argtypes = [C.c_void_p, C.c_double]
        L.c3control_set_horizon_step(ctl.h, delta)
    return L, ctl, w, (vf, cs, xg, rk, psi)


@pytest.mark.parametrize("beta", [0.4, 0.0])
@pytest.mark.parametrize("delta", [None, 0.05])
def test_host_twin_takes_stop_libs_decision_at_every_interior_node(beta, delta):
    import ctypes as C

    import facade_lib as fl

    rng = np.random.default_rng(11)
    V = rng.uniform(0.0, 3.0, size=(11, 11))
    L, ctl, w, keep = _stop_control(V, SL.LQR_PRM, beta, delta)
    h2, t = BR.mca_constants(w)
    xg = w.xgrid()
    C2 = np.asarray(w.cands, dtype=np.float64)
    checked = stops = 0
    for a in range(1, 10):
        for b in range(1, 10):
            x = np.array([xg[0][a], xg[1][b]])
            S = np.array([[V[a - 1, b], V[a + 1, b], V[a, b - 1], V[a, b + 1], V[a, b]]])
            vals, _, _ = BR.candidate_values(H.lqr_host, w.params, x[None], S, C2, h2, t, beta, delta=delta)
            _, ui, mg = SL.stop_backup(vals, SL.lqr_psi(w.params, x[None]))
            _, _, cmg = BR.backup(vals)
            u = np.full(2, 7.0)
            stopped = C.c_int(-1)
            assert L.c3control_policy_eval_stop(ctl.h, C.c_double(0.0), fl.dp(fl.f64(x)), fl.dp(u), C.byref(stopped)) == 0
            if mg[0] > 1e-9 and (ui[0] == len(C2) or cmg[0] > 1e-9):
                assert stopped.value == int(ui[0] == len(C2))
                np.testing.assert_array_equal(u, [0.0, 0.0] if ui[0] == len(C2) else C2[ui[0]])
                checked += 1
                stops += stopped.value
                u2 = np.full(2, 7.0)
                assert L.c3control_policy_eval(ctl.h, C.c_double(0.0), fl.dp(fl.f64(x)), fl.dp(u2)) == 0
                np.testing.assert_array_equal(u2, u)
    assert checked > 60 and 0 < stops < checked


@pytest.mark.parametrize("call", ["c3control_pi_solve", "c3control_step_pi"])
def test_policy_iteration_is_refused_in_stop_mode(call):
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
        psi = fl.BOUND_FN(lambda t, x, out: 0)
        L.c3control_add_stopcost(ctl.h, psi)
        L.c3control_set_stopping.argtypes = [C.c_void_p, C.c_int]
        L.c3control_set_stopping(ctl.h, 1)
        if {call!r} == "c3control_pi_solve":
            L.c3control_pi_solve(ctl.h, C.c_size_t(3), C.c_double(1e-6), None, None, ctl.opt, 0, None)
        else:
            L.c3control_step_pi(ctl.h, None, None, None, ctl.opt, 0, None)
        print("NOT REFUSED")
    """)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NOT REFUSED" not in r.stdout
    assert "policy iteration is not offered for stopping problems" in r.stderr, r.stderr[-2000:]


def test_single_trajectory_loops_are_refused_in_stop_mode():
    import ctypes as C

    import facade_lib as fl

    V = np.ones((11, 11))
    L, ctl, w, keep = _stop_control(V, SL.LQR_PRM, 0.1, None)
    x0 = fl.f64([0.1, 0.2])
    traj = np.zeros((4, 2))
    assert L.c3control_simulate(ctl.h, fl.dp(x0), C.c_double(0.01), C.c_size_t(3), None, fl.dp(traj), None) != 0
    assert L.c3control_integrate(ctl.h, b"rk4", C.c_double(0.0), C.c_double(0.01), C.c_size_t(3), fl.dp(x0), None, None, fl.dp(traj),
                                 None, None, None, None) != 0
