"""Correlated noise through libc3sc.so without a GPU: the host twin in bellman_optimal (c3control_add_covariance,
c3control_set_correlation, read through c3control_policy_eval_value) against corr_lib node by node to 1e-14 of the value scale, at
nodes of the ragged 21 x 70 grid -- interior, on the periodic ends of dimension 1, and on a 21 x 70 grid whose second dimension
reflects -- in the minimising form and in the forced form (a list of the one candidate to apply), in the infinite-horizon and
the explicit scheme; the known answer x0 x1 + delta a to 1e-14 through the host path; the twin's own dominance test speaks at the
nodes corr_lib names and keeps the algebra's value; the rollouts and closed loops are refused in correlation mode, and
interventions and correlation refuse each other."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from c3sc_amd import workloads as wl
import backup_ref as BR
import corr_lib as CL
import facade_lib as fl
import horizon_lib as H
import jump_lib as JL
import stop_lib as SL


def _control(w, callbacks, V, covar, pairs, delta=None):
    """a C3Control over workload w with host callbacks, its policy the nodal value function V, correlation on"""
    import facade_lib as fl

    L = fl.lib()
    L.valuef_create_nodal.restype = C.c_void_p
    ctl = fl.Control(w, callbacks=callbacks, device_model=False, consistent_ends=None)
    ranks, cores = H.full_rank_train(V)
    rk = fl.usz(ranks)
    cs = [np.ascontiguousarray(c, dtype=np.float64) for c in cores]
    vf = C.c_void_p(L.valuef_create_nodal(C.c_size_t(2), fl.sp(fl.usz(w.ngrid)), fl.sp(rk), fl.ptrs(cs)))
    xg = [fl.f64(g) for g in w.xgrid()]
    L.valuef_attach_grid(vf, fl.ptrs(xg))
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    keep = [vf, cs, xg, rk, CL.add_covariance(L, ctl, covar, w.params, w.dx, pairs)]
    assert L.c3control_get_correlation(ctl.h) == 1
    if delta:
        L.c3control_set_horizon_step.argtypes = [C.c_void_p, C.c_double]
        L.c3control_set_horizon_step(ctl.h, delta)
    L.c3control_policy_eval_value.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                              C.POINTER(C.c_double)]
    return L, ctl, keep


def _eval(L, ctl, x, du):
    import facade_lib as fl

    u, stopped, val = np.full(du, 7.0), C.c_int(-1), C.c_double(0.0)
    assert L.c3control_policy_eval_value(ctl.h, C.c_double(0.0), fl.dp(fl.f64(x)), fl.dp(u), C.byref(stopped), C.byref(val)) == 0
    return val.value, u


def _nodes_and_reference(w, V, delta):
    """nodes of the grid outside the obstacle and off the absorbing faces -- the ends of the periodic or reflecting dimension 1
    included -- with corr_lib's values [P, nc] of every candidate there"""
    n0, n1 = w.ngrid
    nodes = np.array([(a, b) for a in range(1, n0 - 1) for b in list(range(0, n1, 3)) + [n1 - 1]])
    xg = w.xgrid()
    x = np.stack([np.asarray(xg[0])[nodes[:, 0]], np.asarray(xg[1])[nodes[:, 1]]], axis=-1)
    keepn = ~JL.target_kinds(w, x)[1]
    x, nodes = x[keepn], nodes[keepn]
    S = np.empty((len(x), 5))
    for m in range(2):
        lo, hi = CL.neighbour_indices(nodes[:, m], w.ngrid[m], w.bc[m])
        a, b = [nodes[:, 0], nodes[:, 1]], [nodes[:, 0], nodes[:, 1]]
        a[m], b[m] = lo, hi
        S[:, 2 * m], S[:, 2 * m + 1] = V[tuple(a)], V[tuple(b)]
    S[:, 4] = V[nodes[:, 0], nodes[:, 1]]
    h2, t = BR.mca_constants(w)
    Cn = np.asarray(w.cands, dtype=np.float64)
    cq, cpv, r = CL.corr_terms(w, CL.lqr_covar, CL.LQR_PAIRS, V, nodes, x, S)
    assert not CL.dominance(w, SL.lqrn_host, CL.LQR_PAIRS, x, r).any()
    plain, _, _ = BR.candidate_values(SL.lqrn_host, w.params, x, S, Cn, h2, t, w.discount, 0.0 * cq, 0.0 * cpv, delta)
    vals, _, _ = BR.candidate_values(SL.lqrn_host, w.params, x, S, Cn, h2, t, w.discount, cq, cpv, delta)
    assert np.abs(vals - plain).max() > 1e-4, "the cross terms move the values"
    return nodes, x, vals


@pytest.mark.parametrize("beta", [0.3, 0.0])
@pytest.mark.parametrize("delta", [None, 0.01], ids=["infinite", "horizon"])
@pytest.mark.parametrize("bc1", [wl.BC_PERIODIC, wl.BC_REFLECT], ids=["periodic", "reflecting"])
def test_host_twin_equals_corr_lib_node_by_node(beta, delta, bc1):
    w = CL.lqr_workload(0, 4, beta)
    w = dataclasses.replace(w, bc=(w.bc[0], bc1))
    n0, n1 = w.ngrid
    # A smooth value function.  The twin reads every neighbour with valuef_eval at the COORDINATE x +- h, which is the node's own
    # coordinate up to an ulp; the interpolant turns that ulp into |dV| / h ulps of the value, so on white noise (|dV| / h ~ 40
    # here) no coordinate-based evaluation can meet 1e-14, on a function with a gradient of order 1 it does
    xg = [np.asarray(g) for g in w.xgrid()]
    V = 1.7 + 0.8 * np.sin(0.5 * np.pi * xg[0] + 0.3)[:, None] * np.cos(0.5 * np.pi * xg[1] - 0.4)[None, :] + 0.1 * xg[0][:, None] ** 2
    if bc1 == wl.BC_PERIODIC:
        V[:, -1] = V[:, 0]  # node 0 and node n - 1 of the periodic dimension are one point
    else:
        V = V + 0.2 * xg[1][None, :]
    nodes, x, vals = _nodes_and_reference(w, V, delta)
    ref, ui, mg = BR.backup(vals)
    L, ctl, keep = _control(w, H.lqr_callbacks(w.params), V, CL.lqr_covar, CL.LQR_PAIRS, delta)
    Cn = np.asarray(w.cands, dtype=np.float64)
    worst = 0.0
    for p in range(len(x)):
        val, u = _eval(L, ctl, x[p], 2)
        worst = max(worst, abs(val - ref[p]) / max(1.0, abs(ref[p])))
        if mg[p] > 1e-9:
            np.testing.assert_array_equal(u, Cn[ui[p]])
    ends = ((nodes[:, 1] == 0) | (nodes[:, 1] == n1 - 1)).sum()
    print("host twin against corr_lib, minimising:", len(x), "nodes,", ends, "on the ends of dimension 1, worst", worst)
    assert worst <= 1e-14
    assert len(x) > 300 and ends > 20
    # the forced form: a list of the one candidate to apply
    worst = 0.0
    for c in (3, 17):
        wf = dataclasses.replace(w, cands=Cn[c:c + 1])
        Lf, ctlf, keepf = _control(wf, H.lqr_callbacks(w.params), V, CL.lqr_covar, CL.LQR_PAIRS, delta)
        for p in range(0, len(x), 5):
            val, u = _eval(Lf, ctlf, x[p], 2)
            np.testing.assert_array_equal(u, Cn[c])
            worst = max(worst, abs(val - vals[p, c]) / max(1.0, abs(vals[p, c])))
    print("host twin against corr_lib, forced: worst", worst)
    assert worst <= 1e-14


@pytest.mark.parametrize("a", [CL.KNOWN_A, -CL.KNOWN_A])
def test_known_answer_through_the_host_path(a):
    w = CL.known_workload(0, a)
    cbs, _ = fl.callbacks2d(lambda x, u: (0.0, 0.0), lambda x, u: (CL.KNOWN_SIGMA, CL.KNOWN_SIGMA), lambda x, u: 0.0, lambda x: 0.0,
                            lambda x: 0.0, lambda x: 0.0)
    xg = w.xgrid()
    V = np.outer(xg[0], xg[1])
    L, ctl, keep = _control(w, cbs, V, CL.known_covar, CL.KNOWN_PAIRS, CL.KNOWN_DELTA)
    for i in (1, 4, 7):
        for j in (1, 5, 11):
            val, _ = _eval(L, ctl, np.array([xg[0][i], xg[1][j]]), 1)
            ref = xg[0][i] * xg[1][j] + CL.KNOWN_DELTA * a
            assert abs(val - ref) <= 1e-14, (i, j, val, ref)
    L.c3control_set_correlation(ctl.h, 0)
    val, _ = _eval(L, ctl, np.array([xg[0][4], xg[1][5]]), 1)
    assert abs(val - xg[0][4] * xg[1][5]) <= 1e-14


def test_rollouts_and_closed_loops_are_refused_in_correlation_mode():
    import facade_lib as fl

    w = CL.lqr_workload(0, 4, 0.3)
    L, ctl, keep = _control(w, H.lqr_callbacks(w.params), np.ones(w.ngrid), CL.lqr_covar, CL.LQR_PAIRS)
    x0 = fl.f64([0.1, 0.2])
    traj = np.zeros((4, 2))
    assert L.c3control_simulate(ctl.h, fl.dp(x0), C.c_double(0.01), C.c_size_t(3), None, fl.dp(traj), None) != 0
    assert L.c3control_integrate(ctl.h, b"rk4", C.c_double(0.0), C.c_double(0.01), C.c_size_t(3), fl.dp(x0), None, None, fl.dp(traj),
                                 None, None, None, None) != 0
    L.c3control_set_correlation(ctl.h, 0)
    assert L.c3control_get_correlation(ctl.h) == 0
    assert L.c3control_simulate(ctl.h, fl.dp(x0), C.c_double(0.01), C.c_size_t(3), None, fl.dp(traj), None) == 0


def test_host_dominance_test_speaks_where_corr_lib_says_and_keeps_the_algebra(capfd):
    """amp = 0.8 against the grid ratio 0.29: at a node corr_lib's dominance test names, c3control_policy_eval_value writes its
    message and still returns corr_lib's value; at a node it does not name, no message"""
    w = CL.lqr_workload(0, 4, 0.3, CL.LQR_DOM_PRM)
    xg = [np.asarray(g) for g in w.xgrid()]
    V = 1.7 + 0.8 * np.sin(0.5 * np.pi * xg[0] + 0.3)[:, None] * np.cos(0.5 * np.pi * xg[1] - 0.4)[None, :] + 0.1 * xg[0][:, None] ** 2
    V[:, -1] = V[:, 0]
    n0, n1 = w.ngrid
    nodes = np.array([(a, b) for a in range(1, n0 - 1) for b in range(1, n1 - 1)])
    x = np.stack([xg[0][nodes[:, 0]], xg[1][nodes[:, 1]]], axis=-1)
    keepn = ~JL.target_kinds(w, x)[1]
    x, nodes = x[keepn], nodes[keepn]
    r, _ = CL.pair_rates(w, CL.lqr_covar, CL.LQR_PAIRS, x)
    bad = CL.dominance(w, SL.lqrn_host, CL.LQR_PAIRS, x, r)
    assert bad.any() and (~bad).any()
    L, ctl, keep = _control(w, H.lqr_callbacks(w.params), V, CL.lqr_covar, CL.LQR_PAIRS)
    h2, t = BR.mca_constants(w)
    Cn = np.asarray(w.cands, dtype=np.float64)
    for p, expect in ((int(np.flatnonzero(bad)[0]), True), (int(np.flatnonzero(~bad)[0]), False)):
        a, b = nodes[p]
        S = np.array([[V[a - 1, b], V[a + 1, b], V[a, b - 1], V[a, b + 1], V[a, b]]])
        cq, cpv, _ = CL.corr_terms(w, CL.lqr_covar, CL.LQR_PAIRS, V, nodes[p:p + 1], x[p:p + 1], S)
        vals, _, _ = BR.candidate_values(SL.lqrn_host, w.params, x[p:p + 1], S, Cn, h2, t, w.discount, cq, cpv)
        ref = BR.backup(vals)[0][0]
        capfd.readouterr()
        val, _ = _eval(L, ctl, x[p], 2)
        err = capfd.readouterr().err
        assert ("dominance condition" in err) == expect, (p, expect, err)
        assert abs(val - ref) <= 1e-14 * max(1.0, abs(ref))


@pytest.mark.parametrize("first", ["correlation", "impulses"])
def test_interventions_and_correlation_refuse_each_other(first):
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    order = ("L.c3control_set_impulses(ctl.h, 1)" if first == "correlation" else
             "L.c3control_set_correlation(ctl.h, 0); L.c3control_set_impulses(ctl.h, 1); L.c3control_set_correlation(ctl.h, 1)")
    prog = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]
        import ctypes as C
        import numpy as np
        import horizon_lib as H, corr_lib as CL, test_corr_host as T
        w = CL.lqr_workload(0, 4, 0.3)
        L, ctl, keep = T._control(w, H.lqr_callbacks(w.params), np.ones(w.ngrid), CL.lqr_covar, CL.LQR_PAIRS)
        FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double))
        cb = FN(lambda x, m, y: 1.0)
        L.c3control_add_impulses.argtypes = [C.c_void_p, C.c_int, FN]
        L.c3control_add_impulses(ctl.h, 1, cb)
        L.c3control_set_impulses.argtypes = [C.c_void_p, C.c_int]
        {order}
        print("NOT REFUSED")
    """)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NOT REFUSED" not in r.stdout
    assert "impulse control with correlated noise is not offered" in r.stderr, r.stderr[-2000:]
