"""Jump diffusions through libc3sc.so without a GPU: the host twin in bellman_optimal (c3control_add_jumps,
c3control_set_jumps, read through c3control_policy_eval_value) against jump_lib node by node to 1e-12 of the value scale, on the
ragged 21 x 70 grid with a periodic dimension and an obstacle, in the infinite-horizon and the explicit form, with and without
the stop action; weights that do not sum to 1 end the program with a message; the known answer g / lambda + exp(-beta / lambda) c
to 1e-14 through the host path; the single-trajectory loops are refused in jump mode."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import backup_ref as BR
import facade_lib as fl
import horizon_lib as H
import jump_lib as JL
import stop_lib as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _control(w, callbacks, V, jumps, njump, delta=None, psi=None):
    """a C3Control over workload w with host callbacks, its policy the nodal value function V, jumps on"""
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
    rate, mark = JL.add_jumps(L, ctl, jumps, w.params, w.dx, njump)
    assert L.c3control_get_jumps(ctl.h) == 1
    keep = [vf, cs, xg, rk, rate, mark]
    if psi is not None:
        cb = fl.BOUND_FN(psi)
        L.c3control_add_stopcost(ctl.h, cb)
        L.c3control_set_stopping.argtypes = [C.c_void_p, C.c_int]
        L.c3control_set_stopping(ctl.h, 1)
        keep.append(cb)
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
    return val.value, u, stopped.value


@pytest.mark.parametrize("beta", [0.3, 0.0])
@pytest.mark.parametrize("delta", [None, 0.01])
@pytest.mark.parametrize("stop", [False, True], ids=["nostop", "stop"])
def test_host_twin_equals_jump_lib_node_by_node(beta, delta, stop):
    rng = np.random.default_rng(17)
    w = JL.lqr_workload(0, 4, beta)
    n0, n1 = w.ngrid
    V = rng.uniform(0.5, 3.0, size=(n0, n1))
    V[:, -1] = V[:, 0]  # node 0 and node n - 1 of the periodic dimension are one point
    prm = w.params
    if stop:
        prm = prm[:4] + (1.6, 0.2) + prm[6:]  # psi inside the range of the continuation values
        w = dataclasses.replace(w, params=prm)
    psi_cb = (lambda t, x, out: (out.__setitem__(0, prm[4] + prm[5] * (x[0] * x[0] + x[1] * x[1])), 0)[1]) if stop else None
    L, ctl, keep = _control(w, H.lqr_callbacks(prm), V, JL.lqr_jumps, JL.LQR_NJUMP, delta, psi_cb)
    h2, t = BR.mca_constants(w)
    xg = w.xgrid()
    Cn = np.asarray(w.cands, dtype=np.float64)
    bcost, ocost = (lambda x: SL.lqrn_terminal(prm, x)), (lambda x: np.full(len(x), 5.0))
    nodes = [(a, b) for a in range(1, n0 - 1) for b in range(1, n1 - 1, 3)]
    x = np.array([[xg[0][a], xg[1][b]] for a, b in nodes])
    keepn = ~JL.target_kinds(w, x)[1]  # outside the obstacle
    x, nodes = x[keepn], [nd for nd, k in zip(nodes, keepn) if k]
    S = np.array([[V[a - 1, b], V[a + 1, b], V[a, b - 1], V[a, b + 1], V[a, b]] for a, b in nodes])
    jrate, J = JL.jump_terms(w, JL.lqr_jumps, JL.Nodal(w, V), x, bcost, ocost)
    vals, _, _ = BR.candidate_values(SL.lqrn_host, prm, x, S, Cn, h2, t, beta, jrate, jrate * J, delta)
    ref, ui, mg = BR.backup(vals, SL.lqr_psi(prm, x) if stop else None)
    kinds = np.zeros(4, dtype=bool)
    _, _, y = JL.lqr_jumps(prm, x)
    for m in range(3):
        _, inobs, beyond, moved = JL.target_kinds(w, y[:, m])
        kinds |= np.array([(~inobs & ~beyond & ~moved).any(), (beyond & ~inobs).any(), inobs.any(), moved.any()])
    assert kinds.all(), kinds
    worst, stops = 0.0, 0
    for p in range(len(x)):
        val, u, stopped = _eval(L, ctl, x[p], 2)
        worst = max(worst, abs(val - ref[p]) / max(1.0, abs(ref[p])))
        if mg[p] > 1e-9:
            assert stopped == int(stop and ui[p] == len(Cn))
            np.testing.assert_array_equal(u, [0.0, 0.0] if stopped else Cn[ui[p]])
            stops += stopped
    print("host twin against jump_lib:", len(x), "nodes, worst", worst, "stops", stops)
    assert worst <= 1e-12
    assert len(x) > 300 and (not stop or 0 < stops < len(x))


def test_known_answer_through_the_host_path():
    w = JL.known_workload(0)
    g, lam, c = w.params
    cbs, _ = fl.callbacks2d(lambda x, u: (0.0, 0.0), lambda x, u: (0.0, 0.0), lambda x, u: g, lambda x: c, lambda x: -1.0, lambda x: 0.0)
    jumps = lambda prm, x: (np.full(len(x), prm[1]), np.broadcast_to(np.array([0.25, 0.25, 0.5]), (len(x), 3)),
                            np.stack([x + np.array([10.0 + m, 0.0]) for m in range(3)], axis=1))
    V = np.random.default_rng(2).uniform(0.0, 5.0, size=w.ngrid)
    L, ctl, keep = _control(w, cbs, V, jumps, JL.KNOWN_NJUMP)
    xg = w.xgrid()
    ref = JL.known_answer()
    for a in (1, 4, 7):
        for b in (0, 5, 12):
            val, u, _ = _eval(L, ctl, np.array([xg[0][a], xg[1][b]]), 1)
            assert abs(val - ref) <= 1e-14 * ref, (a, b, val, ref)


def test_weights_that_do_not_sum_to_one_end_the_program():
    prog = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]
        import numpy as np
        import horizon_lib as H, jump_lib as JL, test_jump_host as T
        w = JL.lqr_workload(0, 4, 0.3)
        def bad(prm, x):
            lam, pi, y = JL.lqr_jumps(prm, x)
            return lam, pi * (1.0 + 1e-9), y
        L, ctl, keep = T._control(w, H.lqr_callbacks(w.params), np.ones(w.ngrid), bad, 3)
        T._eval(L, ctl, np.array([0.0, 0.0]), 2)
        print("NOT REFUSED")
    """)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NOT REFUSED" not in r.stdout
    assert "jump weights sum to" in r.stderr, r.stderr[-2000:]


def test_single_trajectory_loops_are_refused_in_jump_mode():
    import facade_lib as fl

    w = JL.lqr_workload(0, 4, 0.3)
    L, ctl, keep = _control(w, H.lqr_callbacks(w.params), np.ones(w.ngrid), JL.lqr_jumps, 3)
    x0 = fl.f64([0.1, 0.2])
    traj = np.zeros((4, 2))
    assert L.c3control_simulate(ctl.h, fl.dp(x0), C.c_double(0.01), C.c_size_t(3), None, fl.dp(traj), None) != 0
    assert L.c3control_integrate(ctl.h, b"rk4", C.c_double(0.0), C.c_double(0.01), C.c_size_t(3), fl.dp(x0), None, None, fl.dp(traj),
                                 None, None, None, None) != 0
    L.c3control_set_jumps(ctl.h, 0)
    assert L.c3control_get_jumps(ctl.h) == 0
    assert L.c3control_simulate(ctl.h, fl.dp(x0), C.c_double(0.01), C.c_size_t(3), None, fl.dp(traj), None) == 0
