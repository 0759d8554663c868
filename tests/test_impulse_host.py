"""Impulse control through libc3sc.so without a GPU: the host twin in bellman_optimal (c3control_add_impulses,
c3control_set_impulses, read through c3control_policy_eval_value and c3control_policy_eval_impulse) against impulse_lib node by
node to 1e-14 of the value scale, at every live node off the faces of the ragged 21 x 70 grid with a periodic dimension and an obstacle, with and without jumps;
the known answer min(continuation, min_m k_m + c) exactly through the host path; the single-trajectory loops, policy iteration
and the finite-horizon solve are refused in impulse mode.

The host has no forced (policy) path in impulse mode -- policy iteration is refused there -- so the minimising form alone is
compared."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import backup_ref as BR
import facade_lib as fl
import horizon_lib as H
import impulse_lib as IL
import jump_lib as JL
import stop_lib as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exact_train(V):
    """a 2-D train of the matrix V[n0, n1] whose nodal values are V to the last bit: core 0 the identity, core 1 the rows of V
    (an SVD train reproduces V only to 1e-14, which is the bound of the comparison below)"""
    n0, n1 = V.shape
    c0 = np.eye(n0).reshape(n0, 1, n0)
    c1 = np.ascontiguousarray(V.T).reshape(n1, n0, 1)
    return [1, n0, 1], [c0, c1]


def _control(w, callbacks, V, impulses, M, jumps=None, njump=0):
    """a C3Control over workload w with host callbacks, its policy the nodal value function V, interventions on"""
    import facade_lib as fl

    L = fl.lib()
    L.valuef_create_nodal.restype = C.c_void_p
    ctl = fl.Control(w, callbacks=callbacks, device_model=False, consistent_ends=None)
    ranks, cores = _exact_train(V)
    rk = fl.usz(ranks)
    cs = [np.ascontiguousarray(c, dtype=np.float64) for c in cores]
    vf = C.c_void_p(L.valuef_create_nodal(C.c_size_t(2), fl.sp(fl.usz(w.ngrid)), fl.sp(rk), fl.ptrs(cs)))
    xg = [fl.f64(g) for g in w.xgrid()]
    L.valuef_attach_grid(vf, fl.ptrs(xg))
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    keep = [vf, cs, xg, rk]
    if jumps is not None:
        keep.append(JL.add_jumps(L, ctl, jumps, w.params, w.dx, njump))
    cb = IL.impulse_callback(impulses, w.params, w.dx)
    L.c3control_add_impulses.argtypes = [C.c_void_p, C.c_int, type(cb)]
    L.c3control_add_impulses(ctl.h, M, cb)
    L.c3control_set_impulses.argtypes = [C.c_void_p, C.c_int]
    L.c3control_set_impulses(ctl.h, 1)
    assert L.c3control_get_impulses(ctl.h) == 1
    keep.append(cb)
    L.c3control_policy_eval_value.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                              C.POINTER(C.c_double)]
    L.c3control_policy_eval_impulse.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    return L, ctl, keep


def _eval(L, ctl, x, du):
    import facade_lib as fl

    u, val, m = np.full(du, 7.0), C.c_double(0.0), C.c_int(-7)
    assert L.c3control_policy_eval_value(ctl.h, C.c_double(0.0), fl.dp(fl.f64(x)), fl.dp(u), None, C.byref(val)) == 0
    assert L.c3control_policy_eval_impulse(ctl.h, fl.dp(fl.f64(x)), C.byref(m)) == 0
    return val.value, u, m.value


@pytest.mark.parametrize("beta", [0.3, 0.0])
@pytest.mark.parametrize("jumps", [False, True], ids=["nojump", "jump"])
def test_host_twin_equals_impulse_lib_node_by_node(beta, jumps):
    rng = np.random.default_rng(17)
    w = IL.lqr_workload(0, 4, beta, 0.9, jumps)  # K inside the spread of the random nodal values below
    n0, n1 = w.ngrid
    V = rng.uniform(0.5, 3.0, size=(n0, n1))
    V[:, -1] = V[:, 0]  # node 0 and node n - 1 of the periodic dimension are one point
    prm = w.params
    L, ctl, keep = _control(w, H.lqr_callbacks(prm), V, IL.lqr_impulses, IL.LQR_NIMPULSE, JL.lqr_jumps if jumps else None, JL.LQR_NJUMP)
    h2, t = BR.mca_constants(w)
    xg = w.xgrid()
    Cn = np.asarray(w.cands, dtype=np.float64)
    bcost, ocost = (lambda x: SL.lqrn_terminal(prm, x)), (lambda x: np.full(len(x), 5.0))
    nodes = [(a, b) for a in range(1, n0 - 1) for b in range(1, n1 - 1)]  # every live node off the seam column
    x = np.array([[xg[0][a], xg[1][b]] for a, b in nodes])
    keepn = ~JL.target_kinds(w, x)[1]  # outside the obstacle
    x, nodes = x[keepn], [nd for nd, k in zip(nodes, keepn) if k]
    S = np.array([[V[a - 1, b], V[a + 1, b], V[a, b - 1], V[a, b + 1], V[a, b]] for a, b in nodes])
    interp = JL.Nodal(w, V)
    jrate, J = JL.jump_terms(w, JL.lqr_jumps, interp, x, bcost, ocost) if jumps else (np.zeros(len(x)), np.zeros(len(x)))
    vals, _, _ = BR.candidate_values(SL.lqrn_host, prm, x, S, Cn, h2, t, beta, jrate, jrate * J)
    c = IL.impulse_values(w, IL.lqr_impulses, interp, x, bcost, ocost)
    ref, ui, mg = BR.backup(vals, c=c)
    nc = len(Cn)
    worst, taken = 0.0, np.zeros(IL.LQR_NIMPULSE, dtype=int)
    for p in range(len(x)):
        val, u, m = _eval(L, ctl, x[p], 2)
        worst = max(worst, abs(val - ref[p]) / max(1.0, abs(ref[p])))
        if mg[p] > 1e-9:
            assert m == (ui[p] - nc - 1 if ui[p] > nc else -1), (p, m, ui[p])
            np.testing.assert_array_equal(u, [0.0, 0.0] if m >= 0 else Cn[ui[p]])
            if m >= 0:
                taken[m] += 1
    print("host twin against impulse_lib:", len(x), "nodes, worst", worst, "interventions", taken)
    assert worst <= 1e-14
    assert len(x) > 1200 and (taken > 0).all() and 0.1 * len(x) < taken.sum() < 0.9 * len(x)
    # an absorbed state takes no intervention: inside the obstacle the value is the obstacle cost and the decision -1
    val, u, m = _eval(L, ctl, np.array([0.9, -0.9]), 2)
    assert val == 5.0 and m == -1 and (u == 0.0).all()


def test_known_answer_through_the_host_path():
    w = IL.known_workload(0)
    prm = w.params
    c = prm[4]
    cbs = fl.callbacks2d(lambda x, u: (u[0], u[1]), lambda x, u: (prm[0], prm[0]),
                         lambda x, u: prm[1] * (x[0] * x[0] + x[1] * x[1]) + prm[2] * (u[0] * u[0] + u[1] * u[1]), lambda x: c, lambda x: -1.0,
                         lambda x: 0.0)[0]
    V = np.random.default_rng(2).uniform(0.3, 0.8, size=w.ngrid)
    L, ctl, keep = _control(w, cbs, V, IL.known_impulses, IL.KNOWN_NIMPULSE)
    xg = w.xgrid()
    L.c3control_set_impulses(ctl.h, 0)
    pts = [np.array([xg[0][a], xg[1][b]]) for a in (1, 4, 7) for b in (1, 5, 11)]
    cont = [_eval(L, ctl, x, 2)[0] for x in pts]
    L.c3control_set_impulses(ctl.h, 1)
    wins = 0
    for x, cv in zip(pts, cont):
        val, u, m = _eval(L, ctl, x, 2)
        assert val == min(cv, IL.KNOWN_TARGET), (x, val, cv)
        assert m == (1 if IL.KNOWN_TARGET < cv else -1), "k_1 = k_2 < k_0: mark 1, by the first strict '<'"
        wins += m >= 0
    assert 0 < wins < len(pts)


def test_loops_without_an_impulse_form_are_refused():
    import facade_lib as fl

    w = IL.lqr_workload(0, 4, 0.3, 0.9)
    L, ctl, keep = _control(w, H.lqr_callbacks(w.params), np.ones(w.ngrid), IL.lqr_impulses, IL.LQR_NIMPULSE)
    x0 = fl.f64([0.1, 0.2])
    traj = np.zeros((4, 2))
    assert L.c3control_simulate(ctl.h, fl.dp(x0), C.c_double(0.01), C.c_size_t(3), None, fl.dp(traj), None) != 0
    assert L.c3control_integrate(ctl.h, b"rk4", C.c_double(0.0), C.c_double(0.01), C.c_size_t(3), fl.dp(x0), None, None, fl.dp(traj),
                                 None, None, None, None) != 0
    L.c3control_set_impulses(ctl.h, 0)
    assert L.c3control_get_impulses(ctl.h) == 0
    assert L.c3control_simulate(ctl.h, fl.dp(x0), C.c_double(0.01), C.c_size_t(3), None, fl.dp(traj), None) == 0


@pytest.mark.parametrize("call,msg", [("pi", "policy iteration is not offered for impulse control"),
                                      ("fh", "impulse control has no horizon form")])
def test_policy_iteration_and_the_horizon_solve_end_the_program(call, msg):
    prog = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, "tests")!r}]
        import ctypes as C
        import numpy as np
        import horizon_lib as H, impulse_lib as IL, test_impulse_host as T
        w = IL.lqr_workload(0, 4, 0.3, 0.9)
        L, ctl, keep = T._control(w, H.lqr_callbacks(w.params), np.ones(w.ngrid), IL.lqr_impulses, 3)
        vf = keep[0]
        if {call!r} == "pi":
            L.c3control_pi_solve(ctl.h, C.c_size_t(1), C.c_double(0.0), vf, None, ctl.opt, C.c_int(0), None)
        else:
            L.c3control_fh_solve(ctl.h, C.c_size_t(2), C.c_double(0.01), vf, None, ctl.opt, C.c_int(0))
        print("NOT REFUSED")
    """)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NOT REFUSED" not in r.stdout
    assert msg in r.stderr, r.stderr[-2000:]
