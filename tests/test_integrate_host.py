"""c3control_integrate (libc3sc.so, include/c3sc/bellman.h): the examples' closed-loop tail (cdyn's controlled forward-Euler / rk4
integrators + the goal test after every trajectory_step) on the host, against closed_loop_lib.simulate_rk4 over the same
controller; its argument checks, and the rejections c3control_integrate_batch makes before any device work.  No GPU involved."""
import ctypes as C

import numpy as np
import pytest

import closed_loop_lib as CL
from c3sc_amd import workloads as wl
from test_policy_tail import _lqg2d_callbacks

ERR_ARG = 1
TRANSFORM_FN = C.CFUNCTYPE(None, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double))


def _lib():
    import facade_lib

    L = facade_lib.lib()
    dpp = C.POINTER(C.c_double)
    L.c3control_integrate.argtypes = [C.c_void_p, C.c_char_p, C.c_double, C.c_double, C.c_size_t, dpp, dpp, dpp, dpp, dpp, dpp,
                                      C.POINTER(C.c_long), C.POINTER(C.c_int)]
    L.c3control_integrate.restype = C.c_int
    L.c3control_integrate_batch.argtypes = [C.c_void_p, C.c_size_t, dpp, C.c_char_p, C.c_double, C.c_double, C.c_size_t, dpp, dpp,
                                            C.c_int, C.c_size_t, dpp, dpp, dpp, C.POINTER(C.c_long), C.POINTER(C.c_int), dpp]
    L.c3control_integrate_batch.restype = C.c_int
    return L, facade_lib


def host_integrate(L, fl, ctl, x0, method, dt_int, dt_out, nout, goal=None, keep=None):
    """c3control_integrate for one trajectory: (traj (nout+1, dx), u (nout, du), cost, stop_step, stop_reason, rc)"""
    w = ctl.w
    traj, U = np.zeros((nout + 1, w.dx)), np.zeros((nout, w.du))
    cost, stp, why = C.c_double(0.0), C.c_long(7), C.c_int(7)
    gb = fl.f64(np.concatenate([goal[0], goal[1]])) if goal is not None else None
    kb = fl.f64(np.concatenate([keep[0], keep[1]])) if keep is not None else None
    rc = L.c3control_integrate(ctl.h, method.encode(), dt_int, dt_out, nout, fl.dp(fl.f64(x0)), fl.dp(gb) if gb is not None else None,
                               fl.dp(kb) if kb is not None else None, fl.dp(traj), fl.dp(U), C.byref(cost), C.byref(stp), C.byref(why))
    return traj, U, cost.value, stp.value, why.value, rc


def _lqg2d(L, fl):
    w = wl.c1_lqg2d().scaled(ngrid=(25, 23), rank=4)
    ctl = fl.Control(w, _lqg2d_callbacks(), device_model=False)
    vf = ctl.valuef(wl.synth_cores(w))
    L.valuef_attach_grid(vf, fl.ptrs([fl.f64(g) for g in ctl.xgrid()]))
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    return w, ctl, vf


def test_integrate_rk4_matches_numpy_rk4_over_the_controller():
    L, fl = _lib()
    w, ctl, vf = _lqg2d(L, fl)
    b_, _, st_, *_ = ctl._cb

    def controller(t, x):
        u = np.zeros(w.du)
        assert L.c3control_controller(C.c_double(t), fl.dp(fl.f64(x)), fl.dp(u), ctl.h) == 0
        return u

    def drift(x, u):
        b = np.zeros(w.dx)
        b_(0.0, fl.dp(fl.f64(x)), fl.dp(fl.f64(u)), fl.dp(b), None, None)
        return b

    def stage(x, u):
        s = np.zeros(1)
        st_(0.0, fl.dp(fl.f64(x)), fl.dp(fl.f64(u)), fl.dp(s), None)
        return s[0]

    dt_out, dt_int, nout, beta = 1e-2, 2.5e-3, 40, w.discount
    for x0 in ([-0.5, 0.5], [1.2, -0.7]):
        traj, U, J, stp, why, rc = host_integrate(L, fl, ctl, x0, "rk4", dt_int, dt_out, nout)
        assert rc == 0 and stp == -1 and why == 0
        x = np.array(x0)
        for j in range(nout):
            np.testing.assert_array_equal(U[j], controller(0.0, x))
            x = CL.simulate_rk4(drift, controller, x, dt_out, dt_out, dt_int)
            np.testing.assert_allclose(traj[j + 1], x, rtol=1e-13, atol=1e-13)
        # the cost component: RK4 of c' = e^{-beta t} stage(y, u(y)) on the same stages
        y, Jw, h = np.array(x0), 0.0, dt_int
        for k in range(nout * 4):
            t = k * h
            ks, cs, kq = np.zeros(w.dx), 0.0, np.zeros(w.dx)
            for q, (a, wq) in enumerate(((0.0, 1.0), (h / 2, 2.0), (h / 2, 2.0), (h, 1.0))):
                ys = y if q == 0 else y + a * kq
                u = controller(t + a, ys)
                kq = drift(ys, u)
                cq = np.exp(-beta * (t + a)) * stage(ys, u)
                ks, cs = (kq, cq) if q == 0 else (ks + wq * kq, cs + wq * cq)
            y, Jw = y + h / 6.0 * ks, Jw + h / 6.0 * cs
        np.testing.assert_allclose(y, traj[-1], rtol=1e-13, atol=1e-13)
        assert J == pytest.approx(Jw, rel=1e-13)
    # forward Euler with one substep is c3control_simulate with no noise, plus the cost
    traj, U, J, stp, why, rc = host_integrate(L, fl, ctl, [0.3, 0.4], "forward-euler", 0.0, dt_out, nout)
    ht, hu = np.zeros((nout + 1, w.dx)), np.zeros((nout, w.du))
    assert L.c3control_simulate(ctl.h, fl.dp(fl.f64([0.3, 0.4])), C.c_double(dt_out), C.c_size_t(nout), None, fl.dp(ht), fl.dp(hu)) == 0
    np.testing.assert_array_equal(traj, ht)
    np.testing.assert_array_equal(U, hu)
    L.valuef_destroy(vf)
    ctl.close()


def test_integrate_stops_freeze_the_state():
    L, fl = _lib()
    w, ctl, vf = _lqg2d(L, fl)
    inf = np.inf
    # keep-in box left after a few steps (x0 moves with x1 = 1.5 > 0): reason 4, frozen from then on, controls 0
    traj, U, J, stp, why, rc = host_integrate(L, fl, ctl, [0.0, 1.5], "rk4", 0.0, 0.02, 30, keep=([-inf, -inf], [0.1, inf]))
    assert rc == 0 and why == 4 and 0 < stp < 30
    assert traj[stp, 0] > 0.1 and traj[stp - 1, 0] <= 0.1
    assert (traj[stp:] == traj[stp]).all() and not U[stp:].any()
    # a goal box around the start: stop at step 0, nothing integrated
    traj, U, J, stp, why, rc = host_integrate(L, fl, ctl, [0.0, 1.5], "rk4", 0.0, 0.02, 30, goal=([-1, 1], [1, 2]))
    assert rc == 0 and (stp, why, J) == (0, 3, 0.0) and (traj == traj[0]).all() and not U.any()
    # the goal wins over the keep-in box when both hold
    _, _, _, stp, why, rc = host_integrate(L, fl, ctl, [0.0, 1.5], "rk4", 0.0, 0.02, 30, goal=([-1, 1], [1, 2]), keep=([1, 1], [2, 2]))
    assert rc == 0 and (stp, why) == (0, 3)
    L.valuef_destroy(vf)
    ctl.close()


def test_integrate_argument_errors(capfd):
    L, fl = _lib()
    w, ctl, vf = _lqg2d(L, fl)
    x0 = [0.1, 0.2]
    for method in ("rk45", "euler", ""):
        assert host_integrate(L, fl, ctl, x0, method, 0.0, 0.01, 5)[-1] == ERR_ARG
        assert "method" in capfd.readouterr().err
    assert host_integrate(L, fl, ctl, x0, "rk4", 0.003, 0.01, 5)[-1] == ERR_ARG  # nsub = 3.33
    assert "integer" in capfd.readouterr().err
    assert host_integrate(L, fl, ctl, x0, "rk4", 0.02, 0.01, 5)[-1] == ERR_ARG  # nsub = 0.5
    assert host_integrate(L, fl, ctl, x0, "rk4", -0.001, 0.01, 5)[-1] == ERR_ARG
    assert host_integrate(L, fl, ctl, x0, "rk4", 0.0, 0.0, 5)[-1] == ERR_ARG
    assert host_integrate(L, fl, ctl, x0, "rk4", 0.0, float("nan"), 5)[-1] == ERR_ARG
    assert host_integrate(L, fl, ctl, x0, "rk4", 0.01 / 3.0, 0.01, 5)[-1] == 0  # 3 substeps to rounding
    assert host_integrate(L, fl, ctl, x0, "rk4", 0.0, 0.01, 5, goal=([0, 1], [1, 0]))[-1] == ERR_ARG
    assert "goal" in capfd.readouterr().err
    assert host_integrate(L, fl, ctl, x0, "rk4", 0.0, 0.01, 5, keep=([0, np.nan], [1, 1]))[-1] == ERR_ARG
    assert "keep-in" in capfd.readouterr().err
    L.valuef_destroy(vf)
    ctl.close()


def _batch(L, fl, ctl, n=4, x0=True, method="rk4", dt_int=0.0, dt_out=0.01, nout=5, goal=None, wrap=0, save_every=0, traj=None):
    x = fl.f64(np.zeros((min(n, 4), ctl.w.dx))) if x0 else None  # never read past the argument checks
    gb = fl.f64(goal) if goal is not None else None
    return L.c3control_integrate_batch(ctl.h, n, fl.dp(x) if x0 else None, method.encode(), dt_int, dt_out, nout,
                                       fl.dp(gb) if gb is not None else None, None, wrap, save_every,
                                       fl.dp(traj) if traj is not None else None, None, None, None, None, None)


def test_integrate_batch_argument_errors(capfd):
    L, fl = _lib()
    w = wl.c2_dubins().scaled(ngrid=(11, 11, 10), rank=4)
    cores = wl.synth_cores(w)
    ctl = fl.Control(w, device_model=False)
    vf = ctl.valuef(cores)
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    assert _batch(L, fl, ctl) == ERR_ARG
    assert "device model" in capfd.readouterr().err
    ctl.close()
    ctl = fl.Control(w)
    assert _batch(L, fl, ctl) == ERR_ARG
    assert "c3control_add_policy_sim" in capfd.readouterr().err
    vf = ctl.valuef(cores)
    tr = TRANSFORM_FN(lambda n, x, y: None)
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, tr)
    assert _batch(L, fl, ctl, wrap=0) == ERR_ARG
    assert "transform" in capfd.readouterr().err
    assert _batch(L, fl, ctl, wrap=1, dt_out=0.0) == ERR_ARG  # accepted with the flag, up to the bad step
    assert "dt_out" in capfd.readouterr().err
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    assert _batch(L, fl, ctl, method="midpoint") == ERR_ARG
    assert _batch(L, fl, ctl, dt_int=0.004) == ERR_ARG
    assert _batch(L, fl, ctl, goal=[0, 0, 0, -1, 1, 1]) == ERR_ARG
    assert _batch(L, fl, ctl, x0=False) == ERR_ARG
    assert _batch(L, fl, ctl, save_every=0, traj=np.zeros((4, 6, 3))) == ERR_ARG
    assert _batch(L, fl, ctl, n=(1 << 31) + 1) == ERR_ARG
    assert _batch(L, fl, ctl, nout=(1 << 30) + 1) == ERR_ARG
    assert _batch(L, fl, ctl, n=0, x0=False) == 0  # nothing to do
    ctl.close()
