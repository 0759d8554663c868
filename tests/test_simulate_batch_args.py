"""c3control_simulate_batch (libc3sc.so, include/c3sc/bellman.h): the argument checks that run before any device work return a
non-zero code with a message instead of aborting.  No GPU involved."""
import ctypes as C

import numpy as np

from c3sc_amd import workloads as wl

ERR_ARG = 1
TRANSFORM_FN = C.CFUNCTYPE(None, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double))


def _lib():
    import facade_lib

    L = facade_lib.lib()
    dpp = C.POINTER(C.c_double)
    L.c3control_simulate_batch.argtypes = [C.c_void_p, C.c_size_t, dpp, C.c_double, C.c_size_t, C.c_uint64, dpp, C.c_int, C.c_size_t,
                                           dpp, dpp, dpp, C.POINTER(C.c_long), dpp]
    L.c3control_simulate_batch.restype = C.c_int
    return L, facade_lib


def _call(L, fl, ctl, n=4, x0=True, dt=0.01, nsteps=5, wrap=0, save_every=0, traj=None):
    x = fl.f64(np.zeros((min(n, 4), ctl.w.dx))) if x0 else None  # never read past the argument checks
    return L.c3control_simulate_batch(ctl.h, n, fl.dp(x) if x0 else None, dt, nsteps, 1, None, wrap, save_every,
                                      fl.dp(traj) if traj is not None else None, None, None, None, None)


def test_simulate_batch_argument_errors(capfd):
    L, fl = _lib()
    w = wl.c2_dubins().scaled(ngrid=(11, 11, 10), rank=4)
    cores = wl.synth_cores(w)
    # no device model
    ctl = fl.Control(w, device_model=False)
    vf = ctl.valuef(cores)
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    assert _call(L, fl, ctl) == ERR_ARG
    assert "device model" in capfd.readouterr().err
    ctl.close()
    # no policy_sim
    ctl = fl.Control(w)
    assert _call(L, fl, ctl) == ERR_ARG
    assert "c3control_add_policy_sim" in capfd.readouterr().err
    # a host transform without the wrap flag; accepted with it (up to the device work, not run here: bad dt stops it)
    vf = ctl.valuef(cores)
    tr = TRANSFORM_FN(lambda n, x, y: None)
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, tr)
    assert _call(L, fl, ctl, wrap=0) == ERR_ARG
    assert "transform" in capfd.readouterr().err
    assert _call(L, fl, ctl, wrap=1, dt=0.0) == ERR_ARG
    assert "dt" in capfd.readouterr().err
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    # bad sizes / arguments
    assert _call(L, fl, ctl, dt=-1.0) == ERR_ARG
    assert _call(L, fl, ctl, dt=float("nan")) == ERR_ARG
    assert _call(L, fl, ctl, x0=False) == ERR_ARG
    assert _call(L, fl, ctl, save_every=0, traj=np.zeros((4, 6, 3))) == ERR_ARG
    assert _call(L, fl, ctl, n=(1 << 31) + 1) == ERR_ARG
    assert _call(L, fl, ctl, nsteps=(1 << 30) + 1) == ERR_ARG
    assert _call(L, fl, ctl, n=0, x0=False) == 0  # nothing to do
    ctl.close()
