"""The switch word of a context (c3sc_hip_set_horizon_step / _stopping / _jumps / _correlation / _impulses): no bit
goes stale.  One context with the 2-D LQR with jumps and a correlated pair, compiled once with horizon, stop, jumps and corr at
rank 4, walks the 16 settings of {horizon step, stopping, jumps, correlation} in Gray-code order and back, one switch per step and
one Bellman call per setting, on the ragged 21 x 70 grid with 48 fibers.  Every result equals corr_lib's numpy restatement of that
setting to 1e-12 of the value scale (the bound of test_gpu_corr.py) and, bit for bit, the result of a fresh context put straight
into the setting; every switch moves the values.  Then interventions: while they are on, stopping, the horizon step and
correlation are refused -- by the model that has no such kernels, and by the rule when the model that has them is set again --
and accepted once they are off."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import backup_ref as BR
import corr_lib as CL
import impulse_lib as IL
import jump_lib as JL
import stop_lib as SL

pytestmark = pytest.mark.gpu
ERR_UNSUPPORTED = 3
HORIZON, STOP, JUMP, CORR = 1, 2, 4, 8  # the bits of a setting in this test
DELTA = 0.01  # Q delta / h^2 < 0.8 on the ragged grid (test_gpu_corr.py: LQR_DELTA)
K, NFIB = 0, 48


def _switch(eng, bit, on):
    if bit == HORIZON:
        eng.set_horizon_step(DELTA if on else 0.0)
    elif bit == STOP:
        eng.set_stopping(on)
    elif bit == JUMP:
        eng.set_jumps(on)
    else:
        eng.set_correlation(on)


def test_gray_code_walk_of_the_switches_leaves_no_stale_bit():
    # the model of test_gpu_corr.py's "lqr_jump" (the same spec and name: one compile per process)
    mid = E.compile_model(CL.LQR_JUMP, 2, 2, ranks=(4,), name="lqr_cd_jump", horizon=True, stop=True, njump=JL.LQR_NJUMP,
                          corr_pairs=CL.LQR_PAIRS, **CL.LQR_MASKS)
    w = CL.lqr_workload(mid, 4, 0.3, JL.LQR_PRM)
    cores = wl.synth_cores(w)
    idx = wl.synth_fibers(w, K, NFIB)
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    costs, ab = eng.stencil_fibers_host(K, idx)
    assert (ab == 1).any() and (ab == -1).any() and (ab == 0).any(), "fibers must include boundary, obstacle and live nodes"
    tr, Vfull = JL.Train(w, cores), CL.full_values(w, cores)
    bcost, ocost = (lambda x: SL.lqrn_terminal(w.params, x)), (lambda x: np.full(len(x), 5.0))

    def reference(s, psi):
        return CL.corr_fibers(w, SL.lqrn_host, CL.lqr_jump_covar, CL.LQR_PAIRS, Vfull, K, idx, costs, ab, bcost, ocost,
                              DELTA if s & HORIZON else None, psi if s & STOP else None, jumps=JL.lqr_jumps if s & JUMP else None,
                              interp=tr, with_corr=bool(s & CORR))[0]

    # psi's constant between two nodes' continuation values at their median, so that both decisions occur (test_gpu_corr.py: _case)
    x = BR.node_states(w, K, idx).reshape(-1, w.dx)
    live = ab.reshape(-1) == 0
    v = np.unique(reference(JUMP | CORR, None).reshape(-1)[live] - w.params[5] * (x[live] ** 2).sum(-1))
    c0 = float(0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]))
    w = dataclasses.replace(w, params=w.params[:4] + (c0,) + w.params[5:])
    tr.w = w
    eng.set_model(w.model, w.params)
    eng.w = w
    psi = lambda xx: SL.lqr_psi(w.params, xx)

    ref, fresh = {}, {}
    for s in range(16):
        ref[s] = reference(s, psi)
        f = E.BellmanEngine(0)
        f.configure(w, cores)
        for bit in (CORR, JUMP, STOP, HORIZON):
            if s & bit:
                _switch(f, bit, True)
        fresh[s] = f.bellman_fibers_host(K, idx)
        f.close()
        err = np.abs(fresh[s][0] - ref[s]).max()
        print("setting", s, "fresh context vs numpy: max err", err)
        assert np.all(np.abs(fresh[s][0] - ref[s]) <= 1e-12 * np.maximum(1.0, np.abs(ref[s]))), (s, err)
    for s in range(16):
        for bit in (HORIZON, STOP, JUMP, CORR):
            assert not np.array_equal(ref[s], ref[s ^ bit]), ("precondition: every switch moves the values", s, bit)

    gray = [i ^ (i >> 1) for i in range(16)]
    walk, cur = gray + gray[-2::-1], 0  # 0 ... 8 and back to 0: 31 settings, one switch apart
    for s in walk:
        for bit in (HORIZON, STOP, JUMP, CORR):
            if (s ^ cur) & bit:
                _switch(eng, bit, bool(s & bit))
        cur = s
        out, ui, fab = eng.bellman_fibers_host(K, idx)
        assert eng.last_kernel().startswith("k_fiber_per_wave<rtc:")
        assert np.all(np.abs(out - ref[s]) <= 1e-12 * np.maximum(1.0, np.abs(ref[s]))), (s, np.abs(out - ref[s]).max())
        np.testing.assert_array_equal(out, fresh[s][0], err_msg=f"setting {s}: values differ from a fresh context's")
        np.testing.assert_array_equal(ui, fresh[s][1], err_msg=f"setting {s}: indices differ from a fresh context's")
        np.testing.assert_array_equal(fab, fresh[s][2])
    assert cur == 0

    # interventions: a model compiled for them (test_gpu_impulse.py's "lqr": the same spec and name)
    L = E.load_library()
    err = lambda: L.c3sc_hip_last_error(eng.h).decode()
    iid = E.compile_model(IL.LQR_JUMP, 2, 2, ranks=(4, 8, 12), name="lqr_ic", njump=JL.LQR_NJUMP, nimpulse=IL.LQR_NIMPULSE, **IL.LQR_MASKS)
    wi = IL.lqr_workload(iid, 4, 0.1, IL.lqr_cost_scale(4))
    refusals = (("stopping", lambda: L.c3sc_hip_set_stopping(eng.h, 1)), ("horizon", lambda: L.c3sc_hip_set_horizon_step(eng.h, C.c_double(DELTA))),
                ("correlated noise", lambda: L.c3sc_hip_set_correlation(eng.h, 1)))
    eng.set_model(iid, wi.params)
    eng.set_impulses(True)
    for what, call in refusals:  # this model has no such kernels
        assert call() == ERR_UNSUPPORTED, what
    eng.set_model(w.model, w.params)  # this one has, and the interventions are still on: the rule refuses
    for what, call in refusals:
        assert call() == ERR_UNSUPPORTED, what
        assert "interventions" in err() and what in err(), err()
    assert L.c3sc_hip_set_impulses(eng.h, 0) == 0
    for what, call in refusals:
        assert call() == 0, (what, err())
    out, ui, fab = eng.bellman_fibers_host(K, idx)  # horizon, stop and corr on, jumps off
    np.testing.assert_array_equal(out, fresh[HORIZON | STOP | CORR][0])
    np.testing.assert_array_equal(ui, fresh[HORIZON | STOP | CORR][1])
    eng.close()
