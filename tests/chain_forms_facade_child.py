"""The reference API of the Markov chain in stopping and jump mode (c3control_simulate_chain_batch, libc3sc.so) on jump_lib's
lqr_jd with a chain-compiled device model -- run in a child process by tests/test_gpu_chain_forms.py: 64 walks of 24 steps with
supplied (v, u1) and with Philox, replayed in lock-step by chain_forms_ref.check; the same control refuses the one-trajectory
host twin, and a device model without chain kernels gets the batch call's old answer."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import chain_forms_ref as CF  # noqa: E402
import jump_lib as JL  # noqa: E402
import stop_lib as SL  # noqa: E402
from chain_facade_child import facade, i32p, dpp  # noqa: E402

NTRAJ = 64


def control(L, fl, mid):
    w, cores, ref = CF.case("lqr", mid, 4, (False, True, True))
    cbs, stop_cb = SL.lqr_callbacks(w.params)
    ctl = fl.Control(w, callbacks=cbs, consistent_ends=None)
    L.c3control_add_stopcost(ctl.h, stop_cb)
    L.c3control_set_stopping.argtypes = [C.c_void_p, C.c_int]
    L.c3control_set_stopping(ctl.h, 1)
    keep = JL.add_jumps(L, ctl, JL.lqr_jumps, w.params, 2, JL.LQR_NJUMP)
    vf = ctl.valuef(cores)
    L.valuef_attach_grid(vf, fl.ptrs([fl.f64(g) for g in ctl.xgrid()]))
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    return w, ref, ctl, (cbs, stop_cb, keep, vf)


def batch(L, ctl, node0, K, seed, unif):
    n, d = node0.shape
    traj, ui = np.zeros((n, K + 1, d), np.int32), np.zeros((n, K), np.int32)
    cost, disc, time, vend = (np.zeros(n) for _ in range(4))
    ex, node = np.zeros(n, np.int64), np.zeros((n, d), np.int32)
    rc = L.c3control_simulate_chain_batch(ctl.h, n, node0.ctypes.data_as(i32p), K, seed, None if unif is None else unif.ctypes.data_as(dpp), 1,
                                          traj.ctypes.data_as(i32p), ui.ctypes.data_as(i32p), cost.ctypes.data_as(dpp),
                                          disc.ctypes.data_as(dpp), time.ctypes.data_as(dpp), vend.ctypes.data_as(dpp),
                                          ex.ctypes.data_as(C.POINTER(C.c_long)), node.ctypes.data_as(i32p))
    return rc, {"node0": node0, "nsteps": K, "traj": traj, "uidx": ui, "cost": cost, "disc": disc, "time": time, "vend": vend, "exit": ex,
                "node": node}


def main():
    from c3sc_amd import engine as E

    L, fl = facade()
    kw = dict(stop=True, njump=JL.LQR_NJUMP, **JL.LQR_MASKS)
    mid = E.compile_model(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc_api", chain=True, **kw)
    w, ref, ctl, keep = control(L, fl, mid)
    node0 = np.ascontiguousarray(CF.start_nodes(ref)[:NTRAJ])
    K = CF.NSTEPS
    unif = np.random.default_rng(CF.SEED + 5).random((NTRAJ, K, 2))
    rc, run = batch(L, ctl, node0, K, 0, unif)
    assert rc == 0, rc
    run["uniform"] = unif
    out = ref.check(run)
    rc, run = batch(L, ctl, node0, K, CF.SEED, None)
    assert rc == 0, rc
    run["uniform"] = CF.Ref.uniforms(CF.SEED, 0, NTRAJ, K)
    out2 = ref.check(run)
    kinds = {E.decode_chain_exit(int(e))[1] for e in run["exit"]}
    assert {"stopped", "exit", "running"} <= kinds, kinds
    # the one-trajectory host twin keeps the plain form: this control is in a mode
    one = np.zeros(2 * K)
    assert L.c3control_simulate_chain(ctl.h, node0.ctypes.data_as(i32p), K, one.ctypes.data_as(dpp), None, None, None, None, None, None, None) == 1
    # a device model without chain kernels: the batch call's old answer
    mid0 = E.compile_model(JL.LQR, 2, 2, ranks=(4,), name="lqr_cd_api", **kw)
    w0, ref0, ctl0, keep0 = control(L, fl, mid0)
    rc0, _ = batch(L, ctl0, node0, K, CF.SEED, None)
    assert rc0 == 1, rc0
    print(f"chain forms facade: {out['steps']} + {out2['steps']} steps held to the numpy walk, {out['unsure'] + out2['unsure']} unsure")


if __name__ == "__main__":
    main()
