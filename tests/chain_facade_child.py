"""The reference API of the Markov chain (c3control_simulate_chain, c3control_simulate_chain_batch; libc3sc.so) on the lqg2d
case of tests/chain_cases.py -- TEST INFRASTRUCTURE ONLY.  tests/test_chain_host.py calls host_twin_against_reference in process
(no GPU); tests/test_gpu_chain_facade.py runs this file as a child process, which holds the batch form to the host twin:

    python tests/chain_facade_child.py

Rules, as in chain_ref.check: a step whose decision has a runner-up within MARGIN_TOL, or whose uniform lies within SAMPLE_TOL of
a cumulative probability, is unsure.  A lane without an unsure step is held to the host twin's whole walk: nodes, decisions and
exit word exactly, J, D, T and vend to TOL max(1, |.|).  In a lane with one, every sure step is replayed by a one-step host
walk from the device's own node: the decision and the next node exactly."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import chain_cases as cc  # noqa: E402
import chain_ref  # noqa: E402

NTRAJ = 32
i32p, dpp = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def facade():
    import facade_lib

    L = facade_lib.lib()
    L.c3control_simulate_chain.argtypes = [C.c_void_p, i32p, C.c_size_t, dpp, i32p, i32p, dpp, dpp, dpp, dpp, C.POINTER(C.c_long)]
    L.c3control_simulate_chain.restype = C.c_int
    L.c3control_simulate_chain_batch.argtypes = [C.c_void_p, C.c_size_t, i32p, C.c_size_t, C.c_uint64, dpp, C.c_size_t, i32p, i32p,
                                                 dpp, dpp, dpp, dpp, C.POINTER(C.c_long), i32p]
    L.c3control_simulate_chain_batch.restype = C.c_int
    return L, facade_lib


def problem(L, fl, beta=0.1):
    from test_policy_tail import _lqg2d_callbacks

    case = cc.CASES[0]
    w = cc.workload(case, beta)
    cores = cc.cores(case, w, False)
    ctl = fl.Control(w, _lqg2d_callbacks(), consistent_ends=None)
    vf = ctl.valuef(cores)
    L.valuef_attach_grid(vf, fl.ptrs([fl.f64(g) for g in ctl.xgrid()]))
    L.c3control_add_policy_sim(ctl.h, vf, ctl.opt, None)
    return w, cores, ctl, vf


def host_walk(L, ctl, d, node0, unif):
    """one walk of the host twin in the layout of a one-lane run of chain_ref"""
    K = len(unif)
    node0 = np.ascontiguousarray(node0, dtype=np.int32)
    u = np.ascontiguousarray(unif, dtype=np.float64)
    traj, ui = np.zeros((K + 1, d), np.int32), np.zeros(max(K, 1), np.int32)
    out = [C.c_double(0) for _ in range(4)]
    ex = C.c_long(0)
    rc = L.c3control_simulate_chain(ctl.h, node0.ctypes.data_as(i32p), K, u.ctypes.data_as(dpp), traj.ctypes.data_as(i32p),
                                    ui.ctypes.data_as(i32p), *[C.byref(o) for o in out], C.byref(ex))
    assert rc == 0, rc
    return {"traj": traj, "uidx": ui[:K], "cost": out[0].value, "disc": out[1].value, "time": out[2].value, "vend": out[3].value,
            "exit": ex.value}


def host_twin_against_reference(nlanes=64):
    """the host twin's walks replayed by the numpy reference (chain_ref.check); returns its counts"""
    L, fl = facade()
    w, cores, ctl, vf = problem(L, fl)
    R = chain_ref.ChainRef(w, cores)
    node0 = cc.start_nodes(w)[:nlanes]
    unif = np.random.default_rng(cc.SEED + 2).random((nlanes, cc.NSTEPS))
    walks = [host_walk(L, ctl, w.dx, node0[i], unif[i]) for i in range(nlanes)]
    run = {"node0": node0, "nsteps": cc.NSTEPS, "uniform": unif}
    for k in ("traj", "uidx", "cost", "disc", "time", "vend", "exit"):
        run[k] = np.array([wk[k] for wk in walks])
    run["node"] = run["traj"][:, -1]
    out = R.check(run)
    L.valuef_destroy(vf)
    ctl.close()
    return out


def _close(a, b):
    return abs(a - b) <= chain_ref.TOL * max(1.0, abs(b))


def batch_against_host_twin():
    L, fl = facade()
    w, cores, ctl, vf = problem(L, fl)
    R = chain_ref.ChainRef(w, cores)
    d, K, n = w.dx, cc.NSTEPS, NTRAJ
    node0 = np.ascontiguousarray(cc.start_nodes(w)[:n])
    unif = np.random.default_rng(cc.SEED + 3).random((n, K))
    traj, ui = np.zeros((n, K + 1, d), np.int32), np.zeros((n, K), np.int32)
    cost, disc, time, vend = (np.zeros(n) for _ in range(4))
    ex, node = np.zeros(n, np.int64), np.zeros((n, d), np.int32)
    rc = L.c3control_simulate_chain_batch(ctl.h, n, node0.ctypes.data_as(i32p), K, 0, unif.ctypes.data_as(dpp), 1, traj.ctypes.data_as(i32p),
                                          ui.ctypes.data_as(i32p), cost.ctypes.data_as(dpp), disc.ctypes.data_as(dpp),
                                          time.ctypes.data_as(dpp), vend.ctypes.data_as(dpp), ex.ctypes.data_as(C.POINTER(C.c_long)),
                                          node.ctypes.data_as(i32p))
    assert rc == 0, rc
    whole = steps = 0
    for i in range(n):
        unsure = []
        for s in range(K):
            nd = R.node(traj[i, s])
            live = nd.flag == 0 and (ex[i] == -1 or s < ex[i])
            unsure.append(live and (len(R.acceptable(nd)) > 1 or R.pick(unif[i, s], R.transitions(nd, max(int(ui[i, s]), 0)).P)[1]))
        if not any(unsure):
            h = host_walk(L, ctl, d, node0[i], unif[i])
            assert np.array_equal(h["traj"], traj[i]) and np.array_equal(h["uidx"], ui[i]) and h["exit"] == ex[i], i
            assert _close(cost[i], h["cost"]) and _close(disc[i], h["disc"]) and _close(time[i], h["time"]) and _close(vend[i], h["vend"]), i
            assert np.array_equal(node[i], traj[i, K])
            whole += 1
            continue
        for s in range(K):
            if unsure[s] or not (ex[i] == -1 or s < ex[i]):
                continue
            h = host_walk(L, ctl, d, traj[i, s], unif[i, s:s + 1])
            assert h["uidx"][0] == ui[i, s] and np.array_equal(h["traj"][1], traj[i, s + 1]), (i, s)
            steps += 1
    assert whole >= n * 3 // 4, whole
    # the rejections of the batch form that need no further set-up
    assert L.c3control_simulate_chain_batch(ctl.h, n, None, K, 0, None, 0, None, None, None, None, None, None, None, None) == 1
    assert L.c3control_simulate_chain_batch(ctl.h, n, node0.ctypes.data_as(i32p), K, 0, None, 0, traj.ctypes.data_as(i32p), None,
                                            None, None, None, None, None, None) == 1
    bad = node0.copy()
    bad[3, 1] = w.ngrid[1]
    assert L.c3control_simulate_chain_batch(ctl.h, n, bad.ctypes.data_as(i32p), K, 0, None, 0, None, None, cost.ctypes.data_as(dpp),
                                            None, None, None, None, None) == 1
    print(f"chain facade: {whole} of {n} lanes held to the host twin's whole walk, {steps} single steps replayed")
    L.valuef_destroy(vf)
    ctl.close()


if __name__ == "__main__":
    batch_against_host_twin()
