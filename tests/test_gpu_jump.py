"""Jump diffusions on the GPU (c3sc_hip_set_jumps).

- The jump forms of the per-wave kernel against the numpy restatement of jump_lib on the ragged 21 x 70 grid (both NPL forms)
  with boundary, obstacle and periodic nodes, whose marks reach interior targets, targets beyond the absorbing face, inside the
  obstacle and across the periodic seam: ranks 4, 8 and 12, beta = 0.3 and 0, minimising and forced, horizon on and off, stop on
  and off.  The L2 form at rank 12 with unequal bond ranks on 5 x 128 x 5.  Values to 1e-12 of the value scale, flags and status
  bits exactly, indices wherever the reference's margin exceeds 1e-9 (a precondition holds that to 99.9 % of the nodes).
- lambda = 0 leaves the plain kernel's values, indices, flags and status bit for bit.
- CONSTELM and LINELM targets differ and agree with jump_lib in both classes.
- The known answer V = g / lambda + exp(-beta / lambda) c to 1e-14, and no STATIONARY bit although b = sigma = 0.
- Merton's American put solved stage by stage equals jump_lib's dense chain to 1e-9 at every stage.
- Rollouts: with zero normals and Philox jumps every lane's event steps, marks and states equal jump_lib's replay from the
  uniforms' host twin, lanes that jump out of the domain decode as exits and pay the discounted cost; with lambda = 0 a noisy
  run keeps the bits of the plain rollout kernel.
- Errors: a game, the box and TABLE calls, a forced pair or quad variant, integrate, a built-in model, a model compiled
  without njump (also one set after the switch)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import backup_ref as BR
import gpu_case_lib as GC
import horizon_lib as H
import jump_lib as JL
import stop_lib as SL

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 3
STATUS_STATIONARY, STATUS_CFL = 1, 2
LQR_DELTA, LQR3_DELTA = 0.01, 0.004  # (Q + h2 lambda) delta / h^2 < 0.8 on the ragged grids


@pytest.fixture(scope="module")
def ids():
    return {
        "lqr": E.compile_model(JL.LQR, 2, 2, ranks=(4, 8, 12), name="lqr_jd", horizon=True, stop=True, njump=JL.LQR_NJUMP, **JL.LQR_MASKS),
        "lqr3": E.compile_model(JL.LQR3, 3, 3, ranks=(12,), name="lqr3_jd", horizon=True, stop=True, njump=JL.LQR3_NJUMP, **JL.LQR3_MASKS),
        "known": E.compile_model(JL.KNOWN, 2, 1, ranks=(4,), name="known_jd", njump=JL.KNOWN_NJUMP, **JL.KNOWN_MASKS),
        "put": E.compile_model(JL.PUT, 2, 1, ranks=(12,), name="put_jd", horizon=True, stop=True, njump=JL.PUT_NJUMP, **JL.PUT_MASKS),
        "lqr_nojump": E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_nojump", **SL.LQR_MASKS),
        "lqr_jump_only": E.compile_model(JL.LQR, 2, 2, ranks=(4,), name="lqr_jump_only", njump=JL.LQR_NJUMP, **JL.LQR_MASKS),
    }


def _costs(model):
    prm = JL.LQR_PRM if model == "lqr" else JL.LQR3_PRM
    return (lambda x: SL.lqrn_terminal(prm, x)), (lambda x: np.full(len(x), 5.0))


def _case(ids, model, rank, discount, horizon, stop):
    """(engine with jumps on, workload, train, psi or None, delta or None) of one case; with stop, psi's constant is put at the
    median of the reference's continuation values, so that both decisions occur"""
    if model == "lqr":
        w, jumps, k0 = JL.lqr_workload(ids["lqr"], rank, discount), JL.lqr_jumps, 0
    else:
        w, jumps, k0 = JL.lqr3_workload(ids["lqr3"], discount=discount), JL.lqr3_jumps, 1
    delta = (LQR_DELTA if model == "lqr" else LQR3_DELTA) if horizon else None
    cores = wl.synth_cores(w)
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    tr = JL.Train(w, cores)
    psi = None
    if stop:
        bcost, ocost = _costs(model)
        idx = wl.synth_fibers(w, k0, 64)
        costs, ab = eng.stencil_fibers_host(k0, idx)
        out, _, _, _, _, _, _ = JL.jump_fibers(w, SL.lqrn_host, jumps, tr, k0, idx, costs, ab, bcost, ocost, delta)
        x = BR.node_states(w, k0, idx).reshape(-1, w.dx)
        live = ab.reshape(-1) == 0
        c1 = w.params[5]
        v = np.unique(out.reshape(-1)[live] - c1 * (x[live] ** 2).sum(-1))
        c0 = float(0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]))  # between two nodes' values: psi ties with no continuation value
        w = dataclasses.replace(w, params=w.params[:4] + (c0,) + w.params[5:])
        eng.set_model(w.model, w.params)
        eng.w = w
        tr.w = w
        psi = lambda xx: SL.lqr_psi(w.params, xx)
        eng.set_stopping(True)
    if delta is not None:
        eng.set_horizon_step(delta)
    eng.set_jumps(True)
    return eng, w, jumps, tr, psi, delta


def _check_case(ids, model, rank, discount, horizon, stop, ks=(0, 1), constelm=False):
    eng, w, jumps, tr, psi, delta = _case(ids, model, rank, discount, horizon, stop)
    bcost, ocost = _costs(model)
    if constelm:
        eng.set_interp(True)
    nc = w.ncand
    kernels, kinds = set(), np.zeros(4, dtype=bool)
    for k in ks:
        idx = wl.synth_fibers(w, k, 257)
        eng.status(clear=True)
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        status = eng.status(clear=True)
        kernels.add(eng.last_kernel())
        assert eng.last_kernel().startswith("k_fiber_per_wave<rtc:")
        costs, sab = eng.stencil_fibers_host(k, idx)
        np.testing.assert_array_equal(ab, sab)  # flags bit-exact
        assert (ab == 1).any() and (ab == -1).any() and (ab == 0).any(), "fibers must include boundary, obstacle and live nodes"
        r_out, r_ui, mg, stat, cfl, rate, J = JL.jump_fibers(w, SL.lqrn_host, jumps, tr, k, idx, costs, ab, bcost, ocost, delta, psi,
                                                             constelm=constelm)
        scale = np.maximum(1.0, np.abs(r_out))
        print(model, rank, discount, horizon, stop, k, "max err", np.abs(out - r_out).max(), "unsure share", (mg <= 1e-9).mean(),
              "max rate", rate.max(), "J range", J.min(), J.max())
        assert np.all(np.abs(out - r_out) <= 1e-12 * scale), (k, np.abs(out - r_out).max())
        live = ab == 0
        assert (mg[live] <= 1e-9).mean() <= 0.001, "precondition: the reference's own decisions are clear at 99.9 % of the nodes"
        sure = mg > 1e-9
        np.testing.assert_array_equal(ui[sure], r_ui[sure])
        assert (ui[live] >= 0).all() and (ui[~live] == -1).all()
        if stop:
            assert (ui[live] == nc).any() and (ui[live] < nc).any(), "both decisions occur"
        assert bool(status & STATUS_STATIONARY) == bool(stat.any()) and bool(status & STATUS_CFL) == bool(cfl.any()), status
        assert status == 0, "the cases stay inside the CFL rule and have no stationary node"
        # the kinds of target the marks reach from the live nodes of these fibers
        x = BR.node_states(w, k, idx).reshape(-1, w.dx)[live.reshape(-1)]
        _, _, y = jumps(w.params, x)
        for m in range(y.shape[1]):
            _, inobs, beyond, moved = JL.target_kinds(w, y[:, m])
            kinds |= np.array([(~inobs & ~beyond & ~moved).any(), (beyond & ~inobs).any(), inobs.any(), moved.any()])
        # the forced path shares Q0 and PV0: the minimising run's own indices reproduce its values, a random policy its own
        f_out, f_ab = eng.policy_fibers_host(k, idx, ui)
        np.testing.assert_array_equal(f_ab, ab)
        assert np.all(np.abs(f_out - out) <= 1e-12 * scale), (k, np.abs(f_out - out).max())
        rng = np.random.default_rng(rank + k)
        pol = rng.integers(0, nc + (1 if stop else 0), size=ab.shape).astype(np.int32)
        q_out, _ = eng.policy_fibers_host(k, idx, pol)
        q_ref = JL.jump_fibers(w, SL.lqrn_host, jumps, tr, k, idx, costs, ab, bcost, ocost, delta, psi, forced=pol, constelm=constelm)[0]
        assert np.all(np.abs(q_out - q_ref) <= 1e-12 * np.maximum(1.0, np.abs(q_ref))), (k, np.abs(q_out - q_ref).max())
    return kernels, kinds, eng


@pytest.mark.parametrize("rank", [4, 8, 12])
@pytest.mark.parametrize("discount", [0.3, 0.0])
@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
@pytest.mark.parametrize("stop", [False, True], ids=["nostop", "stop"])
def test_per_wave_jump_vs_numpy(ids, rank, discount, horizon, stop):
    kernels, kinds, _ = _check_case(ids, "lqr", rank, discount, horizon, stop)
    assert all(f",{rank}," in k for k in kernels), kernels
    assert any(",1>" in k for k in kernels) and any(",2>" in k for k in kernels), kernels  # N = 21 and N = 70: both NPL forms
    assert kinds.all(), ("interior, beyond the absorbing face, inside the obstacle, across the seam", kinds)


@pytest.mark.parametrize("discount", [0.3, 0.0])
@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
@pytest.mark.parametrize("stop", [False, True], ids=["nostop", "stop"])
def test_per_wave_jump_rank_12_l2_form(ids, discount, horizon, stop):
    """bond ranks 12 and 9, padded to 12: a launch along the 128-node middle dimension needs more than the 160 KB the launcher
    stages in, so the jump kernel that reads the varying core from global memory runs"""
    w = JL.lqr3_workload(ids["lqr3"], discount=discount)
    cw = 3 + 1 + 2 * 3 + 1
    assert GC.fpw_lds_bytes(w, 1, 12, 2, cw) > 160 * 1024, "the staged form would fit: this case would not run the L2 form"
    assert GC.fpw_lds_bytes(w, 1, 12, 2, cw) - 8 * 128 * 145 < 160 * 1024  # ... and the L2 form's own layout fits
    kernels, kinds, _ = _check_case(ids, "lqr3", 12, discount, horizon, stop, ks=(1,))
    assert kernels == {"k_fiber_per_wave<rtc:lqr3_jd,12,2>"}, kernels
    assert kinds[0] and kinds[1] and kinds[3]


@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
@pytest.mark.parametrize("stop", [False, True], ids=["nostop", "stop"])
@pytest.mark.parametrize("discount", [0.3, 0.0])
def test_zero_rate_equals_the_plain_kernel_bit_for_bit(ids, horizon, stop, discount):
    w = JL.lqr_workload(ids["lqr"], 4, discount, JL.LQR_ZERO_RATE_PRM)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    if horizon:
        eng.set_horizon_step(LQR_DELTA)
    eng.set_stopping(stop)
    for k in (0, 1):
        idx = wl.synth_fibers(w, k, 129)
        eng.set_jumps(False)
        eng.status(clear=True)
        p_out, p_ui, p_ab = eng.bellman_fibers_host(k, idx)
        p_kernel, p_st = eng.last_kernel(), eng.status(clear=True)
        eng.set_jumps(True)
        j_out, j_ui, j_ab = eng.bellman_fibers_host(k, idx)
        assert eng.last_kernel() == p_kernel  # the entry is the same; the launcher takes its jump form
        np.testing.assert_array_equal(j_out, p_out)
        np.testing.assert_array_equal(j_ui, p_ui)
        np.testing.assert_array_equal(j_ab, p_ab)
        assert eng.status(clear=True) == p_st
    # ... and with the rate back the values move: the switch does select another kernel
    eng.set_model(w.model, JL.LQR_PRM)
    m_out, _, _ = eng.bellman_fibers_host(1, idx)
    assert np.abs(m_out - p_out)[p_ab == 0].max() > 1e-3


def test_constelm_and_linelm_targets(ids):
    _, _, eng = _check_case(ids, "lqr", 4, 0.3, False, False, ks=(1,), constelm=True)
    idx = wl.synth_fibers(eng.w, 1, 257)
    c_out, _, ab = eng.bellman_fibers_host(1, idx)
    eng.set_interp(False)
    l_out, _, _ = eng.bellman_fibers_host(1, idx)
    live = ab == 0
    assert (np.abs(c_out - l_out)[live] > 1e-6 * np.abs(l_out[live])).mean() > 0.5, "off-node targets: the classes differ"
    _check_case(ids, "lqr", 4, 0.3, False, False, ks=(1,), constelm=False)


def test_known_answer(ids):
    w = JL.known_workload(ids["known"])
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    ref = JL.known_answer()
    for k in (0, 1):
        idx = wl.synth_fibers(w, k, 16)
        eng.set_jumps(False)
        eng.status(clear=True)
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        live = ab == 0
        assert live.any() and (out[live] == 0.0).all() and (ui[live] == -1).all()
        assert eng.status(clear=True) & STATUS_STATIONARY  # without jumps every live node is stationary
        eng.set_jumps(True)
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        assert eng.status(clear=True) == 0, "lambda > 0: Q > 0, the node is not stationary"
        assert (ui[live] == 0).all()
        err = np.abs(out[live] - ref).max() / ref
        print("known answer", ref, "max rel err", err)
        assert err <= 1e-14
        assert (out[ab == 1] == JL.KNOWN_PRM[2]).all()


# ---------------------------------------------------------------------------------------------------- the Merton put, stage by stage
@pytest.fixture(scope="module")
def put_solve(ids):
    """Merton's put solved stage by stage on the device (jump, stop and horizon forms, each stage uploaded as its exact train)
    and by the dense chain: (engine, device stages, dense stages, trains, workload, device indices, dense indices)"""
    w = JL.put_workload(ids["put"], rank=11)
    psi = lambda x: SL.put_psi(JL.PUT_PRM, x)
    dense, dec, cfl = JL.dense_chain(w, SL.put_host, JL.put_jumps, psi, JL.PUT_DELTA, JL.PUT_STAGES)
    plain, _, _ = SL.dense_chain(dataclasses.replace(w, params=SL.PUT_PRM), SL.put_host, psi, JL.PUT_DELTA, JL.PUT_STAGES)
    assert not cfl
    assert np.abs(dense[0] - plain[0]).max() > 1e-3, "the jumps move the price"
    eng = E.BellmanEngine(0)
    n = SL.PUT_N
    Vn = dense[-1]
    ranks, cores = GC.train(Vn, 12)
    eng.configure(dataclasses.replace(w, ranks=tuple(ranks)), cores)
    eng.set_horizon_step(JL.PUT_DELTA)
    eng.set_stopping(True)
    eng.set_jumps(True)
    idx = np.zeros((n, 2), dtype=np.int32)
    idx[:, 1] = np.arange(n)
    dev, uis, trains = [Vn], [], [(ranks, cores)]
    for _ in range(JL.PUT_STAGES):
        eng.upload_value(ranks, cores)
        out, ui, ab = eng.bellman_fibers_host(0, idx)  # fiber j along dim 0: out[j, i] = V_n(x_i, x_j)
        Vn = np.ascontiguousarray(out.T)
        dev.append(Vn)
        uis.append(np.ascontiguousarray(ui.T))
        ranks, cores = GC.train(Vn, 12)
        trains.append((ranks, cores))
    assert eng.status() == 0
    return eng, np.array(dev[::-1]), dense, trains[::-1], w, uis, dec


def test_stage_by_stage_merton_put_equals_the_dense_chain(put_solve):
    _, dev, dense, _, w, uis, dec = put_solve
    assert dev.shape == dense.shape
    for s in range(dev.shape[0]):
        err = np.abs(dev[s] - dense[s]).max() / max(1.0, np.abs(dense[s]).max())
        assert err <= 1e-9, (s, err)
    inner = (slice(1, -1), slice(1, -1))
    assert (uis[-1][inner] == dec[0][inner]).mean() >= 0.98
    assert (dec[0][inner] == w.ncand).mean() >= 0.10 and (dec[0][inner] == 0).mean() >= 0.10


def test_noisy_put_rollouts_estimate_v0(put_solve):
    """8192 noisy rollouts of Merton's put from three states under the device's own value stack: the mean cost estimates the dense
    chain's V_0 within 4 standard errors plus the discretisation bound pinned on the CPU (jump_lib.PUT_BOUND: twice the gap of
    the numpy rollout restatement with 2^18 paths).  This ties the compound-Poisson step to the backup's jump term"""
    import torch

    eng, dev, dense, trains, w, _, _ = put_solve
    eng.upload_value_stack([t[0] for t in trains], [t[1] for t in trains])
    xg = w.xgrid()[0]
    n = 8192
    for x0 in JL.PUT_X0:
        i, j = (int(np.argmin(np.abs(xg - v))) for v in x0)
        v0 = dense[0][i, j]
        x0_t = torch.tensor([x0] * n, dtype=torch.float64, device="cuda")
        r = eng.simulate(x0_t, JL.PUT_DELTA, JL.PUT_STAGES, seed=11)
        torch.cuda.synchronize()
        assert "put_jd" in eng.last_kernel()
        J = r["cost"].cpu().numpy()
        step, stopped = E.decode_exit(r["exit"].cpu().numpy())
        se = J.std() / np.sqrt(n)
        print("merton put rollouts", x0, "mean", J.mean(), "v0", v0, "se", se, "stopped", stopped.mean(), "exited",
              ((step >= 0) & (stopped == 0)).mean())
        assert abs(J.mean() - v0) <= 4 * se + JL.PUT_BOUND, (x0, J.mean(), v0, se)
    assert eng.status() & STATUS_CFL == 0


# ---------------------------------------------------------------------------------------------------- errors
def test_errors(ids):
    import torch

    L = E.load_library()
    # built-in model
    w = wl.c4_car7d().scaled(ngrid=(7,) * 7, rank=4)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    assert L.c3sc_hip_set_jumps(eng.h, 1) == ERR_UNSUPPORTED
    assert L.c3sc_hip_set_jumps(eng.h, 0) == 0
    # a run-time model compiled without njump
    wp = JL.lqr_workload(ids["lqr_nojump"], 4, 0.1)
    eng = E.BellmanEngine(0)
    eng.configure(wp, wl.synth_cores(wp))
    assert L.c3sc_hip_set_jumps(eng.h, 1) == ERR_UNSUPPORTED
    assert "jump kernels" in L.c3sc_hip_last_error(eng.h).decode()
    # a forced pair variant, integrate, simulate, the box and TABLE calls, a game on top
    wr = JL.lqr_workload(ids["lqr"], 4, 0.1)
    eng = E.BellmanEngine(0)
    eng.configure(wr, wl.synth_cores(wr))
    eng.set_jumps(True)
    idx = np.ascontiguousarray(wl.synth_fibers(wr, 0, 8), dtype=np.int32)
    out = np.empty((8, wr.ngrid[0]))
    for variant in (E.VARIANT_FIBER_PAIR, E.VARIANT_FIBER_QUAD):
        eng.set_variant(variant)
        assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    eng.set_variant(E.VARIANT_AUTO)
    # policy iteration across two contexts that differ in jump mode: improvement and evaluation would apply two operators
    other = E.BellmanEngine(0)
    other.configure(wr, wl.synth_cores(wr))
    assert L.c3sc_hip_cross_iteration_pi(eng.h, other.h, 1, None) == ERR_UNSUPPORTED
    assert "jump mode" in L.c3sc_hip_last_error(eng.h).decode()
    x0 = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(E.C3scHipError, match="not offered for jump diffusions"):
        eng.integrate(x0, 0.1, 3, method="rk4")
    tables = np.zeros((8, wr.ngrid[0], wr.ncand, 5))
    costs2 = np.zeros((8, wr.ngrid[0], 2))
    assert L.c3sc_hip_bellman_fibers_tables_host(eng.h, 0, 8, idx.ctypes.data, tables.ctypes.data, costs2.ctypes.data,
                                                 out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "jump" in L.c3sc_hip_last_error(eng.h).decode()
    L.c3sc_hip_bellman_fibers_box_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 4
    lb, ub = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    L.c3sc_hip_set_control_box.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    assert L.c3sc_hip_set_control_box(eng.h, 2, lb.ctypes.data, ub.ctypes.data, 5, 1) == 0
    assert L.c3sc_hip_bellman_fibers_box_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "jumps" in L.c3sc_hip_last_error(eng.h).decode()
    U, W = np.array([[0.0]]), np.array([[1.0]])
    up, wp_ = U.ctypes.data_as(C.POINTER(C.c_double)), W.ctypes.data_as(C.POINTER(C.c_double))
    assert L.c3sc_hip_set_game(eng.h, 1, 1, up, 1, wp_, 0) == ERR_UNSUPPORTED
    assert "jumps" in L.c3sc_hip_last_error(eng.h).decode()
    # the horizon step or the stopping switch on top needs a model compiled with those flags as well
    wo = JL.lqr_workload(ids["lqr_jump_only"], 4, 0.1)
    eng2 = E.BellmanEngine(0)
    eng2.configure(wo, wl.synth_cores(wo))
    eng2.set_jumps(True)
    assert L.c3sc_hip_set_horizon_step(eng2.h, C.c_double(0.01)) == ERR_UNSUPPORTED
    assert L.c3sc_hip_set_stopping(eng2.h, 1) == ERR_UNSUPPORTED
    assert L.c3sc_hip_bellman_fibers_host(eng2.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == 0
    # a model without jump kernels set after the switch: caught at launch
    eng.set_model(ids["lqr_nojump"], SL.LQR_PRM)
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "jump kernels" in L.c3sc_hip_last_error(eng.h).decode()
    with pytest.raises(E.C3scHipError, match="jump kernels"):
        eng.simulate(x0, 0.02, 3)
    # game first, jumps second
    gid = E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_game_jd", game=True, **SL.LQR_MASKS)
    wg = JL.lqr_workload(gid, 4, 0.1)
    eng3 = E.BellmanEngine(0)
    eng3.configure(wg, wl.synth_cores(wg))
    eng3.set_game(np.array([[0.0], [1.0]]), np.array([[0.0], [0.5]]))
    assert L.c3sc_hip_set_jumps(eng3.h, 1) == ERR_UNSUPPORTED
    # switching it off restores the plain operator
    eng.set_model(ids["lqr"], JL.LQR_PRM)
    eng.set_jumps(False)
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == 0


# ---------------------------------------------------------------------------------------------------- rollouts
@pytest.mark.parametrize("rank", [4, 12])
def test_noise_free_rollouts_replay_the_jumps(ids, rank):
    """zero normals and Philox jumps: every lane's event steps, marks and states equal jump_lib's replay from the uniforms' host
    twin; a lane that jumps beyond the absorbing face or into the obstacle decodes as an exit and pays the discounted cost"""
    import torch

    beta, dt, N, seed, off = 0.3, 0.02, 48, 2024, 1000
    w = JL.lqr_workload(ids["lqr"], rank, beta)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    eng.set_jumps(True)
    rng = np.random.default_rng(5)
    n = 96
    x0 = np.stack([rng.uniform(-1.9, 1.9, n), rng.uniform(-1.9, 1.9, n)], axis=-1)
    x0[:24, 0] = 1.95  # a mark-0 jump from here lands beyond the absorbing face (while the drift has not carried x0 below 1.47)
    x0[24:32] = (0.85, -0.95)  # inside the obstacle: exits at step 0
    x0_t = torch.tensor(x0, dtype=torch.float64, device="cuda")
    noise = torch.zeros((n, N, 2), dtype=torch.float64, device="cuda")
    r = eng.simulate(x0_t, dt, N, seed=seed, noise_t=noise, wrap_periodic=True, save_every=1, traj_offset=off)
    torch.cuda.synchronize()
    assert eng.last_kernel() == f"k_rollout<rtc:lqr_jd,{rank}>"
    traj, u, J, ex = (r[k].cpu().numpy() for k in ("traj", "u", "cost", "exit"))
    bcost, ocost = _costs("lqr")
    stage = lambda x, uu: SL.lqrn_host(w.params, x, uu)[2]
    nxt, events, marks, r_ex, r_J = JL.replay(w, JL.lqr_jumps, lambda x, uu: uu, stage, bcost, ocost, traj, u, seed, dt, beta,
                                               traj_offset=off)
    err = np.abs(traj[:, 1:] - nxt).max()
    print("rollout replay: events", events.sum(), "marks", [(marks == m).sum() for m in range(3)], "exits", (r_ex >= 0).sum(),
          "max state err", err, "max cost err", np.abs(J - r_J).max())
    assert err <= 1e-12
    np.testing.assert_array_equal(ex, r_ex)
    assert np.all(np.abs(J - r_J) <= 1e-12 * np.maximum(1.0, np.abs(r_J)))
    assert events.sum() >= 50 and all((marks == m).sum() >= 5 for m in range(3)), "every mark occurs"
    assert (r_ex[24:32] == 0).all()
    # the steps at which a state moved by more than the drift can are exactly the event steps, and the moves are the marks'
    moved = np.abs(traj[:, 1:] - traj[:, :-1]).max(axis=2) > 1.5 * dt + 1e-9
    np.testing.assert_array_equal(moved, events & (np.abs(nxt - traj[:, :-1]).max(axis=2) > 1.5 * dt + 1e-9))
    # lanes that left through the absorbing face by a jump: the exit step follows an event of mark 0
    by_jump = [i for i in range(n) if r_ex[i] > 0 and events[i, r_ex[i] - 1] and marks[i, r_ex[i] - 1] == 0 and traj[i, r_ex[i], 0] > 2.0]
    assert len(by_jump) >= 2, "lanes jump beyond the absorbing face"
    for i in by_jump:
        k = r_ex[i]
        paid = np.exp(-beta * k * dt) * bcost(traj[i:i + 1, k])[0]
        assert paid > 1.0 and J[i] >= paid - 1e-9
    into_obs = [i for i in range(32, n) if r_ex[i] > 0 and marks[i, r_ex[i] - 1] == 2]
    print("exits by a jump beyond the face", len(by_jump), "into the obstacle", len(into_obs))


def test_jumps_leave_the_diffusion_noise_its_bits(ids):
    """with lambda = 0 a noisy run of the jump rollout kernel gives the states of the plain rollout kernel bit for bit"""
    import torch

    w = JL.lqr_workload(ids["lqr"], 4, 0.3, JL.LQR_ZERO_RATE_PRM)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    x0_t = torch.tensor(np.random.default_rng(1).uniform(-1.5, 1.5, (64, 2)), dtype=torch.float64, device="cuda")
    a = eng.simulate(x0_t, 0.02, 16, seed=3, wrap_periodic=True, save_every=1)
    eng.set_jumps(True)
    b = eng.simulate(x0_t, 0.02, 16, seed=3, wrap_periodic=True, save_every=1)
    torch.cuda.synchronize()
    for k in ("traj", "u", "cost", "exit"):
        assert torch.equal(a[k], b[k]), k
    assert a["traj"].std() > 0.05


# ---------------------------------------------------------------------------------------------------- the reference API
def test_vi_solve_through_the_reference_api(tmp_path):
    """the jump LQR through libc3sc.so in a child process: c3control_vi_solve sweep by sweep (11 x 11, rank 11, host callbacks and
    c3control_add_jumps beside the jump model).  The first sweep passes the first-fiber check against the host twin; every sweep
    equals the dense Markov-chain value iteration to 1e-9"""
    out = tmp_path / "vi.npz"
    r = GC.child(f"import jump_lib; jump_lib.vi_child({str(out)!r})")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    V = np.load(out)["V"]
    w = JL.lqr_vi_workload(0)
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    bcost = lambda x: H.lqr_terminal(JL.LQR_PRM, x)
    dense = JL.dense_vi(w, SL.lqrn_host, JL.lqr_jumps, bcost, H.lqr_terminal(JL.LQR_PRM, X), JL.LQR_VI_SWEEPS)
    plain = JL.dense_vi(dataclasses.replace(w, params=JL.LQR_ZERO_RATE_PRM), SL.lqrn_host, JL.lqr_jumps, bcost,
                        H.lqr_terminal(JL.LQR_PRM, X), JL.LQR_VI_SWEEPS)
    assert np.abs(dense[-1] - plain[-1]).max() > 1e-2, "the jumps move the solution"
    assert V.shape == dense.shape
    for s in range(len(V)):
        err = np.abs(V[s] - dense[s]) / np.maximum(1.0, np.abs(dense[s]))
        assert err.max() <= 1e-9, (s, err.max())
    # c3control_simulate_batch in jump mode: the synced context draws the jumps, and the run replays from the uniforms' twin
    z = np.load(out)
    assert int(z["rc"]) == 0
    stage = lambda x, uu: SL.lqrn_host(JL.LQR_PRM, x, uu)[2]
    nxt, events, marks, r_ex, r_J = JL.replay(w, JL.lqr_jumps, lambda x, uu: uu, stage, bcost, lambda x: np.full(len(x), 5.0),
                                               z["traj"], z["u"], JL.SIM_SEED, JL.SIM_DT, JL.LQR_VI_BETA)
    print("simulate_batch in jump mode: events", events.sum(), "exits", (r_ex >= 0).sum())
    assert np.abs(z["traj"][:, 1:] - nxt).max() <= 1e-12
    np.testing.assert_array_equal(z["exit"], r_ex)
    assert np.all(np.abs(z["cost"] - r_J) <= 1e-12 * np.maximum(1.0, np.abs(r_J)))
    assert events.sum() >= 20 and (r_ex > 0).any()


def test_fh_solve_of_the_merton_put_through_the_reference_api(tmp_path):
    """Merton's American put through libc3sc.so in a child process: c3control_fh_solve in stop and jump mode equals the dense chain
    stage by stage to 1e-9"""
    out = tmp_path / "fh.npz"
    r = GC.child(f"import jump_lib; jump_lib.fh_child({str(out)!r})")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    V = np.load(out)["V"]
    w = JL.put_workload(0)
    dense, _, _ = JL.dense_chain(w, SL.put_host, JL.put_jumps, lambda x: SL.put_psi(JL.PUT_PRM, x), JL.PUT_DELTA, JL.PUT_STAGES)
    assert V.shape == dense.shape
    for s in range(len(V)):
        err = np.abs(V[s] - dense[s]) / np.maximum(1.0, np.abs(dense[s]))
        assert err.max() <= 1e-9, (s, err.max())
