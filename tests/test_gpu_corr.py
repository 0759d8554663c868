"""Correlated noise on the GPU (c3sc_hip_set_correlation).

- The corr forms of the per-wave kernel against the numpy restatement of corr_lib on the ragged 21 x 70 grid (both NPL forms)
  with boundary, obstacle and periodic nodes and covariances of both signs: ranks 4, 8 and 12, beta = 0.3 and 0, minimising and
  forced, horizon on and off, stop on and off.  The L2 form at rank 12 with bond ranks 12 and 9 on 5 x 128 x 5, and the two-pair
  model on 9 x 12 x 7 (absorbing, periodic, reflecting).  Values to 1e-12 of the value scale, flags and status bits exactly,
  indices wherever the reference's margin exceeds 1e-9 (a precondition holds that to 99.9 % of the nodes).
- The known answer x0 x1 + delta a to 1e-14 for both signs of a; without the switch the device returns x0 x1.
- covar = 0 leaves the plain kernel's values, indices, flags and status bit for bit.
- A model that violates dominance at known nodes raises C3SC_STATUS_DOMINANCE and still equals corr_lib.
- One case with jumps, horizon and stop on top.
- bellman_fibers_all and policy_fibers_all equal the per-dimension calls bit for bit: segments of 5, 37 and 130 fibers in three
  dimensions, of 5 and 37 in two (one segment per dimension).
- simulate, integrate and a forced pair variant are refused.
- c3control_fh_solve of the Heston put and c3control_vi_solve of the correlated LQR through libc3sc.so, in child processes,
  equal the dense chains to 1e-9 at every stage / sweep."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import backup_ref as BR
import corr_lib as CL
import gpu_case_lib as GC
import horizon_lib as H
import jump_lib as JL
import stop_lib as SL

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 3
STATUS_STATIONARY, STATUS_CFL, STATUS_DOMINANCE = 1, 2, 4
LQR_DELTA, LQR3_DELTA = 0.01, 0.004  # Q delta / h^2 < 0.8 on the ragged grids


@pytest.fixture(scope="module")
def ids():
    return {
        "lqr": E.compile_model(CL.LQR, 2, 2, ranks=(4, 8, 12), name="lqr_cd", horizon=True, stop=True, corr_pairs=CL.LQR_PAIRS, **CL.LQR_MASKS),
        "lqr3": E.compile_model(CL.LQR3, 3, 3, ranks=(4, 12), name="lqr3_cd", horizon=True, stop=True, corr_pairs=CL.LQR3_PAIRS, **CL.LQR3_MASKS),
        "known": E.compile_model(CL.KNOWN, 2, 1, ranks=(4,), name="known_cd", horizon=True, corr_pairs=CL.KNOWN_PAIRS, **CL.KNOWN_MASKS),
        "lqr_jump": E.compile_model(CL.LQR_JUMP, 2, 2, ranks=(4,), name="lqr_cd_jump", horizon=True, stop=True, njump=JL.LQR_NJUMP,
                                    corr_pairs=CL.LQR_PAIRS, **CL.LQR_MASKS),
        "lqr_nocorr": E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_nocorr", **SL.LQR_MASKS),
    }


def _costs(w):
    return (lambda x: SL.lqrn_terminal(w.params, x)), (lambda x: np.full(len(x), 5.0))


def _workload(ids, model, rank, discount, prm=None):
    """(workload, covar, pairs, jumps, the dimension the stop constant is tuned along)"""
    if model == "lqr":
        return CL.lqr_workload(ids["lqr"], rank, discount, CL.LQR_PRM if prm is None else prm), CL.lqr_covar, CL.LQR_PAIRS, None, 0
    if model == "lqr_jump":
        return CL.lqr_workload(ids["lqr_jump"], rank, discount, JL.LQR_PRM), CL.lqr_jump_covar, CL.LQR_PAIRS, JL.lqr_jumps, 0
    if model == "lqr3":
        return CL.lqr3_workload(ids["lqr3"], discount=discount), CL.lqr3_covar, CL.LQR3_PAIRS, None, 1
    return CL.lqr3_workload(ids["lqr3"], ngrid=(9, 12, 7), ranks=(1, 4, 4, 1), discount=discount), CL.lqr3_covar, CL.LQR3_PAIRS, None, 1


def _case(ids, model, rank, discount, horizon, stop, prm=None):
    """(engine with correlation on, workload, covar, pairs, jumps, train, full array, psi or None, delta or None) of one case;
    with stop, psi's constant is put at the median of the reference's continuation values, so that both decisions occur"""
    w, covar, pairs, jumps, k0 = _workload(ids, model, rank, discount, prm)
    delta = (LQR_DELTA if w.dx == 2 else LQR3_DELTA) if horizon else None
    cores = wl.synth_cores(w)
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    tr, Vfull = JL.Train(w, cores), CL.full_values(w, cores)
    psi = None
    if stop:
        bcost, ocost = _costs(w)
        idx = wl.synth_fibers(w, k0, 64)
        costs, ab = eng.stencil_fibers_host(k0, idx)
        out = CL.corr_fibers(w, SL.lqrn_host, covar, pairs, Vfull, k0, idx, costs, ab, bcost, ocost, delta, jumps=jumps, interp=tr)[0]
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
    if jumps is not None:
        eng.set_jumps(True)
    eng.set_correlation(True)
    return eng, w, covar, pairs, jumps, tr, Vfull, psi, delta


def _check_case(ids, model, rank, discount, horizon, stop, ks=(0, 1), prm=None, expect_dominance=False):
    eng, w, covar, pairs, jumps, tr, Vfull, psi, delta = _case(ids, model, rank, discount, horizon, stop, prm)
    bcost, ocost = _costs(w)
    nc = w.ncand
    kernels = set()
    signs = np.zeros(2, dtype=bool)
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
        r_out, r_ui, mg, stat, cfl, dom = CL.corr_fibers(w, SL.lqrn_host, covar, pairs, Vfull, k, idx, costs, ab, bcost, ocost, delta, psi,
                                                         jumps=jumps, interp=tr)
        p_out = CL.corr_fibers(w, SL.lqrn_host, covar, pairs, Vfull, k, idx, costs, ab, bcost, ocost, delta, psi, jumps=jumps, interp=tr,
                               with_corr=False)[0]
        scale = np.maximum(1.0, np.abs(r_out))
        print(model, rank, discount, horizon, stop, k, "max err", np.abs(out - r_out).max(), "unsure share", (mg <= 1e-9).mean(),
              "the term moves the values by", np.abs(r_out - p_out).max(), "dominance violated at", int(dom.sum()), "status", status)
        assert np.abs(r_out - p_out).max() > 1e-6, "the cross terms move the values"
        assert np.all(np.abs(out - r_out) <= 1e-12 * scale), (k, np.abs(out - r_out).max())
        live = ab == 0
        if not expect_dominance:
            assert (mg[live] <= 1e-9).mean() <= 0.001, "precondition: the reference's own decisions are clear at 99.9 % of the nodes"
        sure = mg > 1e-9
        np.testing.assert_array_equal(ui[sure], r_ui[sure])
        assert (ui[live] >= 0).all() and (ui[~live] == -1).all()
        if stop:
            assert (ui[live] == nc).any() and (ui[live] < nc).any(), "both decisions occur"
        assert bool(status & STATUS_STATIONARY) == bool(stat.any()) and bool(status & STATUS_CFL) == bool(cfl.any()), status
        assert bool(status & STATUS_DOMINANCE) == bool(dom.any()), (status, int(dom.sum()))
        assert bool(dom.any()) == expect_dominance
        if not expect_dominance:
            assert status == 0, "the cases stay inside the CFL rule and dominance and have no stationary node"
        a = covar(w.params, BR.node_states(w, k, idx).reshape(-1, w.dx)[live.reshape(-1)])
        signs |= np.array([(a > 0).any(), (a < 0).any()])
        # the forced path shares Q0 and PV0: the minimising run's own indices reproduce its values, a random policy its own
        f_out, f_ab = eng.policy_fibers_host(k, idx, ui)
        np.testing.assert_array_equal(f_ab, ab)
        assert np.all(np.abs(f_out - out) <= 1e-12 * scale), (k, np.abs(f_out - out).max())
        rng = np.random.default_rng(rank + k)
        pol = rng.integers(0, nc + (1 if stop else 0), size=ab.shape).astype(np.int32)
        q_out, _ = eng.policy_fibers_host(k, idx, pol)
        q_ref = CL.corr_fibers(w, SL.lqrn_host, covar, pairs, Vfull, k, idx, costs, ab, bcost, ocost, delta, psi, forced=pol, jumps=jumps,
                               interp=tr)[0]
        assert np.all(np.abs(q_out - q_ref) <= 1e-12 * np.maximum(1.0, np.abs(q_ref))), (k, np.abs(q_out - q_ref).max())
    assert signs.all(), "covariances of both signs"
    return kernels, eng


@pytest.mark.parametrize("rank", [4, 8, 12])
@pytest.mark.parametrize("discount", [0.3, 0.0])
@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
@pytest.mark.parametrize("stop", [False, True], ids=["nostop", "stop"])
def test_per_wave_corr_vs_numpy(ids, rank, discount, horizon, stop):
    kernels, _ = _check_case(ids, "lqr", rank, discount, horizon, stop)
    assert all(f",{rank}," in k for k in kernels), kernels
    assert any(",1>" in k for k in kernels) and any(",2>" in k for k in kernels), kernels  # N = 21 and N = 70: both NPL forms


@pytest.mark.parametrize("discount", [0.3, 0.0])
@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
@pytest.mark.parametrize("stop", [False, True], ids=["nostop", "stop"])
def test_per_wave_corr_rank_12_l2_form(ids, discount, horizon, stop):
    """bond ranks 12 and 9, padded to 12: a launch along the 128-node middle dimension needs more than the 160 KB the launcher
    stages in, so the corr kernel that reads the varying core from global memory runs"""
    w = CL.lqr3_workload(ids["lqr3"], discount=discount)
    cw = 3 + 1 + 2 * 3 + 1
    assert GC.fpw_lds_bytes(w, 1, 12, 2, cw) > 160 * 1024, "the staged form would fit: this case would not run the L2 form"
    assert GC.fpw_lds_bytes(w, 1, 12, 2, cw) - 8 * 128 * 145 < 160 * 1024  # ... and the L2 form's own layout fits
    kernels, _ = _check_case(ids, "lqr3", 12, discount, horizon, stop, ks=(1,))
    assert kernels == {"k_fiber_per_wave<rtc:lqr3_cd,12,2>"}, kernels


@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
def test_two_pairs_on_an_absorbing_a_periodic_and_a_reflecting_dimension(ids, horizon):
    """pairs (0,1) and (1,2) of opposite sign on 9 x 12 x 7, fibers along every dimension: the diagonal neighbours cross the
    periodic seam of dimension 1 and fold back at the reflecting ends of dimension 2"""
    kernels, _ = _check_case(ids, "lqr3_small", 4, 0.3, horizon, False, ks=(0, 1, 2))
    assert all(",4," in k for k in kernels), kernels


@pytest.mark.parametrize("a", [CL.KNOWN_A, -CL.KNOWN_A])
def test_known_answer(ids, a):
    w = CL.known_workload(ids["known"], a)
    eng = E.BellmanEngine(0)
    eng.configure(w, CL.known_cores(w))
    eng.set_horizon_step(CL.KNOWN_DELTA)
    xg = w.xgrid()
    for k in (0, 1):
        idx = wl.synth_fibers(w, k, 16)
        x = BR.node_states(w, k, idx)
        ixs = BR.node_indices(w, k, idx).reshape(x.shape)
        interior = np.all((ixs > 0) & (ixs < np.array(w.ngrid) - 1), axis=-1)
        eng.set_correlation(False)
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        assert interior.any() and (ab[interior] == 0).all()
        assert np.abs(out[interior] - x[interior][:, 0] * x[interior][:, 1]).max() <= 1e-14, "without the cross term V stays x0 x1"
        eng.set_correlation(True)
        eng.status(clear=True)
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        assert eng.status(clear=True) == 0
        ref = x[..., 0] * x[..., 1] + CL.KNOWN_DELTA * a
        err = np.abs(out[interior] - ref[interior]).max()
        print("known answer a =", a, "max err", err)
        assert err <= 1e-14
        assert (ui[interior] == 0).all()


@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
@pytest.mark.parametrize("stop", [False, True], ids=["nostop", "stop"])
@pytest.mark.parametrize("discount", [0.3, 0.0])
def test_zero_covariance_equals_the_plain_kernel_bit_for_bit(ids, horizon, stop, discount):
    w = CL.lqr_workload(ids["lqr"], 4, discount, CL.LQR_ZERO_PRM)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    if horizon:
        eng.set_horizon_step(LQR_DELTA)
    eng.set_stopping(stop)
    for k in (0, 1):
        idx = wl.synth_fibers(w, k, 129)
        eng.set_correlation(False)
        eng.status(clear=True)
        p_out, p_ui, p_ab = eng.bellman_fibers_host(k, idx)
        p_kernel, p_st = eng.last_kernel(), eng.status(clear=True)
        eng.set_correlation(True)
        c_out, c_ui, c_ab = eng.bellman_fibers_host(k, idx)
        assert eng.last_kernel() == p_kernel  # the entry is the same; the launcher takes its corr form
        np.testing.assert_array_equal(c_out, p_out)
        np.testing.assert_array_equal(c_ui, p_ui)
        np.testing.assert_array_equal(c_ab, p_ab)
        assert eng.status(clear=True) == p_st
    # ... and with the covariance back the values move: the switch does select another kernel
    eng.set_model(w.model, CL.LQR_PRM)
    m_out, _, _ = eng.bellman_fibers_host(1, idx)
    assert np.abs(m_out - p_out)[p_ab == 0].max() > 1e-6


@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
def test_dominance_violation_raises_the_status_bit_and_keeps_the_algebra(ids, horizon):
    """amp = 0.8 against the grid ratio 0.29: corr_lib names the violating nodes, the device raises C3SC_STATUS_DOMINANCE and
    returns corr_lib's values; the well-posed models leave the bit clear (every other test here asserts status == 0)"""
    _check_case(ids, "lqr", 4, 0.3, horizon, False, prm=CL.LQR_DOM_PRM, expect_dominance=True)


def test_with_jumps_horizon_and_stop(ids):
    kernels, _ = _check_case(ids, "lqr_jump", 4, 0.3, True, True)
    assert all("lqr_cd_jump,4," in k for k in kernels), kernels


@pytest.mark.parametrize("model", ["lqr", "lqr3_small"])
def test_all_forms_equal_the_per_dimension_calls(ids, model):
    import torch

    w = _workload(ids, model, 4, 0.3)[0]
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    eng.set_correlation(True)
    L, h, d, nc = eng.L, eng.h, w.dx, w.ncand
    sizes = (5, 37, 130)[:d]
    ks = list(range(d))
    idx = [torch.from_numpy(wl.synth_fibers(w, k, F, seed=0xA11 + F)).cuda() for k, F in zip(ks, sizes)]
    shapes = [(F, w.ngrid[k]) for k, F in zip(ks, sizes)]
    gen = torch.Generator(device="cuda").manual_seed(5)
    pol = [torch.randint(0, nc, s, dtype=torch.int32, device="cuda", generator=gen) for s in shapes]
    KS, FS = (C.c_int * d)(*ks), (C.c_size_t * d)(*sizes)

    def fresh():
        return ([torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in shapes],
                [torch.full(s, -7, dtype=torch.int32, device="cuda") for s in shapes],
                [torch.full(s, -7, dtype=torch.int32, device="cuda") for s in shapes])

    out, ui, ab = fresh()
    for s, k in enumerate(ks):
        assert L.c3sc_hip_bellman_fibers(h, k, sizes[s], idx[s].data_ptr(), out[s].data_ptr(), ui[s].data_ptr(), ab[s].data_ptr(), None) == 0
        assert eng.last_kernel().startswith("k_fiber_per_wave<rtc:"), eng.last_kernel()
    a_out, a_ui, a_ab = fresh()
    assert L.c3sc_hip_bellman_fibers_all(h, d, KS, FS, GC.ptrs(idx), GC.ptrs(a_out), GC.ptrs(a_ui), GC.ptrs(a_ab), C.c_void_p(None)) == 0
    torch.cuda.synchronize()
    for s in range(d):
        assert not torch.isnan(out[s]).any() and (ab[s] == 0).any()
        assert torch.equal(a_out[s], out[s]) and torch.equal(a_ui[s], ui[s]) and torch.equal(a_ab[s], ab[s]), f"bellman, dimension {s}"
    # the switch is honoured: without it the same calls give other values
    eng.set_correlation(False)
    n_out, n_ui, n_ab = fresh()
    assert L.c3sc_hip_bellman_fibers_all(h, d, KS, FS, GC.ptrs(idx), GC.ptrs(n_out), GC.ptrs(n_ui), GC.ptrs(n_ab), C.c_void_p(None)) == 0
    torch.cuda.synchronize()
    assert any(not torch.equal(n_out[s], out[s]) for s in range(d))
    eng.set_correlation(True)
    p_out, _, p_ab = fresh()
    for s, k in enumerate(ks):
        assert L.c3sc_hip_policy_fibers(h, k, sizes[s], idx[s].data_ptr(), pol[s].data_ptr(), p_out[s].data_ptr(), p_ab[s].data_ptr(), None) == 0
    q_out, _, q_ab = fresh()
    assert L.c3sc_hip_policy_fibers_all(h, d, KS, FS, GC.ptrs(idx), GC.ptrs(pol), GC.ptrs(q_out), GC.ptrs(q_ab), C.c_void_p(None)) == 0
    torch.cuda.synchronize()
    for s in range(d):
        assert torch.equal(q_out[s], p_out[s]) and torch.equal(q_ab[s], p_ab[s]) and torch.equal(p_ab[s], ab[s]), f"policy, dimension {s}"
    assert eng.status(clear=True) == 0
    eng.close()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(ids):
    import torch

    L = E.load_library()
    err = lambda e: L.c3sc_hip_last_error(e.h).decode()
    # built-in model
    w = wl.c4_car7d().scaled(ngrid=(7,) * 7, rank=4)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    assert L.c3sc_hip_set_correlation(eng.h, 1) == ERR_UNSUPPORTED
    assert L.c3sc_hip_set_correlation(eng.h, 0) == 0
    # a run-time model compiled without pairs
    wp = CL.lqr_workload(ids["lqr_nocorr"], 4, 0.1, SL.LQR_PRM)
    eng = E.BellmanEngine(0)
    eng.configure(wp, wl.synth_cores(wp))
    assert L.c3sc_hip_set_correlation(eng.h, 1) == ERR_UNSUPPORTED
    assert "corr kernels" in err(eng)
    # simulate, integrate, a forced pair or quad variant, the box and TABLE calls, a game on top
    wr = CL.lqr_workload(ids["lqr"], 4, 0.1)
    eng = E.BellmanEngine(0)
    eng.configure(wr, wl.synth_cores(wr))
    eng.set_correlation(True)
    idx = np.ascontiguousarray(wl.synth_fibers(wr, 0, 8), dtype=np.int32)
    out = np.empty((8, wr.ngrid[0]))
    for variant in (E.VARIANT_FIBER_PAIR, E.VARIANT_FIBER_QUAD):
        eng.set_variant(variant)
        assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
        assert "corr form" in err(eng)
    eng.set_variant(E.VARIANT_AUTO)
    x0 = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(E.C3scHipError, match="not offered with correlated noise"):
        eng.simulate(x0, 0.02, 3)
    with pytest.raises(E.C3scHipError, match="not offered with correlated noise"):
        eng.integrate(x0, 0.1, 3, method="rk4")
    other = E.BellmanEngine(0)
    other.configure(wr, wl.synth_cores(wr))
    assert L.c3sc_hip_cross_iteration_pi(eng.h, other.h, 1, None) == ERR_UNSUPPORTED
    assert "correlation mode" in err(eng)
    tables = np.zeros((8, wr.ngrid[0], wr.ncand, 5))
    costs2 = np.zeros((8, wr.ngrid[0], 2))
    assert L.c3sc_hip_bellman_fibers_tables_host(eng.h, 0, 8, idx.ctypes.data, tables.ctypes.data, costs2.ctypes.data,
                                                 out.ctypes.data, None, None) == ERR_UNSUPPORTED
    L.c3sc_hip_bellman_fibers_box_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 4
    lb, ub = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    L.c3sc_hip_set_control_box.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    assert L.c3sc_hip_set_control_box(eng.h, 2, lb.ctypes.data, ub.ctypes.data, 5, 1) == 0
    assert L.c3sc_hip_bellman_fibers_box_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    U, W = np.array([[0.0]]), np.array([[1.0]])
    up, wp_ = U.ctypes.data_as(C.POINTER(C.c_double)), W.ctypes.data_as(C.POINTER(C.c_double))
    assert L.c3sc_hip_set_game(eng.h, 1, 1, up, 1, wp_, 0) == ERR_UNSUPPORTED
    assert "correlated noise" in err(eng)
    # a model without corr kernels set after the switch: caught at launch
    eng.set_controls(wr.cands)
    eng.set_model(ids["lqr_nocorr"], SL.LQR_PRM)
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "corr kernels" in err(eng)
    # switching it off restores the plain operator
    eng.set_correlation(False)
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == 0


# ---------------------------------------------------------------------------------------------------- the reference API
def test_vi_solve_through_the_reference_api(tmp_path):
    """the correlated LQR through libc3sc.so in a child process: c3control_vi_solve sweep by sweep (11 x 11, rank 11, host
    callbacks and c3control_add_covariance beside the device model).  The first sweep passes the first-fiber check against the
    host twin; every sweep equals the dense Markov-chain value iteration to 1e-9"""
    out = tmp_path / "vi.npz"
    r = GC.child(f"import corr_lib; corr_lib.vi_child({str(out)!r})")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    V = np.load(out)["V"]
    w = CL.lqr_vi_workload(0)
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    bcost = lambda x: H.lqr_terminal(w.params, x)
    dense = CL.dense_vi(w, SL.lqrn_host, CL.lqr_covar, CL.LQR_PAIRS, bcost, H.lqr_terminal(w.params, X), CL.LQR_VI_SWEEPS)
    plain = CL.dense_vi(w, SL.lqrn_host, CL.lqr_covar, CL.LQR_PAIRS, bcost, H.lqr_terminal(w.params, X), CL.LQR_VI_SWEEPS, with_corr=False)
    print("vi_solve: the cross term moves the solution by", np.abs(dense[-1] - plain[-1]).max())
    assert np.abs(dense[-1] - plain[-1]).max() > 1e-3, "the cross term moves the solution"
    assert V.shape == dense.shape
    for s in range(len(V)):
        err = np.abs(V[s] - dense[s]) / np.maximum(1.0, np.abs(dense[s]))
        assert err.max() <= 1e-9, (s, err.max())


def test_fh_solve_of_the_heston_put_through_the_reference_api(tmp_path):
    """the American put under Heston through libc3sc.so in a child process: c3control_fh_solve in stop and correlation mode on
    11 x 11 with 20 stages equals the dense chain stage by stage to 1e-9, and differs from the rho = 0 chain by far more"""
    out = tmp_path / "fh.npz"
    r = GC.child(f"import corr_lib; corr_lib.fh_child({str(out)!r})")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "C3SC_STATUS_DOMINANCE" not in r.stderr and "C3SC_STATUS_CFL" not in r.stderr
    V = np.load(out)["V"]
    w = CL.heston_workload(0)
    psi = lambda x: CL.heston_psi(CL.HESTON_PRM, x)
    dense, _, cfl, dom = CL.dense_chain(w, CL.heston_host, CL.heston_covar, CL.HESTON_PAIRS, psi, CL.HESTON_DELTA, CL.HESTON_STAGES)
    assert not cfl and not dom
    rho0, _, _, _ = CL.dense_chain(dataclasses.replace(w, params=CL.HESTON_RHO0_PRM), CL.heston_host, CL.heston_covar, CL.HESTON_PAIRS, psi,
                                   CL.HESTON_DELTA, CL.HESTON_STAGES)
    print("heston put: rho moves V_0 by", np.abs(dense[0] - rho0[0]).max())
    assert np.abs(dense[0] - rho0[0]).max() > 1e-5, "the correlation moves the price"
    assert V.shape == dense.shape
    for s in range(len(V)):
        err = np.abs(V[s] - dense[s]) / np.maximum(1.0, np.abs(dense[s]))
        assert err.max() <= 1e-9, (s, err.max())
