"""Impulse control on the GPU (c3sc_hip_set_impulses).

- The impulse forms of the per-wave kernel against the numpy restatement of impulse_lib on the ragged 21 x 70 grid (both NPL
  forms) with boundary, obstacle and periodic nodes, whose interventions reach interior targets, targets beyond the absorbing
  face, inside the obstacle and across the periodic seam, one of them not admissible on half the domain: ranks 4, 8 and 12,
  beta = 0.3 and 0, minimising and forced (forced indices drawn over controls and interventions; a forced -1 gives 0.0), with
  and without jumps.  The L2 form at rank 12 with bond ranks 12 and 9 on 5 x 128 x 5.  Values to 1e-12 of the value scale,
  flags and status bits exactly, indices wherever the reference's margin exceeds 1e-9 (tests/test_impulse_lib.py holds the
  preconditions on the CPU; they are asserted again here on the device's own stencils).
- Costs that are all +inf leave the plain kernel's values, indices, flags and status bit for bit, and the jump kernel's with
  jumps on.
- CONSTELM and LINELM targets differ and agree with impulse_lib in both classes.
- The known answer min(continuation, min_m k_m + c) to 1e-14, the tie k_1 = k_2 going to mark 1.
- bellman_fibers_all and policy_fibers_all equal the per-dimension calls bit for bit on 5, 37 and 130 fibers.
- Every refusal of c3sc_hip_set_impulses and of the launches in impulse mode returns its code and leaves the context usable.
- Rollouts: without noise every lane's intervention steps, marks, states and costs equal impulse_lib's replay to 1e-12, a lane
  whose intervention leaves the domain decodes as an exit at the next step; with costs +inf a noisy run keeps the bits of the
  plain rollout kernel, and of the jump rollout kernel with jumps on; 8192 noisy rollouts of the inventory problem from three
  states estimate V(x_0) within 4 standard errors plus the allowance measured on the CPU.
- Forced indices that name no action (the stop index, an index above ncand + M) give 0.0."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import backup_ref as BR
import gpu_case_lib as GC
import impulse_lib as IL
import jump_lib as JL
import stop_lib as SL

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def ids():
    return {
        "lqr": E.compile_model(IL.LQR_JUMP, 2, 2, ranks=(4, 8, 12), name="lqr_ic", njump=JL.LQR_NJUMP, nimpulse=IL.LQR_NIMPULSE, **IL.LQR_MASKS),
        "lqr3": E.compile_model(IL.LQR3, 3, 3, ranks=(4, 12), name="lqr3_ic", njump=JL.LQR3_NJUMP, nimpulse=IL.LQR3_NIMPULSE, **IL.LQR3_MASKS),
        "known": E.compile_model(IL.KNOWN, 2, 2, ranks=(4,), name="known_ic", nimpulse=IL.KNOWN_NIMPULSE, **IL.KNOWN_MASKS),
        "lqr_plain": E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_noimpulse", horizon=True, stop=True, **SL.LQR_MASKS),
        "lqr_impulse_only": E.compile_model(IL.LQR, 2, 2, ranks=(4,), name="lqr_impulse_only", nimpulse=IL.LQR_NIMPULSE, **IL.LQR_MASKS),
    }


def _costs(w):
    return (lambda x: SL.lqrn_terminal(w.params, x)), (lambda x: np.full(len(x), 5.0))


def _case(ids, model, rank, discount, jumps):
    if model == "lqr":
        w, imp, jmp = IL.lqr_workload(ids["lqr"], rank, discount, IL.lqr_cost_scale(rank)), IL.lqr_impulses, JL.lqr_jumps
    else:
        w, imp, jmp = IL.lqr3_workload(ids["lqr3"], discount=discount), IL.lqr3_impulses, JL.lqr3_jumps
    cores = wl.synth_cores(w)
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    eng.set_jumps(jumps)
    eng.set_impulses(True)
    return eng, w, imp, (jmp if jumps else None), JL.Train(w, cores)


def _close(a, ref):
    """|a - ref| <= 1e-12 max(1, |ref|), and the same non-finite entries (a forced intervention that is not admissible is +inf)"""
    fin = np.isfinite(ref)
    return np.array_equal(fin, np.isfinite(a)) and np.array_equal(a[~fin], ref[~fin]) and \
        bool(np.all(np.abs(a[fin] - ref[fin]) <= 1e-12 * np.maximum(1.0, np.abs(ref[fin]))))


def _check_case(ids, model, rank, discount, jumps, ks=(0, 1), constelm=False):
    eng, w, imp, jmp, tr = _case(ids, model, rank, discount, jumps)
    bcost, ocost = _costs(w)
    if constelm:
        eng.set_interp(True)
    nc = w.ncand
    M = IL.LQR_NIMPULSE if model == "lqr" else IL.LQR3_NIMPULSE
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
        r_out, r_ui, mg, stat, c = IL.impulse_fibers(w, SL.lqrn_host, imp, tr, k, idx, costs, ab, bcost, ocost, constelm=constelm, jumps=jmp)
        live = ab == 0
        share = (r_ui[live] > nc).mean()
        print(model, rank, discount, jumps, k, "max err", np.abs(out - r_out).max(), "unsure share", (mg[live] <= 1e-9).mean(),
              "interventions win at", share, [(r_ui[live] == nc + 1 + m).mean() for m in range(M)])
        assert _close(out, r_out), (k, np.abs(out - r_out).max())
        # the preconditions, on the device's own stencils
        assert 0.10 <= share <= 0.90, share
        assert all((r_ui[live] == nc + 1 + m).any() for m in range(M)), "each intervention wins somewhere"
        assert (mg[live] > 1e-9).mean() >= 0.999, "the reference's own decisions are clear at 99.9 % of the nodes"
        sure = mg > 1e-9
        np.testing.assert_array_equal(ui[sure], r_ui[sure])
        assert (ui[live] >= 0).all() and (ui[~live] == -1).all() and not (ui == nc).any()
        kind, mark = E.decode_action(ui, nc)
        assert set(np.unique(kind)) == {"absorbed", "control", "impulse"} and mark[kind == "impulse"].max() == M - 1
        assert not stat.any() and status == 0, "no stationary node, and an intervention raises no bit"
        x = BR.node_states(w, k, idx).reshape(-1, w.dx)[live.reshape(-1)]
        kk, y = imp(w.params, x)
        for m in range(M):
            adm = np.isfinite(kk[:, m])
            _, inobs, beyond, moved = JL.target_kinds(w, y[adm, m])
            kinds |= np.array([(~inobs & ~beyond & ~moved).any(), (beyond & ~inobs).any(), inobs.any(), moved.any()])
        # forced: the minimising run's own indices reproduce its values; a random policy over controls and interventions its own
        f_out, f_ab = eng.policy_fibers_host(k, idx, ui)
        np.testing.assert_array_equal(f_ab, ab)
        assert _close(f_out, out), (k, np.abs(f_out - out).max())
        rng = np.random.default_rng(rank + k)
        # 0 .. nc-1 and nc+1 .. nc+M, an intervention at three nodes in ten: the stop index is not drawn
        pol = np.where(rng.random(ab.shape) < 0.3, nc + 1 + rng.integers(0, M, size=ab.shape), rng.integers(0, nc, size=ab.shape))
        hole = rng.random(ab.shape) < 0.1
        pol = np.where(hole, -1, pol).astype(np.int32)
        q_out, q_ab = eng.policy_fibers_host(k, idx, pol)
        np.testing.assert_array_equal(q_ab, ab)
        q_ref = IL.impulse_fibers(w, SL.lqrn_host, imp, tr, k, idx, costs, ab, bcost, ocost, forced=pol, constelm=constelm, jumps=jmp)[0]
        assert (pol[live] > nc).mean() > 0.05 and (hole & live).any()
        assert (q_out[hole & live] == 0.0).all(), "a forced -1 gives 0.0"
        assert _close(q_out, q_ref), (k, np.nanmax(np.abs(q_out - q_ref)))
        assert eng.status(clear=True) == 0
    return kernels, kinds, eng


@pytest.mark.parametrize("rank", [4, 8, 12])
@pytest.mark.parametrize("discount", [0.3, 0.0])
@pytest.mark.parametrize("jumps", [False, True], ids=["nojump", "jump"])
def test_per_wave_impulse_vs_numpy(ids, rank, discount, jumps):
    kernels, kinds, eng = _check_case(ids, "lqr", rank, discount, jumps)
    assert all(f",{rank}," in k for k in kernels), kernels
    assert any(",1>" in k for k in kernels) and any(",2>" in k for k in kernels), kernels  # N = 21 and N = 70: both NPL forms
    assert kinds.all(), ("interior, beyond the absorbing face, inside the obstacle, across the seam", kinds)
    eng.close()


@pytest.mark.parametrize("discount", [0.3, 0.0])
@pytest.mark.parametrize("jumps", [False, True], ids=["nojump", "jump"])
def test_per_wave_impulse_rank_12_l2_form(ids, discount, jumps):
    """bond ranks 12 and 9, padded to 12: a launch along the 128-node middle dimension needs more than the 160 KB the launcher
    stages in, so the impulse kernel that reads the varying core from global memory runs"""
    w = IL.lqr3_workload(ids["lqr3"], discount=discount)
    cw = 3 + 1 + 2 * 3 + 1
    assert GC.fpw_lds_bytes(w, 1, 12, 2, cw) > 160 * 1024, "the staged form would fit: this case would not run the L2 form"
    assert GC.fpw_lds_bytes(w, 1, 12, 2, cw) - 8 * 128 * 145 < 160 * 1024  # ... and the L2 form's own layout fits
    kernels, kinds, eng = _check_case(ids, "lqr3", 12, discount, jumps, ks=(1,))
    assert kernels == {"k_fiber_per_wave<rtc:lqr3_ic,12,2>"}, kernels
    assert kinds[0] and kinds[3]
    eng.close()


@pytest.mark.parametrize("jumps", [False, True], ids=["nojump", "jump"])
@pytest.mark.parametrize("discount", [0.3, 0.0])
def test_infinite_costs_equal_the_kernel_without_interventions_bit_for_bit(ids, jumps, discount):
    w = IL.lqr_workload(ids["lqr"], 4, discount, np.inf)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    eng.set_jumps(jumps)
    for k in (0, 1):
        idx = wl.synth_fibers(w, k, 129)
        eng.set_impulses(False)
        eng.status(clear=True)
        p_out, p_ui, p_ab = eng.bellman_fibers_host(k, idx)
        p_kernel, p_st = eng.last_kernel(), eng.status(clear=True)
        eng.set_impulses(True)
        i_out, i_ui, i_ab = eng.bellman_fibers_host(k, idx)
        assert eng.last_kernel() == p_kernel  # the entry is the same; the launcher takes its impulse form
        np.testing.assert_array_equal(i_out, p_out)
        np.testing.assert_array_equal(i_ui, p_ui)
        np.testing.assert_array_equal(i_ab, p_ab)
        assert eng.status(clear=True) == p_st
    # ... and with finite costs the values move: the switch does select another kernel
    eng.set_model(w.model, IL.lqr_prm(IL.lqr_cost_scale(4)))
    m_out, m_ui, _ = eng.bellman_fibers_host(1, idx)
    assert (m_out[p_ab == 0] < p_out[p_ab == 0]).mean() > 0.1 and (m_ui > w.ncand).any()
    eng.close()


def test_constelm_and_linelm_targets(ids):
    _, _, eng = _check_case(ids, "lqr", 4, 0.3, False, ks=(1,), constelm=True)
    idx = wl.synth_fibers(eng.w, 1, 257)
    c_out, c_ui, ab = eng.bellman_fibers_host(1, idx)
    eng.set_interp(False)
    l_out, l_ui, _ = eng.bellman_fibers_host(1, idx)
    won = (ab == 0) & (c_ui > eng.w.ncand) & (l_ui > eng.w.ncand)
    assert won.sum() > 100 and (np.abs(c_out - l_out)[won] > 1e-6 * np.abs(l_out[won])).mean() > 0.5, "off-node targets: the classes differ"
    eng.close()


def test_known_answer(ids):
    w = IL.known_workload(ids["known"])
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    for k in (0, 1):
        idx = wl.synth_fibers(w, k, 16)
        eng.set_impulses(False)
        cont, cu, ab = eng.bellman_fibers_host(k, idx)
        eng.set_impulses(True)
        out, ui, ab2 = eng.bellman_fibers_host(k, idx)
        np.testing.assert_array_equal(ab, ab2)
        live = ab == 0
        want = np.where(live, np.minimum(cont, IL.KNOWN_TARGET), cont)
        err = np.abs(out - want).max()
        print("known answer", IL.KNOWN_TARGET, "wins at", (ui[live] > w.ncand).mean(), "max err", err)
        assert err <= 1e-14
        wins = live & (IL.KNOWN_TARGET < cont)
        assert wins.any() and (live & ~wins).any()
        assert (ui[wins] == w.ncand + 2).all(), "k_1 = k_2 < k_0: mark 1, by the first strict '<'"
        np.testing.assert_array_equal(ui[~wins], cu[~wins])
    assert eng.status(clear=True) == 0
    eng.close()


def test_forced_indices_that_name_nothing_give_zero(ids):
    """the stop index (no stop action is compiled with interventions) and an index above ncand + M: 0.0 at the live nodes, the
    boundary and obstacle costs and every flag unchanged, as a forced -1 and an out-of-range candidate index give"""
    w = IL.lqr_workload(ids["lqr"], 4, 0.3, IL.lqr_cost_scale(4))
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    eng.set_impulses(True)
    nc, M = w.ncand, IL.LQR_NIMPULSE
    for k in (0, 1):
        idx = wl.synth_fibers(w, k, 67)
        out, _, ab = eng.bellman_fibers_host(k, idx)
        live = ab == 0
        for fu in (nc, nc + M + 1, nc + M + 40, 1 << 30):
            z_out, z_ab = eng.policy_fibers_host(k, idx, np.full(ab.shape, fu, dtype=np.int32))
            np.testing.assert_array_equal(z_ab, ab)
            assert (z_out[live] == 0.0).all() and np.array_equal(z_out[~live], out[~live]), fu
        l_out, _ = eng.policy_fibers_host(k, idx, np.full(ab.shape, nc + M, dtype=np.int32))  # the last intervention: applied
        assert (l_out[live] != 0.0).all()
    assert eng.status(clear=True) == 0
    eng.close()


# ---------------------------------------------------------------------------------------------------- the _all forms
@pytest.mark.parametrize("model", ["lqr", "lqr3"])
@pytest.mark.parametrize("jumps", [False, True], ids=["nojump", "jump"])
def test_all_forms_equal_the_per_dimension_calls(ids, model, jumps):
    import torch

    if model == "lqr":
        w = IL.lqr_workload(ids["lqr"], 4, 0.3, IL.lqr_cost_scale(4))
        M = IL.LQR_NIMPULSE
    else:
        w = dataclasses.replace(IL.lqr3_workload(ids["lqr3"], ranks=wl.uniform_ranks(3, 4)), ngrid=(5, 16, 5))
        M = IL.LQR3_NIMPULSE
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    eng.set_jumps(jumps)
    eng.set_impulses(True)
    L, h, d, nc = eng.L, eng.h, w.dx, w.ncand
    sizes = (5, 37, 130)[:d]
    ks = list(range(d))
    idx = [torch.from_numpy(wl.synth_fibers(w, k, F, seed=0xA11 + F)).cuda() for k, F in zip(ks, sizes)]
    shapes = [(F, w.ngrid[k]) for k, F in zip(ks, sizes)]
    gen = torch.Generator(device="cuda").manual_seed(5)
    pol = [torch.randint(0, nc + M, s, dtype=torch.int32, device="cuda", generator=gen) for s in shapes]
    pol = [torch.where(p >= nc, p + 1, p).contiguous() for p in pol]
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
    assert any((t > nc).any() for t in ui), "interventions win in these batches"
    for s in range(d):
        assert not torch.isnan(out[s]).any() and (ab[s] == 0).any()
        assert torch.equal(a_out[s], out[s]) and torch.equal(a_ui[s], ui[s]) and torch.equal(a_ab[s], ab[s]), f"bellman, dimension {s}"
    p_out, _, p_ab = fresh()
    for s, k in enumerate(ks):
        assert L.c3sc_hip_policy_fibers(h, k, sizes[s], idx[s].data_ptr(), pol[s].data_ptr(), p_out[s].data_ptr(), p_ab[s].data_ptr(), None) == 0
    q_out, _, q_ab = fresh()
    assert L.c3sc_hip_policy_fibers_all(h, d, KS, FS, GC.ptrs(idx), GC.ptrs(pol), GC.ptrs(q_out), GC.ptrs(q_ab), C.c_void_p(None)) == 0
    torch.cuda.synchronize()
    for s in range(d):
        # inf == inf where a forced intervention is not admissible
        assert torch.equal(q_out[s], p_out[s]) and torch.equal(q_ab[s], p_ab[s]) and torch.equal(p_ab[s], ab[s]), f"policy, dimension {s}"
    assert eng.status(clear=True) == 0
    eng.close()


# ---------------------------------------------------------------------------------------------------- errors
def test_errors(ids):
    import torch

    L = E.load_library()
    err = lambda e: L.c3sc_hip_last_error(e.h).decode()
    # no model yet
    eng = E.BellmanEngine(0)
    assert L.c3sc_hip_set_impulses(eng.h, 1) == ERR_ARG and "set_model first" in err(eng)
    assert L.c3sc_hip_set_impulses(None, 1) == ERR_ARG
    # built-in model
    w = wl.c4_car7d().scaled(ngrid=(7,) * 7, rank=4)
    eng.configure(w, wl.synth_cores(w))
    assert L.c3sc_hip_set_impulses(eng.h, 1) == ERR_UNSUPPORTED
    assert L.c3sc_hip_set_impulses(eng.h, 0) == 0
    idx7 = wl.synth_fibers(w, 0, 8)
    assert np.isfinite(eng.bellman_fibers_host(0, idx7)[0]).all()  # still usable
    # a run-time model compiled without nimpulse
    wp = JL.lqr_workload(ids["lqr_plain"], 4, 0.1)
    eng = E.BellmanEngine(0)
    eng.configure(wp, wl.synth_cores(wp))
    assert L.c3sc_hip_set_impulses(eng.h, 1) == ERR_UNSUPPORTED
    assert "impulse kernels" in err(eng)
    # the model with impulse kernels
    wr = IL.lqr_workload(ids["lqr"], 4, 0.1, IL.lqr_cost_scale(4))
    eng = E.BellmanEngine(0)
    eng.configure(wr, wl.synth_cores(wr))
    eng.set_impulses(True)
    idx = np.ascontiguousarray(wl.synth_fibers(wr, 0, 8), dtype=np.int32)
    out = np.empty((8, wr.ngrid[0]))
    launch = lambda e: L.c3sc_hip_bellman_fibers_host(e.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None)
    for variant in (E.VARIANT_FIBER_PAIR, E.VARIANT_FIBER_QUAD):
        eng.set_variant(variant)
        assert launch(eng) == ERR_UNSUPPORTED
        assert "fiber-per-wave kernel only" in err(eng)
    eng.set_variant(E.VARIANT_AUTO)
    assert launch(eng) == 0
    # the horizon step, the stopping switch and a game are refused while it is on
    assert L.c3sc_hip_set_horizon_step(eng.h, C.c_double(0.01)) == ERR_UNSUPPORTED
    assert L.c3sc_hip_set_stopping(eng.h, 1) == ERR_UNSUPPORTED
    U, W = np.array([[0.0]]), np.array([[1.0]])
    up, wp_ = U.ctypes.data_as(C.POINTER(C.c_double)), W.ctypes.data_as(C.POINTER(C.c_double))
    assert L.c3sc_hip_set_game(eng.h, 1, 1, up, 1, wp_, 0) == ERR_UNSUPPORTED
    assert "interventions" in err(eng)
    # policy iteration across contexts, integrate, the TABLE and box calls
    other = E.BellmanEngine(0)
    other.configure(wr, wl.synth_cores(wr))
    assert L.c3sc_hip_cross_iteration_pi(eng.h, other.h, 1, None) == ERR_UNSUPPORTED
    assert "impulse control" in err(eng)
    assert L.c3sc_hip_cross_iteration_pi(other.h, eng.h, 1, None) == ERR_UNSUPPORTED
    x0 = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(E.C3scHipError, match="not offered for impulse control"):
        eng.integrate(x0, 0.1, 3, method="rk4")
    tables = np.zeros((8, wr.ngrid[0], wr.ncand, 5))
    costs2 = np.zeros((8, wr.ngrid[0], 2))
    assert L.c3sc_hip_bellman_fibers_tables_host(eng.h, 0, 8, idx.ctypes.data, tables.ctypes.data, costs2.ctypes.data,
                                                 out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "impulse" in err(eng)
    eng.set_model(ids["lqr"], wr.params)  # the TABLE call sets its model before it refuses
    L.c3sc_hip_bellman_fibers_box_host.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 4
    lb, ub = np.array([-1.0, -1.0]), np.array([1.0, 1.0])
    L.c3sc_hip_set_control_box.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    assert L.c3sc_hip_set_control_box(eng.h, 2, lb.ctypes.data, ub.ctypes.data, 5, 1) == 0
    assert L.c3sc_hip_bellman_fibers_box_host(eng.h, 0, 8, idx.ctypes.data, out.ctypes.data, None, None) == ERR_UNSUPPORTED
    assert "interventions" in err(eng)
    with pytest.raises(E.C3scHipError, match=rf"\(code {ERR_UNSUPPORTED}\): simulate: interventions have no control-box form"):
        eng.simulate(x0, 0.02, 3, box=True)
    assert launch(eng) == 0  # still usable
    assert torch.isfinite(eng.simulate(x0, 0.02, 3)["cost"]).all()
    # the horizon step or the stopping switch first: set_impulses is refused
    eng2 = E.BellmanEngine(0)
    eng2.configure(wp, wl.synth_cores(wp))
    eng2.set_stopping(True)
    eng2.set_model(ids["lqr"], wr.params)
    assert L.c3sc_hip_set_impulses(eng2.h, 1) == ERR_UNSUPPORTED and "stop" in err(eng2)
    eng2.set_stopping(False)
    eng2.set_model(ids["lqr_plain"], wp.params)
    eng2.set_horizon_step(0.01)
    eng2.set_model(ids["lqr"], wr.params)
    assert L.c3sc_hip_set_impulses(eng2.h, 1) == ERR_UNSUPPORTED and "horizon" in err(eng2)
    eng2.set_horizon_step(0.0)
    assert L.c3sc_hip_set_impulses(eng2.h, 1) == 0
    # jumps on top need a model compiled with jump kernels as well
    wo = IL.lqr_workload(ids["lqr_impulse_only"], 4, 0.1, IL.lqr_cost_scale(4))
    eng3 = E.BellmanEngine(0)
    eng3.configure(wo, wl.synth_cores(wo))
    eng3.set_impulses(True)
    assert L.c3sc_hip_set_jumps(eng3.h, 1) == ERR_UNSUPPORTED
    assert launch(eng3) == 0
    # a model without impulse kernels set after the switch: caught at launch
    eng.set_model(ids["lqr_plain"], SL.LQR_PRM)
    assert launch(eng) == ERR_UNSUPPORTED
    assert "impulse kernels" in err(eng)
    with pytest.raises(E.C3scHipError, match="impulse kernels"):
        eng.simulate(x0, 0.02, 3)
    # game first, interventions second
    gid = E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_game_ic", game=True, **SL.LQR_MASKS)
    wg = JL.lqr_workload(gid, 4, 0.1)
    eng4 = E.BellmanEngine(0)
    eng4.configure(wg, wl.synth_cores(wg))
    eng4.set_game(np.array([[0.0], [1.0]]), np.array([[0.0], [0.5]]))
    assert L.c3sc_hip_set_impulses(eng4.h, 1) == ERR_UNSUPPORTED
    # switching it off restores the plain operator
    eng.set_model(ids["lqr"], wr.params)
    eng.set_impulses(False)
    assert launch(eng) == 0


# ---------------------------------------------------------------------------------------------------- rollouts
@pytest.mark.parametrize("rank", [4, 12])
def test_noise_free_rollouts_replay_the_interventions(ids, rank):
    """zero normals, jumps off: at every step the move of a lane is either the drift's or exactly y_m(xin) of one intervention; the
    marks read off the device's trajectory equal impulse_lib's decision on the off-grid stencil wherever its margin is clear,
    and the replay with them gives the device's states and costs to 1e-12.  A lane whose intervention lands beyond the absorbing
    face or inside the obstacle decodes as an exit at the next step"""
    import torch

    beta, dt, N = 0.3, 0.02, 40
    w = IL.lqr_workload(ids["lqr"], rank, beta, IL.lqr_cost_scale(rank))
    # a cheap boundary (s = 0.02 for 2): beyond the absorbing face lies the cheapest place there is, so the controller of a lane
    # near it does choose the intervention that leaves the domain
    w = dataclasses.replace(w, params=w.params[:3] + (0.02,) + w.params[4:])
    cores = wl.synth_cores(w)
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    eng.set_impulses(True)
    tr = JL.Train(w, cores)
    rng = np.random.default_rng(5)
    n = 96
    x0 = np.stack([rng.uniform(-1.9, 1.9, n), rng.uniform(-1.9, 1.9, n)], axis=-1)
    x0[:24, 0] = rng.uniform(1.5, 1.95, 24)  # intervention 1 from here lands beyond the absorbing face
    x0[24:32] = (0.85, -0.95)  # inside the obstacle: exits at step 0
    x0_t = torch.tensor(x0, dtype=torch.float64, device="cuda")
    noise = torch.zeros((n, N, 2), dtype=torch.float64, device="cuda")
    r = eng.simulate(x0_t, dt, N, seed=1, noise_t=noise, wrap_periodic=True, save_every=1)
    torch.cuda.synchronize()
    assert eng.last_kernel() == f"k_rollout<rtc:lqr_ic,{rank}>"
    traj, u, J, ex = (r[k].cpu().numpy() for k in ("traj", "u", "cost", "exit"))
    bcost, ocost = _costs(w)
    # the marks as the trajectory shows them: the step whose next state is y_m of the wrapped state, bit for bit or to rounding
    marks = np.full((n, N), -1)
    unsure = 0
    for s in range(N):
        xin = JL.wrap(w, traj[:, s])
        kk, y = IL.lqr_impulses(w.params, xin)
        for m in range(IL.LQR_NIMPULSE):
            hit = (np.abs(traj[:, s + 1] - y[:, m]).max(axis=1) <= 1e-12) & np.isfinite(kk[:, m]) & (np.abs(u[:, s]).max(axis=1) == 0.0)
            marks[:, s] = np.where(hit & (marks[:, s] < 0), m, marks[:, s])
        # the reference's decision at the states the device visited
        V_t, ab_t = eng.stencil_points(torch.tensor(xin, dtype=torch.float64, device="cuda"))
        ui, mg = IL.point_decisions(w, SL.lqrn_host, IL.lqr_impulses, tr, xin, V_t.cpu().numpy(), ab_t.cpu().numpy(), bcost, ocost)
        alive = (ex < 0) | (ex > s)
        sure = alive & (mg > 1e-9) & (ui >= 0)
        unsure += int((alive & ~sure).sum())
        want = np.where(ui > w.ncand, ui - w.ncand - 1, -1)
        np.testing.assert_array_equal(marks[sure, s], want[sure], err_msg=f"step {s}")
    stage = lambda x, uu: SL.lqrn_host(w.params, x, uu)[2]
    nxt, r_ex, r_J = IL.replay(w, IL.lqr_impulses, lambda x, uu: uu, stage, bcost, ocost, traj, u, marks, dt, beta, wrap=True)
    err = np.abs(traj[:, 1:] - nxt).max()
    print("rollout replay: interventions", [(marks == m).sum() for m in range(3)], "exits", (r_ex >= 0).sum(), "unsure steps", unsure,
          "max state err", err, "max cost err", np.abs(J - r_J).max())
    assert err <= 1e-12
    np.testing.assert_array_equal(ex, r_ex)
    assert np.all(np.abs(J - r_J) <= 1e-12 * np.maximum(1.0, np.abs(r_J)))
    assert all((marks == m).sum() >= 3 for m in range(3)), "every intervention occurs"
    assert (r_ex[24:32] == 0).all()
    # lanes whose intervention left the domain: the exit step follows the intervention, and the exit cost is paid there
    left = [i for i in range(n) if r_ex[i] > 0 and marks[i, r_ex[i] - 1] >= 0]
    print("exits by an intervention", len(left))
    assert len(left) >= 3, "lanes whose intervention leaves the domain"
    for i in left:
        s1 = r_ex[i]
        assert traj[i, s1, 0] > 2.0 and (traj[i, s1:] == traj[i, s1]).all(), "beyond the absorbing face, and frozen there"
    # the saved control of an intervention step is 0
    assert (np.abs(u[marks >= 0]) == 0.0).all()
    eng.close()


@pytest.mark.parametrize("jumps", [False, True], ids=["nojump", "jump"])
def test_infinite_costs_leave_the_rollouts_their_bits(ids, jumps):
    """with every cost +inf a noisy run of the impulse rollout kernel gives the states of the rollout kernel without
    interventions bit for bit, and of the jump rollout kernel with jumps on"""
    import torch

    w = IL.lqr_workload(ids["lqr"], 4, 0.3, np.inf)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    eng.set_jumps(jumps)
    x0_t = torch.tensor(np.random.default_rng(1).uniform(-1.5, 1.5, (64, 2)), dtype=torch.float64, device="cuda")
    a = eng.simulate(x0_t, 0.02, 16, seed=3, wrap_periodic=True, save_every=1)
    eng.set_impulses(True)
    b = eng.simulate(x0_t, 0.02, 16, seed=3, wrap_periodic=True, save_every=1)
    torch.cuda.synchronize()
    for k in ("traj", "u", "cost", "exit"):
        assert torch.equal(a[k], b[k]), k
    assert a["traj"].std() > 0.05
    eng.close()


# ---------------------------------------------------------------------------------------------------- the reference API
def test_vi_solve_through_the_reference_api(tmp_path):
    """the inventory problem of examples/inventory_impulse.c through libc3sc.so in a child process: c3control_vi_solve sweep by
    sweep (11 x 11, rank 11, host callbacks and c3control_add_impulses beside the impulse model).  The first sweep passes the
    first-fiber check against the host twin; every sweep, before and after it, equals dense_vi to 1e-9"""
    import os
    import subprocess
    import sys

    out = tmp_path / "vi.npz"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, C3SC_CROSS_TRACE="1")
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, "-c", f"import impulse_lib; impulse_lib.vi_child({str(out)!r})"],
                       cwd=os.path.dirname(os.path.abspath(__file__)), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert IL.IMPULSE_MARKER in r.stderr
    V = np.load(out)["V"]
    w = IL.inv_workload(0)
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    bcost = lambda x: IL.inv_bcost(w.params, x)
    dense, dec = IL.dense_vi(w, IL.inv_host, IL.inv_impulses, bcost, bcost(X), IL.INV_VI_SWEEPS)
    plain, _ = IL.dense_vi(w, IL.inv_host, IL.inv_impulses, bcost, bcost(X), IL.INV_VI_SWEEPS, with_impulses=False)
    assert np.abs(dense[-1] - plain[-1]).max() > 1e-1, "the orders move the solution"
    assert all((dec[s] > w.ncand).any() for s in range(IL.INV_VI_SWEEPS))
    assert V.shape == dense.shape
    for s in range(len(V)):
        err = np.abs(V[s] - dense[s]) / np.maximum(1.0, np.abs(dense[s]))
        print("sweep", s, "max err", err.max())
        assert err.max() <= 1e-9, (s, err.max())


# ---------------------------------------------------------------------------------------------------- noisy rollouts
def test_noisy_rollouts_estimate_the_value_function():
    """8192 noisy rollouts of the inventory problem from three states under its dense fixed point V: the mean of the cost, with
    the discounted V(x_N) of the trajectories still alive after N steps, estimates V(x_0) within 4 standard errors plus the
    discretisation allowance pinned on the CPU (impulse_lib.INV_ALLOWANCE: at each state twice the gap of the numpy rollout
    restatement with 2^18 paths there).  This ties the one-step-slot convention of the rollouts -- an intervention pays the discounted k_m,
    no stage cost and no increment -- to the value function under noise"""
    import torch

    mid = E.compile_model(IL.INV, 2, 2, ranks=(12,), name="inventory_sim", nimpulse=IL.INV_NIMPULSE, **IL.INV_MASKS)
    w = IL.inv_workload(mid)
    V, dec = IL.inv_fixed_point(w)
    ranks, cores = GC.train(V, 12)
    eng = E.BellmanEngine(0)
    eng.configure(dataclasses.replace(w, ranks=tuple(ranks)), cores)
    eng.set_impulses(True)
    xg = w.xgrid()[0]
    n, dt, N = 8192, IL.INV_SIM_DT, IL.INV_SIM_STEPS
    for x0, allow in zip(IL.INV_X0, IL.INV_ALLOWANCE):
        i, j = (int(np.argmin(np.abs(xg - v))) for v in x0)
        v0 = V[i, j]
        x0_t = torch.tensor([x0] * n, dtype=torch.float64, device="cuda")
        r = eng.simulate(x0_t, dt, N, seed=11)
        torch.cuda.synchronize()
        assert "inventory_sim" in eng.last_kernel()
        cost, ex, vend = (r[k].cpu().numpy() for k in ("cost", "exit", "vend"))
        J = cost + np.where(ex < 0, np.exp(-w.discount * N * dt) * vend, 0.0)
        se = J.std() / np.sqrt(n)
        print("inventory rollouts", x0, "mean", J.mean(), "v0", v0, "se", se, "exited", (ex >= 0).mean())
        assert abs(J.mean() - v0) <= 4 * se + allow, (x0, J.mean(), v0, se, allow)
    assert eng.status() == 0
    eng.close()
