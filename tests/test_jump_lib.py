"""The numpy restatement of the jump backup (tests/jump_lib.py) checked on its own, and the host twin of the rollouts' jump
uniforms (c3sc_hip_jump_uniforms).  No GPU is needed.

- Its interpolant equals the extended-precision reference of the off-grid tests (offgrid_ref) in both interpolation classes.
- The known answer: with b = sigma = 0, constant lambda and g and every mark beyond an absorbing face of cost c, the backup of
  every node is g / lambda + exp(-beta / lambda) c to 1e-14.
- lambda = 0 gives stop_lib's dense chain of the put bit for bit; with lambda > 0 the price moves and stays inside the CFL rule.
- The weights of every test model sum to 1, and the marks of the 2-D LQR reach the four kinds of target.
- The index-margin precondition of the GPU tests, on the stencils the restatement forms itself along the periodic dimension of
  the ragged grid (end-point rule included): at most 0.1 % of the live nodes have |best - second| below 1e-9.
- The uniforms' twin: in (0, 1), a function of (seed, trajectory, step) alone, on a counter no normal uses."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import horizon_lib as H
import jump_lib as JL
import offgrid_ref as OR
import stop_lib as SL


@pytest.mark.parametrize("model", ["lqr", "lqr3"])
def test_interpolant_equals_the_extended_precision_reference(model):
    w = JL.lqr_workload(0, 8, 0.3) if model == "lqr" else JL.lqr3_workload(0)
    cores = wl.synth_cores(w)
    tr, ref = JL.Train(w, cores), OR.OffgridRef(w, cores)
    rng = np.random.default_rng(3)
    y = rng.uniform(-2.4, 2.4, size=(40, w.dx))
    y[:4] = [[g[3] for g in w.xgrid()], [g[0] for g in w.xgrid()], [g[-1] for g in w.xgrid()], [g[1] + 1e-13 for g in w.xgrid()]]
    for constelm in (False, True):
        got = tr.value(y, constelm)
        for p in range(len(y)):
            v, vabs = ref.value(y[p], constelm)
            assert abs(got[p] - float(v)) <= 1e-13 * float(vabs), (p, constelm)


def test_known_answer():
    w = JL.known_workload(0)
    cores = wl.synth_cores(w)
    tr = JL.Train(w, cores)
    idx = wl.synth_fibers(w, 1, 9)
    N = w.ngrid[1]
    costs = np.random.default_rng(0).uniform(1.0, 2.0, size=(9, N, 5))
    ab = np.zeros((9, N), dtype=np.int32)
    host = lambda prm, x, u: (np.zeros(x.shape), np.zeros(x.shape), np.full(x.shape[:-1], prm[0]))
    jumps = lambda prm, x: (np.full(len(x), prm[1]), np.broadcast_to(np.array([0.25, 0.25, 0.5]), (len(x), 3)),
                            np.stack([x + np.array([10.0 + m, 0.0]) for m in range(3)], axis=1))
    bcost, ocost = (lambda x: np.full(len(x), w.params[2])), (lambda x: np.full(len(x), -1.0))
    out, ui, _, stat, _, _, J = JL.jump_fibers(w, host, jumps, tr, 1, idx, costs, ab, bcost, ocost)
    assert not stat.any() and (ui == 0).all() and (J == w.params[2]).all()
    assert np.abs(out - JL.known_answer()).max() <= 1e-14 * JL.known_answer()
    out0, ui0, _, stat0, _, _, _ = JL.jump_fibers(w, host, jumps, tr, 1, idx, costs, ab, bcost, ocost, with_jumps=False)
    assert stat0.all() and (ui0 == -1).all() and (out0 == 0.0).all()  # without jumps every node is stationary


def test_zero_rate_chain_is_the_put_without_jumps():
    w = JL.put_workload(0)
    psi = lambda x: SL.put_psi(JL.PUT_PRM, x)
    plain, pdec, _ = SL.dense_chain(dataclasses.replace(w, params=SL.PUT_PRM), SL.put_host, psi, JL.PUT_DELTA, JL.PUT_STAGES)
    w0 = dataclasses.replace(w, params=JL.PUT_PRM[:3] + (0.0,) + JL.PUT_PRM[4:])
    zero, zdec, _ = JL.dense_chain(w0, SL.put_host, JL.put_jumps, psi, JL.PUT_DELTA, JL.PUT_STAGES)
    np.testing.assert_array_equal(zero, plain)
    np.testing.assert_array_equal(zdec == w.ncand, pdec)
    merton, _, cfl = JL.dense_chain(w, SL.put_host, JL.put_jumps, psi, JL.PUT_DELTA, JL.PUT_STAGES)
    assert not cfl
    assert np.abs(merton[0] - plain[0]).max() > 1e-3
    assert (merton[0] <= plain[0] + 1e-15).all(), "downward-skewed jumps make the put worth more (a cost: more negative)"


def test_weights_sum_to_one_and_the_marks_reach_every_kind_of_target():
    w = JL.lqr_workload(0, 4, 0.3)
    xg = w.xgrid()
    x = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1).reshape(-1, 2)
    lam, pi, y = JL.lqr_jumps(w.params, x)
    assert (lam > 0).all() and (pi >= 0).all() and np.abs(pi.sum(axis=1) - 1.0).max() <= 1e-12
    kinds = np.zeros(4, dtype=bool)
    for m in range(JL.LQR_NJUMP):
        _, inobs, beyond, moved = JL.target_kinds(w, y[:, m])
        kinds |= np.array([(~inobs & ~beyond & ~moved).any(), (beyond & ~inobs).any(), inobs.any(), moved.any()])
    assert kinds.all(), kinds
    for jumps, wk in ((JL.lqr3_jumps, JL.lqr3_workload(0)), (JL.put_jumps, JL.put_workload(0))):
        xs = np.random.default_rng(1).uniform(0.3, 1.7, size=(50, wk.dx))
        assert np.abs(jumps(wk.params, xs)[1].sum(axis=1) - 1.0).max() <= 1e-12


def _periodic_fibers(w, tr, idx):
    """stencils and flags of fibers along the periodic dimension 1 of the ragged 2-D grid, as the kernels form them: a fiber on
    an absorbing face is absorbed, its end points are live again (the end-point rule), neighbours across the seam"""
    xg = w.xgrid()
    n0, N = w.ngrid
    x = H.node_states(w, 1, idx)
    F = len(idx)
    inobs = JL.target_kinds(w, x.reshape(-1, 2))[1].reshape(F, N)
    V, ab = np.zeros((F, N, 5)), np.zeros((F, N), dtype=np.int32)
    val = lambda i0, j: tr.value(np.stack([xg[0][i0], xg[1][j]], axis=-1))
    j = np.arange(N)
    for f in range(F):
        i0 = idx[f, 0]
        face = i0 in (0, n0 - 1)
        lo0, hi0 = (i0, i0) if face else (i0 - 1, i0 + 1)
        a = np.where(face, 1, np.where(inobs[f], -1, 0))
        a[0] = a[-1] = 0
        lo, hi = np.where(a == 0, j - 1, j), np.where(a == 0, j + 1, j)
        lo[0] = lo[-1] = N - 2
        hi[0] = hi[-1] = 1
        V[f, :, 4] = val(np.full(N, i0), j)
        V[f, :, 0], V[f, :, 1] = val(np.full(N, lo0), j), val(np.full(N, hi0), j)
        V[f, :, 2], V[f, :, 3] = V[f, lo, 4], V[f, hi, 4]
        ab[f] = a
    return V, ab


@pytest.mark.parametrize("rank", [4, 8, 12])
@pytest.mark.parametrize("discount", [0.3, 0.0])
def test_index_margin_precondition(rank, discount):
    w = JL.lqr_workload(0, rank, discount)
    tr = JL.Train(w, wl.synth_cores(w))
    idx = wl.synth_fibers(w, 1, 257)
    V, ab = _periodic_fibers(w, tr, idx)
    bcost, ocost = (lambda x: SL.lqrn_terminal(w.params, x)), (lambda x: np.full(len(x), 5.0))
    live = ab == 0
    assert ((ab == 1) & (V[..., 0] == V[..., 1])).any() and live[:, 0].all(), "fibers on an absorbing face, with live end points"
    for delta in (None, 0.01):
        _, _, mg, stat, cfl, _, _ = JL.jump_fibers(w, SL.lqrn_host, JL.lqr_jumps, tr, 1, idx, V, ab, bcost, ocost, delta)
        assert (mg[live] <= 1e-9).mean() <= 0.001, (delta, (mg[live] <= 1e-9).mean())
        assert not stat.any() and not cfl.any()


def test_put_rollout_restatement_holds_the_pinned_gap():
    """the constant next to which the gap is written: 2^18 paths of the numpy rollouts of the put from the first state stay
    within PUT_GAP plus 4 standard errors of the dense chain's V_0"""
    w = JL.put_workload(0)
    psi = lambda x: SL.put_psi(JL.PUT_PRM, x)
    dense, _, _ = JL.dense_chain(w, SL.put_host, JL.put_jumps, psi, JL.PUT_DELTA, JL.PUT_STAGES)
    J = JL.put_rollouts(w, dense, JL.PUT_X0[0], 1 << 18, JL.PUT_DELTA, np.random.default_rng(31))
    v0 = dense[0][5, 5]
    se = J.std() / np.sqrt(len(J))
    assert abs(J.mean() - v0) <= JL.PUT_GAP + 4 * se, (J.mean(), v0, se)
    assert JL.PUT_BOUND == 2 * JL.PUT_GAP


def test_jump_uniforms_twin():
    L = E.load_library()
    u = np.array([E.jump_uniforms(7, t, s) for t in range(64) for s in range(64)])
    assert ((u > 0.0) & (u < 1.0)).all()
    assert abs(u.mean() - 0.5) < 0.02 and abs(np.corrcoef(u[:, 0], u[:, 1])[0, 1]) < 0.05
    assert E.jump_uniforms(7, 3, 5) == E.jump_uniforms(7, 3, 5) != E.jump_uniforms(8, 3, 5)
    assert E.jump_uniforms(7, 3, 5) != E.jump_uniforms(7, 5, 3)
    assert E.jump_uniforms(7, (1 << 40) + 3, 5) != E.jump_uniforms(7, 3, 5)  # the high word of the trajectory index counts
    assert L.c3sc_hip_jump_uniforms(1, 0, 0, None) == 1
    # no normal of the same (seed, trajectory, step) is made from these uniforms: Box-Muller of (u0, u1) is none of them
    z = np.empty(12)
    assert L.c3sc_hip_normals(7, 3, 1, 5, 1, 12, z.ctypes.data_as(C.POINTER(C.c_double))) == 0
    u0, u1 = E.jump_uniforms(7, 3, 5)
    bm = np.sqrt(-2.0 * np.log(u0)) * np.array([np.cos(2 * np.pi * u1), np.sin(2 * np.pi * u1)])
    assert np.abs(z[:, None] - bm[None, :]).min() > 1e-6
