"""The numpy restatement of the jump backup (tests/jump_lib.py) checked on its own, and the host twin of the rollouts' jump
uniforms (c3sc_hip_jump_uniforms).  No GPU is needed.

- Its interpolant equals the extended-precision reference of the off-grid tests (offgrid_ref) in both interpolation classes.
- The known answer: with b = sigma = 0, constant lambda and g and every mark beyond an absorbing face of cost c, the backup of
  every node is g / lambda + exp(-beta / lambda) c to 1e-14.
- lambda = 0 gives stop_lib's dense chain of the put bit for bit; with lambda > 0 the price moves and stays inside the CFL rule.
- The weights of every test model sum to 1, and the marks of the 2-D LQR reach the four kinds of target.
- The index-margin precondition of the GPU tests, on the stencils the restatement forms itself along the periodic dimension of
  the ragged grid (end-point rule included): at most 0.1 % of the live nodes have |best - second| below 1e-9.
- The uniforms' twin: in (0, 1), a function of (seed, trajectory, step) alone, on a counter no normal uses.
- Dense policy iteration (jump_lib.dense_pi), the reference of tests/test_gpu_jump_policy.py: its first sweep is dense_vi's bit
  for bit, the greedy policy of s |x|^2 has a margin of at least 1e-6 at every live node, the jump term changes it at 20 nodes
  or more, and a policy without the jump term, an evaluation without it and a policy re-taken every sweep each move the result
  by more than 1e-2; successive sweeps contract.
- The policy memo in jump mode (jump_policy_model.py): both step-level cases of the GPU test pass on a numpy device, and fail
  with the policy taken from the jump-free operator or the policy tag not reset."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import cross_memo_model as mm
import backup_ref as BR
import horizon_lib as H
import jump_lib as JL
import jump_policy_model as JP
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
    x = BR.node_states(w, 1, idx)
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


# ---------------------------------------------------------------------------------------------------- dense policy iteration
@pytest.fixture(scope="module")
def lqr_pi():
    """the 11 x 11 jump LQR of the reference-API tests: (workload, boundary cost, P = s |x|^2 at the nodes, dense_pi of six sweeps)"""
    w = JL.lqr_vi_workload(0)
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    bcost = lambda x: H.lqr_terminal(JL.LQR_PRM, x)
    P = H.lqr_terminal(JL.LQR_PRM, X)
    return w, bcost, P, JL.dense_pi(w, SL.lqrn_host, JL.lqr_jumps, bcost, P, 6)


def test_dense_pi_first_sweep_is_the_value_iteration_sweep(lqr_pi):
    w, bcost, P, (mu, margin, V) = lqr_pi
    vi = JL.dense_vi(w, SL.lqrn_host, JL.lqr_jumps, bcost, P, 2)
    np.testing.assert_array_equal(V[0], P)
    np.testing.assert_array_equal(V[1], vi[1])
    live = mu >= 0
    assert live.sum() == 81 and (mu[~live] == -1).all() and np.isinf(margin[~live]).all()
    print("dense_pi: smallest margin of the greedy policy over the live nodes", margin[live].min())
    assert margin[live].min() >= 1e-6, "every node is compared: the greedy candidate of P is pinned at every live node"
    # a frozen policy is not value iteration: the second sweep already differs
    assert np.abs(vi[2] - V[2]).max() > 1e-2


def test_dense_pi_sees_the_jumps_in_the_policy_and_in_the_evaluation(lqr_pi):
    """the preconditions of tests/test_gpu_jump_policy.py: the jumps and the frozen policy move the solution"""
    w, bcost, P, (mu, _, V) = lqr_pi
    w0 = dataclasses.replace(w, params=JL.LQR_ZERO_RATE_PRM)
    mu0, _, _ = JL.dense_pi(w0, SL.lqrn_host, JL.lqr_jumps, bcost, P, 0)
    live = mu >= 0
    print("dense_pi: the jump term changes the greedy candidate at", (mu0 != mu)[live].sum(), "of", live.sum(), "live nodes")
    assert (mu0 != mu)[live].sum() >= 20
    _, _, Va = JL.dense_pi(w, SL.lqrn_host, JL.lqr_jumps, bcost, P, 4, mu=mu0)   # greedy policy of the jump-free operator
    _, _, Vb = JL.dense_pi(w0, SL.lqrn_host, JL.lqr_jumps, bcost, P, 4, mu=mu)   # evaluation without the jump term
    print("dense_pi after four sweeps: policy without jumps", np.abs(Va[4] - V[4]).max(), "evaluation without jumps", np.abs(Vb[4] - V[4]).max())
    assert np.abs(Va[4] - V[4]).max() > 1e-2
    assert np.abs(Vb[4] - V[4]).max() > 1e-2
    # mu given back reproduces the chain bit for bit
    np.testing.assert_array_equal(JL.dense_pi(w, SL.lqrn_host, JL.lqr_jumps, bcost, P, 4, mu=mu)[2], V[:5])


def test_dense_pi_sweeps_contract(lqr_pi):
    _, _, _, (_, _, V) = lqr_pi
    steps = [np.abs(V[s + 1] - V[s]).max() for s in range(6)]
    print("dense_pi: max |V_{s+1} - V_s|", steps)
    assert all(b < a for a, b in zip(steps, steps[1:])), steps


# ---------------------------------------------------------------------------------------------------- the policy memo in jump mode
def _sim_maker(oracle, case, fault=None):
    _, jumps = JP.workload(case)
    return lambda w, cores: JP.JumpSimDevice(oracle, w, cores, jumps, fault=fault)


@pytest.mark.parametrize("case", JP.CASES, ids=[c[0] for c in JP.CASES])
def test_jump_policy_cases_pass_on_the_stand_in(oracle, case):
    """the cases of tests/test_gpu_jump_policy.py on the numpy stand-in: admitted (margins, 10 % of the hits of the second call
    where P1 and P2 choose differently) and passed, before a GPU sees them"""
    reps = JP.scenario(_sim_maker(oracle, case), oracle, case)
    assert len(reps) == 3 and reps[0]["policies_stored"] > 0 and reps[1]["hits"] > 0
    if case[0] in JP.CASES_WITH_NEW_NODES:  # 'stored nodes keep P1's candidate and new nodes take P2's'
        assert reps[1]["policies_stored"] > 0
    w, _ = JP.workload(case)
    assert len(set(w.bc)) == w.dx, "every dimension has a boundary type of its own"


@pytest.mark.parametrize("case", JP.CASES, ids=[c[0] for c in JP.CASES])
@pytest.mark.parametrize("fault,match", [("policy-without-jumps", "tag 7 under P1"), ("policy-tag-not-reset", "tag 8 under P2")])
def test_a_mistake_planted_in_the_jump_policy_stand_in_is_caught(oracle, case, fault, match):
    assert fault in JP.FAULTS
    with pytest.raises(AssertionError, match=match) as e:
        JP.scenario(_sim_maker(oracle, case, fault), oracle, case)
    assert not isinstance(e.value, mm.CaseRefused), f"the case was refused, not failed: {e.value}"
    print(f"{case[0]}, {fault}: {type(e.value).__name__}: {str(e.value)[:200]}")


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
