"""The numpy restatement of the correlated backup (tests/corr_lib.py) on the CPU: the known answer
x0 x1 + delta a for both signs of a; every test model's chain has row sums 1 and non-negative probabilities (the dominance model
is the exception, at the nodes the dominance test names) and reproduces the first two moments b dt and a dt; and the
precondition of the index comparisons of tests/test_gpu_corr.py -- the reference's own decision is clear at 99.9 % of the live
nodes -- holds on every model used there."""
import dataclasses

import numpy as np
import pytest

from c3sc_amd import workloads as wl
import backup_ref as BR
import corr_lib as CL
import jump_lib as JL
import stop_lib as SL


def _dense_stencils(w, V):
    """(ix [P, D], x [P, D], axis stencils [P, 2D+1]) of every node of the full array V, by corr_lib's neighbour rule"""
    grids = np.meshgrid(*[np.arange(n) for n in w.ngrid], indexing="ij")
    ix = np.stack([g.reshape(-1) for g in grids], axis=-1)
    xg = w.xgrid()
    x = np.stack([np.asarray(xg[m])[ix[:, m]] for m in range(w.dx)], axis=-1)
    S = np.empty((len(ix), 2 * w.dx + 1))
    for m in range(w.dx):
        lo, hi = CL.neighbour_indices(ix[:, m], w.ngrid[m], w.bc[m])
        a, b = [ix[:, q] for q in range(w.dx)], [ix[:, q] for q in range(w.dx)]
        a[m], b[m] = lo, hi
        S[:, 2 * m], S[:, 2 * m + 1] = V[tuple(a)], V[tuple(b)]
    S[:, 2 * w.dx] = V.reshape(-1)
    return ix, x, S


@pytest.mark.parametrize("a", [CL.KNOWN_A, -CL.KNOWN_A])
def test_known_answer(a):
    w = CL.known_workload(1000, a)
    V = CL.full_values(w, CL.known_cores(w))
    xg = w.xgrid()
    np.testing.assert_allclose(V, np.outer(xg[0], xg[1]), rtol=0, atol=1e-15)
    ix, x, S = _dense_stencils(w, V)
    h2, t = BR.mca_constants(w)
    C = np.asarray(w.cands, dtype=np.float64)
    interior = np.all((ix > 0) & (ix < np.array(w.ngrid) - 1), axis=1)
    cq, cpv, r = CL.corr_terms(w, CL.known_covar, CL.KNOWN_PAIRS, V, ix, x, S)
    assert not CL.dominance(w, CL.known_host, CL.KNOWN_PAIRS, x, r).any()
    vals, _, cfl = BR.candidate_values(CL.known_host, w.params, x, S, C, h2, t, 0.0, cq, cpv, CL.KNOWN_DELTA)
    assert not cfl.any()
    ref = x[:, 0] * x[:, 1] + CL.KNOWN_DELTA * a
    assert np.abs(vals[interior, 0] - ref[interior]).max() <= 1e-14
    plain, _, _ = BR.candidate_values(CL.known_host, w.params, x, S, C, h2, t, 0.0, 0.0 * cq, 0.0 * cpv, CL.KNOWN_DELTA)
    assert np.abs(plain[interior, 0] - x[interior, 0] * x[interior, 1]).max() <= 1e-14


def _models():
    return {
        "lqr": (CL.lqr_workload(1000, 4, 0.3), SL.lqrn_host, CL.lqr_covar, CL.LQR_PAIRS),
        "lqr_vi": (CL.lqr_vi_workload(1000), SL.lqrn_host, CL.lqr_covar, CL.LQR_PAIRS),
        "lqr3_l2": (CL.lqr3_workload(1000), SL.lqrn_host, CL.lqr3_covar, CL.LQR3_PAIRS),
        "lqr3_small": (CL.lqr3_workload(1000, ngrid=(9, 12, 7), ranks=(1, 4, 4, 1)), SL.lqrn_host, CL.lqr3_covar, CL.LQR3_PAIRS),
        "heston": (CL.heston_workload(1000), CL.heston_host, CL.heston_covar, CL.HESTON_PAIRS),
        "known": (CL.known_workload(1000), CL.known_host, CL.known_covar, CL.KNOWN_PAIRS),
    }


def _sample_nodes(w, rng, n=60):
    """interior nodes and nodes on the reflecting / periodic ends"""
    ix = np.stack([rng.integers(0, w.ngrid[m], size=n) for m in range(w.dx)], axis=-1)
    for m in range(w.dx):
        if w.bc[m] != wl.BC_ABSORB:
            ix[m::7, m] = 0
            ix[(m + 3)::7, m] = w.ngrid[m] - 1
        else:
            ix[:, m] = np.clip(ix[:, m], 1, w.ngrid[m] - 2)
    return ix


@pytest.mark.parametrize("model", ["lqr", "lqr_vi", "lqr3_l2", "lqr3_small", "heston", "known"])
def test_chain_rows_sum_to_one_are_non_negative_and_have_the_right_moments(model):
    w, host, covar, pairs = _models()[model]
    rng = np.random.default_rng(5)
    xg = [np.asarray(g) for g in w.xgrid()]
    hs = np.array([g[1] - g[0] for g in xg])
    h2, _ = BR.mca_constants(w)
    C = np.asarray(w.cands, dtype=np.float64)
    for ix in _sample_nodes(w, rng):
        x = np.array([xg[m][ix[m]] for m in range(w.dx)])
        u = C[rng.integers(0, len(C))]
        rows, Q = CL.chain_rows(w, host, covar, pairs, x, ix, u)
        p = {k: v / Q for k, v in rows.items()}
        assert abs(sum(p.values()) - 1.0) <= 1e-13
        assert min(rows.values()) >= 0.0, (model, ix, rows)
        if np.any((ix == 0) | (ix == np.array(w.ngrid) - 1)):
            continue  # the moments are those of the diffusion where every neighbour is one node away
        dt = h2 / Q
        b, s, _ = host(w.params, x[None], u[None])
        a = covar(w.params, x[None])[0]
        dx = {k: (np.array(k) - ix) * hs for k in p}
        m1 = sum(pk * dx[k] for k, pk in p.items())
        m2 = sum(pk * np.outer(dx[k], dx[k]) for k, pk in p.items())
        np.testing.assert_allclose(m1, b[0] * dt, rtol=0, atol=1e-13 * max(1.0, np.abs(b).max()))
        cov = np.diag(s[0] ** 2)
        for q, (i, j) in enumerate(pairs):
            cov[i, j] = cov[j, i] = a[q]
        # the upwind chain's second moment carries the drift's h |b| dt on the diagonal: compare the off-diagonal entries
        # with a dt exactly and the diagonal up to that term
        off = ~np.eye(w.dx, dtype=bool)
        np.testing.assert_allclose(m2[off], (cov * dt)[off], rtol=0, atol=1e-13)
        np.testing.assert_allclose(np.diag(m2), np.diag(cov) * dt + hs * np.abs(b[0]) * dt, rtol=0, atol=1e-13)


def test_the_dominance_model_has_negative_probabilities_exactly_where_the_test_says():
    w = CL.lqr_workload(1000, 4, 0.3, CL.LQR_DOM_PRM)
    rng = np.random.default_rng(6)
    xg = [np.asarray(g) for g in w.xgrid()]
    C = np.asarray(w.cands, dtype=np.float64)
    seen = set()
    for ix in _sample_nodes(w, rng, 200):
        x = np.array([xg[m][ix[m]] for m in range(w.dx)])
        r, _ = CL.pair_rates(w, CL.lqr_covar, CL.LQR_PAIRS, x[None])
        bad = bool(CL.dominance(w, SL.lqrn_host, CL.LQR_PAIRS, x[None], r)[0])
        # at zero drift the axis rates are the diffusion's alone: the sign of the smallest is the dominance test's verdict
        rows, _ = CL.chain_rows(w, SL.lqrn_host, CL.lqr_covar, CL.LQR_PAIRS, x, ix, np.zeros(2))
        if np.all((ix > 0) & (ix < np.array(w.ngrid) - 1)):
            assert (min(rows.values()) < 0.0) == bad, (ix, rows)
            seen.add(bad)
    assert seen == {True, False}


def _index_case(name):
    """(w, host, covar, pairs, k0, delta) of the workloads whose indices the GPU tests compare"""
    if name == "lqr":
        return CL.lqr_workload(1000, 4, 0.3), CL.lqr_covar, CL.LQR_PAIRS, 0.01
    if name == "lqr_beta0":
        return CL.lqr_workload(1000, 8, 0.0), CL.lqr_covar, CL.LQR_PAIRS, 0.01
    if name == "lqr3_l2":
        return CL.lqr3_workload(1000), CL.lqr3_covar, CL.LQR3_PAIRS, 0.004
    return CL.lqr3_workload(1000, ngrid=(9, 12, 7), ranks=(1, 4, 4, 1)), CL.lqr3_covar, CL.LQR3_PAIRS, 0.004


@pytest.mark.parametrize("name", ["lqr", "lqr_beta0", "lqr3_l2", "lqr3_small"])
@pytest.mark.parametrize("horizon", [False, True], ids=["infinite", "horizon"])
def test_precondition_the_references_decisions_are_clear(name, horizon):
    """at least 99.9 % of the live nodes have a margin above 1e-9 between the best and the second-best candidate"""
    w, covar, pairs, delta = _index_case(name)
    cores = wl.synth_cores(w)
    V = CL.full_values(w, cores)
    ix, x, S = _dense_stencils(w, V)
    h2, t = BR.mca_constants(w)
    C = np.asarray(w.cands, dtype=np.float64)
    live = np.ones(len(ix), dtype=bool)
    for m in range(w.dx):
        if w.bc[m] == wl.BC_ABSORB:
            live &= (ix[:, m] > 0) & (ix[:, m] < w.ngrid[m] - 1)
    _, inobs, _, _ = JL.target_kinds(dataclasses.replace(w, bc=tuple(0 if b == 2 else b for b in w.bc)), x)
    live &= ~inobs
    cq, cpv, r = CL.corr_terms(w, covar, pairs, V, ix, x, S)
    assert not CL.dominance(w, SL.lqrn_host, pairs, x, r)[live].any(), "the well-posed models satisfy dominance"
    vals, _, _ = BR.candidate_values(SL.lqrn_host, w.params, x[live], S[live], C, h2, t, w.discount, cq[live], cpv[live], delta if horizon else None)
    _, _, mg = BR.backup(vals)
    assert (mg <= 1e-9).mean() <= 0.001, (name, (mg <= 1e-9).mean())
