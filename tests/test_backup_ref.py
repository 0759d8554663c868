"""The shared numpy restatement of the Bellman backup (tests/backup_ref.py) held to the rule in words: one per-node,
per-candidate Python loop (backup_ref.loop_backup), in each of the 18 forms without a game that form_offered accepts for the
per-wave kernel.  No GPU is needed.

- Every form: values to a relative 1e-13, indices and flags exactly, on about 100 nodes with 2-D stencils and the 25-candidate
  LQR list; one candidate is stationary at some nodes, all of them at a few; exact ties are planted between two candidates (the
  first wins), between psi and the best candidate and between an intervention and the best candidate (the candidate wins), and
  between two interventions (the lower m wins).
- psi together with c is refused.
- No RuntimeWarning leaves backup at a node with fewer than two finite actions."""
import warnings

import numpy as np
import pytest

import backup_ref as BR
import stop_lib as SL
from test_form_rule import PER_WAVE, C as CORR, G as GAME, H as HORIZON, I as IMPULSE, J as JUMP, S as STOP

FORMS = [m for m in PER_WAVE if not m & GAME]
H2, T = 0.04, [0.2, 1.0, 0.2, 1.0]  # h = 0.2 in both dimensions
PRM = (0.3, 1.0, 1.0)
P, M = 104, 3
# node ranges: the planted ties; then the nodes where u = 0 is stationary and those where every candidate is
TIES = {"cand": slice(0, 12), "psi": slice(12, 24), "imp_cand": slice(24, 36), "imp_imp": slice(36, 48)}
ONE_STATIONARY, ALL_STATIONARY = slice(48, 60), slice(60, 66)


def _host(prm, x, u):
    """the LQR x_i' = u_i without diffusion where x0 > 0.5 (the candidate u = 0 is stationary there) and without drift as well
    where x1 > 1 (every candidate is)"""
    b = u * np.where(x[..., 1:2] > 1.0, 0.0, 1.0) + 0.0 * x
    s = np.where(x[..., 0:1] > 0.5, 0.0, prm[0]) + 0.0 * b
    return b, s, prm[1] * (x ** 2).sum(-1) + prm[2] * (u ** 2).sum(-1)


def _case(form, beta):
    """(x, V, C, q0, pv0, psi, c, delta) of one form; the node ranges of the planted ties are TIES"""
    rng = np.random.default_rng(100 + form)
    x = rng.uniform(-2.0, 2.0, size=(P, 2))
    V = rng.uniform(0.0, 3.0, size=(P, 5))
    # equal neighbours per dimension, those of dimension 0 far cheaper: the candidates (+a, 0) and (-a, 0) tie for the minimum
    V[TIES["cand"]] = np.stack([rng.uniform(0.0, 0.3, size=12)] * 2 + [rng.uniform(2.5, 3.0, size=12)] * 3, axis=-1)
    x[:48] = np.stack([-np.abs(x[:48, 0]), np.minimum(x[:48, 1], 0.9)], axis=-1)  # the nodes of the ties have diffusion and drift
    x[ONE_STATIONARY] = rng.uniform([0.6, -2.0], [2.0, 0.9], size=(12, 2))
    x[ALL_STATIONARY] = rng.uniform([0.6, 1.1], [2.0, 2.0], size=(6, 2))
    C = SL.lqr_cands()
    q0 = pv0 = None
    if form & (JUMP | CORR):  # stand-ins for h2 lambda, h2 lambda J and the pairs' correction; zero at a third of the nodes
        on = rng.uniform(size=P) > 0.33
        on[48:66] = False
        q0, pv0 = np.zeros(P), np.zeros(P)
        if form & JUMP:
            lam = np.where(on, rng.uniform(0.0, 0.1, size=P), 0.0)
            q0, pv0 = q0 + lam, pv0 + lam * rng.uniform(0.0, 3.0, size=P)
        if form & CORR:
            q0, pv0 = q0 + np.where(on, rng.uniform(-0.02, 0.0, size=P), 0.0), pv0 + np.where(on, rng.uniform(-0.05, 0.05, size=P), 0.0)
    delta = 0.15 if form & HORIZON else None  # Q delta / h^2 > 1 for the faster candidates
    vals, _, _ = BR.candidate_values(_host, PRM, x, V, C, H2, T, beta, q0, pv0, delta)
    best = np.nanmin(np.where(np.isnan(vals).all(axis=1, keepdims=True), 0.0, vals), axis=1)
    psi = c = None
    if form & STOP:
        psi = np.median(best) + 0.3 * (x ** 2).sum(-1) - 0.4
        psi[TIES["psi"]] = best[TIES["psi"]]
    if form & IMPULSE:
        c = np.median(best) + rng.uniform(-0.5, 1.0, size=(P, M))
        c[rng.uniform(size=c.shape) < 0.3] = np.inf
        c[TIES["imp_cand"]] = np.inf
        c[TIES["imp_cand"], 1] = best[TIES["imp_cand"]]
        c[TIES["imp_imp"], 0] = np.inf
        c[TIES["imp_imp"], 1] = c[TIES["imp_imp"], 2] = best[TIES["imp_imp"]] - 1.0
    return x, V, C, q0, pv0, psi, c, delta


@pytest.mark.parametrize("beta", [0.3, 0.0])
@pytest.mark.parametrize("form", FORMS)
def test_restatement_equals_the_rule_in_words(form, beta):
    x, V, C, q0, pv0, psi, c, delta = _case(form, beta)
    nc = len(C)
    vals, stat, cfl = BR.candidate_values(_host, PRM, x, V, C, H2, T, beta, q0, pv0, delta)
    out, ui, _ = BR.backup(vals, psi, c)
    l_out, l_ui, l_stat, l_cfl = BR.loop_backup(_host, PRM, x, V, C, H2, T, beta, q0, pv0, psi, c, delta)
    np.testing.assert_array_equal(ui, l_ui)
    np.testing.assert_array_equal(stat, l_stat)
    np.testing.assert_array_equal(cfl.any(axis=1), l_cfl)
    np.testing.assert_allclose(out, l_out, rtol=1e-13, atol=0.0)
    # the case holds what it is meant to hold
    skipped = np.isnan(vals)
    if form & HORIZON:
        assert not skipped.any() and not stat.any() and cfl.any() and not cfl.all()
    else:
        assert not cfl.any()
        assert (skipped[ONE_STATIONARY].sum(axis=1) == 1).all() and skipped[ALL_STATIONARY].all(), "one candidate skipped; all of them"
        none = skipped.all(axis=1) & (psi is None) & (True if c is None else ~np.isfinite(c).any(axis=1))
        assert (ui[none] == -1).all() and (out[none] == 0.0).all()
    filled = np.where(skipped, np.inf, vals)
    tie = TIES["cand"]
    assert ((filled[tie] == filled[tie].min(axis=1, keepdims=True)).sum(axis=1) >= 2).all(), "two candidates tie for the minimum"
    first = np.array([int(np.flatnonzero(r == r.min())[0]) for r in filled[tie]])
    if psi is None and c is None:
        np.testing.assert_array_equal(ui[tie], first)
    if psi is not None:
        assert (ui == nc).any() and (ui < nc).any(), "both decisions occur"
        assert (ui[TIES["psi"]] < nc).all() and (out[TIES["psi"]] == psi[TIES["psi"]]).all(), "psi ties with the best candidate: the candidate wins"
    if c is not None:
        assert (ui > nc).any() and (ui < nc).any()
        a, b = TIES["imp_cand"], TIES["imp_imp"]
        assert (ui[a] < nc).all() and (out[a] == c[a, 1]).all(), "an intervention ties with the best candidate: the candidate wins"
        assert (ui[b] == nc + 1 + 1).all(), "interventions 1 and 2 tie: the lower m wins"


def test_stop_and_impulse_together_are_refused():
    vals = np.ones((3, 4))
    with pytest.raises(ValueError):
        BR.backup(vals, psi=np.ones(3), c=np.ones((3, 2)))
    with pytest.raises(ValueError):
        BR.backup(vals, psi=np.ones(3), c=np.ones((3, 2)), forced=np.zeros(3, dtype=int))


def test_no_warning_with_fewer_than_two_finite_actions():
    vals = np.array([[np.nan, np.nan, np.nan], [np.nan, 2.0, np.nan], [1.0, 2.0, 3.0]])
    inf = np.full((3, 2), np.inf)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for psi, c in ((None, None), (np.full(3, np.inf), None), (None, inf)):
            out, ui, mg = BR.backup(vals, psi, c)
            assert ui.tolist() == [-1, 1, 0] and out.tolist() == [0.0, 2.0, 1.0]
            assert np.isinf(mg[:2]).all() and mg[2] == 1.0
        out, ui, mg = BR.backup(vals[:2], np.array([5.0, 5.0]))
        assert ui.tolist() == [3, 1] and out.tolist() == [5.0, 2.0] and np.isinf(mg[0]) and mg[1] == 1.5
        assert np.isinf(BR.stop_margin(vals, np.full(3, 5.0))[0])
