"""tests/rollout_ref.py held to what the GPU comparison (tests/test_gpu_rollout_forms.py) relies on, on the CPU alone.

- The vectorised float64 stencil equals offgrid_ref.OffgridRef (longdouble, one point at a time) to 1e-12 of the |G| product on
  interior, face, seam, reflecting-face and obstacle points, multilinear and CONSTELM.
- Every row of ROWS, on the reference's own closed loop: check accepts the run with zero mismatches; at most 2.5 % of the
  decisions are unsure (half of the device test's cap, since device and reference visit states that differ by rounding); every
  action kind of the form occurs at least 3 times (stop at step 0 and later, every intervention, every jump mark, 3 distinct
  candidates); exits occur through an absorbing face, from a start inside the obstacle, by a jump, and by an intervention where
  an intervention can leave cheaply (the 2-D impulse LQR, whose boundary is cheap; the 3-D one moves along the periodic and the
  reflecting dimension only); at least half of the lanes run at mid-run; in horizon rows the decisions under stage k differ from
  those under k + 1; in jump rows the decisions without the jump term differ on at least 1 % of the steps -- except in the
  form horizon + jump without stop, where the jump term is the same constant in every candidate's value and no decision can
  depend on it (rollout_ref.has_feature states the algebra); in wrap rows xin != x occurs on live lanes.
- Every planted fault (rollout_ref.FAULTS) gives a run that check rejects, on every row that has the fault's feature.  The
  '<=' fault differs from '<' on exact ties only, and check accepts either action of a tie by its own rule (margin 0 <=
  MARGIN_TOL): it is held on the rows' contexts with psi tied to the scan's result on every other lane, by the strict check
  that a run of the reference's own arithmetic allows (every decision must be the reference's)."""
import dataclasses

import numpy as np
import pytest

import offgrid_ref as OR
import rollout_ref as RR
from c3sc_amd import workloads as wl
from rollout_ref import MARGIN_TOL

ROWS = {r.id: r for r in RR.ROWS}
assert len(ROWS) == len(RR.ROWS), "row ids are unique"
MAX_UNSURE = 0.025
_cache = {}


def _row(rid):
    if rid not in _cache:
        row = ROWS[rid]
        ctx = RR.make_ctx(row)
        run, log = RR.rollout(row.form, ctx)
        _cache[rid] = (row, ctx, run, log)
    return _cache[rid]


# ---------------------------------------------------------------------------------------------------- the stencil
def _sample(w, rng):
    lo, hi = np.array(w.lb), np.array(w.ub)
    pts = list(lo + (hi - lo) * rng.uniform(-0.1, 1.1, (40, w.dx)))
    xg = w.xgrid()
    for m in range(w.dx):
        g = xg[m]
        h = g[1] - g[0]
        for v in (g[0], g[-1], g[0] + h, g[-1] - h, g[3], g[0] - 0.3 * h, g[-1] + 0.3 * h, g[0] + 0.4 * h, g[-1] - 0.4 * h, g[-1] + 1.7):
            for e in (v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)):
                p = lo + (hi - lo) * rng.uniform(0.05, 0.95, w.dx)
                p[m] = e
                pts.append(p)
    for c, wd in w.obstacles:
        c, wd = np.array(c), np.array(wd)
        pts += list(c + wd * rng.uniform(-0.5, 0.5, (6, w.dx)))
        pts += [c - wd / 2.0, c + wd / 2.0, c + wd * 0.50001]
    return np.ascontiguousarray(pts)


@pytest.mark.parametrize("constelm", [False, True], ids=["linelm", "constelm"])
@pytest.mark.parametrize("rid", ["lqr_jd-c12-seed", "lqr3_jd-jump-c12-seed", "lqgame-game-c4-seed-minmax"])
def test_vectorised_stencil_equals_offgrid_ref(rid, constelm):
    row = ROWS[rid]
    ctx = RR.make_ctx(row)
    w = dataclasses.replace(ctx.w, ranks=ctx.ranks[0])
    ref = OR.OffgridRef(w, ctx.cores[0])
    x = _sample(w, np.random.default_rng(3))
    V, ab = RR.stencil(w, ctx.trains[0], x, constelm)
    worst = 0.0
    for i, p in enumerate(x):
        rV, rA, flag = ref.stencil(p, constelm)
        assert flag == ab[i]
        worst = max(worst, float(OR.rel_err(V[i], rV, rA).max()))
    assert (ab == -1).any() and (ab == 0).any()
    assert worst <= 1e-12, worst


# ---------------------------------------------------------------------------------------------------- the rows
@pytest.mark.parametrize("rid", list(ROWS))
def test_row_preconditions(rid):
    row, ctx, run, log = _row(rid)
    form, nc = row.form, len(ctx.C)
    counts, bad, err = RR.check(form, ctx, run)
    assert not bad, bad
    assert err["state"] == 0.0 and err["cost"] == 0.0 and err["vend"] == 0.0, err
    c = log.counts()
    assert {q: counts[q] for q in counts if q != "unsure"} == {q: c[q] for q in c if q != "unsure"}
    assert c["unsure"] <= MAX_UNSURE * c["checked"], (c["unsure"], c["checked"])
    RR.assert_occurrences(row, c)
    assert c["exit_obstacle0"] >= 1 and c["exit_face"] >= 1
    if ctx.wrap:
        assert c["wrapped"] >= 3
    if "horizon" in form:
        _, other = RR.rollout(form, ctx, fault="stage_k")
        assert (other.act != log.act).any(), "the stage index decides nothing in this row"
    if RR.has_feature(form, "jump_decides"):
        differ = live = 0
        alive = np.ones(row.n, dtype=bool)
        for k in range(row.N):
            a = RR.step(form, ctx, k, run["traj"][:, k], alive)
            b = RR.step(form, ctx, k, run["traj"][:, k], alive, fault="nojump")
            on = alive & ~a.gone
            differ += int((a.ui != b.ui)[on].sum())
            live += int(on.sum())
            alive = a.alive
        assert differ >= 0.01 * live, (differ, live)


# ---------------------------------------------------------------------------------------------------- planted faults
FAULT_CASES = [(rid, f) for rid, r in ROWS.items() for f, feat in RR.FAULTS.items() if RR.has_feature(r.form, feat, r.spec)]


@pytest.mark.parametrize("rid,fault", FAULT_CASES, ids=[f"{r}-{f}" for r, f in FAULT_CASES])
def test_planted_fault_is_rejected(rid, fault):
    row, ctx, _, _ = _row(rid)
    if fault.endswith("_at_x"):
        assert ctx.wrap
    strict = False
    if fault == "le":  # ties only: see the module docstring
        ctx = dataclasses.replace(ctx, tie_psi=True)
        strict = True
        good, _ = RR.rollout(row.form, ctx)
        assert not RR.check(row.form, ctx, good, strict=True)[1]
    run, _ = RR.rollout(row.form, ctx, fault=fault)
    _, bad, _ = RR.check(row.form, ctx, run, strict=strict)
    assert bad, f"{fault} went unnoticed on {rid}"


def test_margin_rule_accepts_either_action_of_a_tie_and_nothing_else():
    """below MARGIN_TOL the run's action is accepted if it is within the margin, the replay goes on with it and the step counts
    as unsure; an action outside the margin is rejected there as everywhere"""
    row, ctx, _, _ = _row("lqr_jd-stop-c4-zero")
    ctx = dataclasses.replace(ctx, tie_psi=True)
    for fault in (None, "le"):  # '<' keeps the candidate on a tie, '<=' stops: both runs are accepted
        run, _ = RR.rollout(row.form, ctx, fault=fault)
        counts, bad, _ = RR.check(row.form, ctx, run)
        assert not bad, bad
        assert counts["unsure"] >= 100
    run, _ = RR.rollout(row.form, ctx)
    lane = int(np.nonzero((run["exit"] == -1) & (np.arange(row.n) % 2 == 1))[0][0])  # no tie on odd lanes
    run["u"][lane, 0] = ctx.C[(int(np.nonzero((ctx.C == run["u"][lane, 0]).all(axis=1))[0][0]) + 7) % len(ctx.C)]
    assert RR.check(row.form, ctx, run)[1]
    assert MARGIN_TOL == 1e-9


def test_table_covers_every_form_at_both_classes():
    forms = {}
    for r in RR.ROWS:
        forms.setdefault(r.form, set()).add(r.rp)
    assert len(forms) == 11
    for f, classes in forms.items():
        assert classes == ({4} if "game" in f else {4, 12}), (sorted(f), classes)
    for f in forms:
        for noise in ("seed", "zero"):
            assert any(r.form == f and r.noise == noise for r in RR.ROWS), (sorted(f), noise)
    assert len(RR.CUT_ROWS) == 3
    assert all(r.n == RR.NLANES and r.n > 256 and r.n % 256 for r in RR.ROWS), "a second workgroup with a repeated tail"
    assert any(len(RR.make_ctx(r).C) > 64 for r in RR.ROWS if len(r.bonds) == 4), "the candidate table is refilled past 64 rows"
    assert wl.BC_PERIODIC in RR.make_ctx(RR.ROWS[0]).w.bc
