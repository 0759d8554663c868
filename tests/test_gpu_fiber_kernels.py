"""Every registered Bellman fiber kernel against the oracle, by name: parametrised over tests/fiber_kernel_cases.py (one row per
family, model or D and padded rank; tests/test_fiber_kernel_cases.py holds that table to the registry and to the selection logic).
Each row runs on two data classes, wl.synth_cores and the signed class synth_cores - 0.35, with bond ranks below the padded rank,
and eng.last_kernel() must name the row's kernel for every k.

The reference is the oracle throughout: its Bellman backup, its stencil, and the per-candidate table Q[fiber, node, c] built from
one oracle run per candidate (fiber_kernel_cases.q_table), which makes the FORCED (policy) forms checkable by a gather and the
argmin checkable without ties.  Flags are bit-exact; values to REL_TOL = 1e-12 of the scale fiber_kernel_cases derives; no node is
left out of a comparison.

The discount is a run-time argument and node_backup picks one of several compiled scans per node by it, so every list row also
runs at six discounts computed from the oracle's own dt and h2 / Q0 of its batches (fiber_kernel_cases.regime_betas: zero, tiny,
small, libm, mixed, vote -- the fraction scan, exp_tiny, exp_small, libm exp, a batch that straddles 2^-7, exp_discount's
polynomial arm), the table rows at three and the box rows at two; the pair and duo rows with 4, 5 and 7 candidates (remainders
against the three candidates per trip of the pair kernel's fraction scan); the LqgNd and Chain rows without diffusion through the
nodes where u = 0 is stationary, against the minimum over the valid candidates built from the oracle's pieces.  Same bar.

Every test prints its row's worst relative error (pytest -s); the worst per family and data class, and the file's run time, are
recorded in DESIGN.md (4.8, coverage of the Bellman fiber kernels)."""
import dataclasses

import numpy as np
import pytest

import fiber_kernel_cases as T

pytestmark = pytest.mark.gpu

DATA = [False, True]
DATA_IDS = ["synth", "signed"]


def _engine(case, w, cs):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    eng.set_variant(case.variant)  # before the upload: the padded rank follows the variant
    eng.configure(w, cs)
    return eng


def _rel(got, ref, scale):
    return float(np.abs(got - ref).max() / scale)


def _rows(*families):
    return [c for c in T.CASES if c.family in families]


def _report(case, signed, worst, label=""):
    print(f"{T.case_id(case)}{' ' + label if label else ''} {'signed' if signed else 'synth'}: worst relative error {worst:.2e}")


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("case", _rows(*T.LIST_FAMILIES), ids=T.case_id)
def test_list_kernels_vs_oracle(oracle, case, signed):
    """fpw / fpp / fq / fqd rows.  Minimising form: flags bit-exact, values against Q.min, an argmin other than the oracle's only
    where Q[node, ui] is within the tolerance of the minimum, status 0 and the row's kernel name for every k.  FORCED form on the
    same rows: a seeded random policy through policy_fibers_host against the gather from Q, equal flags, the same kernel name,
    identical bits on a repeat."""
    _check_list(oracle, case, signed, T.workload(case))


def _check_list(oracle, case, signed, w, label=""):
    """the checks of test_list_kernels_vs_oracle on the workload w (the row's own, or the row's at another discount or with
    another candidate list)"""
    cs = T.cores(case, w, signed)
    P = oracle.Problem(w, cs)
    eng = _engine(case, w, cs)
    rng = np.random.default_rng(20 + case.rp)
    worst = 0.0
    for k in case.ks:
        idx = T.fibers(w, k, case.nfib)
        ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
        Q, _ = T.q_table(oracle, w, cs, k, idx)
        qmin = Q.min(axis=-1)
        scale = T.scale_of(oracle, w, cs, k, idx, ref, signed)
        tol = T.REL_TOL * scale
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        assert eng.status() == 0
        assert eng.last_kernel() == case.kernels[k], (k, eng.last_kernel())
        np.testing.assert_array_equal(ab, ref_ab)
        live = ref_ab == 0
        assert live.any()
        err = _rel(out, qmin, scale)
        worst = max(worst, err)
        assert err <= T.REL_TOL, f"{T.case_id(case)} k={k}: min form, relative error {err:.3e} (scale {scale:.3e})"
        assert (ui[live] >= 0).all() and (ui[live] < w.ncand).all()
        at = np.take_along_axis(Q, np.clip(ui, 0, w.ncand - 1)[..., None], axis=-1)[..., 0]
        assert (at[live] - qmin[live]).max() <= tol, f"{T.case_id(case)} k={k}: an argmin that does not attain the minimum"
        # FORCED
        pol = rng.integers(0, w.ncand, size=out.shape).astype(np.int32)
        want = np.take_along_axis(Q, pol[..., None], axis=-1)[..., 0]
        got, ab2 = eng.policy_fibers_host(k, idx, pol)
        assert eng.status() == 0
        assert eng.last_kernel() == case.kernels[k], (k, eng.last_kernel())
        np.testing.assert_array_equal(ab2, ref_ab)
        fscale = max(scale, float(np.abs(want).max()))
        err = _rel(got, want, fscale)
        worst = max(worst, err)
        assert err <= T.REL_TOL, f"{T.case_id(case)} k={k}: FORCED form, relative error {err:.3e} (scale {fscale:.3e})"
        again, ab3 = eng.policy_fibers_host(k, idx, pol)
        assert np.array_equal(again, got) and np.array_equal(ab3, ab2)
    eng.close()
    _report(case, signed, worst, label)


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("case", _rows("table"), ids=T.case_id)
def test_table_kernels_vs_oracle(oracle, case, signed):
    """TableModel<D> at every registered (D, RP, NPL): (drift, sigma, stage) tables and costs from the oracle's model callbacks; the
    minimising call against Q.min and the policy call (BellmanEngine.policy_fibers_tables_host) against the gather from Q"""
    _check_table(oracle, case, signed, T.workload(case))


def _check_table(oracle, case, signed, w, label=""):
    cs = T.cores(case, w, signed)
    P = oracle.Problem(w, cs)
    eng = _engine(case, w, cs)
    rng = np.random.default_rng(30 + case.rp)
    worst = 0.0
    for k in case.ks:
        idx = T.fibers(w, k, case.nfib)
        tables, costs2 = T.model_tables(oracle, w, k, idx)
        ref, _, ref_ab = P.bellman_fibers(k, idx)
        Q, _ = T.q_table(oracle, w, cs, k, idx)
        qmin = Q.min(axis=-1)
        scale = T.scale_of(oracle, w, cs, k, idx, ref, signed)
        out, ui, ab = eng.bellman_fibers_tables_host(k, idx, tables, costs2)
        assert eng.status() == 0
        assert eng.last_kernel() == case.kernels[k], (k, eng.last_kernel())
        np.testing.assert_array_equal(ab, ref_ab)
        live = ref_ab == 0
        err = _rel(out, qmin, scale)
        worst = max(worst, err)
        assert err <= T.REL_TOL, f"{T.case_id(case)} k={k}: relative error {err:.3e}"
        assert (ui[live] >= 0).all() and (ui[live] < w.ncand).all()
        at = np.take_along_axis(Q, np.clip(ui, 0, w.ncand - 1)[..., None], axis=-1)[..., 0]
        assert (at[live] - qmin[live]).max() <= T.REL_TOL * scale
        pol = rng.integers(0, w.ncand, size=out.shape).astype(np.int32)
        want = np.take_along_axis(Q, pol[..., None], axis=-1)[..., 0]
        got, ab2 = eng.policy_fibers_tables_host(k, idx, tables, costs2, pol)
        assert eng.status() == 0
        assert eng.last_kernel() == case.kernels[k], (k, eng.last_kernel())
        np.testing.assert_array_equal(ab2, ref_ab)
        fscale = max(scale, float(np.abs(want).max()))
        err = _rel(got, want, fscale)
        worst = max(worst, err)
        assert err <= T.REL_TOL, f"{T.case_id(case)} k={k}: policy call, relative error {err:.3e}"
        again, _ = eng.policy_fibers_tables_host(k, idx, tables, costs2, pol)
        assert np.array_equal(again, got)
    eng.close()
    _report(case, signed, worst, label)


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("case", _rows("stencil"), ids=T.case_id)
def test_stencil_kernels_vs_oracle(oracle, case, signed):
    """the on-grid stencil kernels at every registered (D, RP, NPL): stencil_fibers_host against P.stencil_fibers, flags exact"""
    w = T.workload(case)
    cs = T.cores(case, w, signed)
    P = oracle.Problem(w, cs)
    eng = _engine(case, w, cs)
    worst = 0.0
    for k in case.ks:
        idx = T.fibers(w, k, case.nfib)
        ref, ref_ab = P.stencil_fibers(k, idx)
        out, ab = eng.stencil_fibers_host(k, idx)
        assert eng.status() == 0
        assert eng.last_kernel() == case.kernels[k], (k, eng.last_kernel())
        np.testing.assert_array_equal(ab, ref_ab)
        scale = T.scale_of(oracle, w, cs, k, idx, ref, signed)
        err = _rel(out, ref, scale)
        worst = max(worst, err)
        assert err <= T.REL_TOL, f"{T.case_id(case)} k={k}: relative error {err:.3e} (scale {scale:.3e})"
    _report(case, signed, worst)


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("case", _rows("fpw_box"), ids=T.case_id)
def test_box_kernels_vs_oracle(oracle, case, signed):
    """the box minimiser (cmode 1) of every C3SC_REG_FPW_BOX registration, on the box of the model's example and a small grid:
    the result on live nodes does not exceed the oracle's scan over that same grid of controls by more than the tolerance; the
    returned controls, evaluated as an explicit candidate list through the list kernel's FORCED form on the same cores (held to
    the oracle by test_list_kernels_vs_oracle), reproduce the box output; absorbed nodes equal the oracle's"""
    _check_box(oracle, case, signed, T.workload(case))


def _check_box(oracle, case, signed, w, label=""):
    from c3sc_amd.engine import BellmanEngine

    cs = T.cores(case, w, signed)
    lb, ub, G = np.array(case.opts["lb"]), np.array(case.opts["ub"]), case.opts["grid"]
    eng = _engine(case, w, cs)
    eng.set_control_box(lb, ub, grid=G, polish=2)
    wscan = T.with_cands(w, T.box_grid(lb, ub, G))
    Pscan = oracle.Problem(wscan, cs)
    worst = 0.0
    for k in case.ks:
        idx = T.fibers(w, k, case.nfib)
        out, uo, ab = eng.bellman_fibers_box_host(k, idx)
        assert eng.status() == 0
        assert eng.last_kernel() == case.kernels[k], (k, eng.last_kernel())
        scan, _, ref_ab = Pscan.bellman_fibers(k, idx)
        np.testing.assert_array_equal(ab, ref_ab)
        live = ref_ab == 0
        assert live.any()
        scale = T.scale_of(oracle, wscan, cs, k, idx, scan, signed)
        tol = T.REL_TOL * scale
        assert np.array_equal(out[~live], scan[~live])  # boundary / obstacle costs
        over = float((out[live] - scan[live]).max())
        assert over <= tol, f"{T.case_id(case)} k={k}: {over:.3e} above the scan of the grid (scale {scale:.3e})"
        assert (uo[live] >= lb - 1e-15).all() and (uo[live] <= ub + 1e-15).all()
        # the returned controls as an explicit candidate list, one candidate per node, through the list kernel's FORCED form
        cands = np.where(live[..., None], uo, lb).reshape(-1, w.du)
        wl2 = T.with_cands(w, cands)
        eng2 = BellmanEngine(0)
        eng2.set_variant(case.variant)
        eng2.configure(wl2, cs)
        pol = np.arange(cands.shape[0], dtype=np.int32).reshape(out.shape)
        back, ab2 = eng2.policy_fibers_host(k, idx, pol)
        assert eng2.status() == 0
        assert eng2.last_kernel() == case.kernels[k], (k, eng2.last_kernel())
        np.testing.assert_array_equal(ab2, ref_ab)
        err = _rel(back, out, max(scale, float(np.abs(out).max())))
        worst = max(worst, err)
        assert err <= T.REL_TOL, f"{T.case_id(case)} k={k}: list kernel on the returned controls, relative error {err:.3e}"
        eng2.close()
    eng.close()
    _report(case, signed, worst, label)


# ------------------------------------------------------------------------------------------------------- discount regimes
def _at(oracle, case, regime, w=None):
    """the row's workload at the regime's discount (fiber_kernel_cases.regime_betas: from the oracle's dt and r0 of the row's own
    batches, over all of its k)"""
    w = w or T.workload(case)
    return dataclasses.replace(w, discount=T.regime_betas(oracle, case, w)[regime])


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("case", _rows(*T.LIST_FAMILIES), ids=T.case_id)
@pytest.mark.parametrize("regime", T.REGIMES)
def test_list_kernels_in_every_regime(oracle, case, signed, regime):
    """every check of test_list_kernels_vs_oracle with the discount of each regime, q_table built with the same discount: the
    fraction scan, exp_tiny, exp_small, libm exp, the straddling batch and exp_discount's polynomial arm
    (tests/test_fiber_kernel_cases.py holds regime -> body on the CPU)"""
    _check_list(oracle, case, signed, _at(oracle, case, regime), regime)


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("case", _rows("table"), ids=T.case_id)
@pytest.mark.parametrize("regime", ("zero", "libm", "mixed"))
def test_table_kernels_in_every_regime(oracle, case, signed, regime):
    """node_backup_tables has one discounted form (libm exp) and the undiscounted one"""
    _check_table(oracle, case, signed, _at(oracle, case, regime), regime)


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("case", _rows("fpw_box"), ids=T.case_id)
@pytest.mark.parametrize("regime", ("zero", "libm"))
def test_box_kernels_in_every_regime(oracle, case, signed, regime):
    """node_backup_box: the factor is 1 at beta = 0, else exp_discount.  The discount is the one of the row's candidate list, which
    spans the same box"""
    _check_box(oracle, case, signed, _at(oracle, case, regime), regime)


TAIL_ROWS = [(c, r) for c in _rows("fpp") for r in ("zero",)] + [(c, r) for c in _rows("fqd") for r in ("zero", "libm")]


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("ncand", (4, 5, 7))
@pytest.mark.parametrize("case,regime", TAIL_ROWS, ids=lambda v: T.case_id(v) if isinstance(v, tuple) else v)
def test_candidate_count_tails(oracle, case, regime, ncand, signed):
    """candidate counts 4, 5 and 7: remainders 1, 2 and 1 against the pair kernel's three candidates per trip of the fraction
    scan (the tail trip clamps the candidate index), and one list longer than the table's six.  The pair rows undiscounted (the
    discounted pair scan takes one candidate per trip), the duo rows undiscounted and in the libm regime.  A list longer than
    the model's own is spread evenly inside its control range."""
    case = case._replace(opts=dict(case.opts, ncand=ncand, spread=True))
    w = T.workload(case)
    assert w.ncand == ncand and ncand % 3 != 0
    _check_list(oracle, case, signed, _at(oracle, case, regime, w), f"{regime} ncand={ncand}")


# ------------------------------------------------------------------------------------------- the skip-and-flag path
@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("case", T.stationary_cases(), ids=T.case_id)
@pytest.mark.parametrize("regime", T.STATIONARY_REGIMES)
def test_stationary_candidates_are_skipped_and_flagged(oracle, case, signed, regime):
    """LqgNd / Chain without diffusion, u = 0 in the list, fibers through the nodes where it is stationary: the value is the
    minimum over the valid candidates (fiber_kernel_cases.q_pieces: the oracle's pieces, nan where transition_assemble
    returns 1), the argmin is a valid candidate that attains it, C3SC_STATUS_STATIONARY is set; on a batch that avoids those
    nodes the same engine leaves it clear and matches the same reference"""
    w0 = T.stationary_workload(case)
    w = dataclasses.replace(w0, discount=T.regime_betas(oracle, case, w0, T.fibers_through)[regime])
    cs = T.cores(case, w, signed)
    mtype = T.MODEL_OF[case.name]
    eng = _engine(case, w, cs)
    worst = 0.0
    for k in case.ks:
        for fib in (T.fibers_clear, T.fibers_through):
            if fib is T.fibers_clear and not any(m != k for m in T.zero_axes(mtype)):
                continue  # every fiber along k crosses the stationary node (the only coordinate that must vanish varies)
            idx = fib(w, k, case.nfib)
            Q, ref_ab, bad = T.q_pieces(oracle, w, cs, k, idx, mtype)
            assert bad == (fib is T.fibers_through)
            qmin = np.nanmin(Q, axis=-1)
            scale = T.scale_of(oracle, w, cs, k, idx, qmin, signed)
            out, ui, ab = eng.bellman_fibers_host(k, idx)
            st = eng.status()
            assert (st & 1) == int(bad) and (st & ~1) == 0, (k, fib.__name__, st)
            assert eng.last_kernel() == case.kernels[k], (k, eng.last_kernel())
            np.testing.assert_array_equal(ab, ref_ab)
            live = ref_ab == 0
            assert live.any()
            err = _rel(out, qmin, scale)
            worst = max(worst, err)
            assert err <= T.REL_TOL, f"{T.case_id(case)} k={k} {fib.__name__}: relative error {err:.3e} (scale {scale:.3e})"
            assert (ui[live] >= 0).all() and (ui[live] < w.ncand).all()
            at = np.take_along_axis(Q, np.clip(ui, 0, w.ncand - 1)[..., None], axis=-1)[..., 0]
            assert np.isfinite(at[live]).all(), f"{T.case_id(case)} k={k}: an argmin on a stationary candidate"
            assert (at[live] - qmin[live]).max() <= T.REL_TOL * scale
    eng.close()
    _report(case, signed, worst, regime)
