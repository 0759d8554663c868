"""CPU side of the random sweep (tests/random_cases.py, run on a device by tests/test_gpu_random_sweep.py): the generator is
reproducible and stays in its domain, the oracle accepts every committed case, the committed seed lists meet the coverage
conditions and the caps, and the checker accepts the oracle's own outputs and rejects every planted fault.  Nothing here needs
a GPU: kernel names and refusals come from the selection restatement, everything else from the oracle."""
import numpy as np
import pytest

import random_cases as R
from c3sc_amd import workloads as wl


def _cases(family):
    return [R.case(family, s) for s in R.SEEDS[family]]


@pytest.mark.parametrize("family", R.FAMILIES)
def test_generator_is_reproducible_and_the_oracle_accepts_every_case(oracle, family):
    """the same (family, seed) gives equal bytes (problem, candidates, every batch), another seed other bytes; every case lies in
    the domain; the oracle accepts it; orc_q_fibers' table has the oracle's own backup as the first minimum of every row, bit
    for bit, with its flags and its argmin; and at most MAX_UNPINNED of a case's live nodes have no pinned control"""
    seeds = R.SEEDS[family]
    assert list(seeds) == sorted(set(seeds))
    seen = set()
    for s in seeds:
        c = R.case(family, s)
        b = c.tobytes()
        assert b == R.case(family, s).tobytes(), repr(c)
        seen.add(b)
        d = len(c.ngrid)
        assert d == R.dim_of(family) and all(5 <= n <= R.MAXN[family] for n in c.ngrid), repr(c)
        assert d < 6 or sorted(c.ngrid)[-2] <= 12, repr(c)
        assert c.ranks[0] == c.ranks[-1] == 1 and all(1 <= r <= R.MAXR for r in c.ranks), repr(c)
        assert c.F in R.F_VALUES and c.comp in R.COMPOSITIONS and len(c.cands) >= 1
        assert c.cand_kind == "own" or len(c.cands) <= 2 or (c.cands[-1] == c.cands[0]).all()  # the repeated row
        P = R.problem(c)
        for k in range(d):
            r = R.reference(c, k)  # raises Rejected where the oracle refuses
            assert r.idx.shape == (c.F, d) and (r.idx >= 0).all() and (r.idx < np.array(c.ngrid)).all() and (r.idx[:, k] == 0).all()
            assert np.isfinite(r.ref).all() and r.scale > 0.0 and r.status == 0
            if c.comp == "faces":  # a run of at least min(F, 64) consecutive fibers on an absorbing face
                dead = np.zeros(c.F, dtype=bool)
                for m in range(d):
                    if m != k and c.bc[m] == wl.BC_ABSORB:
                        dead |= (r.idx[:, m] == 0) | (r.idx[:, m] == c.ngrid[m] - 1)
                runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], dead.astype(np.int8), [0]]))))[::2]
                assert runs.max() >= min(c.F, 64), (repr(c), k)
            if c.comp == "repeats" and c.F >= 8:
                assert len({tuple(row) for row in r.idx}) <= c.F // 4
            if c.F <= 130:
                ref, ui, ab = P.bellman_fibers(k, r.idx)
                assert np.array_equal(ab, r.ab) and np.array_equal(ref, r.ref) and np.array_equal(ui, r.ui), (repr(c), k)
        share = R.unpinned_share(c)
        assert share <= R.MAX_UNPINNED, (repr(c), share)
    assert len(seen) == len(seeds)


def _tally(family):
    """per coverage item, the number of committed cases that have it; per leg, the cases with a refusal"""
    have, refused = {}, {v: 0 for v in R.legs(family)}
    for c in _cases(family):
        once, fams, names = R.coverage_items(c)
        for i in list(once) + [("family", f) for f in fams] + [("kernel", n) for n in names]:
            have[i] = have.get(i, 0) + 1
        for v in R.refused_legs(c):
            refused[v] += 1
    return have, refused


@pytest.mark.parametrize("family", R.FAMILIES)
def test_seed_lists_meet_the_coverage_conditions(family):
    """with the selection restatement: every kernel family the registry holds for the model (and the stencil kernel of its
    dimension) is launched by at least 5 cases, every registered pair / quad / duo kernel by at least 2 (UNREACHED says which
    cannot be and why, and none of those is launched), every F, composition and kind of candidate list occurs, and where MAXN
    allows a case has N on each side of 64"""
    have, _ = _tally(family)
    want = R.needs(family)
    short = {i: (have.get(i, 0), n) for i, n in want.items() if have.get(i, 0) < n}
    assert not short, short
    assert {f for (kind, f) in want if kind == "F"} == set(R.F_VALUES)
    fams = {f for (kind, f) in want if kind == "family"}
    assert fams == {R.KIND_FAMILY[e.kind] for e in R.entries_of(family)} | {"stencil"} and "per-wave" in fams
    for e in R.entries_of(family):
        if e.variant in (R.PAIR, R.QUAD):
            assert (("kernel", e.name) in want) != (e.name in R.UNREACHED)
            assert e.name not in R.UNREACHED or ("kernel", e.name) not in have
    if R.MAXN[family] > 64:
        assert want[("side", True)] == want[("side", False)] == 1


def test_unreached_names_registered_kernels():
    names = {e.name for f in R.FAMILIES for e in R.entries_of(f)}
    assert set(R.UNREACHED) <= names
    assert all(isinstance(w, str) and w.strip() for w in R.UNREACHED.values())
    assert {f for f in R.FAMILIES if R.MAXN[f] > 64} == {"lqg2d", "dubins3d"}


@pytest.mark.parametrize("family", R.FAMILIES)
def test_refusals_stay_under_the_cap(family):
    """per (model, variant) leg, the cases with a launch that is refused as predicted are at most MAX_REFUSED of the list; a
    model's legs are AUTO, per-wave and the pair / quad variant it has registrations for"""
    _, refused = _tally(family)
    n = len(R.SEEDS[family])
    assert set(refused) == set(R.legs(family)) and {R.AUTO, R.PER_WAVE} <= set(refused)
    for v, m in refused.items():
        assert m <= R.MAX_REFUSED * n, (R.VARIANT_NAME[v], m, n)


# ------------------------------------------------------------------------------------------------------ planted faults
def _site(r, pinned=False):
    """a live node of the reference (pinned: one whose control is compared), or None"""
    at = np.argwhere(r.pinned if pinned else (r.ab == 0))
    return tuple(at[len(at) // 2]) if len(at) else None


def _plant(fault, c, r, name):
    """(outputs, kernel name, status) with the fault planted into the oracle's own outputs, or None where the case has no
    place for it"""
    out, ui, ab = r.ref.copy(), r.ui.copy(), r.ab.copy()
    if fault == "value":
        at = _site(r)
        if at is None:
            return None
        out[at] += 1e-10 * r.scale
    elif fault == "absorbed":
        at = (r.ref.shape[0] // 2, r.ref.shape[1] // 2)
        ab[at] = 1 if ab[at] == 0 else 0
    elif fault == "control":
        at = _site(r, pinned=True)
        if at is None:
            return None
        worse = int(r.Q[at].argmax())
        if r.Q[at][worse] - r.ref[at] <= R.PIN_MARGIN * r.scale:
            return None
        ui[at] = worse
    elif fault == "prefill":
        out[-1, -1] = np.nan
    elif fault == "prefill-index":
        ui[0, 0] = R.PREFILL
    elif fault == "fiber-63":
        if c.F != 65 or np.abs(r.ref[64] - r.ref[63]).max() <= 1e-6 * r.scale:
            return None
        out[64], ui[64], ab[64] = out[63], ui[63], ab[63]
    elif fault == "name":
        return (out, ui, ab), name.replace("K=", "K=1") if "K=" in name else name + "x", 0
    elif fault == "status":
        return (out, ui, ab), name, R.STATUS_STATIONARY
    elif fault == "refusal":
        return R.Refused(R.REFUSALS[2]), None, 0
    else:
        raise KeyError(fault)
    return (out, ui, ab), name, 0


FAULTS = ("value", "absorbed", "control", "prefill", "prefill-index", "fiber-63", "name", "status", "refusal")


@pytest.mark.parametrize("family", R.FAMILIES)
def test_checker_rejects_planted_faults(oracle, family):
    """check() accepts the oracle's own outputs under the predicted kernel name on every committed case, accepts a predicted
    refusal only with its own reason, and rejects every planted fault wherever a case has a place for it -- each fault on at
    least one case of the family"""
    planted = {f: 0 for f in FAULTS}
    launches = refusals = 0
    for c in _cases(family):
        d = len(c.ngrid)
        for v in R.legs(family):
            for k in range(d):
                name, reason = R.predict(c, v, k)
                if name is None:  # a predicted refusal: that answer alone passes
                    refusals += 1
                    assert R.check(c, v, k, R.Refused(reason), None, 0)[0] == "refused: " + reason
                    other = [x for x in R.REFUSALS if x != reason][0]
                    with pytest.raises(AssertionError):
                        R.check(c, v, k, R.Refused(other), None, 0)
                    with pytest.raises(AssertionError):  # a launch passes through where a refusal is predicted
                        R.check(c, v, k, (np.zeros((c.F, c.ngrid[k])),) * 3, "k_fiber_per_wave<x>", 0)
        v = R.legs(family)[-1]
        ks = [k for k in range(d) if R.predict(c, v, k)[0]]
        if not ks:
            v, ks = R.PER_WAVE, [k for k in range(d) if R.predict(c, R.PER_WAVE, k)[0]]
        k = ks[c.seed % len(ks)]
        name = R.predict(c, v, k)[0]
        r = R.reference(c, k)
        verdict, err = R.check(c, v, k, (r.ref.copy(), r.ui.copy(), r.ab.copy()), name, 0, r)
        assert (verdict, err) == ("ok", 0.0)
        launches += 1
        for f in FAULTS:
            p = _plant(f, c, r, name)
            if p is None:
                continue
            planted[f] += 1
            with pytest.raises(AssertionError) as info:
                R.check(c, v, k, p[0], p[1], p[2], r)
            assert repr(c) in str(info.value) and f"k {k}" in str(info.value)  # a failure names its case
    assert launches == len(R.SEEDS[family])
    assert all(n >= 1 for n in planted.values()), planted
    # a repeated candidate row is no difference: the device may name either copy
    for c in _cases(family):
        if c.cand_kind != "own" and len(c.cands) > 2:
            k = [k for k in range(len(c.ngrid)) if R.predict(c, R.PER_WAVE, k)[0]][0]
            r = R.reference(c, k)
            ui = np.where(r.ui == 0, len(c.cands) - 1, r.ui)
            assert R.check(c, R.PER_WAVE, k, (r.ref.copy(), ui, r.ab.copy()), R.predict(c, R.PER_WAVE, k)[0], 0, r)[0] == "ok"
            break


def test_refusal_of_reads_launch_bellmans_answers():
    """only launch_bellman's three UNSUPPORTED answers count as a refusal; any other error is not one"""
    msg = "bellman_fibers_host failed (code 3): bellman_fibers: "
    assert R.refusal_of(RuntimeError(msg + "no kernel instantiation for (model, dim, rank, N)")).reason == R.REFUSALS[0]
    assert R.refusal_of(RuntimeError(msg + "N x rank^2 of the varying core exceeds the 160 KB of LDS the per-wave kernel stages it in")).reason == R.REFUSALS[1]
    assert R.refusal_of(RuntimeError(msg + "no kernel instantiation serves this call (model, dim, rank, N, control mode)")).reason == R.REFUSALS[2]
    assert R.refusal_of(RuntimeError("bellman_fibers_host failed (code 2): bellman_fibers: null buffer")) is None
    assert R.refusal_of(RuntimeError("bellman_fibers_host failed (code 5): hipErrorIllegalAddress")) is None
    assert R.refusal_of(RuntimeError("upload_value failed (code 3): upload_value: no kernel instantiation for this (dim, rank)")) is None


# ------------------------------------------------------------------------------------------------------- the forms leg
def _form_cases(family):
    return [R.form_case(family, s) for s in R.FORM_SEEDS[family]]


@pytest.mark.parametrize("family", R.FORM_FAMILIES)
def test_form_generator_coverage_and_preconditions(oracle, family):
    """a forms case is reproducible and in its domain; the committed seeds cover every F, class, k, discount, obstacle or none and
    N on each side of 64 along the launched k -- for lqr_cd_jump all 16 subsets of the four switches on each side, for lqr_ic
    both impulse forms on each side; the restatement runs on the oracle's stencil, leaves at most MAX_UNPINNED of the live nodes
    unpinned, and, from the reference alone: the horizon step keeps Q delta / h^2 <= 0.8 on the whole grid (no CFL bit), and
    dominance holds on the whole grid wherever correlation is on (a draw that breaks it was redrawn: no DOMINANCE bit)"""
    import backup_ref as BR

    seeds = R.FORM_SEEDS[family]
    assert list(seeds) == sorted(set(seeds))
    have, seen = set(), set()
    for c in _form_cases(family):
        assert c.tobytes() == R.form_case(family, c.seed).tobytes()
        seen.add(c.tobytes())
        assert all(5 <= n <= 128 for n in c.ngrid) and c.rank in R.FORM_RANKS[family] and c.F in R.FORM_F and c.k in (0, 1)
        assert c.discount in (0.3, 0.0) and (c.delta > 0.0) == c.switches[0]
        have |= R.form_items(c)
        if family == "lqr_cd_jump" and (c.switches[0] or c.switches[3]):
            qmax, broken = R._grid_preconditions(c)
            assert not broken, repr(c)
            if c.switches[0]:
                h2, _ = BR.mca_constants(c.workload())
                assert 0.7 < qmax * c.delta / h2 <= 0.8, (repr(c), qmax * c.delta / h2)
        for label in c.labels():
            r = R.form_reference(c, label)
            assert r.ref.shape == (c.F, c.ngrid[c.k]) and (r.ab == 0).any(), repr(c)
            assert not (r.status & (R.STATUS_CFL | R.STATUS_DOMINANCE)), (repr(c), r.status)
        assert R.form_unpinned_share(c) <= R.MAX_UNPINNED, repr(c)
    assert len(seen) == len(seeds)
    assert R.form_needs(family) <= have, R.form_needs(family) - have
    if family == "lqr_cd_jump":
        assert len({i for i in R.form_needs(family) if i[0] == "switches"}) == 32
    if family == "lqr_ic":
        assert {i[1][2] for i in R.form_needs(family) if i[0] == "switches"} == {False, True}


@pytest.mark.parametrize("family", R.FORM_FAMILIES)
def test_form_checker_rejects_planted_faults(oracle, family):
    """check_form accepts the restatement's own outputs and rejects a value off by 1e-10 max(1, |ref|), a flipped flag, another
    action at a pinned node, a node left at the pre-fill, a wrong kernel name, a status bit and a refusal, on every case"""
    for c in _form_cases(family):
        for label in c.labels():
            r = R.form_reference(c, label)
            own = lambda: (r.ref.copy(), r.ui.astype(np.int32), r.ab.copy())
            assert R.check_form(c, label, own(), c.kernel(), r.status, r) == 0.0
            live = np.argwhere((r.ab == 0) & np.isfinite(r.ref))
            at = tuple(live[len(live) // 2])
            faults = []
            out, ui, ab = own()
            out[at] += 1e-10 * max(1.0, abs(out[at]))
            faults.append(((out, ui, ab), c.kernel(), r.status))
            out, ui, ab = own()
            ab[at] = 1
            faults.append(((out, ui, ab), c.kernel(), r.status))
            pinned = np.argwhere((r.ab == 0) & (r.margin > R.PIN_MARGIN))
            if len(pinned):
                out, ui, ab = own()
                p = tuple(pinned[0])
                ui[p] = ui[p] + 1 if ui[p] == 0 else 0
                faults.append(((out, ui, ab), c.kernel(), r.status))
            out, ui, ab = own()
            out[-1, -1] = np.nan
            faults.append(((out, ui, ab), c.kernel(), r.status))
            faults.append((own(), c.kernel().replace(",1>", ",3>").replace(",2>", ",1>"), r.status))
            faults.append((own(), c.kernel(), r.status ^ R.STATUS_STATIONARY))
            faults.append((own(), c.kernel(), r.status | R.STATUS_DOMINANCE))
            faults.append((R.Refused(R.REFUSALS[0]), None, 0))
            for f in faults:
                with pytest.raises(AssertionError) as info:
                    R.check_form(c, label, f[0], f[1], f[2], r)
                assert repr(c) in str(info.value)
