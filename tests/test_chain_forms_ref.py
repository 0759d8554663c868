"""The numpy restatement of the chain's eight forms (chain_forms_ref.py) on its own, without a GPU: the probabilities sum to one,
the outcomes recombine to backup_ref's value (the identity that makes the chain the backup's own), the walk table of the GPU
tests meets its preconditions under the reference alone, and `check` rejects a run with a planted mistake."""
import numpy as np
import pytest

import backup_ref as BR
import chain_forms_ref as CF

MID = 1000  # no kernel runs here: any id
CASES = [("lqr", 4), ("lqr", 12), ("lqr3", 12)]
CASE_IDS = ["lqr-4", "lqr-12", "lqr3"]
FORM_IDS = [CF.form_id(f) for f in CF.FORMS]


_UNIFORMS = {}


def _uniforms(n, nsteps, seed=CF.SEED):
    """the table of the GPU tests: the host twin of the device's Philox draw"""
    if (n, nsteps, seed) not in _UNIFORMS:
        _UNIFORMS[(n, nsteps, seed)] = CF.Ref.uniforms(seed, 0, n, nsteps)
    return _UNIFORMS[(n, nsteps, seed)]


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(model, rank, form, nstack=0):
        key = (model, rank, form, nstack)
        if key not in memo:
            memo[key] = CF.case(model, MID, rank, form, nstack=nstack)
        return memo[key]

    return get


@pytest.mark.parametrize("form", CF.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("model,rank", CASES, ids=CASE_IDS)
def test_probabilities_and_the_identity(cases, model, rank, form):
    w, cores, ref = cases(model, rank, form)
    T = ref.table()
    nodes = T.ix[:: (1 if model == "lqr" else 3)]
    res = ref.reference_outcomes(nodes)
    live = res["flag"] == 0
    moving = live & (res["uidx"] >= 0) & (res["uidx"] < ref.nc)
    stopping = live & (res["uidx"] == ref.nc)
    assert moving.any() and (stopping.any() == form[1]) and (res["flag"] == 1).any() and (res["flag"] == -1).any()
    total = res["P"].sum(-1) + res["pmark"].sum(-1) + res["pself"]
    assert np.abs(total[moving] - 1.0).max() <= 1e-14 * (2 * w.dx + 4)
    assert (total[~moving] == 0.0).all()
    if form[0]:
        assert (res["pself"][moving] > 0.0).all(), "the cases stay inside the CFL rule"
        assert (res["dt"][moving] == ref.delta).all()
    if form[2]:
        assert (res["pmark"][moving] > 0.0).all()
    # the identity: what the outcomes recombine to is backup_ref's value, psi at the stopping nodes
    rec = ref.identity(nodes, res)
    value = T.value[[ref.flat(ix) for ix in nodes]]
    assert np.abs(rec[moving] - value[moving]).max() <= CF.TOL * max(1.0, np.abs(value).max())
    if form[1]:
        assert (rec[stopping] == T.psi[[ref.flat(ix) for ix in nodes]][stopping]).all()
    assert np.isnan(rec[~live]).all()


@pytest.mark.parametrize("form", CF.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("model,rank", CASES, ids=CASE_IDS)
def test_walk_table_preconditions(cases, model, rank, form):
    horizon, stop, jump = form
    w, cores, ref = cases(model, rank, form, CF.NSTEPS + 1 if horizon else 0)
    run = ref.walk(CF.start_nodes(ref), CF.NSTEPS, _uniforms(CF.NLANES, CF.NSTEPS))
    st = ref.stats
    want = {"axis"}
    if horizon:
        want.add("self")
    if stop:
        want.add("stop")
    if jump:
        M = ref.table(0 if horizon else None).M
        want |= {"mark%d:inside" % m for m in range(M)}
        if model == "lqr":
            want |= {"mark0:face", "mark2:obstacle"}
        else:  # no live node of 5 x 128 x 5 has a mark beyond the absorbing face: a mark into the obstacle leaves
            assert any(k.endswith(":obstacle") for k in st["kinds"]), sorted(st["kinds"])
    assert want <= st["kinds"], sorted(want - st["kinds"])
    assert st["exits"] == {"absorbed", "obstacle"}
    assert st["alive_mid"] >= CF.NLANES // 2, st["alive_mid"]
    assert st["unsure"] <= 0.025 * st["steps"], (st["unsure"], st["steps"])
    got = ref.check(run)
    assert got["steps"] == st["steps"]


def _faulty_forms(fault):
    feat = "hsj".index(CF.FAULTS[fault][0])
    return [f for f in CF.FORMS if f[feat]]


@pytest.mark.parametrize("fault,form", [(f, fm) for f in CF.FAULTS for fm in _faulty_forms(f)],
                         ids=lambda v: v if isinstance(v, str) else CF.form_id(v))
def test_check_rejects_a_planted_fault(cases, fault, form):
    w, cores, ref = cases("lqr", 4, form, CF.NSTEPS + 1 if form[0] else 0)
    run = ref.walk(CF.start_nodes(ref), CF.NSTEPS, _uniforms(CF.NLANES, CF.NSTEPS), fault=fault)
    with pytest.raises(AssertionError):
        ref.check(run)
