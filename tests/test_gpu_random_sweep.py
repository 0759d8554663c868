"""The seeded random sweep of the Bellman fiber kernels on a device: every committed case of tests/random_cases.py (the seed
lists that tests/test_random_cases.py holds to the coverage conditions) under AUTO, the per-wave, the pair and the quad variant --
the quad on an engine of its own, whose upload pads to the quad kernels' classes -- at every k, each launch through
random_cases.check: values within 1e-12 of the case's scale, absorbed flags exact, every output written, controls equal where the
oracle pins them, status word, the kernel name of the selection restatement, and a refusal only where the restatement predicts
that refusal.  A batch of 1025 fibers runs again with C3SC_FIBER_PARTITION=1 and must not change a bit.  A third of the cases
run the stencil kernel against the oracle's stencil, half of them policy evaluation with the oracle's argmin forced.

One test is a chunk of CHUNK seeds of one model.  A failure prints the case (its family and seed replay it: `python
tools/fuzz_parity.py --case FAMILY SEED`), the variant, k, the kernel and the worst node.  -s shows the launches and the worst
relative error per kernel family."""
import contextlib

import pytest

import random_cases as R

pytestmark = pytest.mark.gpu
CHUNK = 5
CHUNKS = [(f, i) for f in R.FAMILIES for i in range(0, len(R.SEEDS[f]), CHUNK)]


@pytest.mark.parametrize("family,start", CHUNKS, ids=[f"{f}-{i}" for f, i in CHUNKS])
def test_random_cases_vs_oracle(oracle, monkeypatch, family, start):
    from c3sc_amd.engine import C3scHipError

    @contextlib.contextmanager
    def partition(value):
        with monkeypatch.context() as m:
            m.setenv("C3SC_FIBER_PARTITION", value)
            yield

    tally = R.Tally()
    for seed in R.SEEDS[family][start:start + CHUNK]:
        c = R.case(family, seed)
        try:
            R.run_case(c, tally, partition_env=partition)
        except C3scHipError as e:  # not one of launch_bellman's refusals: those go through check
            raise AssertionError(f"{c!r}\n  {e}") from e
    print(f"{family} seeds {R.SEEDS[family][start:start + CHUNK]}: " + "; ".join(tally.lines()))
    assert tally.runs


FORM_CHUNKS = [(f, i) for f in R.FORM_FAMILIES for i in range(0, len(R.FORM_SEEDS[f]), 8)]


@pytest.mark.parametrize("family,start", FORM_CHUNKS, ids=[f"{f}-{i}" for f, i in FORM_CHUNKS])
def test_random_form_cases_vs_numpy(oracle, family, start):
    """the forms leg: lqr_cd_jump (any subset of horizon, stop, jump, correlation), lqr_ic (interventions, with and without
    jumps) and lqgame (both orders) on random 2-D grids, each launch through random_cases.check_form against the feature's numpy
    restatement on the oracle's stencil"""
    from c3sc_amd.engine import C3scHipError

    tally = R.Tally()
    for seed in R.FORM_SEEDS[family][start:start + 8]:
        c = R.form_case(family, seed)
        try:
            R.run_form_case(c, tally)
        except C3scHipError as e:
            raise AssertionError(f"{c!r}\n  {e}") from e
    print(f"{family} seeds {R.FORM_SEEDS[family][start:start + 8]}: " + "; ".join(tally.lines()))
    assert tally.runs
