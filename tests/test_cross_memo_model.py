"""The memo model and the memo cases on the CPU (cross_memo_model.py): every case of tests/test_gpu_cross_memo.py runs here first
with SimDevice -- the restated iteration over a first-value-stays dict -- standing in for the device, and is checked by a fresh
model exactly as the GPU test checks the device.  The admission conditions of the cases are enforced by the scenarios themselves
(CaseRefused) and printed here, so no GPU case can pass with nothing to see:
  two value functions   at least 100 hits whose T_A and T_B differ by more than 1e-3 of the scale
  literal ends          at least 2 conflicting nodes inside one iteration
  policy                at least 10 % of the hits of the second call at nodes where the greedy index of P1 and P2 differs and the two
                        Q entries differ by more than 1e-6 of the scale; best and second-best Q at least 1e-9 of the scale apart
Then one mistake at a time is planted in the stand-in, and the case's named assertion must fail."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_memo_model as mm  # noqa: E402
import cross_reference as cr  # noqa: E402

DUBINS, CAR = mm.TWO_VALUE_CASES


def _maker(oracle, fault=None):
    return lambda w, cores, **kw: mm.SimDevice(oracle, w, cores, fault=fault, **kw)


def _small_table(monkeypatch, log2):
    monkeypatch.setenv("C3SC_MEMO_MIN_LOG2", str(log2))
    monkeypatch.setenv("C3SC_MEMO_SCALE", "0")


# ------------------------------------------------------------------------------------------------ the model itself
class _Table:
    """a 'problem' whose value of node (i, j) along k is 100 k + 10 i + j: direction dependent, like literal ends"""

    def __init__(self, w, offset=0.0):
        self.w, self.offset = w, offset

    def bellman_fibers(self, k, idx):
        idx = np.asarray(idx)
        N = self.w.ngrid[k]
        out = np.zeros((len(idx), N))
        for f, t in enumerate(idx):
            for j in range(N):
                node = list(t)
                node[k] = j
                out[f, j] = self.offset + 100.0 * k + 10.0 * node[0] + node[1]
        return out, np.zeros((len(idx), N), dtype=np.int32), np.zeros((len(idx), N), dtype=np.int32)


def test_node_ids_use_the_strides_of_check_iteration():
    w = mm._workload("dubins3d", (12, 13, 9))
    idx = np.array([[3, 0, 5], [11, 0, 8]], dtype=np.int32)
    ids = mm.node_ids(w, 1, idx)
    assert ids.shape == (2, 13)
    assert ids[0, 0] == 3 * 13 * 9 + 5 and ids[0, 12] == 3 * 13 * 9 + 12 * 9 + 5 and ids[1, 4] == 11 * 13 * 9 + 4 * 9 + 8
    # the varying entry of a tuple is ignored
    assert np.array_equal(mm.node_ids(w, 1, np.array([[3, 7, 5]])), ids[:1])


def test_first_value_stays_and_the_counts_are_kept():
    w = mm._workload("dubins3d", (4, 5, 3))
    m = mm.MemoProblem(_Table(w))
    a, _, _ = m.bellman_fibers(0, np.array([[0, 2, 1]]))          # nodes (0..3, 2, 1) along 0
    assert list(a[0]) == [2.0, 12.0, 22.0, 32.0] and m.stores == 4 and m.hits == 0
    b, _, _ = m.bellman_fibers(1, np.array([[1, 0, 1]]))          # nodes (1, 0..4, 1) along 1: (1, 2, 1) was stored along 0
    assert list(b[0]) == [110.0, 111.0, 12.0, 113.0, 114.0]
    assert m.stores == 8 and m.hits == 1 and len(m.conflicts) == 1 and m.differing(mm.SEE_TOL) == 1
    m.switch(_Table(w, offset=0.5))                               # another value function, same epoch: the stored values stay
    c, _, _ = m.bellman_fibers(0, np.array([[0, 2, 1], [0, 3, 1]]))
    assert list(c[0]) == [2.0, 12.0, 22.0, 32.0] and list(c[1]) == [3.5, 113.0, 23.5, 33.5] and m.stores == 11
    m.new_epoch()
    d, _, _ = m.bellman_fibers(0, np.array([[0, 2, 1]]))
    assert list(d[0]) == [2.5, 12.5, 22.5, 32.5] and len(m.stored_ids()) == 4
    full = mm.MemoProblem(_Table(w), capacity=3)                  # a full table: the value is returned, not stored
    e, _, _ = full.bellman_fibers(0, np.array([[0, 2, 1]]))
    assert list(e[0]) == [2.0, 12.0, 22.0, 32.0] and full.stores == 3 and full.overflow == 1


def test_a_policy_case_without_a_gap_is_refused(oracle):
    """a constant policy value function: the candidates of dubins3d differ only in the drift along the heading, a constant has
    no slope to see it with, best and second-best Q tie, and the model refuses the batch with a message"""
    w, V, _, ranks, I, J = mm.make_case(DUBINS, max_cands=6)
    flat = [np.ones_like(c) for c in V]
    model = mm.PolicyMemoProblem(oracle, w, V, flat)
    with pytest.raises(mm.CaseRefused, match="not pinned"):
        model.bellman_fibers(2, cr.fiber_index_list(w.dx, 2, I[2], J[2]))


# ------------------------------------------------------------------------------------------------ every case, clean
@pytest.mark.parametrize("case", mm.TWO_VALUE_CASES, ids=[c[0] for c in mm.TWO_VALUE_CASES])
def test_replay_continue_and_new_epoch_pass_on_the_stand_in(oracle, case):
    first, second = mm.scenario_replay(_maker(oracle), case)
    rep1, rep2, rep3 = mm.scenario_continue_and_new_epoch(_maker(oracle), oracle, case)
    assert first[3][0] == rep1["nodes"]


@pytest.mark.parametrize("case", mm.LITERAL_CASES, ids=[c[0] for c in mm.LITERAL_CASES])
def test_literal_ends_pass_on_the_stand_in(oracle, case):
    mm.scenario_literal(_maker(oracle), oracle, case)


@pytest.mark.parametrize("case,log2", [(CAR, 11), (DUBINS, 10)], ids=["car7d-7", "dubins3d-12-13-9"])
def test_growth_without_overflow_passes_on_the_stand_in(oracle, monkeypatch, case, log2):
    _small_table(monkeypatch, log2)
    first, _ = mm.scenario_replay(_maker(oracle), case, grow=2)
    assert first[3][0] <= 1 << log2


def test_overflow_passes_on_the_stand_in(oracle, monkeypatch):
    _small_table(monkeypatch, 10)
    mm.scenario_overflow(_maker(oracle), oracle, CAR, 1024)


def test_epoch_wrap_passes_on_the_stand_in(oracle):
    mm.scenario_epoch_wrap(_maker(oracle), oracle, DUBINS)


@pytest.mark.parametrize("case", mm.POLICY_CASES, ids=[c[0] for c in mm.POLICY_CASES])
def test_policy_memo_passes_on_the_stand_in(oracle, case):
    reps = mm.scenario_policy(_maker(oracle), oracle, case)
    assert len(reps) == 3
    if case[0] in mm.POLICY_CASES_WITH_NEW_NODES:  # 'stored nodes keep P1's candidate and new nodes take P2's'
        assert reps[1]["policies_stored"] > 0
    mm.scenario_policy_refuses_the_pair_kernel(_maker(oracle), case)


# ------------------------------------------------------------------------------------------------ one planted mistake at a time
SAME_EPOCH = r"iteration 2 under B, same epoch"
LITERAL = r"literal \(per-wave epilogue\) (left|right|core|info)"  # the memo model's own check, not the guard behind it
PLANTED = [
    # fault, scenario, what must fail
    ("no-memo", "replay", "a hit did not return the stored value"),
    ("no-memo", "continue", SAME_EPOCH),
    ("no-memo", "literal", LITERAL),
    ("no-memo", "growth", "a hit did not return the stored value"),
    ("last-value-stays", "replay", "a hit did not return the stored value"),
    ("last-value-stays", "continue", SAME_EPOCH),
    ("last-value-stays", "literal", LITERAL),
    ("epoch-not-cleared", "continue", "new epoch under B"),
    ("epoch-not-cleared", "wrap", "epoch wrap at epoch 0x7FFF|epoch wrap after the wrap"),
    ("wrap-not-cleared", "wrap", "epoch wrap after the wrap"),
    ("growth-drops-every-seventh", "growth", "a hit did not return the stored value|the replay stored"),
    ("growth-drops-every-seventh", "overflow", "the replay stored"),
    ("hit-returns-next-id", "replay", "a hit did not return the stored value"),
    ("hit-returns-next-id", "continue", "iteration 1 under A"),  # the hits inside the first iteration already show it
    ("hit-returns-next-id", "literal", LITERAL),
    ("policy-tag-not-reset", "policy", "tag 8 under P2"),
]


def _run(oracle, monkeypatch, scenario, make):
    if scenario == "replay":
        for case in mm.TWO_VALUE_CASES:
            mm.scenario_replay(make, case)
    elif scenario == "continue":
        for case in mm.TWO_VALUE_CASES:
            mm.scenario_continue_and_new_epoch(make, oracle, case)
    elif scenario == "literal":
        for case in mm.LITERAL_CASES:
            mm.scenario_literal(make, oracle, case)
    elif scenario == "growth":
        _small_table(monkeypatch, 10)
        mm.scenario_replay(make, DUBINS, grow=2)
    elif scenario == "overflow":
        _small_table(monkeypatch, 10)
        mm.scenario_overflow(make, oracle, CAR, 1024)
    elif scenario == "wrap":
        mm.scenario_epoch_wrap(make, oracle, DUBINS)
    elif scenario == "policy":
        mm.scenario_policy(make, oracle, mm.POLICY_CASES[0])
    else:
        raise KeyError(scenario)


@pytest.mark.parametrize("fault,scenario,match", PLANTED, ids=[f"{f}-{s}" for f, s, _ in PLANTED])
def test_a_planted_mistake_is_caught(oracle, monkeypatch, fault, scenario, match):
    assert fault in mm.FAULTS
    with pytest.raises(AssertionError, match=match) as e:
        _run(oracle, monkeypatch, scenario, _maker(oracle, fault))
    assert not isinstance(e.value, mm.CaseRefused), f"the case was refused, not failed: {e.value}"
    print(f"{fault} in {scenario}: {type(e.value).__name__}: {str(e.value)[:200]}")


@pytest.mark.parametrize("case", mm.LITERAL_CASES + mm.TWO_VALUE_CASES, ids=[c[0] for c in mm.LITERAL_CASES + mm.TWO_VALUE_CASES])
def test_every_planted_value_mistake_fails_every_case_it_can_show_in(oracle, case):
    """the table above stops at the first failing case of a scenario; here each case on its own"""
    for fault in ("no-memo", "last-value-stays", "hit-returns-next-id"):
        with pytest.raises(AssertionError) as e:
            if case in mm.LITERAL_CASES:
                mm.scenario_literal(_maker(oracle, fault), oracle, case)
            else:
                mm.scenario_continue_and_new_epoch(_maker(oracle, fault), oracle, case)
        assert not isinstance(e.value, mm.CaseRefused), f"{fault}: the case was refused, not failed: {e.value}"


# ------------------------------------------------------------------------------------------------ the checks depend on the dict
class _Blind(mm.MemoProblem):
    def lookup(self, node, own):
        value, hit = super().lookup(node, own)
        return own, hit


class _BlindPolicy(mm.PolicyMemoProblem):
    def candidate(self, node, greedy):
        _, hit = super().candidate(node, greedy)
        return greedy, hit


def test_a_model_that_ignores_its_dict_fails_a_correct_device(oracle, monkeypatch):
    """The other direction: the stand-in is right and the CHECKING model ignores what it stored.  Every case that is held to the
    model -- (b), (d), (h) -- must then fail; (a), (e), (g) use no model (bit equality of two device results)."""
    monkeypatch.setattr(mm, "MemoProblem", _Blind)
    monkeypatch.setattr(mm, "PolicyMemoProblem", _BlindPolicy)
    for case in mm.TWO_VALUE_CASES:
        with pytest.raises(cr.CrossCheckError, match=SAME_EPOCH):
            mm.scenario_continue_and_new_epoch(_maker(oracle), oracle, case)
    for case in mm.LITERAL_CASES:
        with pytest.raises(cr.CrossCheckError, match=LITERAL):
            mm.scenario_literal(_maker(oracle), oracle, case)
    with pytest.raises(cr.CrossCheckError, match="tag 7 under P2"):
        mm.scenario_policy(_maker(oracle), oracle, mm.POLICY_CASES[0])
