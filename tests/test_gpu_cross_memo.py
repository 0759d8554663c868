"""The device node memo at step level, against a first-value-stays model (cross_memo_model.py, where the cases are written and
explained; tests/test_cross_memo_model.py runs every one of them on the CPU first, clean and with planted mistakes).

Elsewhere the memo is invisible: every step-level test runs under consistent ends with one value function, where a hit returns
what the lane would have computed anyway, and only the count info[0] is asserted.  Here a hit is made to matter:
  (a) replay        A, then B uploaded and the same iteration again in the same epoch: all hits, bit-identical, nothing stored
  (b) continue      B from the sets A's iteration returned, same epoch: the model loaded with iteration 1's nodes
  (c) new epoch     then a new sweep under B: the plain oracle, full count
  (d) literal ends  the first direction that reaches a node decides its value; the plain literal oracle must FAIL the result
  (e) growth        c3sc_hip_cross_grow_memo twice between A and the replay (k_cross_memo_rehash keeps every entry)
  (f) overflow      1024 slots for 1386 nodes: exactly 1024 stored, correct values, the rest stored after a doubling
  (g) epoch wrap    set-ups up to epoch 0x7FFF, an iteration there on other nodes, then the wrap: entries of epoch 1 must be gone
  (h) policy memo   c3sc_hip_cross_iteration_pi: the first greedy candidate stays for a policy tag, a new tag resets it
(a) to (e) run once with the variant left at AUTO -- the per-wave kernel, memo in its epilogue -- and once with the pair and quad
kernels forced where the model has them -- the separate k_cross_memo pass; last_kernel must name the family.  A fresh context per
case: a context's table never shrinks.  Not asserted: which slots hold which keys (only what lookups return); the sharded NaN
mark, c3sc_hip_cross_speculate and the host FastMemo are out of scope."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cross_memo_model as mm  # noqa: E402
from cross_device_lib import DeviceCross  # noqa: E402

pytestmark = pytest.mark.gpu

DUBINS, CAR = mm.TWO_VALUE_CASES
NAMES = {mm.AUTO: "auto", mm.PAIR: "pair", mm.QUAD: "quad"}
TWO_VALUE = [(c, v) for c in mm.TWO_VALUE_CASES for v in mm.VARIANTS[c[1]]]
LITERAL = [(c, v) for c in mm.LITERAL_CASES for v in mm.VARIANTS[c[1]]]


def _ids(rows):
    return [f"{c[0]}-{NAMES[v]}" for c, v in rows]


def _small_table(monkeypatch, log2):
    """cross_setup reads both with getenv on every call"""
    monkeypatch.setenv("C3SC_MEMO_MIN_LOG2", str(log2))
    monkeypatch.setenv("C3SC_MEMO_SCALE", "0")


@pytest.mark.parametrize("case,variant", TWO_VALUE, ids=_ids(TWO_VALUE))
def test_a_replay_under_another_value_function_returns_the_stored_values(case, variant):
    mm.scenario_replay(DeviceCross, case, variant=variant)


@pytest.mark.parametrize("case,variant", TWO_VALUE, ids=_ids(TWO_VALUE))
def test_the_next_iteration_keeps_stored_nodes_and_a_new_epoch_forgets_them(oracle, case, variant):
    mm.scenario_continue_and_new_epoch(DeviceCross, oracle, case, variant=variant)


@pytest.mark.parametrize("case,variant", LITERAL, ids=_ids(LITERAL))
def test_under_literal_ends_the_first_value_stays(oracle, case, variant):
    mm.scenario_literal(DeviceCross, oracle, case, variant=variant)


GROWTH = [(CAR, 11, v) for v in mm.VARIANTS["car7d"]] + [(DUBINS, 10, v) for v in mm.VARIANTS["dubins3d"]]


@pytest.mark.parametrize("case,log2,variant", GROWTH, ids=[f"{c[0]}-{NAMES[v]}" for c, _, v in GROWTH])
def test_growth_keeps_every_entry(monkeypatch, case, log2, variant):
    """car7d 7^7: 1386 nodes in 2048 slots, 2048 -> 4096 -> 8192; dubins3d: 548 in 1024"""
    _small_table(monkeypatch, log2)
    first, _ = mm.scenario_replay(DeviceCross, case, variant=variant, grow=2)
    assert first[3][0] <= 1 << log2


def test_overflow_stores_exactly_the_slots_and_the_rest_after_a_doubling(oracle, monkeypatch):
    _small_table(monkeypatch, 10)
    mm.scenario_overflow(DeviceCross, oracle, CAR, 1024)


def test_the_epoch_wrap_clears_the_table(oracle):
    """The iteration after the wrap visits nodes that still hold their entry of epoch 1 under A (cross_memo_model.scenario_epoch_wrap).
    The wrap is reached the plain way, by 32 765 set-ups without an iteration; their time is printed (DESIGN 4.6 has the figure)."""
    _, seconds = mm.scenario_epoch_wrap(DeviceCross, oracle, DUBINS)
    print(f"set-up loop: {seconds:.2f} s")


@pytest.mark.parametrize("case", mm.POLICY_CASES, ids=[c[0] for c in mm.POLICY_CASES])
def test_the_policy_memo_keeps_the_first_candidate_for_a_tag(oracle, case):
    mm.scenario_policy(DeviceCross, oracle, case)


def test_the_policy_pass_refuses_a_forced_pair_kernel():
    mm.scenario_policy_refuses_the_pair_kernel(DeviceCross, DUBINS)
