"""Self-tests of the dense cross reference (cross_reference.py) on the CPU: numpy makes the 'device' result itself, and the
checker must accept it and reject a core or a set that is subtly wrong."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_reference as cr  # noqa: E402


def _matrix(m=60, n=6, seed=3):
    return np.random.default_rng(seed).standard_normal((m, n))


def test_a_correct_maxvol_result_is_accepted():
    A = _matrix()
    rows, B = cr.maxvol_rows(A, 0.05)
    dom, cond = cr.check_pivots(A, rows, 0.05, "maxvol")
    res = cr.check_interpolatory(A, rows, B, "maxvol")
    assert dom <= 1.05 * cr.DOMINANCE_SLACK and res <= 1e-13 and cond < 1e3


def test_a_core_perturbed_by_1e_8_is_rejected():
    A = _matrix()
    rows, B = cr.maxvol_rows(A, 0.05)
    Bp = B.copy()
    i = next(i for i in range(A.shape[0]) if i not in set(rows))
    Bp[i, 2] += 1e-8 * np.abs(B).max()
    with pytest.raises(cr.CrossCheckError, match="does not interpolate"):
        cr.check_interpolatory(A, rows, Bp, "perturbed core")
    Bq = B.copy()  # and off the identity on a pivot row
    Bq[rows[1], 0] = 1e-8
    with pytest.raises(cr.CrossCheckError, match="identity"):
        cr.check_interpolatory(A, rows, Bq, "perturbed pivot row")


def test_a_set_with_a_dominated_row_is_rejected():
    A = _matrix()
    rows, B = cr.maxvol_rows(A, 0.05)
    c = 3
    others = [i for i in range(A.shape[0]) if i not in set(rows)]
    i = min(others, key=lambda q: abs(abs(B[q, c]) - 0.3))  # |B[i, c]| ~ 0.3: swapping it in shrinks the volume
    bad = np.sort(np.array([i if q == c else r for q, r in enumerate(rows)]))
    with pytest.raises(cr.CrossCheckError, match="not dominant"):
        cr.check_pivots(A, bad, 0.05, "dominated row")


def test_sets_are_mapped_to_rows_and_checked_for_nesting():
    I = np.array([[4, 1], [2, 7]])
    assert list(cr.rows_of_set(np.array([[2, 7, 0], [4, 1, 3]]), I, 5, "lr")) == [1, 6]  # a + r0 j
    J = np.array([[9], [8], [7]])
    assert list(cr.rows_of_set(np.array([[3, 8], [0, 7]]), J, 5, "rl")) == [8, 10]      # j + N b
    with pytest.raises(cr.CrossCheckError, match="not nested"):
        cr.rows_of_set(np.array([[3, 6]]), J, 5, "rl")


def test_a_whole_numpy_iteration_is_accepted_and_a_wrong_one_rejected(oracle):
    """The iteration-level checker on a small car7d train, numpy's cross iteration standing in for the device."""
    from c3sc_amd import workloads as wl

    w = wl.c4_car7d().scaled(ngrid=(9, 8, 10, 7, 6, 5, 11), rank=4)
    P = oracle.Problem(w, wl.synth_cores(w), consistent_ends=True)
    ranks = (1, 4, 5, 5, 4, 3, 3, 1)
    rng = np.random.default_rng(2)
    d = w.dx
    J = []
    for k in range(d):
        dims = range(k + 1, d)
        seen = set()
        while len(seen) < ranks[k + 1]:
            seen.add(tuple(int(rng.integers(1, w.ngrid[m] - 1)) for m in dims))
        J.append(np.array(sorted(seen), dtype=np.int32).reshape(ranks[k + 1], d - 1 - k))
    cores, I, Jn = cr.simulate_iteration(P, ranks, J)
    rep = cr.check_iteration(P, ranks, J, cores, I, Jn, None, label="numpy")
    assert len(rep["steps"]) == 2 * (d - 1)
    with pytest.raises(cr.CrossCheckError, match="nodes"):
        cr.check_iteration(P, ranks, J, cores, I, Jn, [rep["nodes"] - 1, 0, 0, 0], label="numpy")
    bad = [c.copy() for c in cores]
    bad[0][5] *= 1.0 + 1e-9
    with pytest.raises(cr.CrossCheckError, match="core 0"):
        cr.check_iteration(P, ranks, J, bad, I, Jn, None, label="numpy")
