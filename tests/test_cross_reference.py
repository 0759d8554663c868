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


# ------------------------------------------------------------------------------------------------ any rank
# lu_maxvol_reference (the algorithm restated) is the 'device' here: the any-rank checks must accept what the algorithm itself
# returns on singular matrices and reject each kind of broken output.
def _deficient_matrices():
    rng = np.random.default_rng(5)
    out = {}
    for ncol in (2, 7):
        A = rng.standard_normal((60, 10))
        A[:, rng.permutation(10)[:ncol]] = 100.0
        out[f"{ncol}-equal-constant-columns"] = A
    for c in (10.0, 100.0, 1000.0):
        out[f"all-constant-{c:g}"] = np.full((12, 5), c)
    A = rng.standard_normal((8, 8))
    A[6] = A[1]
    out["square-one-repeated-row"] = A
    A = rng.standard_normal((12, 10))
    A[[3, 7, 11]] = A[[0, 1, 2]]
    out["12x10-three-repeated-rows"] = A
    out["rank-4-of-40-columns"] = rng.standard_normal((120, 4)) @ rng.standard_normal((4, 40))
    out["all-zero"] = np.zeros((9, 4))
    return out


DEFICIENT = _deficient_matrices()


def _check_step(A, f, warm=None):
    cr.check_row_bookkeeping(A, f.rows, "step")
    span = cr.check_span(A, f.rows, "step")
    res, big = cr.check_core_any_rank(A, f.rows, f.B, 0.05, "step")
    cr.check_tie_rule(A, f.rows, warm, "step")
    return span, res, big


@pytest.mark.parametrize("name", sorted(DEFICIENT))
def test_the_restated_algorithm_passes_every_any_rank_check_on_singular_matrices(name):
    A = DEFICIENT[name]
    f = cr.lu_maxvol_reference(A, 0.05)
    span, res, big = _check_step(A, f)
    print(f"{name}: {A.shape[0]}x{A.shape[1]} ratio {f.ratio:.2e}, {f.zero_pivots} exact zero pivots, {f.swaps} swaps, span {span:.1e}, "
          f"interpolation {res:.1e}, max|B| {big:.6f}")
    assert f.flag == 1 and not f.capped
    assert not (cr.ADMIT_BELOW <= f.ratio <= cr.ADMIT_ABOVE)
    if name == "all-zero":
        assert f.ratio == 0.0 and f.zero_pivots == 4 and span == 0.0 and res == 0.0 and list(f.rows) == [0, 1, 2, 3]


@pytest.mark.parametrize("c", [10.0, 100.0, 1000.0])
def test_a_constant_matrix_of_a_boundcost_takes_its_rows_in_index_order(c):
    """The tie rule rests on c * (1 / c) == 1.0 for the three boundcosts: confirmed here, not assumed.  One nonzero pivot, the
    rest exactly zero (inv = 0), rows 0 .. n-1; a warm row is boosted and goes first, the others follow in index order."""
    assert c * (1.0 / c) == 1.0
    A = np.full((12, 5), c)
    f = cr.lu_maxvol_reference(A, 0.05)
    assert list(f.rows) == [0, 1, 2, 3, 4] and f.zero_pivots == 4 and f.swaps == 0 and np.all(np.isfinite(f.B))
    warm = np.zeros(12, dtype=bool)
    warm[[9, 11]] = True
    g = cr.lu_maxvol_reference(A, 0.05, warm)
    assert list(g.rows) == [0, 1, 2, 3, 9]
    _check_step(A, g, warm)
    with pytest.raises(cr.CrossCheckError, match="exactly constant"):
        cr.check_tie_rule(A, np.arange(1, 6), None, "rows 1 .. n")
    with pytest.raises(cr.CrossCheckError, match="exactly constant"):
        cr.check_tie_rule(A, f.rows, warm, "the warm row ignored")


def test_broken_output_on_a_singular_matrix_is_rejected():
    A = DEFICIENT["12x10-three-repeated-rows"]
    f = cr.lu_maxvol_reference(A, 0.05)
    twice = f.rows.copy()
    twice[1] = twice[0]
    with pytest.raises(cr.CrossCheckError, match="repeated"):
        cr.check_row_bookkeeping(A, twice, "a repeated row")
    beyond = f.rows.copy()
    beyond[-1] = A.shape[0]
    with pytest.raises(cr.CrossCheckError, match="outside"):
        cr.check_row_bookkeeping(A, beyond, "a row past the matrix")
    with pytest.raises(cr.CrossCheckError, match="not a row"):
        cr.rows_of_set(np.array([[5, 7]]), np.array([[7], [8]]), 5, "rl")  # j = N
    Bn = f.B.copy()
    Bn[4, 3] = np.nan
    with pytest.raises(cr.CrossCheckError, match="not finite"):
        cr.check_core_any_rank(A, f.rows, Bn, 0.05, "a NaN in the core")
    # rows 0, 1, 2 and their copies 3, 7, 11 leave four places for the six remaining independent rows: two are not spanned
    outside = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 11])
    with pytest.raises(cr.CrossCheckError, match="do not span"):
        cr.check_span(A, outside, "both copies of three rows")
    Bb = f.B.copy()
    i = next(i for i in range(A.shape[0]) if i not in set(f.rows))
    Bb[i, 0] += 0.2
    with pytest.raises(cr.CrossCheckError, match="does not interpolate|not dominant"):
        cr.check_core_any_rank(A, f.rows, Bb, 0.05, "a perturbed core")


@pytest.mark.parametrize("name", ["all-zero", "all-constant-10", "all-constant-100", "all-constant-1000", "7-equal-constant-columns"])
def test_dropping_the_zero_pivot_guard_is_caught(name):
    """inv = 1 / dp without the dp != 0 guard, on the matrices that reach an EXACT zero pivot (random repeated rows leave 1e-17
    of rounding instead): the zero pivot's column becomes 0 * inf = NaN, and it reaches the core."""
    A = DEFICIENT[name]
    assert cr.lu_maxvol_reference(A, 0.05).zero_pivots > 0
    f = cr.lu_maxvol_reference(A, 0.05, guard_zero_pivot=False)
    with pytest.raises(cr.CrossCheckError):
        _check_step(A, f)


@pytest.mark.parametrize("name", ["all-zero", "all-constant-10", "all-constant-100", "all-constant-1000"])
def test_flipping_the_tie_order_is_caught(name):
    """ties to the HIGHER index: a constant matrix then gives up its LAST rows"""
    A = DEFICIENT[name]
    f = cr.lu_maxvol_reference(A, 0.05, lower_index_first=False)
    assert list(f.rows) != list(range(A.shape[1]))
    with pytest.raises(cr.CrossCheckError, match="exactly constant"):
        _check_step(A, f)


# ------------------------------------------------------------------------------------------------ the singular cases, simulated
import cross_singular_cases as sc  # noqa: E402
from cross_device_lib import step_classes  # noqa: E402

ALL_CASES = sc.SINGULAR_CASES + [sc.CONTROL_CASE]


@pytest.fixture(scope="module")
def simulated(oracle):
    """Every case of the table through two iterations of the restated algorithm (the second warm-started from the first), once."""
    out = {}
    for case in ALL_CASES:
        cid, ranks = case[0], case[3]
        w, cores, I, J = sc.make_case(case)
        P = oracle.Problem(w, cores, consistent_ends=True)
        its, prevI, prevJ = [], I, J
        for _ in range(2):
            c1, I1, J1 = cr.simulate_iteration(P, ranks, prevJ, restatement=True, I_in=prevI)
            its.append((prevI, prevJ, c1, I1, J1))
            prevI, prevJ = I1, J1
        out[cid] = (w, P, its)
    return out


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_every_singular_case_reaches_its_deficiency_and_stays_inside_the_bounds(simulated, case):
    """Before any GPU run: the case reaches the dispatch classes and the deficiency it is meant for, the restated algorithm alone
    stays inside every bound of the any-rank mode (both iterations), every pivot ratio is admitted, and no step reaches the
    200-swap cap."""
    cid, _, _, ranks, _, want, must_see, must_tie = case
    w, P, its = simulated[cid]
    classes = step_classes(w.ngrid, ranks)
    assert want <= set(classes.values()), f"case {cid} reaches {sorted(set(classes.values()))}, meant for {sorted(want)}"
    seen, tied, stored = set(), set(), None
    for t, (I0, J0, c1, I1, J1) in enumerate(its):
        rep = cr.check_iteration(P, ranks, J0, c1, I1, J1, None, label=cid, allow_deficient=True, I_in=I0, stored=stored)
        cr.check_iteration(P, ranks, J0, c1, I1, J1, [rep["nodes"], rep["flag"], 0, 0], label=cid, allow_deficient=True, I_in=I0,
                           stored=stored)
        stored = rep["stored"]
        lines, by = sc.summarise(f"{cid} iteration {t + 1}", classes, rep)
        print("\n".join(lines))
        assert not any(s["capped"] for s in rep["steps"]), f"{cid}: a step reached the 200-swap cap"
        seen |= {c for c, b in by.items() if b["deficient"]}
        tied |= {c for c, b in by.items() if b["const"]}
        if t == 0:
            assert rep["flag"] == (0 if case is sc.CONTROL_CASE else 1)
    assert must_see <= seen, f"{cid}: deficient matrices in {sorted(seen)}, meant for {sorted(must_see)}"
    assert must_tie <= tied, f"{cid}: exactly constant matrices in {sorted(tied)}, meant for {sorted(must_tie)}"
    if case is sc.CONTROL_CASE:
        assert not seen


def test_the_table_reaches_exact_zero_pivots_and_constant_matrices(simulated):
    zeros = const = 0
    for case in sc.SINGULAR_CASES:
        w, P, its = simulated[case[0]]
        I0, J0, c1, I1, J1 = its[0]
        rep = cr.check_iteration(P, case[3], J0, c1, I1, J1, None, label=case[0], allow_deficient=True, I_in=I0)
        zeros += sum(s["zero_pivots"] for s in rep["steps"])
        const += sum(s["constant"] for s in rep["steps"])
    assert zeros > 0 and const > 0


def test_a_wrong_flag_or_a_tuple_off_the_grid_is_rejected_at_iteration_level(simulated):
    case = sc.by_id("square-first-bond")
    w, P, its = simulated[case[0]]
    I0, J0, c1, I1, J1 = its[0]
    rep = cr.check_iteration(P, case[3], J0, c1, I1, J1, None, allow_deficient=True, I_in=I0)
    assert rep["flag"] == 1
    with pytest.raises(cr.CrossCheckError, match=r"info\[1\]"):
        cr.check_iteration(P, case[3], J0, c1, I1, J1, [rep["nodes"], 0, 0, 0], allow_deficient=True, I_in=I0)
    with pytest.raises(cr.CrossCheckError, match="rank deficient|singular"):  # the strict mode still refuses the case
        cr.check_iteration(P, case[3], J0, c1, I1, J1, [rep["nodes"], 1, 0, 0])
    bad = [a.copy() for a in I1]
    bad[3][2, -1] = w.ngrid[2]
    with pytest.raises(cr.CrossCheckError, match="not a row|not nested"):
        cr.check_iteration(P, case[3], J0, c1, bad, J1, None, allow_deficient=True, I_in=I0)
    ctl = sc.CONTROL_CASE
    w, P, its = simulated[ctl[0]]
    I0, J0, c1, I1, J1 = its[0]
    rep = cr.check_iteration(P, ctl[3], J0, c1, I1, J1, None, allow_deficient=True, I_in=I0)
    with pytest.raises(cr.CrossCheckError, match=r"info\[1\]"):
        cr.check_iteration(P, ctl[3], J0, c1, I1, J1, [rep["nodes"], 1, 0, 0], allow_deficient=True, I_in=I0)


@pytest.mark.parametrize("cid,seed", sc.CONFIRM_SEEDS, ids=[c[0] for c in sc.CONFIRM_SEEDS])
def test_the_confirmation_cases_reach_index_sets_that_stop_changing(oracle, cid, seed):
    """The A / B protocol of the batched confirmation needs a first confirmation that fails and a later one that succeeds: with
    the restated algorithm the sets of each case change in iteration 2 and stop changing within 12 iterations."""
    case = sc.by_id(cid)
    w, cores, I, J = sc.make_case(case, seed=seed)
    P = oracle.Problem(w, cores, consistent_ends=True)

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))

    pI, pJ = I, J
    for t in range(12):
        _, I1, J1 = cr.simulate_iteration(P, case[3], pJ, restatement=True, I_in=pI)
        if t > 0 and same(I1, pI) and same(J1, pJ):
            break
        pI, pJ = I1, J1
    else:
        pytest.fail(f"{cid}: the index sets still change after 12 iterations")
    print(f"{cid}: iteration {t + 1} kept the sets")
    assert t >= 2
