"""The device-resident cross core steps on SINGULAR and numerically deficient matrices, against the dense reference's any-rank
mode (cross_reference.check_iteration(..., allow_deficient=True)).

test_cross_core_steps.py keeps every matrix at full rank on purpose.  Production does not: the headline solve (car7d 41^7, cross
rank 48) runs its first bond at r_1 = N_0 = 41 on an absorbing dimension, so the first core step of every sweep factors an exactly
singular square matrix and the right-to-left step behind it has two equal constant columns; a rank-1 bond of car7d puts its one
pivot on an absorbing face.  Every form of the step carries the branch inv = dp != 0 ? 1 / dp : 0 and ends by raising counters[1]
when the smallest pivot is below 1e-12 of the largest.  Here those branches are reached in every form and held to the oracle:

  asserted      sets in range, nested, distinct, ascending; the chosen rows span the matrix; right-to-left cores finite,
                the identity on their rows, interpolatory, max |B| <= (1 + swap_tol)(1 + 2^-20); info[1] equal to the flag the restated
                algorithm (cross_reference.lu_maxvol_reference) predicts on the oracle's matrices along the device's own path; on
                an exactly constant matrix the rows the tie rule dictates (0 .. n-1 when no row is warm), bit for bit; info[0]
  not asserted  dominance of deficient left-to-right steps (no core to bound, inv(A[P]) does not exist); which rows are picked in
                noise directions (the pivot is chosen among roundings that differ between the oracle and the device)

The cases (cross_singular_cases.py; value rank 4, consistent ends on, seed 7) and why they differ from a first sketch.  car7d and
dubins3d absorb on dimensions 0 and 1 only, and a right set J[k] covers the dimensions k+1 .. d-1: only J[0] can carry a face index.
Constant columns behind step 0 therefore come through the LEFT sets -- a square first bond, or a bond above the number of distinct
rows -- and the grids are the smallest that put a deficient matrix into each form (asserted per case, on the CPU and here):
  square-first-bond    car7d 7^7, (1,7,8,8,8,8,7,1): 7 x 7 with two equal rows, then two constant columns in right-to-left step 1
  face-columns-regs2   dubins3d (8,65,9), (1,8,8,1): N_0 = 8 instead of 9 makes the first bond square, or the 520 x 8 two-row step
                       never sees the two constant columns; two tuples of J[0] on a face
  face-columns-lds     car7d (5,5,9,9,9,9,9), (1,5,17,17,17,17,9,1): N_0 = N_1 = 5 leaves the 25 x 17 step 1 ten distinct rows (seven
                       exact zero pivots), I[2] then holds the face tuples and the 153 x 17 right-to-left step 2 their constant columns
  global-40-48         car7d 7^7, (1,7,33,41,41,33,7,1): 49 x 33 with 26 distinct rows at NR = 40, 231 x 7 with two constant columns
                       at NR = 32; the NR = 48 steps of this layout have full rank
  global-48            car7d 7^7, (1,7,41,41,41,33,7,1): added so that NR = 48 factors a deficient matrix too (49 x 41, 287 x 41)
  global-32-le32       dubins3d (24,31,31), (1,24,24,1): N_0 = 24 instead of 31 for the square first bond (24 x 24 x 31 x 8 B is
                       still over the LDS cap): 744 x 24 with two constant columns
  tall                 dubins3d (24,101,24), (1,24,24,1): 2424 x 24 with two constant columns
  rank-1-face          car7d 7^7, (1,4,1,4,4,4,4,1): the one pivot behind the rank-1 bond is the boundcost; every matrix after
                       it is exactly constant (nine of them per iteration: the tie rule, with and without warm rows)
  all-constant         car7d 7^7, (1,4,4,4,4,4,4,1): every tuple of J[0] on a face: step 0 is exactly constant
  rank-1-face-lds      car7d 7^7, (1,4,1,7,17,17,7,1)    the same rank-1 bond in front of each remaining form, so that every form
  rank-1-face-global   car7d 7^7, (1,4,1,7,33,41,7,1)    factors exactly constant matrices -- the only place where the ORDER of equal
  rank-1-face-regs2    dubins3d (9,65,9), (1,1,8,1)      keys shows (lds 49x17, 119x17; NR = 32, 40, 48 panels; two-row 520x1; tall
  rank-1-face-tall     dubins3d (9,101,33), (1,1,33,1)   3333x1; r_3 <= 7 because the step behind the bond has N_2 = 7 rows)
  control-regs-one-row car7d 11^7, (1,6,6,6,6,6,6,1): interior tuples, full rank, flag 0

Pivot ratios (smallest / largest pivot of a step's LU) by the restated algorithm on the oracle's matrices, both iterations.  A case is
admitted only if every step stays below 1e-14 or above 1e-10; every deficient step of these cases is deficient EXACTLY (ratio 0,
an exact zero pivot), the column "above" is the smallest ratio of a full-rank step:
  case                  deficient steps it 1 / it 2   worst below   worst above   exact zero pivots it 1 / it 2   constant matrices
  square-first-bond              2 / 2                    0.0         4.2e-04              2 / 2                     0 / 0
  face-columns-regs2             2 / 2                    0.0         1.0e-05              3 / 3                     0 / 0
  face-columns-lds               4 / 4                    0.0         1.2e-06             19 / 18                    0 / 0
  global-40-48                   4 / 4                    0.0         1.3e-08             19 / 18                    0 / 0
  global-48                      4 / 4                    0.0         2.7e-08             35 / 34                    0 / 0
  global-32-le32                 2 / 2                    0.0         1.2e-06              3 / 3                     0 / 0
  tall                           2 / 2                    0.0         1.7e-06              3 / 3                     0 / 0
  rank-1-face                    8 / 8                    0.0         5.9e-04             24 / 24                    9 / 9
  all-constant                   1 / 0                    0.0         1.4e-03              3 / 0                     1 / 0
  rank-1-face-lds                8 / 8                    0.0         2.2e-03             88 / 88                    9 / 9
  rank-1-face-global             8 / 8                    0.0         1.5e-03            168 / 168                   9 / 9
  rank-1-face-regs2              2 / 2                    0.0         1.0e+00             14 / 14                    3 / 3
  rank-1-face-tall               2 / 2                    0.0         1.0e+00             64 / 64                    3 / 3
  control-regs-one-row           0 / 0                     --         7.9e-04              0 / 0                     0 / 0
(test_cross_reference.py prints them: the CPU simulation of every case; the device followed the same path on an MI355X, swap
counts included.)

What would fail if a form were wrong (by reading; the CPU self-tests plant both mistakes in the restated algorithm).  Without
the dp != 0 guard the multipliers of an exact zero pivot are x * inf: NaN where x = 0 (every case here has such a column), and the NaN
reaches the core through the substitution -- "not finite" fails; in left-to-right steps the NaN keys (all exponent bits set)
win every later pivot search, rows repeat or leave the matrix, and the bookkeeping or rows_of_set fails.  With the tie order
flipped in one form, a constant matrix gives up its LAST rows there and the tie rule fails: rank-1-face and all-constant for the
one-row register step, rank-1-face-regs2 / -lds / -global / -tall for the two-row, LDS, panel and tall forms (on matrices that are
singular but not constant a flipped order only picks other null rows, which nothing here could tell from the right ones).  Every
form meets an exact zero pivot in a right-to-left step (56x7 one-row, 520x8 two-row, 153x17 LDS, 231x7 / 287x33 / 287x41 panels,
2424x24 tall), so its core would carry the NaN; the confirmation forms share core_step and core_step_global with the
sequential ones and must reproduce their cores bit for bit (NaN never equals NaN).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cross_reference as cr  # noqa: E402
import cross_singular_cases as sc  # noqa: E402
from cross_device_lib import SWAP_TOL, DeviceCross, step_classes  # noqa: E402

pytestmark = pytest.mark.gpu

ALL_CASES = sc.SINGULAR_CASES + [sc.CONTROL_CASE]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_singular_core_steps_against_the_dense_reference(oracle, case):
    """setup, iteration, fetch, check; then the warm-started second iteration (its boost multiplies zeros and noise), checked the
    same way against the first iteration's sets."""
    cid, _, _, ranks, _, want, must_see, must_tie = case
    w, cores, I, J = sc.make_case(case)
    classes = step_classes(w.ngrid, ranks)
    assert want <= set(classes.values()), f"case {cid} reaches {sorted(set(classes.values()))}, meant for {sorted(want)}"
    dev = DeviceCross(w, cores)
    try:
        rc = dev.setup(ranks, I, J)
        assert rc == 0, f"cross_setup: code {rc}: {dev.err()}"
        dev.iteration()
        first = dev.fetch()
        dev.iteration()
        second = dev.fetch()
    finally:
        dev.close()
    P = oracle.Problem(w, cores, consistent_ends=True)
    seen, tied, zeros, flags, stored = set(), set(), 0, [], None
    for t, (I0, J0, got) in enumerate(((I, J, first), (first[1], first[2], second))):
        gcores, gI, gJ, info = got
        print(f"{cid} iteration {t + 1}: info {info}")
        rep = cr.check_iteration(P, ranks, J0, gcores, gI, gJ, info, swap_tol=SWAP_TOL, label=f"{cid} iteration {t + 1}",
                                 allow_deficient=True, I_in=I0, stored=stored)
        stored = rep["stored"]  # the second iteration runs in the same memo epoch: the first one's nodes are hits
        lines, by = sc.summarise(f"{cid} iteration {t + 1}", classes, rep)
        print("\n".join(lines))
        assert not any(s["capped"] for s in rep["steps"]), f"{cid}: the restated algorithm reached the 200-swap cap"
        seen |= {c for c, b in by.items() if b["deficient"]}
        tied |= {c for c, b in by.items() if b["const"]}
        zeros += sum(s["zero_pivots"] for s in rep["steps"])
        flags.append(int(info[1]))
    assert must_see <= seen, f"{cid}: deficient matrices in {sorted(seen)}, meant for {sorted(must_see)}"
    assert must_tie <= tied, f"{cid}: exactly constant matrices in {sorted(tied)}, meant for {sorted(must_tie)}"
    # the table did its job: every deficient case ends with info[1] == 1 and reaches an exactly zero pivot (by the restated
    # algorithm's count on the oracle's matrices), the well-conditioned control ends with info[1] == 0 and reaches none
    control = case is sc.CONTROL_CASE
    assert flags[0] == (0 if control else 1), f"{cid}: info[1] = {flags[0]} after the first iteration"
    assert (zeros == 0) if control else (zeros > 0), f"{cid}: {zeros} exact zero pivots"


# ------------------------------------------------------------------------------------------------ the batched confirmation
@pytest.mark.parametrize("cid,seed", sc.CONFIRM_SEEDS, ids=[c[0] for c in sc.CONFIRM_SEEDS])
def test_batched_confirmation_under_deficiency(oracle, cid, seed):
    """The A / B protocol of test_cross_core_steps.py::test_batched_confirmation_matches_the_sequential_iteration on singular
    matrices (square-first-bond and face-columns-lds confirm in LDS, global-40-48 with k_cross_confirm_g<48>; the control has
    full rank).  After every iteration that changed the sets A confirms and B iterates: confirmed must equal 'B's sets did not
    change', and a confirmed A holds B's cores and sets bit for bit, with the flag the restated algorithm predicts.  A failed
    confirmation is followed by the sequential iteration on A too, and then A's info[0] and info[1] must equal B's: the
    confirm-mode steps count into the same counters[1] and [2] as the real ones, and after a mismatch those counts wait for the
    next fetch -- a failed confirmation, factored against sets that have already changed, must not deliver a deficiency flag
    that no accepted iteration produced."""
    case = sc.by_id(cid)
    ranks = case[3]
    w, cores, I, J = sc.make_case(case, seed=seed)
    A, B = DeviceCross(w, cores), DeviceCross(w, cores)
    P = oracle.Problem(w, cores, consistent_ends=True)
    outcomes = []
    try:
        for dev in (A, B):
            rc = dev.setup(ranks, I, J)
            assert rc == 0, f"cross_setup: code {rc}: {dev.err()}"
            dev.iteration()
        a, b = A.fetch(), B.fetch()
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2]), "A and B differ after the same iteration"
        assert a[3][:3] == b[3][:3], f"A's counters {a[3]} and B's {b[3]} differ after the same iteration"
        prev = b
        for t in range(12):
            confirmed = A.confirm()
            B.iteration()
            b = B.fetch()
            unchanged = _same(b[1], prev[1]) and _same(b[2], prev[2])
            outcomes.append(confirmed)
            assert confirmed == unchanged, f"iteration {t + 2}: confirmed {confirmed}, but the sequential iteration " \
                                           f"{'kept' if unchanged else 'changed'} the index sets"
            if confirmed:
                a = A.fetch()
                for k in range(w.dx):
                    assert np.array_equal(a[0][k], b[0][k]), f"core {k}: confirmed core differs from the sequential one " \
                                                             f"(max {np.abs(a[0][k] - b[0][k]).max():.3e})"
                assert _same(a[1], b[1]) and _same(a[2], b[2]), "confirmed index sets differ from the sequential ones"
                rep = cr.check_iteration(P, ranks, prev[2], b[0], b[1], b[2], None, swap_tol=SWAP_TOL, label=cid,
                                         allow_deficient=True, I_in=prev[1])
                print("\n".join(sc.summarise(cid, step_classes(w.ngrid, ranks), rep)[0]))
                assert rep["flag"] == (0 if case is sc.CONTROL_CASE else 1), f"{cid}: the restated algorithm predicts flag {rep['flag']}"
                assert b[3][1] == rep["flag"], f"the sequential iteration's flag is {b[3][1]}, expected {rep['flag']}"
                assert a[3][1] == rep["flag"], f"the confirmed iteration's flag is {a[3][1]}, expected {rep['flag']}"
                break
            A.iteration()
            a = A.fetch()
            assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2]), "A and B differ after the same iteration"
            print(f"{cid} iteration {t + 2}: after a failed confirmation A's info {a[3]}, B's {b[3]}")
            assert a[3][0] == b[3][0], f"info[0]: A stored {a[3][0]} nodes, B {b[3][0]}"
            assert a[3][1] == b[3][1], f"info[1]: A's flag is {a[3][1]} after a failed confirmation and the iteration, B's {b[3][1]}"
            assert a[3][2] == b[3][2], f"info[2]: A counts {a[3][2]} swaps after a failed confirmation and the iteration, B {b[3][2]}"
            prev = b
        else:
            pytest.fail(f"{cid}: the index sets still change after 12 iterations")
    finally:
        A.close()
        B.close()
    print(f"{cid}: confirmations {outcomes}")
    assert outcomes[0] is False and outcomes[-1] is True, f"{cid}: confirmations {outcomes}"
