"""Dense float64 reference for one device-resident cross iteration (c3sc_hip_cross_iteration / _confirm) -- numpy only.

Given the workload, the value cores, the index sets that went into the iteration and the cores, sets and counters that
c3sc_hip_cross_fetch returned, every core step's fiber matrix is rebuilt from the oracle (oracle_lib.Problem(...,
consistent_ends=True).bellman_fibers) and the step is checked with plain linear algebra -- independent of how the kernel
factors (the checks use no LU and no pivot keys: numpy solves; lu_maxvol_reference, which restates the algorithm, only predicts
the deficiency flag and serves the self-tests as the 'device').

Index sets follow the C-ABI (include/c3sc_hip.h): I[k] holds r_k tuples over dims 0..k-1, J[k] holds r_{k+1} tuples over dims
k+1..d-1; fiber f = a + r_k b of core step k is (I[k][a], *, J[k][b]).  Layouts (cross_device.hip: core_step,
write_sets_and_next):
  left-to-right step k < d-1: rows i = a + r_k j over I[k] x grid_k, columns b over the INPUT J[k]; the new I[k+1] lists the
      pivot rows in ascending order as the tuples (I[k][a], j).
  right-to-left step k >= 1: rows i = j + N_k b over grid_k x J[k] (the new one: step k+1 wrote it), columns a over I[k] (new);
      the new J[k-1] lists the pivot rows in ascending order as (j, J[k][b]).  The core is B = G_k.reshape(N_k r_{k+1}, r_k)
      (G_k[a + r_k (j + N_k b)]), and column c of B belongs to J[k-1][c].
  core 0 (copy step): the raw fiber values on grid_0 x J[0].
The left-to-right step d-1 only evaluates the list I[d-1] x J[d-1] that the right-to-left step d-1 then factors.

Rank-deficient matrices (check_iteration(..., allow_deficient=True)).  The production solve factors exactly singular matrices in
every sweep (a square first bond on an absorbing dimension has two equal rows, index tuples on absorbing faces give equal
constant columns), so inv(A[P]) does not exist and cond(A[P]) says nothing.  In that mode every step is held to what survives:
nested, distinct, ascending, in-range sets; rows that span the matrix (A pinv(A[P]) A[P] = A with the project's own 1e-12
cut-off); for right-to-left steps a finite, interpolatory core whose OWN largest entry meets maxvol's termination bound; the
deficiency flag info[1] that lu_maxvol_reference -- a plain restatement of the algorithm as c3sc_cross.c defines it -- predicts on
the oracle's matrices; and on an exactly constant matrix the rows that the tie rule (lower index first) dictates: 0 .. n-1 if no row is warm.
NOT asserted there: dominance of deficient left-to-right steps (they return no core to bound, and A inv(A[P]) does not exist),
and WHICH rows are picked in noise directions (the pivot is chosen among roundings that differ between the oracle and the device).
"""
from __future__ import annotations

import numpy as np

DOMINANCE_SLACK = 1.0 + 2.0 ** -20  # the pivot keys drop 22 mantissa bits: an entry a hair above 1 + swap_tol may stand
RESIDUAL_TOL = 1e-10
# B[P] is the identity to the last bit, except where maxvol swapped a row in at a NEGATIVE pivot p < -1: the swap subtracts
# 1 * (B[i] - e_j) from the row, and its pivot entry p - (p - 1) carries the rounding of p - 1 (|p - 1| > |p| gains an exponent) --
# one ulp of 1.  The host twin (lu_maxvol) does the same, bit for bit.
IDENTITY_TOL = 2.0 ** -51
RAW_TOL = 1e-12
DEFICIENT_RATIO = 1e-12  # lu_maxvol / k_cross_core: a factorisation is flagged when its smallest pivot is <= 1e-12 of the largest
# a case is admitted to the deficient mode only if every step's pivot ratio stays two decades clear of that threshold on either
# side: the device's fiber values differ from the oracle's by up to 1e-12 of the scale, so a ratio in between could flip the flag
ADMIT_BELOW, ADMIT_ABOVE = 1e-14, 1e-10
PIV_IDX_BITS = 22        # c3sc_cross.c: mantissa bits dropped from the pivot key (their place holds the inverted index)
WARM_BOOST = 64.0        # c3sc_cross.c: 2^WARM_BOOST_LOG2
MAXVOL_CAP = 200         # c3sc_cross.c: at most 200 swaps


class CrossCheckError(AssertionError):
    pass


def _fail(msg):
    raise CrossCheckError(msg)


# ------------------------------------------------------------------------------------------------ step level
def lr_matrix(vals, r0, N, r1):
    """fiber values vals[f = a + r0 b, j] -> A[a + r0 j, b]"""
    return np.ascontiguousarray(vals.reshape(r1, r0, N).transpose(2, 1, 0).reshape(N * r0, r1))


def rl_matrix(vals, r0, N, r1):
    """fiber values vals[f = a + r0 b, j] -> A[j + N b, a]"""
    return np.ascontiguousarray(vals.reshape(r1, r0, N).transpose(0, 2, 1).reshape(r1 * N, r0))


def rows_of_set(new_set, prefix_set, N, side):
    """Rows of a step's matrix named by the tuples of the set it produced.  side 'lr': tuples (prefix_set[a], j) -> a + r0 j;
    side 'rl': tuples (j, prefix_set[b]) -> j + N b.  Raises if a tuple is not a row (the set is not nested)."""
    new_set = np.asarray(new_set, dtype=np.int64).reshape(len(new_set), -1)
    prefix_set = np.asarray(prefix_set, dtype=np.int64).reshape(len(prefix_set), -1)
    lookup = {tuple(t): a for a, t in enumerate(prefix_set)}
    if len(lookup) != len(prefix_set):
        _fail("the input index set has repeated tuples")
    rows = []
    for t in new_set:
        t = tuple(int(v) for v in t)
        head, j = (t[:-1], t[-1]) if side == "lr" else (t[1:], t[0])
        if head not in lookup or not 0 <= j < N:
            _fail(f"index tuple {t} is not a row of the step's matrix (not nested in the input set)")
        a = lookup[head]
        rows.append(a + len(prefix_set) * j if side == "lr" else j + N * a)
    return np.array(rows, dtype=np.int64)


def check_row_bookkeeping(A, rows, what):
    """One pivot row per column, all rows of the matrix, distinct, in ascending order."""
    m, n = A.shape
    if len(rows) != n:
        _fail(f"{what}: {len(rows)} pivot rows for {n} columns")
    if len(rows) and (int(np.min(rows)) < 0 or int(np.max(rows)) >= m):
        _fail(f"{what}: pivot rows {rows} outside the matrix ({m} rows)")
    if len(np.unique(rows)) != n:
        _fail(f"{what}: repeated pivot rows {rows}")
    if np.any(np.diff(rows) <= 0):
        _fail(f"{what}: the set does not list its rows in ascending order")


def check_pivots(A, rows, swap_tol, what):
    """Nested, distinct, ascending pivot rows and maxvol dominance max |A inv(A[P])| <= (1 + swap_tol)(1 + 2^-20).
    Returns (dominance, cond(A[P]))."""
    check_row_bookkeeping(A, rows, what)
    AP = A[rows]
    cond = float(np.linalg.cond(AP))
    if not np.isfinite(cond) or cond > 1e12:
        _fail(f"{what}: A[P] is singular (cond {cond:.3e})")
    Bref = np.linalg.solve(AP.T, A.T).T  # A inv(A[P])
    dom = float(np.abs(Bref).max())
    if not dom <= (1.0 + swap_tol) * DOMINANCE_SLACK:
        _fail(f"{what}: not dominant, max |A inv(A[P])| = {dom:.9f} > 1 + {swap_tol}")
    return dom, cond


def check_interpolatory(A, rows, B, what):
    """B[P] == identity (to IDENTITY_TOL) and ||B A[P] - A||_max <= 1e-10 ||A||_max.  Returns the relative residual."""
    n = A.shape[1]
    if B.shape != A.shape:
        _fail(f"{what}: core of shape {B.shape} for a matrix {A.shape}")
    dev = float(np.abs(B[rows] - np.eye(n)).max())
    if not dev <= IDENTITY_TOL:
        _fail(f"{what}: the core is not the identity on the pivot rows (max dev {dev:.3e})")
    res = float(np.abs(B @ A[rows] - A).max() / np.abs(A).max())
    if not res <= RESIDUAL_TOL:
        _fail(f"{what}: the core does not interpolate: ||B A[P] - A|| / ||A|| = {res:.3e}")
    return res


def maxvol_rows(A, swap_tol=0.05, maxit=200):
    """A plain pivoted-LU start + maxvol in numpy (the checker's self-tests and the choice of well-conditioned cases use it as
    the 'device'): pivot rows in ascending order and B = A inv(A[P]) in that column order."""
    m, n = A.shape
    W = A.copy()
    piv = []
    for c in range(n):
        cand = np.abs(W[:, c]).copy()
        cand[piv] = -1.0
        p = int(np.argmax(cand))
        piv.append(p)
        if W[p, c] != 0.0:
            W -= np.outer(W[:, c] / W[p, c], W[p])
    piv = np.array(piv)
    B = np.linalg.solve(A[piv].T, A.T).T
    for _ in range(maxit):
        i, j = np.unravel_index(np.argmax(np.abs(B)), B.shape)
        if abs(B[i, j]) <= 1.0 + swap_tol:
            break
        piv[j] = i
        B = np.linalg.solve(A[piv].T, A.T).T
    order = np.argsort(piv)
    rows = piv[order]
    B = B[:, order]
    B[rows] = np.eye(n)
    return rows, B


# ------------------------------------------------------------------------------------------------ any rank
def _residual(R, A):
    """max |R| relative to max |A|; an all-zero A must be met exactly (0 <= 0 passes, nothing is divided by zero)"""
    scale = float(np.abs(A).max()) if A.size else 0.0
    res = float(np.abs(R).max()) if R.size else 0.0
    if not np.isfinite(res):
        return np.inf
    return res / scale if scale > 0.0 else (0.0 if res == 0.0 else np.inf)


def check_span(A, rows, what):
    """The chosen rows span the matrix: with X = A pinv(A[P], rcond=1e-12), max |X A[P] - A| <= RESIDUAL_TOL max |A|.  Holds in
    exact arithmetic at every rank (A = L U, and the pivot rows carry all of U); replaces cond(A[P]).  Returns the residual.
    X A[P] = A V V^T with V the right singular vectors of A[P] above the cut-off, and it is evaluated in that form: the product
    through the explicit pseudo-inverse loses eps cond(kept part) -- 4.5e-9 on a 49 x 33 fiber matrix of 25 significant
    directions down to 4e-10 whose exact core leaves B A[P] - A = 0 -- which is the reference's error, not the rows'."""
    AP = A[rows]
    _, sv, Vt = np.linalg.svd(AP, full_matrices=False)
    V = Vt[sv > DEFICIENT_RATIO * sv[0]].T if sv.size and sv[0] > 0.0 else np.zeros((A.shape[1], 0))
    res = _residual((A @ V) @ V.T - A, A)
    if not res <= RESIDUAL_TOL:
        _fail(f"{what}: the chosen rows do not span the matrix: ||A pinv(A[P]) A[P] - A|| / ||A|| = {res:.3e}")
    return res


def check_core_any_rank(A, rows, B, swap_tol, what):
    """A right-to-left step's core at any rank: finite, the identity on the pivot rows, interpolatory, and dominant by its OWN
    entries, max |B| <= (1 + swap_tol)(1 + 2^-20) -- maxvol's termination condition (inv(A[P]) need not exist).
    Returns (residual, max |B|)."""
    n = A.shape[1]
    if B.shape != A.shape:
        _fail(f"{what}: core of shape {B.shape} for a matrix {A.shape}")
    if not np.all(np.isfinite(B)):
        _fail(f"{what}: the core holds {int(np.sum(~np.isfinite(B)))} entries that are not finite")
    dev = float(np.abs(B[rows] - np.eye(n)).max())
    if not dev <= IDENTITY_TOL:
        _fail(f"{what}: the core is not the identity on the pivot rows (max dev {dev:.3e})")
    res = _residual(B @ A[rows] - A, A)
    if not res <= RESIDUAL_TOL:
        _fail(f"{what}: the core does not interpolate: ||B A[P] - A|| / ||A|| = {res:.3e}")
    big = float(np.abs(B).max())
    if not big <= (1.0 + swap_tol) * DOMINANCE_SLACK:
        _fail(f"{what}: not dominant, max |B| = {big:.9f} > 1 + {swap_tol}")
    return res, big


def is_constant(A):
    return bool(A.size) and bool(np.all(A == A.flat[0]))


def check_tie_rule(A, rows, warm, what):
    """On an exactly constant matrix every pivot key of a column ties, nothing is noise (the constant is Model::boundcost on the
    device and in the oracle alike), and the definition leaves no choice: the first pivot is the lowest warm row -- its magnitude
    is boosted -- or row 0 if none is warm; that elimination leaves exact zeros (c * (1 / c) == 1.0 for the boundcosts 10, 100,
    1000), 64 * 0 ties with 0, and every later pivot is the lowest unused row.  Without warm rows that is 0 .. n-1.  The set must
    name exactly these rows."""
    if not is_constant(A):
        return
    n = A.shape[1]
    first = int(np.flatnonzero(warm)[0]) if (warm is not None and np.any(warm) and A.flat[0] != 0.0) else 0
    want = np.sort(np.array([first] + [i for i in range(n) if i != first][: n - 1], dtype=np.int64))
    if not np.array_equal(np.asarray(rows, dtype=np.int64), want):
        _fail(f"{what}: the matrix is exactly constant ({float(A.flat[0])!r}), ties go to the lower index: rows {want} expected, got {rows}")


def _pivot_keys(x, index):
    bits = np.abs(np.asarray(x, dtype=np.float64)).view(np.uint64)
    sh, mask = np.uint64(PIV_IDX_BITS), np.uint64((1 << PIV_IDX_BITS) - 1)
    return ((bits >> sh) << sh) | (mask - index.astype(np.uint64))


class LuMaxvol:
    """What lu_maxvol_reference returns: rows (ascending), B in that column order, ratio = smallest / largest pivot magnitude
    of the LU (0.0 for an all-zero matrix), zero_pivots = pivots that were exactly 0.0, swaps, capped = the 200-swap cap was reached."""

    def __init__(self, rows, B, ratio, zero_pivots, swaps, capped):
        self.rows, self.B, self.ratio, self.zero_pivots, self.swaps, self.capped = rows, B, ratio, zero_pivots, swaps, capped

    @property
    def flag(self):
        return int(self.ratio <= DEFICIENT_RATIO)


def lu_maxvol_reference(A, swap_tol=0.05, warm=None, guard_zero_pivot=True, lower_index_first=True):
    """The algorithm of lu_maxvol (c3sc_cross.c) restated in numpy, same operations in the same order: tall LU with row pivoting,
    the pivot the largest key among unused rows (magnitude with 22 mantissa bits dropped, then the LOWER index; warm rows' magnitudes
    times 64), inv = 0 on a zero pivot, B = L inv(L[rows]) by substitution, maxvol swaps while max |B| > 1 + swap_tol (at most 200),
    rows in ascending order.  guard_zero_pivot=False and lower_index_first=False are the two mistakes the negative tests plant:
    1 / 0 on a zero pivot, and ties to the HIGHER index."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    assert m >= n and m * n <= (1 << PIV_IDX_BITS) - 1
    W = np.array(A, order="F")
    warm = np.zeros(m, dtype=bool) if warm is None else np.asarray(warm, dtype=bool)
    used = np.zeros(m, dtype=bool)
    rows = np.zeros(n, dtype=np.int64)
    pivabs = np.zeros(n)

    def order(count):
        idx = np.arange(count, dtype=np.int64)
        return idx if lower_index_first else count - 1 - idx

    ridx = order(m)
    with np.errstate(all="ignore"):
        for kc in range(n):
            ak = W[:, kc]
            keys = _pivot_keys(np.where(warm, ak * WARM_BOOST, ak), ridx)
            keys[used] = 0
            p = int(np.argmax(keys))
            dp = ak[p]
            rows[kc], pivabs[kc] = p, abs(dp)
            used[p] = True
            inv = 1.0 / dp if (dp != 0.0 or not guard_zero_pivot) else 0.0
            free = ~used
            colv = ak[free] * inv
            W[free, kc] = colv
            if kc + 1 < n:
                W[free, kc + 1:] -= np.outer(colv, W[p, kc + 1:])
        Lr = np.eye(n)
        for q in range(n):
            Lr[q, :q] = W[rows[q], :q]
        free = ~used
        for j in range(n - 1, -1, -1):
            for t in range(j + 1, n):
                W[free, j] -= W[free, t] * Lr[t, j]
        W[rows] = np.eye(n)
        cidx = order(m * n)
        swaps = 0
        for _ in range(MAXVOL_CAP):
            lin = int(np.argmax(_pivot_keys(W.ravel(order="F"), cidx)))
            bj, bi = divmod(lin, m)
            piv = W[bi, bj]
            if not abs(piv) > 1.0 + swap_tol:
                break
            rowv = W[bi].copy()
            rowv[bj] -= 1.0
            W -= np.outer(W[:, bj] / piv, rowv)
            rows[bj] = bi
            swaps += 1
    perm = np.argsort(rows, kind="stable")
    mx, mn = float(pivabs.max()), float(pivabs.min())
    ratio = mn / mx if mx > 0.0 else 0.0
    return LuMaxvol(rows[perm], np.ascontiguousarray(W[:, perm]), ratio, int(np.sum(pivabs == 0.0)), swaps, swaps == MAXVOL_CAP)


def warm_rows(old_set, prefix_set, N, side, m):
    """Rows named by the previous index set, matched through the current tuples of the neighbouring set (first match), as
    cross_sweep_lr / cross_sweep_rl and mark_warm_rows do: tuples that are no rows any more are skipped."""
    warm = np.zeros(m, dtype=bool)
    if old_set is None:
        return warm
    prefix_set = np.asarray(prefix_set, dtype=np.int64).reshape(len(prefix_set), -1)
    old_set = np.asarray(old_set, dtype=np.int64).reshape(-1, prefix_set.shape[1] + 1)
    lookup = {}
    for a, t in enumerate(prefix_set):
        lookup.setdefault(tuple(int(v) for v in t), a)
    for t in old_set:
        t = tuple(int(v) for v in t)
        head, j = (t[:-1], t[-1]) if side == "lr" else (t[1:], t[0])
        if head in lookup and 0 <= j < N:
            warm[lookup[head] + len(prefix_set) * j if side == "lr" else j + N * lookup[head]] = True
    return warm


# ------------------------------------------------------------------------------------------------ iteration level
def fiber_index_list(d, k, Ik, Jk):
    r0, r1 = len(Ik), len(Jk)
    idx = np.zeros((r0 * r1, d), dtype=np.int32)
    for b in range(r1):
        for a in range(r0):
            f = a + r0 * b
            idx[f, :k] = Ik[a]
            idx[f, k + 1:] = Jk[b]
    return idx


def simulate_iteration(problem, ranks, J_in, swap_tol=0.05, restatement=False, I_in=None, ratios=None):
    """One cross iteration in numpy in the layouts above: (cores, I, J).  The 'device' of the iteration-level self-tests, and a
    way to see on the CPU whether a case's matrices are well conditioned.  Every step is maxvol_rows, or with restatement=True
    lu_maxvol_reference with the warm rows of the previous sets (I_in: the left sets before the iteration, or None); a list
    given as `ratios` then receives every step's pivot ratio (what the deficiency flag is made of).  The fiber lists are asked
    of `problem` in the device's order of core steps, so a problem that keeps a memo (cross_memo_model.MemoProblem) sees the
    nodes in the order the device's memo does."""
    w = problem.w
    d, N = w.dx, list(w.ngrid)
    r = [int(v) for v in ranks]
    I = [np.zeros((1, 0), dtype=np.int64)] + [None] * (d - 1)
    J = [_tuples(J_in[k], r[k + 1], d - 1 - k) for k in range(d)]
    cores = [None] * d

    def factor(A, old_set, prefix_set, Nk, side):
        if not restatement:
            return maxvol_rows(A, swap_tol)
        f = lu_maxvol_reference(A, swap_tol, warm_rows(old_set, prefix_set, Nk, side, A.shape[0]))
        if ratios is not None:
            ratios.append(f.ratio)
        return f.rows, f.B

    for k in range(d - 1):
        vals, _, _ = problem.bellman_fibers(k, fiber_index_list(d, k, I[k], J[k]))
        rows, _ = factor(lr_matrix(vals, r[k], N[k], r[k + 1]), None if I_in is None else I_in[k + 1], I[k], N[k], "lr")
        I[k + 1] = np.array([list(I[k][q % r[k]]) + [q // r[k]] for q in rows], dtype=np.int64).reshape(r[k + 1], k + 1)
    for k in range(d - 1, 0, -1):
        vals, _, _ = problem.bellman_fibers(k, fiber_index_list(d, k, I[k], J[k]))
        rows, B = factor(rl_matrix(vals, r[k], N[k], r[k + 1]), J[k - 1], J[k], N[k], "rl")
        J[k - 1] = np.array([[q % N[k]] + list(J[k][q // N[k]]) for q in rows], dtype=np.int64).reshape(r[k], d - k)
        cores[k] = B.ravel()
    vals, _, _ = problem.bellman_fibers(0, fiber_index_list(d, 0, I[0], J[0]))
    cores[0] = vals.ravel().copy()
    return cores, I, J


def _tuples(S, r, length):
    return np.asarray(S, dtype=np.int64).reshape(r, length)


def check_iteration(problem, ranks, J_in, cores, I_out, J_out, info, swap_tol=0.05, label="", allow_deficient=False, I_in=None, stored=None):
    """Check one finished cross iteration against the dense reference.  problem: oracle_lib.Problem(w, value_cores,
    consistent_ends=True); ranks: the cross ranks (d+1); J_in: the right index sets the iteration started from; cores, I_out,
    J_out, info: what c3sc_hip_cross_fetch returned.  Returns a report: per step (direction, k, m, n, residual, dominance, cond).

    allow_deficient=True drops cond(A[P]) <= 1e12 and info[1] == 0 (see the module docstring) and asserts instead, per step:
    the set bookkeeping as before; check_span; for right-to-left steps check_core_any_rank; check_tie_rule; and over the
    iteration info[1] == OR of (ratio <= 1e-12), the ratio being lu_maxvol_reference's on the oracle's matrix of the device's own
    path (I_in: the left sets before the iteration, for the warm rows; None: none were warm).  A step whose ratio lies in
    [1e-14, 1e-10] is refused: the case is too close to the threshold to predict the flag.  No dominance is asserted on
    left-to-right steps in this mode -- they return no core to bound -- and the device's rows are not compared with the
    restatement's.  The report then holds per step (direction, k, m, n, span, residual, maxB, ratio, zero_pivots, constant, swaps,
    capped) and the expected flag.

    stored: the node ids the memo already holds (an earlier iteration of the same epoch: the "stored" entry of its report); they
    are hits now, and info[0] counts the distinct nodes of this iteration that are not among them."""
    w = problem.w
    d, N = w.dx, list(w.ngrid)
    r = [int(v) for v in ranks]
    I = [_tuples(I_out[k], r[k], k) for k in range(d)]
    Jn = [_tuples(J_out[k], r[k + 1], d - 1 - k) for k in range(d)]
    Ji = [_tuples(J_in[k], r[k + 1], d - 1 - k) for k in range(d)]
    strides = np.ones(d, dtype=np.int64)
    for m in range(d - 2, -1, -1):
        strides[m] = strides[m + 1] * N[m + 1]
    cache, node_ids, report = {}, [], []

    def any_rank_step(side, k, A, rows, B, warm, what):
        check_row_bookkeeping(A, rows, what)
        span = check_span(A, rows, what)
        res, big = check_core_any_rank(A, rows, B, swap_tol, what) if B is not None else (None, None)
        check_tie_rule(A, rows, warm, what)
        f = lu_maxvol_reference(A, swap_tol, warm)
        if ADMIT_BELOW <= f.ratio <= ADMIT_ABOVE:
            _fail(f"{what}: pivot ratio {f.ratio:.3e} is within two decades of the deficiency threshold: the case is not admitted")
        return dict(dir=side, k=k, m=A.shape[0], n=A.shape[1], span=span, residual=res, maxB=big, ratio=f.ratio,
                    zero_pivots=f.zero_pivots, constant=is_constant(A), swaps=f.swaps, capped=f.capped)

    def values(k, Ik, Jk):
        key = (k, Ik.tobytes(), Jk.tobytes())
        if key not in cache:
            out, _, _ = problem.bellman_fibers(k, fiber_index_list(d, k, Ik, Jk))
            cache[key] = out
            pre = Ik @ strides[:k] if k else np.zeros(1, dtype=np.int64)
            suf = Jk @ strides[k + 1:] if k < d - 1 else np.zeros(1, dtype=np.int64)
            node_ids.append(np.add.outer(np.add.outer(suf, np.arange(N[k], dtype=np.int64) * strides[k]), pre).ravel())
        return cache[key]

    for k in range(d):  # left-to-right half sweep
        vals = values(k, I[k], Ji[k])
        if k == d - 1:
            continue
        what = f"{label} left-to-right step {k}"
        A = lr_matrix(vals, r[k], N[k], r[k + 1])
        new = I[k + 1]
        if len(np.unique(new, axis=0)) != len(new):
            _fail(f"{what}: the new set I[{k + 1}] repeats a tuple")
        rows = rows_of_set(new, I[k] if k else np.zeros((1, 0)), N[k], "lr")
        if allow_deficient:
            old = None if I_in is None else _tuples(I_in[k + 1], r[k + 1], k + 1)
            report.append(any_rank_step("lr", k, A, rows, None, warm_rows(old, I[k], N[k], "lr", A.shape[0]), what))
            continue
        dom, cond = check_pivots(A, rows, swap_tol, what)
        report.append(dict(dir="lr", k=k, m=A.shape[0], n=A.shape[1], residual=None, dominance=dom, cond=cond))
    for k in range(d - 1, 0, -1):  # right-to-left half sweep
        what = f"{label} right-to-left step {k}"
        vals = values(k, I[k], Jn[k])
        A = rl_matrix(vals, r[k], N[k], r[k + 1])
        new = Jn[k - 1]
        if len(np.unique(new, axis=0)) != len(new):
            _fail(f"{what}: the new set J[{k - 1}] repeats a tuple")
        rows = rows_of_set(new, Jn[k] if k < d - 1 else np.zeros((1, 0)), N[k], "rl")
        B = np.asarray(cores[k], dtype=np.float64).reshape(N[k] * r[k + 1], r[k])
        if allow_deficient:
            report.append(any_rank_step("rl", k, A, rows, B, warm_rows(Ji[k - 1], Jn[k], N[k], "rl", A.shape[0]), what))
            continue
        dom, cond = check_pivots(A, rows, swap_tol, what)
        res = check_interpolatory(A, rows, B, what)
        report.append(dict(dir="rl", k=k, m=A.shape[0], n=A.shape[1], residual=res, dominance=dom, cond=cond))
    vals0 = values(0, I[0], Jn[0])
    raw = float(np.abs(np.asarray(cores[0], dtype=np.float64).ravel() - vals0.ravel()).max() / np.abs(vals0).max())
    if not raw <= RAW_TOL:
        _fail(f"{label} core 0 differs from the oracle's fiber values by {raw:.3e} of the value scale")
    # info[0]: nodes stored in the memo during the iteration -- with a fresh epoch every distinct node of the 2 d fiber lists is
    # stored exactly once (a repeat is a hit; one batch never holds a node twice: distinct tuples, one varying dimension)
    ids = np.unique(np.concatenate(node_ids))
    distinct = len(ids) if stored is None else len(np.setdiff1d(ids, stored, assume_unique=True))
    all_stored = ids if stored is None else np.union1d(ids, stored)
    flag = int(any(s["ratio"] <= DEFICIENT_RATIO for s in report)) if allow_deficient else 0
    if info is None:  # a numpy iteration (simulate_iteration) has no counters
        return dict(steps=report, raw=raw, nodes=distinct, flag=flag, stored=all_stored)
    if int(info[0]) != distinct:
        _fail(f"{label} info[0] = {int(info[0])} nodes stored, the fiber lists hold {distinct} distinct nodes")
    if allow_deficient:
        if int(info[1]) != flag:
            worst = min(s["ratio"] for s in report)
            _fail(f"{label} info[1] = {int(info[1])}, but the smallest pivot ratio of the iteration is {worst:.3e}: flag {flag} expected")
    elif int(info[1]) != 0:
        _fail(f"{label} info[1] = {int(info[1])}: a factorisation was flagged rank deficient")
    return dict(steps=report, raw=raw, nodes=distinct, flag=flag, stored=all_stored)
