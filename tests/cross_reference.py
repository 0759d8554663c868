"""Dense float64 reference for one device-resident cross iteration (c3sc_hip_cross_iteration / _confirm) -- numpy only.

Given the workload, the value cores, the index sets that went into the iteration and the cores, sets and counters that
c3sc_hip_cross_fetch returned, every core step's fiber matrix is rebuilt from the oracle (oracle_lib.Problem(...,
consistent_ends=True).bellman_fibers) and the step is checked with plain linear algebra -- independent of how the kernel
factors (no LU, no pivot keys here: numpy solves).

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


def check_pivots(A, rows, swap_tol, what):
    """Nested, distinct, ascending pivot rows and maxvol dominance max |A inv(A[P])| <= (1 + swap_tol)(1 + 2^-20).
    Returns (dominance, cond(A[P]))."""
    m, n = A.shape
    if len(rows) != n:
        _fail(f"{what}: {len(rows)} pivot rows for {n} columns")
    if len(np.unique(rows)) != n:
        _fail(f"{what}: repeated pivot rows {rows}")
    if np.any(np.diff(rows) <= 0):
        _fail(f"{what}: the set does not list its rows in ascending order")
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


def simulate_iteration(problem, ranks, J_in, swap_tol=0.05):
    """One cross iteration in numpy (maxvol_rows per step) in the layouts above: (cores, I, J).  The 'device' of the
    iteration-level self-test, and a way to see on the CPU whether a case's matrices are well conditioned."""
    w = problem.w
    d, N = w.dx, list(w.ngrid)
    r = [int(v) for v in ranks]
    I = [np.zeros((1, 0), dtype=np.int64)] + [None] * (d - 1)
    J = [_tuples(J_in[k], r[k + 1], d - 1 - k) for k in range(d)]
    cores = [None] * d
    for k in range(d - 1):
        vals, _, _ = problem.bellman_fibers(k, fiber_index_list(d, k, I[k], J[k]))
        rows, _ = maxvol_rows(lr_matrix(vals, r[k], N[k], r[k + 1]), swap_tol)
        I[k + 1] = np.array([list(I[k][q % r[k]]) + [q // r[k]] for q in rows], dtype=np.int64).reshape(r[k + 1], k + 1)
    for k in range(d - 1, 0, -1):
        vals, _, _ = problem.bellman_fibers(k, fiber_index_list(d, k, I[k], J[k]))
        rows, B = maxvol_rows(rl_matrix(vals, r[k], N[k], r[k + 1]), swap_tol)
        J[k - 1] = np.array([[q % N[k]] + list(J[k][q // N[k]]) for q in rows], dtype=np.int64).reshape(r[k], d - k)
        cores[k] = B.ravel()
    vals, _, _ = problem.bellman_fibers(0, fiber_index_list(d, 0, I[0], J[0]))
    cores[0] = vals.ravel().copy()
    return cores, I, J


def _tuples(S, r, length):
    return np.asarray(S, dtype=np.int64).reshape(r, length)


def check_iteration(problem, ranks, J_in, cores, I_out, J_out, info, swap_tol=0.05, label=""):
    """Check one finished cross iteration against the dense reference.  problem: oracle_lib.Problem(w, value_cores,
    consistent_ends=True); ranks: the cross ranks (d+1); J_in: the right index sets the iteration started from; cores, I_out,
    J_out, info: what c3sc_hip_cross_fetch returned.  Returns a report: per step (direction, k, m, n, residual, dominance, cond)."""
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
        dom, cond = check_pivots(A, rows, swap_tol, what)
        B = np.asarray(cores[k], dtype=np.float64).reshape(N[k] * r[k + 1], r[k])
        res = check_interpolatory(A, rows, B, what)
        report.append(dict(dir="rl", k=k, m=A.shape[0], n=A.shape[1], residual=res, dominance=dom, cond=cond))
    vals0 = values(0, I[0], Jn[0])
    raw = float(np.abs(np.asarray(cores[0], dtype=np.float64).ravel() - vals0.ravel()).max() / np.abs(vals0).max())
    if not raw <= RAW_TOL:
        _fail(f"{label} core 0 differs from the oracle's fiber values by {raw:.3e} of the value scale")
    # info[0]: nodes stored in the memo during the iteration -- with a fresh epoch every distinct node of the 2 d fiber lists is
    # stored exactly once (a repeat is a hit; one batch never holds a node twice: distinct tuples, one varying dimension)
    distinct = len(np.unique(np.concatenate(node_ids)))
    if info is None:  # a numpy iteration (simulate_iteration) has no counters
        return dict(steps=report, raw=raw, nodes=distinct)
    if int(info[0]) != distinct:
        _fail(f"{label} info[0] = {int(info[0])} nodes stored, the fiber lists hold {distinct} distinct nodes")
    if int(info[1]) != 0:
        _fail(f"{label} info[1] = {int(info[1])}: a factorisation was flagged rank deficient")
    return dict(steps=report, raw=raw, nodes=distinct)
