"""Reference model of the fiber partition pre-pass (c3sc_amd/csrc/fiber_partition.hpp), in numpy: which key dimensions a launch
groups by (fpart_plan on top of kernel_common.hpp's fpp_group_levels), the permutation it must produce (a STABLE sort: live fibers
first by (major, minor) key, batch order inside a key, dead fibers last in batch order), a checker that names the property a
permutation breaks, and seeded batch builders for the block and scan arithmetic of the three kernels.

A helper module for tests/test_fiber_partition_ref.py (CPU: the checker against planted mistakes, `plan` against the C++) and
tests/test_gpu_fiber_partition.py (the device pass against `reference_perm` beyond one block)."""
import numpy as np

from c3sc_amd import workloads as wl

FPART_BLOCK = 1024       # fibers per block of the count and the scatter
FPART_MAX_BINS = 2048    # keys + the dead bin
FPART_MIN_PER_BIN = 128  # the default floor: mean fibers per bin below which a key level is dropped
FPP_DIRECT_MAXD = 3      # kernel_common.hpp: the direct-fold kernels (d <= 3 at padded ranks <= 8) stage nothing
OPTOUT = {(7, 10, 1)}    # kernel_common.hpp: fpp_group_fold_optout -- (d, padded rank, K)


def key_levels(d, k, tab=True):
    """kernel_common.hpp: fpp_key_levels -- the key dimensions, major first"""
    lfirst = 2 if (tab and k >= 2) else 1
    rfirst = d - 3 if (tab and k <= d - 3) else d - 2
    nl, nr = max(k - lfirst, 0), max(rfirst - k, 0)
    if nl and nr:
        return [k - 1, k + 1]
    if nl:
        return [k - 1, k - 2][:min(nl, 2)]
    if nr:
        return [k + 1, k + 2][:min(nr, 2)]
    return []


def group_levels(d, rp, k):
    """kernel_common.hpp: fpp_group_levels -- none for the direct-fold kernels and the opt-outs"""
    if (d <= FPP_DIRECT_MAXD and rp <= 8) or (d, rp, k) in OPTOUT:
        return []
    return key_levels(d, k, tab=d >= 4)


def floor_of(env):
    """the floor C3SC_FIBER_GROUP stands for (c3sc_hip.hip: fiber_group_floor): unset -> 128, "0" -> no grouping (< 0), n -> n"""
    if env is None or env == "":
        return FPART_MIN_PER_BIN
    v = int(env)
    return v if v > 0 else -1


def plan_grid(d, ngrid, k, rp, F, floor):
    """fpart_plan for the grid `ngrid` of d dimensions: (key dimensions in use, major first; nbins)"""
    kl = group_levels(d, rp, k)
    if floor < 0 or not kl:
        return [], 2
    nmaj = ngrid[kl[0]]
    if nmaj + 1 > FPART_MAX_BINS or F < floor * nmaj:
        return [], 2
    if len(kl) < 2:
        return kl[:1], nmaj + 1
    nkeys = nmaj * ngrid[kl[1]]
    if nkeys + 1 > FPART_MAX_BINS or F < floor * nkeys:
        return kl[:1], nmaj + 1
    return kl, nkeys + 1


def plan(w, k, rp, F, floor):
    """the key dimensions a launch of F fibers of workload w along K = k groups by at padded rank rp, and its number of bins"""
    return plan_grid(w.dx, w.ngrid, k, rp, F, floor)


def dead_mask(w, k, idx):
    """fiber_dead: a fixed index on a face of an absorbing dimension other than k"""
    dead = np.zeros(idx.shape[0], dtype=bool)
    for m in range(w.dx):
        if m != k and w.bc[m] == wl.BC_ABSORB:
            dead |= (idx[:, m] == 0) | (idx[:, m] == w.ngrid[m] - 1)
    return dead


def fiber_keys(w, idx, keys):
    """the bin of every fiber were it live: major * N_minor + minor (0 without keys)"""
    key = np.zeros(idx.shape[0], dtype=np.int64)
    for m in keys:
        key = key * w.ngrid[m] + idx[:, m]
    return key


def reference_perm(w, k, idx, keys):
    """(perm, nlive): a numpy stable sort of the live fibers by (major, minor), the dead ones behind them in batch order"""
    dead = dead_mask(w, k, idx)
    live = np.flatnonzero(~dead)
    key = fiber_keys(w, idx, keys)
    perm = np.concatenate([live[np.argsort(key[live], kind="stable")], np.flatnonzero(dead)]).astype(np.int32)
    return perm, int(live.size)


def check_partition(w, k, idx, perm, nlive, keys):
    """Raises AssertionError naming the property of fiber_partition.hpp's order that (perm, nlive) breaks; `keys`: the key
    dimensions in use, major first (empty: the plain partition).  Ends with exact equality to reference_perm."""
    F = idx.shape[0]
    perm = np.asarray(perm)
    assert perm.shape == (F,), f"perm has one entry per fiber: shape {perm.shape}, the batch has {F} fibers"
    seen = np.bincount(perm[(perm >= 0) & (perm < F)], minlength=F)
    assert (perm >= 0).all() and (perm < F).all() and (seen == 1).all(), \
        f"perm is a bijection: {int((seen == 0).sum())} fibers missing, {int((seen > 1).sum())} more than once"
    dead = dead_mask(w, k, idx)
    want_nlive = int((~dead).sum())
    assert nlive == want_nlive, f"nlive is right: {nlive}, the batch has {want_nlive} live fibers"
    pd = dead[perm]
    assert not pd[:nlive].any() and pd[nlive:].all(), \
        f"live fibers come first: {int(pd[:nlive].sum())} dead fibers in front of nlive, {int((~pd[nlive:]).sum())} live ones behind"
    lp = perm[:nlive].astype(np.int64)
    lk = fiber_keys(w, idx, keys)[lp]
    down = np.flatnonzero(lk[1:] < lk[:-1])
    assert down.size == 0, f"keys ascend, major then minor: {down.size} descents, the first at position {down[:1]}"
    back = np.flatnonzero((lk[1:] == lk[:-1]) & (lp[1:] < lp[:-1]))
    assert back.size == 0, f"batch order holds inside a key: {back.size} inversions, the first at position {back[:1]}"
    dp = perm[nlive:]
    assert (dp[1:] > dp[:-1]).all(), f"dead fibers are in batch order: {int((dp[1:] <= dp[:-1]).sum())} inversions"
    want, _ = reference_perm(w, k, idx, keys)
    diff = np.flatnonzero(perm != want)
    assert diff.size == 0, f"perm equals the reference permutation: {diff.size} positions differ, the first at {diff[:1]}"


# ---- batches

def car7d_grid(k, nkey=(41, 41), nk=6, n=5):
    """car7d at rank 10 with N = nkey in the two key dimensions of K = k (major, minor -- the geometric levels, also for the
    opted-out K = 1), N_K = nk and n elsewhere: the benchmark's 41 x 41 + 1 bins with short fibers"""
    kd = key_levels(7, k)
    ng = [n] * 7
    ng[kd[0]], ng[kd[1]], ng[k] = nkey[0], nkey[1], nk
    return wl.c4_car7d().scaled(ngrid=tuple(ng), rank=10)


def live_values(w, m):
    """indices of dimension m a live fiber may have, ascending: an absorbing dimension keeps off its faces"""
    n = w.ngrid[m]
    return np.arange(1, n - 1) if w.bc[m] == wl.BC_ABSORB else np.arange(n)


def faces(w, k):
    return [m for m in range(w.dx) if m != k and w.bc[m] == wl.BC_ABSORB]


def _kill(w, k, idx, rows, rng):
    """put the fibers `rows` on a face of an absorbing dimension other than k (their other indices stay)"""
    fs = faces(w, k)
    m = rng.integers(0, len(fs), size=rows.size)
    hi = rng.integers(0, 2, size=rows.size).astype(bool)
    for q, dim in enumerate(fs):
        sel = rows[m == q]
        idx[sel, dim] = np.where(hi[m == q], w.ngrid[dim] - 1, 0)


def batch(w, k, F, kind, kdims, seed=0xF1BE):
    """F fibers along K = k, int32 (F, d), every index drawn from the LIVE values of its dimension unless the fiber is meant to
    be dead; kdims: the dimensions whose indices the composition shapes, major first (none: no key structure).
      random      keys uniform over all key pairs, one fiber in eight dead, scattered
      onebin      every fiber live with the same key
      extremes    the lowest and the highest live key pair alternating, one fiber in eight dead
      descending  every fiber live, keys falling with the batch position
      alldead     every fiber on an absorbing face"""
    rng = np.random.default_rng([seed, k, F, len(kind)])
    idx = np.empty((F, w.dx), dtype=np.int32)
    for m in range(w.dx):
        idx[:, m] = rng.choice(live_values(w, m), size=F)
    vals = [live_values(w, m) for m in kdims]
    if kind == "onebin":
        for m, v in zip(kdims, vals):
            idx[:, m] = v[len(v) // 2]
    elif kind == "extremes":
        top = (np.arange(F) % 2).astype(bool)
        for m, v in zip(kdims, vals):
            idx[:, m] = np.where(top, v[-1], v[0])
    elif kind == "descending":
        nkeys = int(np.prod([len(v) for v in vals])) if vals else 1
        rank = ((F - 1 - np.arange(F, dtype=np.int64)) * (nkeys - 1)) // max(F - 1, 1)  # nkeys-1 .. 0, non-increasing
        for m, v in zip(reversed(kdims), reversed(vals)):
            idx[:, m] = v[rank % len(v)]
            rank = rank // len(v)
    elif kind not in ("random", "alldead"):
        raise KeyError(kind)
    if kind in ("random", "extremes"):
        _kill(w, k, idx, np.flatnonzero(rng.integers(0, 8, size=F) == 0), rng)
    if kind == "alldead":
        _kill(w, k, idx, np.arange(F), rng)
    idx[:, k] = 0
    return np.ascontiguousarray(idx)
