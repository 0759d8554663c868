"""Three-core product tables of the pair kernel (kernel_common.hpp: pair_tab3L_off; kernel_fiber_pair.hpp: Side::td() == 3,
k_fiber_pair_part3; c3sc_hip.hip: k_pair_tab3, ensure_tab3).

car7d at the padded rank 10 with true ranks 1, 7, 9, 10, 10, 8, 6, 1 (the zero padding of the tables shows) on the grid
(5, 6, 7, 6, 7, 6, 5): the three dimensions of each table all differ, so a swapped index or stride cannot cancel.
C3SC_FIBER_PARTITION=1 and C3SC_FIBER_GROUP=1 put a batch of about 2 000 fibers on the partitioned, grouped path; C3SC_PAIR_TABLE3=0
runs the two-core kernel of the same build.  The batch: random fibers, planted ones on the indices 0, 1, N-2 and N-1 of every table
dimension, and 160 fibers that share both key levels (a tile uniform in both keys; confirmed from the read-back permutation).

Every K, minimising and policy evaluation, literal and consistent ends:
  (a) against the oracle: `absorbed` and `uidx` exact, values within 1e-12 of the scale;
  (b) against C3SC_PAIR_TABLE3=0: flags exact; values bit-identical at K = 0 .. 3 (no merged vector exists ahead of an absorbed
      level: every row is the vector the two-core kernel folds); within the oracle's bar at K = 4 .. 6, where U_L would become a sum
      of products instead of a product of a sum.  The K on the opt-out list (fpp_table3_optout: K = 2 .. 6) run the two-core kernel
      under both settings and are trivially bit-identical; the count of three-core launches says which kernel ran;
  (c) staleness: upload A, launch; upload B, launch; upload A, an unpartitioned launch, then a partitioned one -- each held to the
      oracle of its own cores;
  (d) one c3sc_hip_bellman_fibers_all call over all K, held to (a);
  (e) no launch leaves a status flag or an error behind."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from c3sc_amd import workloads as wl

REL_TOL = 1e-12
NGRID = (5, 6, 7, 6, 7, 6, 5)
TRUE_RANKS = (1, 7, 9, 10, 10, 8, 6, 1)
TABLE_DIMS = (0, 1, 2, 4, 5, 6)
OPTOUT = (2, 3, 4, 5, 6)  # kernel_common.hpp: fpp_table3_optout(7, 10, k): K = 2, 3 measured no faster, K = 4 .. 6 see (b)
ENV_PART, ENV_GROUP, ENV_T3 = "C3SC_FIBER_PARTITION", "C3SC_FIBER_GROUP", "C3SC_PAIR_TABLE3"
SEED_A, SEED_B = 0xC35C, 0xB0B


def _workload():
    return dataclasses.replace(wl.c4_car7d().scaled(ngrid=NGRID, rank=10), ranks=TRUE_RANKS)


def key_levels(d, k):
    """kernel_common.hpp: fpp_key_levels(d, k, true) -- the pre-pass keeps the two-core kernel's levels"""
    lfirst = 2 if k >= 2 else 1
    rfirst = d - 3 if k <= d - 3 else d - 2
    nl, nr = max(k - lfirst, 0), max(rfirst - k, 0)
    if nl and nr:
        return [k - 1, k + 1]
    if nl:
        return [k - 1, k - 2][:min(nl, 2)]
    return [k + 1, k + 2][:min(nr, 2)]


def _live(w, idx):
    """indices moved off the absorbing faces"""
    idx = idx.copy()
    for m in range(w.dx):
        if w.bc[m] == wl.BC_ABSORB:
            idx[:, m] = 1 + idx[:, m] % (w.ngrid[m] - 2)
    return idx


def _batch(w, k):
    rnd = wl.synth_fibers(w, k, 1900).astype(np.int32)  # about 60 % live: dimensions 0 and 1 absorb
    planted = []
    mid = _live(w, wl.synth_fibers(w, k, 4 * len(TABLE_DIMS), seed=0x7AB1E).astype(np.int32))
    r = 0
    for m in TABLE_DIMS:
        for v in (0, 1, w.ngrid[m] - 2, w.ngrid[m] - 1):
            row = mid[r].copy()
            row[m] = v  # a face index of an absorbing dimension makes the fiber a dead one: its rows are read by its neighbours
            planted.append(row)
            r += 1
    kl = key_levels(w.dx, k)
    shared = _live(w, wl.synth_fibers(w, k, 160, seed=0x5AA3ED).astype(np.int32))
    for m in kl:
        shared[:, m] = 1 + (w.ngrid[m] - 2) // 2
    idx = np.concatenate([rnd, np.array(planted, dtype=np.int32), shared])
    idx = idx[np.random.default_rng(77 + k).permutation(idx.shape[0])]
    idx[:, k] = 0
    return np.ascontiguousarray(idx)


class _Setup:
    def __init__(self, oracle):
        from c3sc_amd.engine import BellmanEngine

        self.w = _workload()
        self.cores = {s: wl.synth_cores(self.w, s) for s in (SEED_A, SEED_B)}
        self.eng = BellmanEngine(0)
        self.eng.set_variant(3)  # the fiber-pair kernel, forced
        self.eng.configure(self.w, self.cores[SEED_A])
        self.uploaded = SEED_A
        self.oracle = oracle
        self.P = {}
        self.refs = {}
        self.idx = {k: _batch(self.w, k) for k in range(7)}
        for a in self.idx.values():
            a.setflags(write=False)

    def upload(self, seed):
        self.eng.upload_value(self.w.ranks, self.cores[seed])
        self.uploaded = seed

    def ref(self, k, cends, seed=SEED_A):
        """the oracle's answers, computed once per (K, end rule, cores) and shared read-only"""
        key = (k, cends, seed)
        if key not in self.refs:
            if (cends, seed) not in self.P:
                self.P[(cends, seed)] = self.oracle.Problem(self.w, self.cores[seed], consistent_ends=bool(cends))
            r = self.P[(cends, seed)].bellman_fibers(k, np.array(self.idx[k]))
            for a in r:
                a.setflags(write=False)
            self.refs[key] = r
        return self.refs[key]


_setup_cache = []


@pytest.fixture(scope="module")
def S(oracle):
    if not _setup_cache:
        _setup_cache.append(_Setup(oracle))
    return _setup_cache[0]


def _t3_count(eng):
    return eng.L.c3sc_hip_table3_launch_count()


def _launch(S, k, table3, part="1", policy=None, cends=0):
    """one launch with pre-filled outputs: (out, ui, ab, three-core launches, perm, nlive)"""
    import torch

    eng, idx = S.eng, S.idx[k]
    env = {ENV_PART: part, ENV_GROUP: "1"}
    if not table3:
        env[ENV_T3] = "0"
    for e in (ENV_PART, ENV_GROUP, ENV_T3):
        os.environ.pop(e, None)
    os.environ.update(env)
    try:
        eng.set_consistent_ends(bool(cends))
        dev = torch.device("cuda", 0)
        F, N = idx.shape[0], eng.ngrid[k]
        idx_t = torch.from_numpy(np.array(idx)).to(dev)
        out_t = torch.full((F, N), float("nan"), dtype=torch.float64, device=dev)
        ui_t = torch.full((F, N), -77, dtype=torch.int32, device=dev) if policy is None else None
        ab_t = torch.full((F, N), -77, dtype=torch.int32, device=dev)
        sp = torch.cuda.current_stream(dev).cuda_stream
        n0 = _t3_count(eng)
        if policy is None:
            eng.bellman_fibers(k, idx_t, out_t, ui_t, ab_t, stream_ptr=sp)
        else:
            pol_t = torch.from_numpy(np.array(policy, dtype=np.int32)).to(dev)  # a writable copy of the shared reference
            eng._chk(eng.L.c3sc_hip_policy_fibers(eng.h, k, F, idx_t.data_ptr(), pol_t.data_ptr(), out_t.data_ptr(), ab_t.data_ptr(), sp),
                     "policy_fibers")
        n3 = _t3_count(eng) - n0
        perm, nlive = eng.last_partition(0) if part != "0" else (None, None)
        torch.cuda.synchronize(dev)  # (e): a fault of the new instantiations would surface here
        assert eng.status() == 0
        assert eng.last_kernel() == f"k_fiber_pair<Car7D,10,K={k}>"
        get = lambda t: None if t is None else t.cpu().numpy()
        out, ui, ab = get(out_t), get(ui_t), get(ab_t)
        assert not np.isnan(out).any() and not (ab == -77).any() and (ui is None or not (ui == -77).any()), "an output was never written"
        return out, ui, ab, n3, perm, nlive
    finally:
        for e in (ENV_PART, ENV_GROUP, ENV_T3):
            os.environ.pop(e, None)
        eng.set_consistent_ends(False)


def _hold(out, ui, ab, ref, ref_ui, ref_ab, what):
    """(a): the project's bar, flags exact"""
    scale = np.abs(ref).max()
    err = np.abs(out - ref).max()
    nui = 0 if ui is None else int((ui != ref_ui).sum())
    print(f"{what}: err {err:.3e} scale {scale:.3e} rel {err / scale:.3e} uidx mismatches {nui}")
    np.testing.assert_array_equal(ab, ref_ab)
    assert err <= REL_TOL * scale, f"{what}: err {err:.3e} scale {scale:.3e}"
    if ui is not None:
        np.testing.assert_array_equal(ui, ref_ui)


def _uniform_tile(idx, perm, nlive, kl):
    for t in range(nlive // 64):
        rows = idx[perm[64 * t:64 * t + 64]]
        if all((rows[:, m] == rows[0, m]).all() for m in kl):
            return True
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("cends", (0, 1), ids=("literal", "consistent"))
@pytest.mark.parametrize("k", range(7))
def test_table3_vs_oracle_and_two_core(S, k, cends):
    """(a), (b) and (e), minimising and policy evaluation"""
    if S.uploaded != SEED_A:
        S.upload(SEED_A)
    ref, ref_ui, ref_ab = S.ref(k, cends)
    expect3 = 0 if k in OPTOUT else 1
    for policy in (None, ref_ui):
        what = f"car7d k={k} cends={cends} {'forced' if policy is not None else 'min'}"
        on = _launch(S, k, True, policy=policy, cends=cends)
        off = _launch(S, k, False, policy=policy, cends=cends)
        assert on[3] == expect3 and off[3] == 0, f"{what}: three-core launches {on[3]} (switch on), {off[3]} (switch off)"
        np.testing.assert_array_equal(on[4], off[4])  # the pre-pass does not depend on the tables
        if k != 1:  # K = 1 is on the grouped fold's opt-out list (fpp_group_fold_optout): its pre-pass does not group
            assert _uniform_tile(S.idx[k], on[4], on[5], key_levels(7, k)), f"{what}: the batch holds no tile uniform in both keys"
        _hold(on[0], on[1], on[2], ref, ref_ui, ref_ab, what)
        _hold(off[0], off[1], off[2], ref, ref_ui, ref_ab, what + " two-core")
        np.testing.assert_array_equal(on[2], off[2])
        if on[1] is not None:
            np.testing.assert_array_equal(on[1], off[1])
        dev = np.abs(on[0] - off[0]).max()
        print(f"{what}: on against off, largest deviation {dev:.3e}")
        if k <= 3:
            np.testing.assert_array_equal(on[0], off[0])
        else:
            assert dev <= REL_TOL * np.abs(ref).max()


@pytest.mark.gpu
def test_table3_follows_every_upload(S):
    """(c): the tables belong to an upload and are rebuilt by the first three-core launch behind it, whatever ran in between"""
    k = 0  # the right side of K reads a three-core table
    a, b = S.ref(k, 0, SEED_A), S.ref(k, 0, SEED_B)
    assert np.abs(a[0] - b[0]).max() > 1e-6 * np.abs(a[0]).max(), "the two uploads must differ for the check to tell them apart"
    S.upload(SEED_A)
    r = _launch(S, k, True)
    assert r[3] == 1
    _hold(*r[:3], *a, "upload A")
    S.upload(SEED_B)
    r = _launch(S, k, True)
    assert r[3] == 1
    _hold(*r[:3], *b, "upload B")
    S.upload(SEED_A)
    r = _launch(S, k, True, part="0")  # an unpartitioned launch runs k_fiber_pair and does not touch the tables
    assert r[3] == 0
    _hold(*r[:3], *a, "upload A again, unpartitioned")
    r = _launch(S, k, True)
    assert r[3] == 1
    _hold(*r[:3], *a, "upload A again, partitioned")
    for kk in (1, 3):  # ... and the other K that runs a three-core kernel, and one that does not
        r = _launch(S, kk, True)
        assert r[3] == (0 if kk in OPTOUT else 1)
        _hold(*r[:3], *S.ref(kk, 0, SEED_A), f"upload A again, k={kk}")


@pytest.mark.gpu
def test_table3_fibers_all(S):
    """(d): one call over all K right behind an upload -- the build is enqueued ahead of the fork and every stream sees it"""
    import torch

    eng = S.eng
    S.upload(SEED_B)
    S.upload(SEED_A)  # stale tables, last built for other cores
    dev = torch.device("cuda", 0)
    ks = list(range(7))
    idx_ts = [torch.from_numpy(np.array(S.idx[k])).to(dev) for k in ks]
    outs = [torch.full((S.idx[k].shape[0], eng.ngrid[k]), float("nan"), dtype=torch.float64, device=dev) for k in ks]
    uis = [torch.full((S.idx[k].shape[0], eng.ngrid[k]), -77, dtype=torch.int32, device=dev) for k in ks]
    abs_ = [torch.full((S.idx[k].shape[0], eng.ngrid[k]), -77, dtype=torch.int32, device=dev) for k in ks]
    arr = lambda ts: (C.c_void_p * 7)(*[t.data_ptr() for t in ts])
    os.environ[ENV_PART], os.environ[ENV_GROUP] = "1", "1"
    os.environ.pop(ENV_T3, None)
    try:
        n0 = _t3_count(eng)
        eng._chk(eng.L.c3sc_hip_bellman_fibers_all(eng.h, 7, (C.c_int * 7)(*ks), (C.c_size_t * 7)(*[t.shape[0] for t in idx_ts]), arr(idx_ts),
                                                    arr(outs), arr(uis), arr(abs_), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                 "bellman_fibers_all")
        torch.cuda.synchronize(dev)
        assert _t3_count(eng) - n0 == 7 - len(OPTOUT)
        assert eng.status() == 0
    finally:
        os.environ.pop(ENV_PART, None)
        os.environ.pop(ENV_GROUP, None)
    for k in ks:
        _hold(outs[k].cpu().numpy(), uis[k].cpu().numpy(), abs_[k].cpu().numpy(), *S.ref(k, 0), f"fibers_all k={k}")
