"""The fiber partition pre-pass (fiber_partition.hpp: k_fpart_count, k_fpart_scan, k_fpart_scatter) beyond one block, held to a
numpy stable sort (tests/fiber_partition_ref.py).

A block of the pre-pass is 1024 fibers and its scan splits the blocks into 64 segments read 8 rows at a time; the batches of the
two pair-partition test files (1 ... 256 fibers, at most 26 bins) never leave the first block.  Here car7d at rank 10 runs on a
grid with N = 41 in the two key dimensions of the K under test (dimensions 2 and 3 for the opted-out K = 1), N_K = 6 and 5
elsewhere: the benchmark's 41 x 41 + 1 = 1682 bins with six values per fiber.  Batch sizes, by what they do to that arithmetic:
  1000, 1024, 1025   a partial block, a full one, a second block of one fiber (below 1681 fibers: one key, 42 bins)
  8 705              9 blocks: one per segment, most segments empty, the last block half full
  65 536, 65 537     64 blocks: every segment one block; 65: two blocks per segment, segments 33 ... 63 empty, a last block of one
  204 800            200 blocks, four per segment: half a chunk
  524 289            513 blocks, nine per segment: a second chunk with one valid row; just above the default partition threshold
and 215 167 / 215 168 with C3SC_FIBER_GROUP unset, where the default floor of 128 fibers per bin switches 42 bins to 1682.
Compositions (fiber_partition_ref.batch): random, onebin, extremes, descending, alldead.

Every case forces the pair variant, pre-fills the outputs with NaN / -77, and holds
  1. the read-back (perm, nlive) to check_partition with the keys `plan` predicts: exact equality with the numpy stable sort;
  2. every output to be written;
  3. values, uidx and absorbed BIT-IDENTICAL to the same batch with C3SC_FIBER_PARTITION=0 (car7d and dubins3d are undiscounted);
  4. about 256 rows -- the first tile of perm, the tile that straddles nlive, the last tile, random rows -- to the oracle at the
     project's bar: absorbed and uidx exact (an argmin may differ on an exact tie only), values within 1e-12 of the scale;
and 4 launches with the pass on, 1 with it off (c3sc_hip_launch_count)."""
import dataclasses
import os

import numpy as np
import pytest

import fiber_partition_ref as fp
from c3sc_amd import workloads as wl

REL_TOL = 1e-12
ENV_PART, ENV_GROUP = "C3SC_FIBER_PARTITION", "C3SC_FIBER_GROUP"
SIZES = (1000, 1024, 1025, 8705, 65536, 65537, 204800, 524289)


def _engine(w, cores):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    eng.set_variant(3)  # the fiber-pair kernel, forced
    eng.configure(w, cores)
    eng.set_consistent_ends(False)
    return eng


_cache = {}


def _setup(oracle, w):
    key = (w.name, w.ngrid, w.bc)
    if key not in _cache:
        cores = wl.synth_cores(w)
        _cache[key] = (_engine(w, cores), oracle.Problem(w, cores))
    return _cache[key]


def _launch(eng, k, idx, part, group):
    """one bellman_fibers call with pre-filled outputs; part / group: the values of the two variables (None: unset).
    Returns (out, ui, ab, launches, perm, nlive)"""
    import torch

    for e, v in ((ENV_PART, part), (ENV_GROUP, group)):
        os.environ.pop(e, None)
        if v is not None:
            os.environ[e] = v
    try:
        dev = torch.device("cuda", 0)
        F, N = idx.shape[0], eng.ngrid[k]
        idx_t = torch.from_numpy(idx).to(dev)
        out_t = torch.full((F, N), float("nan"), dtype=torch.float64, device=dev)
        ui_t = torch.full((F, N), -77, dtype=torch.int32, device=dev)
        ab_t = torch.full((F, N), -77, dtype=torch.int32, device=dev)
        sp = torch.cuda.current_stream(dev).cuda_stream
        n0 = eng.L.c3sc_hip_launch_count()
        eng.bellman_fibers(k, idx_t, out_t, ui_t, ab_t, stream_ptr=sp)
        launches = eng.L.c3sc_hip_launch_count() - n0
        perm, nlive = eng.last_partition(0) if part != "0" else (None, None)
        torch.cuda.synchronize(dev)
        assert eng.status() == 0
        assert "k_fiber_pair" in eng.last_kernel()
        return out_t.cpu().numpy(), ui_t.cpu().numpy(), ab_t.cpu().numpy(), launches, perm, nlive
    finally:
        for e in (ENV_PART, ENV_GROUP):
            os.environ.pop(e, None)


def _written(out, ui, ab):
    assert not np.isnan(out).any(), f"{int(np.isnan(out).sum())} values were never written"
    for a in (ui, ab):
        assert not (a == -77).any(), "an integer output row was never written"


def _hold(out, ui, ab, ref, ref_ui, ref_ab, what):
    scale = np.abs(ref).max()
    np.testing.assert_array_equal(ab, ref_ab)
    err = np.abs(out - ref).max()
    print(f"{what}: err {err:.3e} scale {scale:.3e}")
    assert err <= REL_TOL * scale, f"{what}: err {err:.3e} scale {scale:.3e}"
    bad = ui != ref_ui  # an argmin may only differ on an exact tie
    assert not bad.any() or np.abs(out - ref)[bad].max() <= REL_TOL * scale


def _sample(perm, nlive, seed):
    """about 256 fibers: the first tile of perm, the tile that straddles nlive, the last tile, random rows"""
    F = perm.shape[0]
    tiles = [0, min(nlive, F - 1) // 64, (F - 1) // 64]
    rows = np.unique(np.concatenate([perm[64 * t:64 * t + 64] for t in tiles]).astype(np.int64))
    more = np.random.default_rng(seed).integers(0, F, size=256 - rows.size)  # the tiles coincide in a small or an all-live batch
    return np.unique(np.concatenate([rows, more]))


def _hold_sample(P, k, idx, res, what):
    rows = _sample(res[4], res[5], idx.shape[0] + k)
    ref, ref_ui, ref_ab = P.bellman_fibers(k, np.ascontiguousarray(idx[rows]))
    _hold(res[0][rows], res[1][rows], res[2][rows], ref, ref_ui, ref_ab, f"{what} ({rows.size} rows)")


def _check(eng, P, w, k, rp, idx, group, what, want_bins=None):
    """the four assertions of the module docstring on one batch; returns the run with the pass on"""
    keys, nbins = fp.plan(w, k, rp, idx.shape[0], fp.floor_of(group))
    print(f"{what}: F {idx.shape[0]} blocks {-(-idx.shape[0] // fp.FPART_BLOCK)} keys {keys} bins {nbins}")
    if want_bins is not None:
        assert nbins == want_bins, f"{what}: the plan gives {nbins} bins"
    on = _launch(eng, k, idx, "1", group)
    off = _launch(eng, k, idx, "0", group)
    assert on[3] == 4 and off[3] == 1, f"{what}: launches {on[3]}, {off[3]}"
    fp.check_partition(w, k, idx, on[4], on[5], keys)
    _written(*on[:3])
    _written(*off[:3])
    for a, b in zip(on[:3], off[:3]):
        np.testing.assert_array_equal(a, b)
    _hold_sample(P, k, idx, on, what)
    return on


def _car(oracle, k, nkey=(41, 41)):
    w = fp.car7d_grid(k, nkey=nkey)
    eng, P = _setup(oracle, w)
    return w, eng, P


@pytest.mark.gpu
@pytest.mark.parametrize("F", SIZES)
@pytest.mark.parametrize("k", (3, 0))
def test_car7d_random_batch_sizes(oracle, k, F):
    """every batch size, grouped from one fiber per bin on; K = 0 has an absorbing key dimension (its faces hold no live fiber)"""
    w, eng, P = _car(oracle, k)
    idx = fp.batch(w, k, F, "random", fp.key_levels(7, k))
    _check(eng, P, w, k, 10, idx, "1", f"car7d k={k} random", want_bins=42 if F < 1681 else 1682)
    assert eng.last_kernel() == f"k_fiber_pair<Car7D,10,K={k}>"


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 2, 4, 5, 6))
def test_car7d_random_every_k(oracle, k):
    """65 blocks at the K that test_car7d_random_batch_sizes leaves out; K = 1 is on the kernel's opt-out list: the plain partition"""
    w, eng, P = _car(oracle, k)
    idx = fp.batch(w, k, 65537, "random", fp.key_levels(7, k))
    _check(eng, P, w, k, 10, idx, "1", f"car7d k={k} random", want_bins=2 if k == 1 else 1682)
    assert eng.last_kernel() == f"k_fiber_pair<Car7D,10,K={k}>"


@pytest.mark.gpu
@pytest.mark.parametrize("F", (1025, 65537))
@pytest.mark.parametrize("kind", ("onebin", "extremes", "descending", "alldead"))
def test_car7d_compositions(oracle, kind, F):
    """one bin that holds the batch (a full block is a single run); bin 0, bin nbins-2 and the dead bin alone (the last scan
    workgroup has 2 of its 16 bins on); keys falling with the batch position (the bitonic sort starts reversed); no live fiber"""
    k = 3
    w, eng, P = _car(oracle, k)
    idx = fp.batch(w, k, F, kind, fp.key_levels(7, k))
    on = _check(eng, P, w, k, 10, idx, "1", f"car7d k={k} {kind}")
    assert on[5] == {"onebin": F, "descending": F, "alldead": 0}.get(kind, on[5])


@pytest.mark.gpu
@pytest.mark.parametrize("F", (65537, 524289))
def test_car7d_grouping_off(oracle, F):
    """C3SC_FIBER_GROUP=0: two bins, the scatter ranks by a prefix count instead of sorting"""
    k = 3
    w, eng, P = _car(oracle, k)
    idx = fp.batch(w, k, F, "random", fp.key_levels(7, k))
    _check(eng, P, w, k, 10, idx, "0", f"car7d k={k} ungrouped", want_bins=2)


@pytest.mark.gpu
@pytest.mark.parametrize("F,bins", ((215167, 42), (215168, 1682)))
def test_car7d_default_floor(oracle, F, bins):
    """C3SC_FIBER_GROUP unset: the minor key comes in at exactly 128 fibers per bin, 128 x 1681 = 215 168"""
    k = 3
    w, eng, P = _car(oracle, k)
    idx = fp.batch(w, k, F, "random", fp.key_levels(7, k))
    _check(eng, P, w, k, 10, idx, None, f"car7d k={k} default floor", want_bins=bins)


@pytest.mark.gpu
@pytest.mark.parametrize("nkey,bins", (((89, 23), 2048), ((64, 32), 65)))
def test_car7d_bin_cap(oracle, nkey, bins):
    """89 x 23 + 1 = 2048 bins, exactly the cap (every thread of the scatter holds 8 bins, the count's histogram is full);
    64 x 32 + 1 = 2049 falls back to the major key, 65 bins.  The pair launcher stages a core of N = 89 at rank 10 in 72 KB of LDS
    and accepts the grid, so the product is 2047 as it stands."""
    k = 3
    w, eng, P = _car(oracle, k, nkey)
    idx = fp.batch(w, k, 65537, "random", fp.key_levels(7, k))
    _check(eng, P, w, k, 10, idx, "1", f"car7d k={k} keys {nkey}", want_bins=bins)
    assert eng.last_kernel() == f"k_fiber_pair<Car7D,10,K={k}>"


@pytest.mark.gpu
def test_scratch_grows_and_is_reused(oracle):
    """one context of its own: two blocks, 513 blocks (the scratch block is freed and allocated again), two blocks in the larger
    block -- each time last_partition has the launch's own length and content"""
    k = 3
    w = fp.car7d_grid(k)
    cores = wl.synth_cores(w)
    eng, P = _engine(w, cores), _setup(oracle, w)[1]
    for F in (1025, 524289, 1025):
        idx = fp.batch(w, k, F, "random", fp.key_levels(7, k), seed=F)
        on = _check(eng, P, w, k, 10, idx, "1", f"car7d k={k} scratch F={F}")
        assert on[4].shape == (F,)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (2, 0))
def test_lqg6d_discounted(oracle, k):
    """lqg6d (discount 0.1, rank 8) with two faces set to absorb, 65 blocks: K = 2 has one key level (dimension 3, N = 31: 32
    bins), K = 0 two (5 x 6 + 1).  Its scan votes per wave on the form of the discount factor, so a fiber's bits may depend on its
    tile-mates: two launches give the same permutation and the same bits, and the sample is within the oracle bar"""
    w0 = wl.c3_lqg6d().scaled(ngrid=(5, 5, 6, 31, 5, 5), rank=8)
    w = dataclasses.replace(w0, bc=(wl.BC_ABSORB, wl.BC_ABSORB) + w0.bc[2:])
    eng, P = _setup(oracle, w)
    F = 65537
    keys, nbins = fp.plan(w, k, 8, F, 1)
    assert (keys, nbins) == (([3], 32) if k == 2 else ([1, 2], 31))
    idx = fp.batch(w, k, F, "random", keys)
    one = _launch(eng, k, idx, "1", "1")
    two = _launch(eng, k, idx, "1", "1")
    assert one[3] == 4 and two[3] == 4
    fp.check_partition(w, k, idx, one[4], one[5], keys)
    np.testing.assert_array_equal(one[4], two[4])
    assert one[5] == two[5]
    for a, b in zip(one[:3], two[:3]):
        np.testing.assert_array_equal(a, b)
    _written(*one[:3])
    _hold_sample(P, k, idx, one, f"lqg6d+faces k={k}")
    assert eng.last_kernel() == f"k_fiber_pair<LqgNd<6>,8,K={k}>"


@pytest.mark.gpu
@pytest.mark.parametrize("k", (0, 2))
def test_dubins3d_plain_partition(oracle, k):
    """a direct-fold kernel stages nothing and groups by nothing: the plain partition at 65 blocks"""
    w = wl.c2_dubins().scaled(ngrid=(6, 5, 7), rank=6)
    eng, P = _setup(oracle, w)
    idx = fp.batch(w, k, 65537, "random", [])
    _check(eng, P, w, k, 6, idx, "1", f"dubins3d k={k}", want_bins=2)
    assert eng.last_kernel() == f"k_fiber_pair<Dubins3D,6,K={k}>"
