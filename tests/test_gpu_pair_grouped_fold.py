"""Grouped fold of the pair kernel (fiber_partition.hpp: the pre-pass groups the live fibers by the indices of the two fold
levels next to K; kernel_fiber_pair.hpp: a tile whose 64 fibers share a key level's index folds that level from SGPRs and
leaves its staging round out).

car7d at rank 10 on the reduced grids of the absorbed-tiles tests (N = 5 in the fixed dimensions, N_K = 5 and 13), the pair variant
forced, C3SC_FIBER_PARTITION=1, every K.  C3SC_FIBER_GROUP=1 groups every batch size (the default floor of fibers per key would
leave these small batches ungrouped), =0 leaves the partition at live fibers first.  Hand-built batches; the tile structure each
one is built for is confirmed in numpy from the read-back permutation before any value is looked at:
  shared  100 fibers that share both keys (the major one on the first, the minor one on the last live index of its dimension: 0
          and N-1 where the dimension reflects or wraps): a uniform tile and a uniform partial last tile
  three   192 live fibers, shuffled, + 40 dead ones with arbitrary keys scattered through (nlive a multiple of 64): tile 0 uniform
          in both keys, tile 1 mixed in the minor key only, tile 2 mixed in both; the first bucket ends exactly on a tile boundary
  ragged  170 live + 30 dead (nlive no multiple of 64): two uniform tiles with a bucket boundary on the tile boundary, then a tile
          of live and dead fibers
  one     F = 1 (too few fibers for a key: the plain partition)
Each holds: the oracle at the project's bar with grouping on (`absorbed` and `uidx` bit-exact, values within 1e-12 of the scale);
on against off bit-identical values, uidx and flags; every output written (pre-filled with NaN / a sentinel); the permutation
(live first, keys non-decreasing, batch order inside a key, dead fibers in batch order); 4 launches with the pass on, 1 with
C3SC_FIBER_PARTITION=0.  K = 1 is on the kernel's opt-out list (fpp_group_fold_optout): its batches run all the same, the
permutation expected there is the plain partition and no tile structure is claimed."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import fiber_partition_ref as fp
from c3sc_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
REL_TOL = 1e-12
ENV_PART, ENV_GROUP = "C3SC_FIBER_PARTITION", "C3SC_FIBER_GROUP"


def key_levels(d, k, tab=True):
    """kernel_common.hpp: fpp_key_levels -- (major, minor) dimensions, nearest staged matrix level first"""
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


def keys_in_use(w, k, F, floor=1):
    """fiber_partition.hpp: fpart_plan -- the key dimensions a batch of F fibers is grouped by"""
    return fp.plan(w, k, max(w.ranks), F, floor)[0]


def _engine(w, cores, cends=0):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    eng.set_variant(3)  # the fiber-pair kernel, forced
    eng.configure(w, cores)
    eng.set_consistent_ends(bool(cends))
    return eng


_cache = {}


def _setup(oracle, w):
    key = (w.name, w.ngrid, w.bc)
    if key not in _cache:
        cores = wl.synth_cores(w)
        _cache[key] = (_engine(w, cores), oracle.Problem(w, cores))
    return _cache[key]


def _car7d(k, nk, n=5):
    return wl.c4_car7d().scaled(ngrid=tuple(nk if m == k else n for m in range(7)), rank=10)


def _live_values(w, m):
    """indices of dimension m a live fiber may have, ascending: an absorbing dimension keeps off its faces"""
    n = w.ngrid[m]
    return list(range(1, n - 1)) if w.bc[m] == wl.BC_ABSORB else list(range(n))


def _live_rows(w, k, F, seed):
    idx = wl.synth_fibers(w, k, F, seed=seed).astype(np.int32)
    for m in range(w.dx):
        if m != k and w.bc[m] == wl.BC_ABSORB:
            idx[:, m] = 1 + idx[:, m] % (w.ngrid[m] - 2)
    return idx


def _batch(w, k, name):
    """(idx, expected (uniform in major, uniform in minor) of the leading tiles, or None where the batch is not grouped)"""
    kl = key_levels(w.dx, k)
    assert len(kl) == 2, "car7d at rank 10 has two key levels at every K"
    kmaj, kmin = kl
    vmaj, vmin = _live_values(w, kmaj), _live_values(w, kmin)
    a = [vmaj[0], vmaj[len(vmaj) // 2], vmaj[-1]]  # the faces 0 and N-1 where the dimension reflects or wraps
    b = [vmin[0], vmin[1], vmin[-1]]
    rng = np.random.default_rng(1000 * k + len(name))

    def rows(groups, ndead, shuffle=True):
        nlive = sum(n for _, _, n in groups)
        idx = _live_rows(w, k, nlive + ndead, seed=0xF1BE + 7 * len(name))
        r = 0
        for ma, mi, n in groups:
            idx[r:r + n, kmaj] = ma
            idx[r:r + n, kmin] = mi
            r += n
        faces = [m for m in range(w.dx) if m != k and w.bc[m] == wl.BC_ABSORB]
        for q in range(ndead):  # dead fibers: a face index in an absorbing dimension, the keys whatever synth_fibers drew
            m = faces[q % len(faces)]
            idx[nlive + q, m] = 0 if (q // len(faces)) % 2 == 0 else w.ngrid[m] - 1
        if shuffle:
            idx = idx[rng.permutation(idx.shape[0])]
        idx[:, k] = 0
        return np.ascontiguousarray(idx)

    if name == "shared":
        return rows([(a[0], b[2], 100)], 0), [(True, True), (True, True)]
    if name == "three":
        return rows([(a[0], b[0], 64), (a[1], b[0], 32), (a[1], b[1], 32), (a[1], b[2], 20), (a[2], b[0], 44)], 40), \
            [(True, True), (True, False), (False, False)]
    if name == "ragged":
        return rows([(a[0], b[2], 64), (a[1], b[1], 64), (a[2], b[0], 42)], 30), [(True, True), (True, True)]
    if name == "one":
        return rows([(a[2], b[2], 1)], 0, shuffle=False), None
    raise KeyError(name)


def _launch(eng, k, idx, part, group, policy=None):
    """one launch with pre-filled outputs; returns (out, ui, ab, launches, perm, nlive)"""
    import torch

    for e in (ENV_PART, ENV_GROUP):
        os.environ.pop(e, None)
    os.environ[ENV_PART] = part
    os.environ[ENV_GROUP] = group
    try:
        dev = torch.device("cuda", 0)
        F, N = idx.shape[0], eng.ngrid[k]
        idx_t = torch.from_numpy(idx).to(dev)
        out_t = torch.full((F, N), float("nan"), dtype=torch.float64, device=dev)
        ui_t = torch.full((F, N), -77, dtype=torch.int32, device=dev) if policy is None else None
        ab_t = torch.full((F, N), -77, dtype=torch.int32, device=dev)
        sp = torch.cuda.current_stream(dev).cuda_stream
        n0 = eng.L.c3sc_hip_launch_count()
        if policy is None:
            eng.bellman_fibers(k, idx_t, out_t, ui_t, ab_t, stream_ptr=sp)
        else:
            pol_t = torch.from_numpy(np.ascontiguousarray(policy, dtype=np.int32)).to(dev)
            eng._chk(eng.L.c3sc_hip_policy_fibers(eng.h, k, F, idx_t.data_ptr(), pol_t.data_ptr(), out_t.data_ptr(), ab_t.data_ptr(), sp),
                     "policy_fibers")
        launches = eng.L.c3sc_hip_launch_count() - n0
        perm, nlive = eng.last_partition(0) if part != "0" else (None, None)
        torch.cuda.synchronize(dev)
        assert eng.status() == 0
        assert "k_fiber_pair" in eng.last_kernel()
        get = lambda t: None if t is None else t.cpu().numpy()
        return get(out_t), get(ui_t), get(ab_t), launches, perm, nlive
    finally:
        for e in (ENV_PART, ENV_GROUP):
            os.environ.pop(e, None)


def _written(out, ui, ab):
    assert not np.isnan(out).any(), f"{int(np.isnan(out).sum())} values were never written"
    for a in (ui, ab):
        if a is not None:
            assert not (a == -77).any(), "an integer output row was never written"


def _hold(out, ui, ab, ref, ref_ui, ref_ab, what):
    scale = np.abs(ref).max()
    np.testing.assert_array_equal(ab, ref_ab)
    err = np.abs(out - ref).max()
    print(f"{what}: err {err:.3e} scale {scale:.3e}")
    assert err <= REL_TOL * scale, f"{what}: err {err:.3e} scale {scale:.3e}"
    if ui is not None:  # an argmin may only differ on an exact tie
        bad = ui != ref_ui
        assert not bad.any() or np.abs(out - ref)[bad].max() <= REL_TOL * scale


def _check_perm(w, k, idx, perm, nlive, keys):
    """the order fiber_partition.hpp promises, with `keys` the key dimensions in use (major first; empty: plain partition)"""
    fp.check_partition(w, k, idx, perm, nlive, keys)


def _tile_structure(idx, perm, kl, ntiles):
    """(uniform in the major key, uniform in the minor key) of the first tiles: a lane past the batch end duplicates fiber F-1"""
    F = idx.shape[0]
    out = []
    for t in range(ntiles):
        pos = np.minimum(np.arange(64 * t, 64 * t + 64), F - 1)
        rows = idx[perm[pos]]
        out.append(tuple(bool((rows[:, m] == rows[0, m]).all()) for m in kl))
    return out


def _check(eng, P, w, k, idx, tiles, what):
    on = _launch(eng, k, idx, "1", "1")
    off = _launch(eng, k, idx, "1", "0")
    nop = _launch(eng, k, idx, "0", "1")
    assert on[3] == 4 and off[3] == 4 and nop[3] == 1, f"{what}: launches {on[3]}, {off[3]}, {nop[3]}"
    _check_perm(w, k, idx, on[4], on[5], keys_in_use(w, k, idx.shape[0]))
    _check_perm(w, k, idx, off[4], off[5], [])
    if tiles is not None and keys_in_use(w, k, idx.shape[0]):
        assert _tile_structure(idx, on[4], key_levels(w.dx, k), len(tiles)) == tiles, f"{what}: the batch does not have the tiles it was built for"
    for r in (on, off, nop):
        _written(*r[:3])
    ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
    _hold(on[0], on[1], on[2], ref, ref_ui, ref_ab, what)
    for other in (off, nop):
        for a, b in zip(on[:3], other[:3]):
            np.testing.assert_array_equal(a, b)
    return ref, ref_ui, ref_ab


@pytest.mark.gpu
@pytest.mark.parametrize("nk", (5, 13))
@pytest.mark.parametrize("k", range(7))
def test_car7d_grouped_batches(oracle, k, nk):
    w = _car7d(k, nk)
    eng, P = _setup(oracle, w)
    for name in ("shared", "three", "ragged", "one"):
        idx, tiles = _batch(w, k, name)
        _check(eng, P, w, k, idx, tiles, f"car7d k={k} N={nk} {name}")
    assert eng.last_kernel() == f"k_fiber_pair<Car7D,10,K={k}>"


@pytest.mark.gpu
def test_policy_evaluation(oracle):
    """the FORCED instantiation: the oracle's own minimiser applied gives the oracle's minimum, grouped or not"""
    k = 3
    w = _car7d(k, 13)
    eng, P = _setup(oracle, w)
    idx, tiles = _batch(w, k, "three")
    ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
    on = _launch(eng, k, idx, "1", "1", policy=ref_ui)
    off = _launch(eng, k, idx, "1", "0", policy=ref_ui)
    assert on[3] == 4 and off[3] == 4
    assert _tile_structure(idx, on[4], key_levels(7, k), len(tiles)) == tiles
    _written(*on[:3])
    _hold(on[0], None, on[2], ref, ref_ui, ref_ab, "car7d k=3 forced")
    np.testing.assert_array_equal(on[0], off[0])
    np.testing.assert_array_equal(on[2], off[2])


@pytest.mark.gpu
@pytest.mark.parametrize("k", (0, 2))
def test_discounted_model_is_deterministic(oracle, k):
    """lqg6d (discount 0.1) with two faces set to absorb: its scan votes per wave, so a fiber's bits may depend on its tile-mates --
    the grouped order is a function of the batch alone, two launches give the same bits; each within the oracle bar"""
    w0 = wl.c3_lqg6d().scaled(ngrid=(5, 5, 6, 5, 5, 5), rank=8)
    w = dataclasses.replace(w0, bc=(wl.BC_ABSORB, wl.BC_ABSORB) + w0.bc[2:])
    eng, P = _setup(oracle, w)
    idx = _live_rows(w, k, 300, seed=0xF1BE)
    idx[::7, 0 if k else 1] = 0  # dead fibers scattered through
    idx[:, k] = 0
    idx = np.ascontiguousarray(idx)
    one = _launch(eng, k, idx, "1", "1")
    two = _launch(eng, k, idx, "1", "1")
    assert one[3] == 4 and two[3] == 4
    _check_perm(w, k, idx, one[4], one[5], keys_in_use(w, k, idx.shape[0]))
    np.testing.assert_array_equal(one[4], two[4])
    for a, b in zip(one[:3], two[:3]):
        np.testing.assert_array_equal(a, b)
    _written(*one[:3])
    ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
    _hold(one[0], one[1], one[2], ref, ref_ui, ref_ab, f"lqg6d+faces k={k}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", (0, 2))
def test_dubins3d_is_not_grouped(oracle, k):
    """a direct-fold kernel stages nothing: the permutation is the plain partition, the outputs are what they were"""
    w = wl.c2_dubins().scaled(ngrid=(6, 5, 7), rank=6)
    eng, P = _setup(oracle, w)
    idx = wl.synth_fibers(w, k, 200).astype(np.int32)
    idx[:, k] = 0
    idx = np.ascontiguousarray(idx)
    on = _launch(eng, k, idx, "1", "1")
    off = _launch(eng, k, idx, "1", "0")
    assert on[3] == 4 and off[3] == 4
    _check_perm(w, k, idx, on[4], on[5], [])
    np.testing.assert_array_equal(on[4], off[4])
    _written(*on[:3])
    ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
    _hold(on[0], on[1], on[2], ref, ref_ui, ref_ab, f"dubins3d k={k}")
    for a, b in zip(on[:3], off[:3]):
        np.testing.assert_array_equal(a, b)
    assert eng.last_kernel() == f"k_fiber_pair<Dubins3D,6,K={k}>"


GROUP_PLAN_CHECKS = r"""
#include "launch_fpp.hpp"
#include "models.hpp"
using namespace c3sc;
#define KEYS(K, MAJ, MIN, UPROD, PROD, ROUNDS, STAGED) \
    static_assert(fpp_key_levels(7, K, true).n == 2 && fpp_key_levels(7, K, true).major == (MAJ) && fpp_key_levels(7, K, true).minor == (MIN), \
                  "car7d key levels, K = " #K); \
    static_assert(fpp_group_levels(7, 10, K).n == (fpp_group_fold_optout(7, 10, K) ? 0 : 2) && \
                  (fpp_group_fold_optout(7, 10, K) || (fpp_group_levels(7, 10, K).major == (MAJ) && fpp_group_levels(7, 10, K).minor == (MIN))), \
                  "car7d: the pre-pass and the kernel use those levels unless K is opted out, K = " #K); \
    static_assert(PairMap<Car7D, K, true>::uniform_products() == (UPROD) && PairMap<Car7D, K, true>::plan().products == (PROD), \
                  "car7d uniform-capable products, K = " #K); \
    static_assert(PairMap<Car7D, K, true>::uniform_rounds() == (ROUNDS) && PairMap<Car7D, K, true>::plan().staged == (STAGED), \
                  "car7d staging rounds left out, K = " #K);
KEYS(0, 1, 2, 16, 31, 2, 4)
KEYS(1, 2, 3, 16, 23, 2, 3)
KEYS(2, 3, 4, 15, 15, 2, 2)
KEYS(3, 2, 4, 14, 14, 2, 2)
KEYS(4, 3, 2, 10, 10, 2, 2)
KEYS(5, 4, 3, 8, 12, 2, 3)
KEYS(6, 5, 4, 12, 20, 2, 4)
// no staged level, no grouping: the direct-fold kernels (dubins3d at ranks <= 8), and a d = 4 problem at K = 1, 2
static_assert(fpp_group_fold_optout(7, 10, 1) && !fpp_group_fold_optout(7, 10, 0) && !fpp_group_fold_optout(7, 4, 1), "the opt-out list: car7d rank 10 K = 1");
static_assert(fpp_group_levels(3, 6, 0).n == 0 && fpp_group_levels(3, 8, 2).n == 0, "direct-fold kernels do not group");
static_assert(fpp_key_levels(4, 2, true).n == 0 && fpp_key_levels(4, 1, true).n == 0, "d = 4, K = 1, 2: the tables absorb every level");
static_assert(fpp_key_levels(6, 2, true).n == 1 && fpp_key_levels(6, 2, true).major == 3, "lqg6d K = 2: one staged level");
// the levels lie inside the kernel's staged ranges
template <int K>
constexpr bool inside()
{
    constexpr FoldPlan p = PairMap<Car7D, K, true>::plan();
    constexpr KeyLevels kl = fpp_key_levels(7, K, true);
    auto in = [&](int m) { return (m >= p.lfirst && m < K) || (m > K && m <= p.rfirst); };
    return in(kl.major) && in(kl.minor);
}
static_assert(inside<0>() && inside<1>() && inside<2>() && inside<3>() && inside<4>() && inside<5>() && inside<6>(), "key levels are staged levels");
int main() { return 0; }
"""


def test_group_plan_static_asserts(tmp_path):
    """Host-only: the key levels and the uniform-capable counts per K for car7d, against the constexpr functions the pre-pass and
    the kernel both use (a syntax-only host pass over the headers; nothing is generated)."""
    src = tmp_path / "group_plan.hip"
    src.write_text(GROUP_PLAN_CHECKS)
    r = subprocess.run([HIPCC, "-std=c++20", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
