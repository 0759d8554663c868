"""The rank of the fiber partition pre-pass (fiber_partition_rank.hpp): k_fpart_rank_count gives every fiber the number of fibers of its
bin in front of it in its block of 1024, k_fpart_rank_scatter only adds it to two prefixes.  Live fibers are ranked by counting the
smaller positions in their bin's list (which atomics fill in any order), dead ones by wave ballots, and a block whose fullest
key bin reaches FPART_RANK_SORT_MIN fibers is sorted instead; k_fpart_rank_scan keeps up to FPART_RSCAN_KEEP rows per thread in
registers and walks twice beyond.

car7d at rank 10 on fiber_partition_ref.car7d_grid(k): 41 x 41 + 1 bins (one key, 42 bins, below 1681 fibers), six nodes per
fiber.  Every case is held by the four assertions of tests/test_gpu_fiber_partition.py (perm and nlive equal to the numpy stable
sort, every output written, outputs bit-identical to C3SC_FIBER_PARTITION=0, a sample at the oracle bar, 4 launches) and is
launched three times in all: the permutation is the same each time.  Batches:
  interleaved   the live fibers alternate between two bins through every block (both far above the switch: sorted), and between
                the two bins of a pair that changes every 16 live fibers (8 per bin: counted)
  straddles     one bin with members at the in-block positions 0, 63, 64, 255, 256, 1023 and at the first and last position of
                the next block: the ends of a wave, of a thread's quarter of the block, of the block
  switch        blocks whose fullest bin holds T - 1, T and T + 1 fibers, T = FPART_RANK_SORT_MIN read from the header; a block of
                one bin beside a block of 1024 bins
  scan bound    exactly FPART_RSCAN_KEEP rows per scan segment, and one block more
  scratch       the rank region through a block that grows and is reused by a smaller batch
  sorting       C3SC_FIBER_RANK=0, the sorting kernels of fiber_partition.hpp in the same build: the same permutation
The host-only test holds the constants read from the header and the place of the rank region by static_asserts."""
import os
import re
import subprocess

import numpy as np
import pytest

import fiber_partition_ref as fp
import test_gpu_fiber_partition as base
from c3sc_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BLOCK = fp.FPART_BLOCK


def _constant(name):
    src = open(os.path.join(CSRC, "fiber_partition_rank.hpp")).read() + open(os.path.join(CSRC, "fiber_partition.hpp")).read()
    m = re.search(r"\b" + name + r" = ([0-9]+)\b", src)
    assert m, f"the partition headers define no {name}"
    return int(m.group(1))


T = _constant("FPART_RANK_SORT_MIN")
SCAN_KEEP, SCAN_THREADS, SCAN_BINS = _constant("FPART_RSCAN_KEEP"), _constant("FPART_RSCAN_THREADS"), _constant("FPART_LINE_INTS")
SCAN_ROWS = SCAN_KEEP * (SCAN_THREADS // SCAN_BINS)  # blocks of a batch whose scan still keeps its rows in registers


def _thrice(eng, P, w, k, idx, what, want_bins=None):
    """the four assertions on one batch, then two more launches with the same permutation"""
    on = base._check(eng, P, w, k, 10, idx, "1", what, want_bins=want_bins)
    for _ in range(2):
        again = base._launch(eng, k, idx, "1", "1")
        assert again[5] == on[5]
        np.testing.assert_array_equal(again[4], on[4])
    return on


def _key_values(w, k):
    """(key dimensions, the live values of each): major first"""
    kd = fp.key_levels(7, k)
    return kd, [fp.live_values(w, m) for m in kd]


def _set_key(w, k, idx, rows, key):
    """make the fibers `rows` live with the key pair number `key` (an index into the live values, major * n_minor + minor)"""
    kd, vals = _key_values(w, k)
    rows = np.asarray(rows)
    for m in fp.faces(w, k):
        idx[rows, m] = np.where((idx[rows, m] == 0) | (idx[rows, m] == w.ngrid[m] - 1), fp.live_values(w, m)[0], idx[rows, m])
    key = np.broadcast_to(np.asarray(key), rows.shape)
    idx[rows, kd[0]] = vals[0][key // len(vals[1])]
    idx[rows, kd[1]] = vals[1][key % len(vals[1])]


def _key_of(w, k, idx):
    """the key pair number of every fiber in the numbering of _set_key, -1 off the live values"""
    kd, vals = _key_values(w, k)
    a = np.searchsorted(vals[0], idx[:, kd[0]])
    b = np.searchsorted(vals[1], idx[:, kd[1]])
    ok = (a < len(vals[0])) & (b < len(vals[1]))
    ok &= (vals[0][np.minimum(a, len(vals[0]) - 1)] == idx[:, kd[0]]) & (vals[1][np.minimum(b, len(vals[1]) - 1)] == idx[:, kd[1]])
    return np.where(ok, a * len(vals[1]) + b, -1)


def _random(w, k, F, seed):
    return fp.batch(w, k, F, "random", fp.key_levels(7, k), seed=seed)


def _fullest(w, k, idx, keys):
    """fibers in the fullest key bin of every block"""
    live = ~fp.dead_mask(w, k, idx)
    key = fp.fiber_keys(w, idx, keys)
    return [int(np.bincount(key[b:b + BLOCK][live[b:b + BLOCK]]).max(initial=0)) for b in range(0, idx.shape[0], BLOCK)]


@pytest.mark.gpu
@pytest.mark.parametrize("F", (1024, 1025, 3073))
@pytest.mark.parametrize("pairs", ("one", "many"))
def test_interleaved_ranks(oracle, F, pairs):
    k = 3
    w, eng, P = base._car(oracle, k)
    idx = _random(w, k, F, seed=0x1A7E)
    live = np.flatnonzero(~fp.dead_mask(w, k, idx))
    n2 = len(_key_values(w, k)[1][1])
    turn = np.arange(live.size)
    keys, nbins = fp.plan(w, k, 10, F, 1)
    if pairs == "one":
        key = np.where(turn % 2 == 0, 7 * n2 + 11, 30 * n2 + 5)  # a, b, a, b, ...: they differ in the major key as well
    elif nbins == 1682:
        key = 5 + (turn // 16) * 2 + turn % 2  # a pair of its own for every 16 live fibers: 8 fibers per bin
    else:
        key = ((turn // 16) * 2 + turn % 2) % 38 * n2 + 3  # one key level: pair after pair of major keys, each comes round again
    _set_key(w, k, idx, live, key)
    full = _fullest(w, k, idx, keys)
    if pairs == "one":
        assert min(full[:-1] or full) >= 400, full
    elif nbins == 1682:
        assert max(full) == 8 < T, full
    _thrice(eng, P, w, k, idx, f"interleaved {pairs} F={F}", want_bins=42 if F < 1681 else 1682)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (3, 0))
def test_wave_and_block_straddles(oracle, k):
    w, eng, P = base._car(oracle, k)
    F = 3073
    idx = _random(w, k, F, seed=0x57AD)
    rows = np.array([0, 63, 64, 255, 256, 1023, 1024, 2047])
    n2 = len(_key_values(w, k)[1][1])
    mine = 20 * n2 + 17
    others = np.setdiff1d(np.flatnonzero(_key_of(w, k, idx) == mine), rows)
    _set_key(w, k, idx, others, mine + 1)  # the bin holds the eight and nothing else
    _set_key(w, k, idx, rows, mine)
    assert np.array_equal(np.flatnonzero((_key_of(w, k, idx) == mine) & ~fp.dead_mask(w, k, idx)), rows)
    on = _thrice(eng, P, w, k, idx, f"straddles k={k}", want_bins=1682)
    at = np.flatnonzero(on[4] == 0)[0]
    np.testing.assert_array_equal(on[4][at:at + rows.size], rows)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (3, 0))
def test_large_bin_switch(oracle, k):
    """blocks 0, 1, 2 have T - 1, T and T + 1 fibers in their fullest bin, at scattered positions; the fourth block is random"""
    w, eng, P = base._car(oracle, k)
    F = 3 * BLOCK + 1000
    idx = _random(w, k, F, seed=0x5317C4)
    rng = np.random.default_rng(T + k)
    n2 = len(_key_values(w, k)[1][1])
    mine = 12 * n2 + 9
    _set_key(w, k, idx, np.flatnonzero(_key_of(w, k, idx) == mine), mine + 1)
    for b, n in enumerate((T - 1, T, T + 1)):
        _set_key(w, k, idx, b * BLOCK + np.sort(rng.choice(BLOCK, size=n, replace=False)), mine)
    keys, nbins = fp.plan(w, k, 10, F, 1)
    full = _fullest(w, k, idx, keys)
    assert full[:3] == [T - 1, T, T + 1] and full[3] < T - 1, full
    _thrice(eng, P, w, k, idx, f"switch at {T} k={k}", want_bins=1682)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (3, 0))
def test_one_bin_beside_distinct_bins(oracle, k):
    """block 0: 1024 live fibers of one bin (sorted); block 1: 1024 live fibers of 1024 bins (every list holds one position);
    block 2: the same keys falling, so that every fiber draws the place of another's"""
    w, eng, P = base._car(oracle, k)
    F = 3 * BLOCK
    idx = _random(w, k, F, seed=0xD157)
    nkeys = int(np.prod([len(v) for v in _key_values(w, k)[1]]))
    assert nkeys >= BLOCK + 100
    _set_key(w, k, idx, np.arange(BLOCK), 777)
    _set_key(w, k, idx, BLOCK + np.arange(BLOCK), 100 + np.arange(BLOCK))
    _set_key(w, k, idx, 2 * BLOCK + np.arange(BLOCK), 100 + np.arange(BLOCK)[::-1])
    keys, nbins = fp.plan(w, k, 10, F, 1)
    assert _fullest(w, k, idx, keys) == [BLOCK, 1, 1]
    on = _thrice(eng, P, w, k, idx, f"one bin beside distinct bins k={k}", want_bins=1682)
    assert on[5] == F


@pytest.mark.gpu
@pytest.mark.parametrize("F", (SCAN_ROWS * BLOCK, SCAN_ROWS * BLOCK + 1025))
def test_scan_register_bound(oracle, F):
    """the last batch whose scan rewrites from registers, and one that walks its rows twice (a block more, and a fiber)"""
    k = 3
    w, eng, P = base._car(oracle, k)
    blocks = -(-F // BLOCK)
    assert (blocks == SCAN_ROWS) == (F == SCAN_ROWS * BLOCK) and blocks <= SCAN_ROWS + 2
    idx = _random(w, k, F, seed=0x5CA9)
    _thrice(eng, P, w, k, idx, f"scan bound {blocks} blocks", want_bins=1682)


@pytest.mark.gpu
def test_rank_region_grows_and_is_reused(oracle):
    """one context of its own: three blocks, 200 blocks (the scratch block is freed and allocated again, the rank region moves),
    three blocks inside the larger block"""
    k = 3
    w = fp.car7d_grid(k)
    eng, P = base._engine(w, wl.synth_cores(w)), base._setup(oracle, w)[1]
    for F in (3073, 204800, 3073):
        idx = _random(w, k, F, seed=F)
        on = _thrice(eng, P, w, k, idx, f"rank scratch F={F}", want_bins=1682)
        assert on[4].shape == (F,)


@pytest.mark.gpu
@pytest.mark.parametrize("F", (3073, 65537))
def test_sorting_kernels_in_the_same_build(oracle, F):
    """C3SC_FIBER_RANK=0 runs the pre-pass with the sorting kernels: the same permutation and the same bits, 4 launches"""
    k = 3
    w, eng, P = base._car(oracle, k)
    idx = _random(w, k, F, seed=0x50A7)
    on = base._check(eng, P, w, k, 10, idx, "1", f"ranking F={F}", want_bins=1682)
    os.environ["C3SC_FIBER_RANK"] = "0"
    try:
        old = base._check(eng, P, w, k, 10, idx, "1", f"sorting F={F}", want_bins=1682)
    finally:
        os.environ.pop("C3SC_FIBER_RANK", None)
    np.testing.assert_array_equal(old[4], on[4])
    for a, b in zip(old[:3], on[:3]):
        np.testing.assert_array_equal(a, b)


# ---- host only

HEADER = r"""
#include "fiber_partition_rank.hpp"
using namespace c3sc;
constexpr bool ranked(long F, int nbins)
{
    const PartOffsets o = fpart_offsets(F, nbins);
    return o.rank >= o.bins + (size_t)F * 2 && o.rank % 256 == 0 && o.end >= o.rank + (size_t)F * 2 && o.end == fpart_bytes(F, nbins);
}
static_assert(FPART_RANK_SORT_MIN == @T@ && FPART_RANK_SORT_MIN >= 2 && FPART_RANK_SORT_MIN <= FPART_BLOCK, "the switch the tests build their blocks around");
static_assert(FPART_RSCAN_KEEP * FPART_RSCAN_SEGS == @ROWS@ && FPART_RSCAN_SEGS * FPART_RSCAN_BINS == FPART_RSCAN_THREADS && FPART_RSCAN_BINS == FPART_LINE_INTS, "the scan's register bound");
"""


def _unit(extra=""):
    lines = [HEADER.replace("@T@", str(T)).replace("@ROWS@", str(SCAN_ROWS))]
    for F in (1000, 65537, 1048576):
        for nbins in (2, 42, 1682):
            lines.append(f'static_assert(ranked({F}L, {nbins}), "the rank region lies behind bins, inside fpart_bytes, 2 F bytes: F={F} nbins={nbins}");')
    lines.append(extra)
    lines.append("int main() { return 0; }\n")
    return "\n".join(lines)


def _syntax_only(path):
    return subprocess.run([HIPCC, "-std=c++20", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(path)],
                          capture_output=True, text=True)


def test_rank_region_static_asserts(tmp_path):
    """Host-only (a syntax-only pass over a generated translation unit): the rank region, the switch and the scan bound"""
    src = tmp_path / "fpart_rank.hip"
    src.write_text(_unit())
    r = _syntax_only(src)
    assert r.returncode == 0, r.stderr[-4000:]
    assert SCAN_ROWS * BLOCK == 1 << 20, "16 rows per thread are what 2^20 fibers need"


def test_rank_region_static_asserts_can_fail(tmp_path):
    src = tmp_path / "fpart_rank_bad.hip"
    src.write_text(_unit('static_assert(fpart_offsets(1000L, 2).rank < fpart_offsets(1000L, 2).bins, "planted");'))
    r = _syntax_only(src)
    assert r.returncode != 0 and "planted" in r.stderr
