"""The reference model of the fiber partition pre-pass (tests/fiber_partition_ref.py), held from both sides on the CPU:
  * `check_partition` rejects ten planted mistakes, each by the assertion named for it, on a 65 537-fiber car7d batch (65 blocks
    of the pre-pass, 41 x 41 + 1 bins), and lets the unaltered reference permutation pass;
  * `plan` is held to fpart_plan / fpp_group_levels of the C++ by static_asserts in a generated translation unit (a syntax-only
    host pass), over the fiber counts at which the plan switches, the bin cap and the models with one or no key level; the same
    pass holds the scratch regions of fpart_carve to lie in order and inside fpart_bytes."""
import os
import subprocess

import numpy as np
import pytest

import fiber_partition_ref as fp
from c3sc_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
K, F = 3, 65537


@pytest.fixture(scope="module")
def case():
    """(w, idx, keys, perm, nlive): the reference permutation of a random batch; the tests alter copies of it"""
    w = fp.car7d_grid(K)
    keys, nbins = fp.plan(w, K, 10, F, 1)
    assert keys == [2, 4] and nbins == 41 * 41 + 1
    idx = fp.batch(w, K, F, "random", keys)
    perm, nlive = fp.reference_perm(w, K, idx, keys)
    perm.setflags(write=False)
    idx.setflags(write=False)
    return w, idx, keys, perm, nlive


def _rejected(case, perm, nlive, name):
    w, idx, keys, ref, _ = case
    assert nlive != case[4] or not np.array_equal(perm, ref), "the planted mistake changed nothing"
    with pytest.raises(AssertionError, match="^" + name):
        fp.check_partition(w, K, idx, perm, nlive, keys)


def test_unaltered_permutation_passes(case):
    w, idx, keys, perm, nlive = case
    assert 0 < nlive < F and abs((F - nlive) / F - 0.125) < 0.01  # one fiber in eight is dead
    fp.check_partition(w, K, idx, perm, nlive, keys)
    plain, nl = fp.reference_perm(w, K, idx, [])
    assert nl == nlive
    fp.check_partition(w, K, idx, plain, nl, [])
    np.testing.assert_array_equal(plain[:nl], np.flatnonzero(~fp.dead_mask(w, K, idx)))


def test_two_fibers_of_one_key_swapped(case):
    w, idx, keys, perm, nlive = case
    lk = fp.fiber_keys(w, idx, keys)[perm[:nlive]]
    same = np.flatnonzero(lk[1:] == lk[:-1])
    i = int(same[len(same) // 3])
    bad = perm.copy()
    bad[[i, i + 1]] = bad[[i + 1, i]]
    _rejected(case, bad, nlive, "batch order holds inside a key")


def test_keys_minor_then_major(case):
    w, idx, keys, perm, nlive = case
    bad, nl = fp.reference_perm(w, K, idx, keys[::-1])
    _rejected(case, bad, nl, "keys ascend, major then minor")


@pytest.mark.parametrize("off", (1, -1))
def test_nlive_off_by_one(case, off):
    _rejected(case, case[3].copy(), case[4] + off, "nlive is right")


def test_dead_fiber_in_front_of_the_live_ones(case):
    w, idx, keys, perm, nlive = case
    j = nlive + 5
    bad = np.concatenate([perm[j:j + 1], perm[:j], perm[j + 1:]])
    _rejected(case, bad, nlive, "live fibers come first")


def test_entry_duplicated(case):
    w, idx, keys, perm, nlive = case
    bad = perm.copy()
    bad[10] = bad[11]
    _rejected(case, bad, nlive, "perm is a bijection")


def test_entry_dropped(case):
    """the length last_partition reports is the launch's own"""
    w, idx, keys, perm, nlive = case
    _rejected(case, perm[:-1].copy(), nlive, "perm has one entry per fiber")


def test_dead_fibers_reversed(case):
    w, idx, keys, perm, nlive = case
    bad = perm.copy()
    bad[nlive:] = bad[nlive:][::-1]
    _rejected(case, bad, nlive, "dead fibers are in batch order")


def test_block_runs_of_one_bin_exchanged(case):
    """what a wrong counts[b][bin] prefix does: inside one bin, block b's run lands behind block b+1's"""
    w, idx, keys, perm, nlive = case
    lp = perm[:nlive]
    lk = fp.fiber_keys(w, idx, keys)[lp]
    blk = lp // fp.FPART_BLOCK
    hit = np.flatnonzero((lk[1:] == lk[:-1]) & (blk[1:] == blk[:-1] + 1))  # a bin with fibers of blocks b and b + 1
    i = int(hit[len(hit) // 2])
    a0 = i
    while a0 > 0 and lk[a0 - 1] == lk[i] and blk[a0 - 1] == blk[i]:
        a0 -= 1
    b1 = i + 2
    while b1 < nlive and lk[b1] == lk[i] and blk[b1] == blk[i + 1]:
        b1 += 1
    bad = perm.copy()
    bad[a0:b1] = np.concatenate([perm[i + 1:b1], perm[a0:i + 1]])
    _rejected(case, bad, nlive, "batch order holds inside a key")


def test_two_highest_bins_merged(case):
    """what a histogram one bin short does: the fibers of the two highest key bins in batch order, as if they were one bin"""
    w, idx, keys, perm, nlive = case
    lk = fp.fiber_keys(w, idx, keys)[perm[:nlive]]
    top = np.unique(lk)[-2:]
    lo = int(np.searchsorted(lk, top[0]))
    bad = perm.copy()
    bad[lo:nlive] = np.sort(perm[lo:nlive])
    _rejected(case, bad, nlive, "keys ascend, major then minor")


def test_final_equality_is_its_own_assertion(case, monkeypatch):
    """the six properties determine the permutation, so no altered permutation reaches the last assertion: a reference that
    disagrees must"""
    w, idx, keys, perm, nlive = case
    monkeypatch.setattr(fp, "reference_perm", lambda *a: (np.roll(perm, 1), nlive))
    with pytest.raises(AssertionError, match="^perm equals the reference permutation"):
        fp.check_partition(w, K, idx, perm, nlive, keys)


def test_batch_builders():
    """each composition is what its name says, on two blocks and a fiber"""
    w = fp.car7d_grid(K)
    kd = [2, 4]
    n = 1025
    key = lambda idx: fp.fiber_keys(w, idx, kd)
    for kind in ("random", "onebin", "extremes", "descending", "alldead"):
        idx = fp.batch(w, K, n, kind, kd)
        assert idx.shape == (n, 7) and idx.dtype == np.int32 and (idx[:, K] == 0).all()
        assert (idx >= 0).all() and (idx < np.array(w.ngrid)).all(), "no index off the grid"
        np.testing.assert_array_equal(idx, fp.batch(w, K, n, kind, kd))  # seeded
        dead = fp.dead_mask(w, K, idx)
        if kind == "onebin":
            assert not dead.any() and np.unique(key(idx)).size == 1
        if kind == "extremes":
            assert dead.any() and set(np.unique(key(idx)[~dead])) == {0, 41 * 41 - 1}
        if kind == "descending":
            assert not dead.any() and (np.diff(key(idx)) <= 0).all() and key(idx)[0] == 41 * 41 - 1 and key(idx)[-1] == 0
        if kind == "alldead":
            assert dead.all()
        if kind == "random":
            # about 897 live fibers thrown into 1681 bins occupy 1681 (1 - exp(-897 / 1681)) = 695 of them
            assert 0.08 < dead.mean() < 0.17 and np.unique(key(idx)[~dead]).size > 600


def test_floor_of_the_environment():
    assert fp.floor_of(None) == 128 and fp.floor_of("") == 128 and fp.floor_of("0") < 0 and fp.floor_of("1") == 1 and fp.floor_of("400") == 400


# ---- plan against the C++

PLAN_F = (1680, 1681, 215167, 215168, 1 << 20)


def _car_grid(k, nkey):
    return fp.car7d_grid(k, nkey=nkey).ngrid


def plan_rows():
    """(d, rp, k, grid, F, floor)"""
    rows = []
    for k in range(7):  # car7d on the benchmark's grid and on the tests' reduced one, around both switches of the plan
        for grid in ((41,) * 7, _car_grid(k, (41, 41))):
            for n in PLAN_F:
                for floor in (128, 1):
                    rows.append((7, 10, k, grid, n, floor))
    for nkey in ((89, 23), (64, 32), (2047, 2), (2048, 2)):  # 2048 bins: the cap; 2049: the major key alone; 2049 major bins: none
        for k in (3, 0, 6):
            for n, floor in ((65537, 1), (1 << 20, 128), (1 << 28, 128)):
                rows.append((7, 10, k, _car_grid(k, nkey), n, floor))
    for k in range(6):  # lqg6d: one key level at K = 2 and 3
        for n, floor in ((30, 1), (31, 1), (65537, 1), (65537, 128), (3967, 128), (3968, 128)):
            rows.append((6, 8, k, (5, 5, 6, 31, 5, 5) if k == 2 else (31,) * 6, n, floor))
    for k in range(3):  # dubins3d: direct fold at ranks <= 8, staged above
        for rp in (6, 8, 10):
            rows.append((3, rp, k, (6, 5, 7), 65537, 1))
    for k in (0, 1, 3):  # grouping switched off
        rows.append((7, 10, k, (41,) * 7, 1 << 20, -1))
    return rows


PLAN_HEADER = r"""
#include "fiber_partition.hpp"
using namespace c3sc;
struct Grid {
    int n[MAXD];
};
constexpr PartArgs planned(int d, int rp, int k, Grid g, long F, long floor)
{
    PartArgs P{};
    P.d = d;
    P.k = k;
    P.F = F;
    for (int m = 0; m < MAXD; m++) {
        P.ngrid[m] = g.n[m];
        P.bctype[m] = 0;
    }
    fpart_plan(P, fpp_group_levels(d, rp, k), floor);
    return P;
}
constexpr bool carved(long F, int nbins)
{
    const PartOffsets o = fpart_offsets(F, nbins);
    return o.perm == 0 && o.counts >= o.perm + (size_t)F * 4 && o.totals >= o.counts + (size_t)fpart_blocks(F) * nbins * 4 &&
           o.nlive >= o.totals + (size_t)nbins * 4 && o.bins >= o.nlive + 4 && o.end >= o.bins + (size_t)F * 2 && o.end == fpart_bytes(F, nbins) &&
           o.counts % 256 == 0 && o.totals % 256 == 0 && o.nlive % 256 == 0 && o.bins % 256 == 0;
}
static_assert(FPART_BLOCK == @BLOCK@ && FPART_MAX_BINS == @MAX_BINS@ && FPART_MIN_PER_BIN == @MIN_PER_BIN@ && FPP_DIRECT_MAXD == @DIRECT_MAXD@, "the constants of the Python model");
"""


def _translation_unit(rows):
    head = PLAN_HEADER
    for name in ("BLOCK", "MAX_BINS", "MIN_PER_BIN"):
        head = head.replace(f"@{name}@", str(getattr(fp, "FPART_" + name)))
    lines = [head.replace("@DIRECT_MAXD@", str(fp.FPP_DIRECT_MAXD))]
    for d, rp, k, grid, n, floor in rows:
        keys, nbins = fp.plan_grid(d, grid, k, rp, n, floor)
        kmaj, kmin = (keys + [-1, -1])[:2]
        nmin = grid[kmin] if kmin >= 0 else 1
        call = f"planned({d}, {rp}, {k}, Grid{{{{{', '.join(map(str, grid))}}}}}, {n}L, {floor}L)"
        what = f"d={d} rp={rp} k={k} grid={grid} F={n} floor={floor}"
        for field, v in (("kmaj", kmaj), ("kmin", kmin), ("nmin", nmin), ("nbins", nbins)):
            lines.append(f'static_assert({call}.{field} == {v}, "{field}: {what}");')
    for n, nbins in ((1, 2), (65537, 1682), (1 << 20, 2048)):
        blocks = -(-n // fp.FPART_BLOCK)
        lines.append(f'static_assert(carved({n}L, {nbins}) && fpart_blocks({n}L) == {blocks}, "fpart_carve: the regions lie in order inside fpart_bytes, F={n} nbins={nbins}");')
    lines.append("int main() { return 0; }\n")
    return "\n".join(lines)


def test_plan_rows_cover_the_switches():
    """the table itself: both car7d switches, the cap from both sides, one key level, none, grouping off"""
    got = {(d, rp, k, grid, n, floor): fp.plan_grid(d, grid, k, rp, n, floor) for d, rp, k, grid, n, floor in plan_rows()}
    g = (41,) * 7
    assert got[(7, 10, 3, g, 1680, 1)] == ([2], 42) and got[(7, 10, 3, g, 1681, 1)] == ([2, 4], 1682)
    assert got[(7, 10, 3, g, 215167, 128)] == ([2], 42) and got[(7, 10, 3, g, 215168, 128)] == ([2, 4], 1682)
    assert got[(7, 10, 3, g, 1680, 128)] == ([], 2) and got[(7, 10, 1, g, 1 << 20, 1)] == ([], 2)
    assert got[(7, 10, 3, _car_grid(3, (89, 23)), 65537, 1)] == ([2, 4], 2048)
    assert got[(7, 10, 3, _car_grid(3, (64, 32)), 65537, 1)] == ([2], 65)
    assert got[(7, 10, 3, _car_grid(3, (2047, 2)), 65537, 1)] == ([2], 2048) and got[(7, 10, 3, _car_grid(3, (2048, 2)), 65537, 1)] == ([], 2)
    assert got[(6, 8, 2, (5, 5, 6, 31, 5, 5), 65537, 1)] == ([3], 32) and got[(6, 8, 2, (5, 5, 6, 31, 5, 5), 30, 1)] == ([], 2)
    assert got[(3, 6, 0, (6, 5, 7), 65537, 1)] == ([], 2) and got[(3, 10, 0, (6, 5, 7), 65537, 1)] != ([], 2)
    assert got[(7, 10, 3, g, 1 << 20, -1)] == ([], 2)
    w = wl.c4_car7d()
    assert fp.plan(w, 3, 10, 1 << 20, fp.floor_of(None)) == ([2, 4], 1682)  # the benchmarked configuration


def test_plan_static_asserts(tmp_path):
    """Host-only: fpart_plan on fpp_group_levels gives what `plan` gives, row by row (a syntax-only host pass over a generated
    translation unit; nothing is built)."""
    src = tmp_path / "fpart_plan.hip"
    src.write_text(_translation_unit(plan_rows()))
    r = subprocess.run([HIPCC, "-std=c++20", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_plan_static_asserts_can_fail(tmp_path):
    """the pass is not vacuous: a row with a wrong expectation does not compile"""
    tu = _translation_unit(plan_rows()[:1]).replace("int main()", 'static_assert(planned(7, 10, 3, Grid{{41, 41, 41, 41, 41, 41, 41}}, 1681L, 1L).nbins == 42, "planted");\nint main()')
    src = tmp_path / "fpart_plan_bad.hip"
    src.write_text(tu)
    r = subprocess.run([HIPCC, "-std=c++20", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "planted" in r.stderr
