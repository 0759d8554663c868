"""The fiber-pair kernel folds the neighbour vectors of the MERGED dimensions -- control-independent dimensions whose upwind
rates are constants of the fiber (kernel_fiber_pair.hpp: PairPark::merged, PairMap) -- rate-weighted into one vector per side of
the varying dimension K.  These tests hold that path to the oracle exactly as tests/test_gpu_parity.py::_check does: flags
bit-exact, values within REL_TOL of the oracle's scale, argmin differing only at ties.

The slot map, by hand (bit m = dimension m; NV = folded vectors, 2(d-1) when nothing merges):

  car7d (controls drive 5, 6; drifts read: 0,1 <- {2,3}; 2 <- {4}; 3 <- {6}; 4 <- {3,4,5}):
    K  merged      NV        K  merged      NV
    0  1,2,3,4      5        4  0,1,3        7
    1  0 | 2,3,4    6        5  0,1,2,3      5
    2  3,4          9        6  0,1,2,4      5
    3  2           11                       48 over a step instead of 84
  lqg6d (controls drive 1,3,5; drift of the even dimension m reads m+1), K = 1: 2 and 4 merge right of K, 0 reads x1 and keeps
    its pair: pairs of 0, 3, 5 + one merged vector = 7 instead of 10.
  dubins3d (control drives 2; drifts of 0 and 1 read theta), K = 0: 1 merges, 2 keeps its pair: 3 instead of 4; K = 2: nothing
    merges, 4.
"""
import os
import subprocess

import numpy as np
import pytest

from c3sc_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
REL_TOL = 1e-12
COUNTS = (1, 70, 130)  # one fiber; a ragged second tile; a ragged third one (two tiles per workgroup slot and one more)

CASES = [
    ("car7d", dict(ngrid=(9, 8, 10, 7, 6, 5, 11), rank=4)),
    ("car7d", dict(ngrid=(11,) * 7, rank=10)),  # the benched instantiation's padded rank
    ("lqg6d", dict(ngrid=(7, 8, 9, 6, 5, 7), rank=8)),
    ("dubins3d", dict(ngrid=(21, 17, 16), rank=4)),
]
IDS = [f"{n}-r{kw['rank']}" for n, kw in CASES]

SLOT_MAP_CHECKS = r"""
#include "launch_fpp.hpp"
#include "models.hpp"
using namespace c3sc;
#define MAP(MODEL, K, MERGED, NVEC) \
    static_assert(PairPark<MODEL, K>::merged() == (MERGED), #MODEL " merged, K = " #K); \
    static_assert(PairMap<MODEL, K>::nv() == (NVEC), #MODEL " vectors, K = " #K);
MAP(Car7D, 0, 0x1Eu, 5)
MAP(Car7D, 1, 0x1Du, 6)
MAP(Car7D, 2, 0x18u, 9)
MAP(Car7D, 3, 0x04u, 11)
MAP(Car7D, 4, 0x0Bu, 7)
MAP(Car7D, 5, 0x0Fu, 5)
MAP(Car7D, 6, 0x17u, 5)
static_assert(PairMap<Car7D, 0>::nv() + PairMap<Car7D, 1>::nv() + PairMap<Car7D, 2>::nv() + PairMap<Car7D, 3>::nv() +
              PairMap<Car7D, 4>::nv() + PairMap<Car7D, 5>::nv() + PairMap<Car7D, 6>::nv() == 48, "car7d: vectors over a step");
MAP(LqgNd<6>, 1, 0x14u, 7)
MAP(Dubins3D, 0, 0x2u, 3)
MAP(Dubins3D, 2, 0x0u, 4)
// a model without dependency information merges nothing
MAP(Scar4D, 1, 0x0u, 6)
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_slot_map_static_asserts(tmp_path):
    """Host-only: the table of the module docstring as static_asserts against the kernel's own constexpr slot map (a syntax-only
    host pass over the headers; nothing is generated)."""
    src = tmp_path / "slot_map.hip"
    src.write_text(SLOT_MAP_CHECKS)
    r = subprocess.run([HIPCC, "-std=c++20", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _engine(w, cores):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    eng.configure(w, cores)
    eng.set_variant(3)  # the fiber-pair kernel, forced
    return eng


def _fibers(w, k):
    """130 fibers of dimension k; the first rows put EVERY fixed dimension (so every merged one) on index 0, on N-1 and on 1
    -- the boundary selects inside a merged vector -- and on the grid's mid point: where an axis is symmetric with an odd
    count (car7d's omega / a axes at N = 11) that coordinate is an exact 0 and the drift it feeds (theta' = omega, v' = a) sits
    in the +-1e-14 dead zone of the upwind rates."""
    ng = np.array(w.ngrid)
    idx = wl.synth_fibers(w, k, max(COUNTS))
    idx[0, :] = 0  # the single fiber of the F = 1 run: every fixed dimension on its lower face
    idx[1, :] = ng - 1
    idx[2, :] = 1
    idx[3, :] = (ng - 1) // 2
    idx[4, :] = np.where(np.arange(w.dx) % 2 == 0, 0, ng - 1)  # mixed faces
    idx[:, k] = 0
    return idx


@pytest.fixture(scope="module", params=range(len(CASES)), ids=IDS)
def case(request, oracle):
    """engine + the oracle's answers for 130 fibers of every varying dimension, computed once and shared (read-only)"""
    name, kw = CASES[request.param]
    w = wl.WORKLOADS[name]().scaled(**kw)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    refs = []
    for k in range(w.dx):
        idx = _fibers(w, k)
        ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
        for a in (idx, ref, ref_ui, ref_ab):
            a.setflags(write=False)
        refs.append((idx, ref, ref_ui, ref_ab))
    return w, _engine(w, cores), refs


def _hold(w, k, out, ui, ab, ref, ref_ui, ref_ab, what):
    scale = np.abs(ref).max()
    if ab is not None:
        np.testing.assert_array_equal(ab, ref_ab)  # integer work: bit-exact
    err = np.abs(out - ref).max()
    print(f"{w.name} k={k} {what}: err {err:.3e} scale {scale:.3e}")
    assert err <= REL_TOL * scale, f"{w.name} k={k} {what}: err {err:.3e} scale {scale:.3e}"
    if ui is not None:  # argmin may only differ on exact ties
        bad = ui != ref_ui
        assert not bad.any() or np.abs(out - ref)[bad].max() <= REL_TOL * scale


@pytest.mark.gpu
@pytest.mark.parametrize("F", COUNTS)
def test_merged_rates_vs_oracle(case, F):
    """every K (car7d: the periodic dimension 2, the reflecting 3..6 and the absorbing 0, 1 as the varying one) at 1, 70 and
    130 fibers"""
    w, eng, refs = case
    for k, (idx, ref, ref_ui, ref_ab) in enumerate(refs):
        out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx[:F]))
        assert eng.status() == 0
        assert "fiber_pair" in eng.last_kernel()
        _hold(w, k, out, ui, ab, ref[:F], ref_ui[:F], ref_ab[:F], f"F={F}")


@pytest.mark.gpu
def test_merged_rates_policy_evaluation(case):
    """the policy-evaluation (FORCED) instantiation on the same inputs: applying the oracle's own minimiser at every node must
    give the oracle's minimum"""
    w, eng, refs = case
    for k, (idx, ref, ref_ui, ref_ab) in enumerate(refs):
        for F in (70, 130):
            pol = np.ascontiguousarray(ref_ui[:F]).astype(np.int32)
            out, ab = eng.policy_fibers_host(k, np.ascontiguousarray(idx[:F]), pol)
            assert eng.status() == 0
            assert "fiber_pair" in eng.last_kernel()
            _hold(w, k, out, None, ab, ref[:F], ref_ui[:F], ref_ab[:F], f"forced F={F}")


@pytest.mark.gpu
@pytest.mark.parametrize("want_uidx,want_absorbed", [(False, False), (True, False), (False, True)])
def test_merged_rates_optional_outputs(case, want_uidx, want_absorbed):
    """uidx / absorbed not requested: the values are the oracle's all the same, and what is still requested is held too"""
    w, eng, refs = case
    for k, (idx, ref, ref_ui, ref_ab) in enumerate(refs):
        out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx[:70]), want_uidx=want_uidx, want_absorbed=want_absorbed)
        assert eng.status() == 0
        assert "fiber_pair" in eng.last_kernel()
        assert (ui is None) == (not want_uidx) and (ab is None) == (not want_absorbed)
        _hold(w, k, out, ui, ab, ref[:70], ref_ui[:70], ref_ab[:70], f"uidx={want_uidx} absorbed={want_absorbed}")
