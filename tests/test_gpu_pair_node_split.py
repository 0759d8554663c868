"""The pair kernel's two node-loop forms against the oracle (kernel_fiber_pair.hpp: fpp_node_split).

Where merging left few enough folded vectors that they fit a lane at full length, wavefront h owns the nodes j = h (mod 2) outright
and only v[j] crosses between the two wavefronts; everywhere else the rank stays split in halves.  car7d at rank 10 has both forms
side by side (K = 0, 1, 5, 6 node-split; K = 2, 3 rank-split by their vector count, K = 4 by the opt-out list); ranks below 10
are on the opt-out list as a whole, so the rank-4 sweep holds the rank split next to it on the same grids.  Every case is held to
the oracle at the project's bar: `absorbed` and `uidx` bit-exact (an argmin may differ on an exact tie only), values within 1e-12
of the value scale.

Grids: N = 5 (odd: the last node has no partner), 6 (even), 2 (a single pair).  Fiber counts: 1; 63 and 65 (lanes past the end, a
second tile); 200 (four tiles)."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from c3sc_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
REL_TOL = 1e-12
COUNTS = (1, 63, 65, 200)
GRIDS = (5, 6, 2)
RANKS = (10, 4)
NS_K, RS_K = 5, 3  # one node-split and one rank-split K of car7d at rank 10 for the extra cases

PREDICATE_CHECKS = r"""
#include "launch_fpp.hpp"
#include "models.hpp"
using namespace c3sc;
#if FPP_NODE_SPLIT
// rank 10: 5 / 6 / 9 / 11 / 7 / 5 / 5 vectors; 7 x 10 doubles is the budget, K = 4 is on the opt-out list
static_assert(fpp_node_split<Car7D, 10, 0>() && fpp_node_split<Car7D, 10, 1>() && fpp_node_split<Car7D, 10, 5>() &&
              fpp_node_split<Car7D, 10, 6>(), "car7d rank 10: K = 0, 1, 5, 6 take the node split");
static_assert(!fpp_node_split<Car7D, 10, 2>() && !fpp_node_split<Car7D, 10, 3>(), "car7d rank 10: K = 2, 3 keep the rank split");
static_assert(PairMap<Car7D, 4>::nv() * 10 * 2 <= FPP_NODE_SPLIT_VGPRS && fpp_node_split_optout(7, 10, 4) && !fpp_node_split<Car7D, 10, 4>(),
              "car7d rank 10: K = 4 fits the budget and is opted out");
// padded ranks below 10 are on the opt-out list as a whole (not timed; the rank split leaves them a third wavefront per SIMD)
static_assert(PairMap<Car7D, 3>::nv() * 4 * 2 <= FPP_NODE_SPLIT_VGPRS && fpp_node_split_optout(7, 4, 3) && !fpp_node_split<Car7D, 4, 3>() &&
              !fpp_node_split<Car7D, 4, 0>() && !fpp_node_split<LqgNd<6>, 8, 1>(), "ranks below 10 keep the rank split");
// direct-fold kernels and models with nothing merged compile as before
static_assert(!fpp_node_split<Dubins3D, 6, 0>() && !fpp_node_split<Dubins3D, 6, 2>(), "direct fold: rank split");
#endif
// the launcher's LDS figure of a node-split tile does not exceed the rank-split one
#define LDS(RP, K) static_assert(fpp_tile_doubles<Car7D, RP, K>(true) <= fpp_tile_doubles<Car7D, RP, K>(false), "LDS, K = " #K);
LDS(10, 0) LDS(10, 1) LDS(10, 4) LDS(10, 5) LDS(10, 6)
LDS(4, 0) LDS(4, 1) LDS(4, 2) LDS(4, 3) LDS(4, 4) LDS(4, 5) LDS(4, 6)
// the hand-over moves half of the components at a time: never more rows in flight than the half swap's buffer
static_assert(fpp_tile_doubles<Car7D, 10, 5>(true) >= (size_t)PairMap<Car7D, 5>::nv() * 5 * 64, "hand-over rows fit");
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_node_split_predicate_and_lds(tmp_path):
    """Host-only: which car7d K take the node split, and the launcher's LDS size for them against the rank-split figure, as
    static_asserts on the constexpr functions the kernel and the launcher use (a syntax-only host pass over the headers)."""
    src = tmp_path / "node_split.hip"
    src.write_text(PREDICATE_CHECKS)
    r = subprocess.run([HIPCC, "-std=c++20", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _engine(w, cores):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    eng.set_variant(3)  # the fiber-pair kernel, forced
    eng.configure(w, cores)
    return eng


def _fibers(w, k, n):
    ng = np.array(w.ngrid)
    idx = wl.synth_fibers(w, k, n)
    idx[0, :] = 0  # the single fiber of the F = 1 run
    idx[1, :] = ng - 1
    idx[2, :] = (ng - 1) // 2
    idx[:, k] = 0
    return idx


def _ref(P, k, idx):
    ref = P.bellman_fibers(k, idx)
    for a in (idx,) + tuple(ref):
        a.setflags(write=False)
    return (idx,) + tuple(ref)


def _hold(w, k, out, ui, ab, ref, ref_ui, ref_ab, what):
    scale = np.abs(ref).max()
    if ab is not None:
        np.testing.assert_array_equal(ab, ref_ab)
    err = np.abs(out - ref).max()
    print(f"{w.name} N={w.ngrid[k]} r={w.ranks[1]} k={k} {what}: err {err:.3e} scale {scale:.3e}")
    assert err <= REL_TOL * scale, f"k={k} {what}: err {err:.3e} scale {scale:.3e}"
    if ui is not None:  # argmin may only differ on exact ties
        bad = ui != ref_ui
        assert not bad.any() or np.abs(out - ref)[bad].max() <= REL_TOL * scale


def _kernel_ok(eng, w, k):
    assert eng.status() == 0
    rp = {10: 10, 4: 4}[w.ranks[1]]
    assert eng.last_kernel() == f"k_fiber_pair<Car7D,{rp},K={k}>"


SWEEP = [(r, n) for r in RANKS for n in GRIDS]


@pytest.fixture(scope="module", params=range(len(SWEEP)), ids=[f"r{r}-N{n}" for r, n in SWEEP])
def case(request, oracle):
    """engine + the oracle's answers for 200 fibers of every varying dimension, computed once and shared (read-only)"""
    r, n = SWEEP[request.param]
    w = wl.c4_car7d().scaled(ngrid=(n,) * 7, rank=r)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    return w, _engine(w, cores), [_ref(P, k, _fibers(w, k, max(COUNTS))) for k in range(w.dx)]


@pytest.mark.gpu
@pytest.mark.parametrize("F", COUNTS)
def test_node_split_vs_oracle(case, F):
    """main sweep: every K (both node-loop forms at rank 10) at every fiber count"""
    w, eng, refs = case
    for k, (idx, ref, ref_ui, ref_ab) in enumerate(refs):
        out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx[:F]))
        _kernel_ok(eng, w, k)
        _hold(w, k, out, ui, ab, ref[:F], ref_ui[:F], ref_ab[:F], f"F={F}")


@pytest.fixture(scope="module")
def base(oracle):
    w = wl.c4_car7d().scaled(ngrid=(6, 5, 6, 5, 6, 5, 6), rank=10)
    cores = wl.synth_cores(w)
    return w, cores


@pytest.mark.gpu
@pytest.mark.parametrize("k", (NS_K, RS_K), ids=("node-split", "rank-split"))
@pytest.mark.parametrize("bc", (wl.BC_PERIODIC, wl.BC_REFLECT, wl.BC_ABSORB), ids=("periodic", "reflect", "absorb"))
def test_boundary_in_dim_k(oracle, base, k, bc):
    """periodic (v[N-2] wraps to node 0: both wavefronts form it), reflecting and absorbing ends of the varying dimension"""
    w0, cores = base
    w = dataclasses.replace(w0, bc=tuple(bc if m == k else b for m, b in enumerate(w0.bc)))
    eng = _engine(w, cores)
    idx, ref, ref_ui, ref_ab = _ref(oracle.Problem(w, cores), k, _fibers(w, k, 65))
    out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx))
    _kernel_ok(eng, w, k)
    _hold(w, k, out, ui, ab, ref, ref_ui, ref_ab, f"bc={bc}")


@pytest.fixture(scope="module")
def extra(oracle, base):
    w, cores = base
    P = oracle.Problem(w, cores)
    refs = {}
    for k in (NS_K, RS_K):
        refs[k] = _ref(P, k, _fibers(w, k, 65))
        face = _fibers(w, k, 65).copy()
        face[:, 0 if k != 0 else 1] = 0  # dimensions 0 and 1 absorb: every fiber sits on a face
        refs[k, "face"] = _ref(P, k, face)
    return w, _engine(w, cores), refs


@pytest.mark.gpu
@pytest.mark.parametrize("k", (NS_K, RS_K), ids=("node-split", "rank-split"))
def test_policy_evaluation(extra, k):
    """the FORCED instantiation: applying the oracle's own minimiser at every node must give the oracle's minimum"""
    w, eng, refs = extra
    idx, ref, ref_ui, ref_ab = refs[k]
    for F in (1, 65):
        out, ab = eng.policy_fibers_host(k, np.ascontiguousarray(idx[:F]), np.ascontiguousarray(ref_ui[:F]).astype(np.int32))
        _kernel_ok(eng, w, k)
        _hold(w, k, out, None, ab, ref[:F], ref_ui[:F], ref_ab[:F], f"forced F={F}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", (NS_K, RS_K), ids=("node-split", "rank-split"))
def test_every_fiber_on_a_face(extra, k):
    """a batch in which every fiber has a face index (its interior nodes are absorbed; what the two end nodes of the varying
    dimension are flagged is the oracle's to say)"""
    w, eng, refs = extra
    idx, ref, ref_ui, ref_ab = refs[k, "face"]
    assert (idx[:, 0] == 0).all() and (ref_ab[:, 1:-1] != 0).all()
    out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx))
    _kernel_ok(eng, w, k)
    _hold(w, k, out, ui, ab, ref, ref_ui, ref_ab, "all on a face")


@pytest.mark.gpu
@pytest.mark.parametrize("k", (NS_K, RS_K), ids=("node-split", "rank-split"))
@pytest.mark.parametrize("want_uidx,want_absorbed", [(False, False), (True, False), (False, True)])
def test_optional_outputs(extra, k, want_uidx, want_absorbed):
    """outputs requested with and without uidx / absorbed (both requested: every other test)"""
    w, eng, refs = extra
    idx, ref, ref_ui, ref_ab = refs[k]
    out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx), want_uidx=want_uidx, want_absorbed=want_absorbed)
    _kernel_ok(eng, w, k)
    assert (ui is None) == (not want_uidx) and (ab is None) == (not want_absorbed)
    _hold(w, k, out, ui, ab, ref, ref_ui, ref_ab, f"uidx={want_uidx} absorbed={want_absorbed}")
