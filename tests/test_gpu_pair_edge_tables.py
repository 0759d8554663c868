"""The staged fiber-pair kernels (d >= 4) take the first matrix level of each side of the varying dimension K from a product
table built once per upload (kernel_fiber_pair.hpp: fpp_edge_tables; c3sc_hip.hip: k_core_images):

  tabL[(a N_1 + b) rp + beta]      = sum_alpha G_0[a][alpha] G_1[b][alpha, beta]
  tabR[(a N_{d-1} + b) rp + alpha] = sum_beta  G_{d-2}[a][alpha, beta] G_{d-1}[b][beta]

A tile gathers L = tabL[i_0, i_1] and the four neighbour rows tabL[i_0 +- 1, i_1], tabL[i_0, i_1 +- 1] (the same on the right)
instead of staging two cores; a side that is the edge core alone (K = 1, K = d-2) reads its rows straight from the arena.  The
bar is tests/test_gpu_pair_merged_rates.py::_hold: flags bit-exact, values within 1e-12 of the oracle's scale, argmin differing
only at ties.

Counted from PairMap::plan() for car7d, per tile (what test_fold_plan_static_asserts holds):

    K                    0   1   2   3   4   5   6   sum
    staging rounds       4   3   2   2   2   3   4    20   (6 each = 42 without the tables)
    products, tables    31  23  15  14  10  12  20   125
    products, without   36  28  25  24  19  16  24   172
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
COUNTS = (1, 70, 130)  # one fiber; a ragged second tile; a ragged third one

# (workload, scaling, the registered kernel names expected: None = any fiber-pair kernel)
CASES = [
    ("car7d", dict(ngrid=(9, 8, 10, 7, 6, 5, 11), rank=4), None),  # all N differ: a swapped a N_1 + b shows
    ("car7d", dict(ngrid=(11,) * 7, rank=10), "k_fiber_pair<Car7D,10,K=%d>"),  # the benched instantiation
    ("lqg6d", dict(ngrid=(7, 8, 9, 6, 5, 7), rank=8), None),
    # d = 4, staged (registered in inst_other_fpp.hip): K = 2 folds with no staging round at all, K = 1 is a table on the right and
    # the edge core read directly on the left; rank 7 under the padded rank 8, so the zero padding of the tables shows
    ("scar4d", dict(ngrid=(12, 11, 10, 9), rank=7), "k_fiber_pair<Scar4D,8,K=%d>"),
]
IDS = [f"{n}-r{kw['rank']}" for n, kw, _ in CASES]

FOLD_PLAN_CHECKS = r"""
#include "launch_fpp.hpp"
#include "models.hpp"
using namespace c3sc;
static_assert(fpp_edge_tables<Car7D, 10>() && fpp_edge_tables<Car7D, 4>() && fpp_edge_tables<Scar4D, 8>() && fpp_edge_tables<LqgNd<6>, 8>(),
              "staged kernels from d = 4 on use the tables");
static_assert(!fpp_edge_tables<Dubins3D, 8>() && !fpp_edge_tables<Dubins3D, 4>(), "d = 3: no side has two cores");
#define PLAN(K, STAGED, PROD, STAGED0, PROD0) \
    static_assert(PairMap<Car7D, K, true>::plan().staged == (STAGED), "car7d staging rounds, K = " #K); \
    static_assert(PairMap<Car7D, K, true>::plan().products == (PROD), "car7d products, K = " #K); \
    static_assert(PairMap<Car7D, K, false>::plan().staged == (STAGED0), "car7d staging rounds without tables, K = " #K); \
    static_assert(PairMap<Car7D, K, false>::plan().products == (PROD0), "car7d products without tables, K = " #K);
PLAN(0, 4, 31, 6, 36)
PLAN(1, 3, 23, 6, 28)
PLAN(2, 2, 15, 6, 25)
PLAN(3, 2, 14, 6, 24)
PLAN(4, 2, 10, 6, 19)
PLAN(5, 3, 12, 6, 16)
PLAN(6, 4, 20, 6, 24)
template <bool TAB, int... Ks>
constexpr int products(std::integer_sequence<int, Ks...>) { return (PairMap<Car7D, Ks, TAB>::plan().products + ...); }
template <bool TAB, int... Ks>
constexpr int staged(std::integer_sequence<int, Ks...>) { return (PairMap<Car7D, Ks, TAB>::plan().staged + ...); }
static_assert(products<true>(std::make_integer_sequence<int, 7>{}) == 125 && products<false>(std::make_integer_sequence<int, 7>{}) == 172,
              "car7d: products over a step");
static_assert(staged<true>(std::make_integer_sequence<int, 7>{}) == 20 && staged<false>(std::make_integer_sequence<int, 7>{}) == 42,
              "car7d: staging rounds over a step");
// a lone edge core (K = 1, K = d-2) is staged without the tables and read from the arena with them: the flag the kernel branches on
static_assert(PairMap<Car7D, 1, false>::plan().ledge && !PairMap<Car7D, 1, true>::plan().ledge &&
              PairMap<Car7D, 5, false>::plan().redge && !PairMap<Car7D, 5, true>::plan().redge && !PairMap<Car7D, 0, false>::plan().ledge,
              "car7d: lone edge cores");
// the slots do not depend on the tables
static_assert(PairMap<Car7D, 3, true>::nv() == PairMap<Car7D, 3>::nv() && PairMap<Car7D, 3, true>::gslot(5) == PairMap<Car7D, 3>::gslot(5),
              "car7d: slot map with and without tables");
// d = 4: K = 2 has a table on the left, the lone edge core on the right, and nothing staged
static_assert(PairMap<Scar4D, 2, true>::plan().staged == 0 && PairMap<Scar4D, 1, true>::plan().staged == 0 &&
              PairMap<Scar4D, 0, true>::plan().staged == 1 && PairMap<Scar4D, 3, true>::plan().staged == 1, "scar4d staging rounds");
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fold_plan_static_asserts(tmp_path):
    """Host-only: the table of the module docstring as static_asserts against PairMap::plan(), the constexpr function the
    kernel takes its staged steps from (a syntax-only host pass over the headers; nothing is generated)."""
    src = tmp_path / "fold_plan.hip"
    src.write_text(FOLD_PLAN_CHECKS)
    r = subprocess.run([HIPCC, "-std=c++20", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _engine(w, cores=None):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    eng.set_variant(3)  # the fiber-pair kernel, forced (before the upload: the padded rank follows the variant)
    eng.configure(w, cores)
    return eng


def _fibers(w, k, n=max(COUNTS)):
    """n fibers of dimension k; the first rows put EVERY fixed dimension on index 0, on N-1, on 1, on the mid point and on
    mixed faces: there the tables are indexed through the clamped / wrapped neighbour indices."""
    ng = np.array(w.ngrid)
    idx = wl.synth_fibers(w, k, n)
    idx[0, :] = 0  # the single fiber of the F = 1 run: every fixed dimension on its lower face
    idx[1, :] = ng - 1
    idx[2, :] = 1
    idx[3, :] = (ng - 1) // 2
    idx[4, :] = np.where(np.arange(w.dx) % 2 == 0, 0, ng - 1)  # mixed faces
    idx[5, :] = np.where(np.arange(w.dx) % 2 == 0, ng - 1, 0)
    idx[6, :] = ng - 2
    idx[:, k] = 0
    return idx


def _refs(P, w, n=max(COUNTS)):
    refs = []
    for k in range(w.dx):
        idx = _fibers(w, k, n)
        ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
        for a in (idx, ref, ref_ui, ref_ab):
            a.setflags(write=False)
        refs.append((idx, ref, ref_ui, ref_ab))
    return refs


@pytest.fixture(scope="module", params=range(len(CASES)), ids=IDS)
def case(request, oracle):
    """engine + the oracle's answers for 130 fibers of every varying dimension, computed once and shared (read-only)"""
    name, kw, kname = CASES[request.param]
    w = wl.WORKLOADS[name]().scaled(**kw)
    cores = wl.synth_cores(w)
    return w, _engine(w, cores), _refs(oracle.Problem(w, cores), w), kname


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


def _kernel_ok(eng, kname, k):
    assert eng.status() == 0
    assert "fiber_pair" in eng.last_kernel()
    if kname is not None:
        assert eng.last_kernel() == kname % k


@pytest.mark.gpu
@pytest.mark.parametrize("F", COUNTS)
def test_edge_tables_vs_oracle(case, F):
    """every K at 1, 70 and 130 fibers"""
    w, eng, refs, kname = case
    for k, (idx, ref, ref_ui, ref_ab) in enumerate(refs):
        out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx[:F]))
        _kernel_ok(eng, kname, k)
        _hold(w, k, out, ui, ab, ref[:F], ref_ui[:F], ref_ab[:F], f"F={F}")


@pytest.mark.gpu
def test_edge_tables_policy_evaluation(case):
    """the policy-evaluation (FORCED) instantiation on the same inputs: applying the oracle's own minimiser at every node must
    give the oracle's minimum"""
    w, eng, refs, kname = case
    for k, (idx, ref, ref_ui, ref_ab) in enumerate(refs):
        for F in COUNTS:
            pol = np.ascontiguousarray(ref_ui[:F]).astype(np.int32)
            out, ab = eng.policy_fibers_host(k, np.ascontiguousarray(idx[:F]), pol)
            _kernel_ok(eng, kname, k)
            _hold(w, k, out, None, ab, ref[:F], ref_ui[:F], ref_ab[:F], f"forced F={F}")


@pytest.mark.gpu
def test_edge_tables_follow_every_upload(oracle):
    """The tables belong to an upload: ONE engine takes cores A, then B (same ranks, another seed), then C at another rank (the
    padded rank and every offset move), then D through upload_value_device, then A again -- and after each upload every K gives
    that upload's oracle answers.  A table left over from an earlier upload would give the earlier answers."""
    import torch

    base = wl.c4_car7d().scaled(ngrid=(9, 8, 10, 7, 6, 5, 11), rank=3)  # rank 3 under the padded rank 4
    wide = base.scaled(rank=7)  # padded rank 10
    F = 70
    uploads = [("A", base, 0xA11CE, False), ("B", base, 0xB0B, False), ("C", wide, 0xC0C0A, False), ("D", base, 0xD1CE, True),
               ("A again", base, 0xA11CE, False)]
    eng = _engine(base)
    dev = torch.device("cuda", 0)
    answers = {}
    for tag, w, seed, on_device in uploads:
        cores = wl.synth_cores(w, seed)
        if (w.ranks, seed) not in answers:
            answers[(w.ranks, seed)] = _refs(oracle.Problem(w, cores), w, F)
        if on_device:
            core_t = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cores]
            eng.upload_value_device(w.ranks, core_t)
            torch.cuda.synchronize(dev)
        else:
            eng.upload_value(w.ranks, cores)
        for k, (idx, ref, ref_ui, ref_ab) in enumerate(answers[(w.ranks, seed)]):
            out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx))
            _kernel_ok(eng, None, k)
            _hold(w, k, out, ui, ab, ref, ref_ui, ref_ab, f"upload {tag}")
    # the uploads differ: the check above could tell them apart
    a, b = answers[(base.ranks, 0xA11CE)][3][1], answers[(base.ranks, 0xB0B)][3][1]
    assert np.abs(a - b).max() > 1e-6 * np.abs(a).max()
