"""The pair kernel's parked node split against the oracle (kernel_fiber_pair.hpp: fpp_parked).

A middle K of car7d at rank 10 carries more folded vectors than a lane holds at full length.  In the node split both wavefronts
hold identical copies of every vector, so the last P of them are kept once, in LDS rows ("homes") above everything else the node
loop keeps there, and read back inside the stencil; the others stay in registers.  K = 2 parks 3 of 9, K = 4 parks FPP_PARKED_K4 of
7; K = 3 keeps the rank split, the edge K their node split.  The kernels of the form (k_fiber_pair_pk, k_fiber_pair_part_pk) stand
in inst_car7d_fpp_pk.hip and keep their resource remarks in pk_res/; C3SC_PAIR_PARKED=0 runs the kernels they replace.

Every GPU case is held to the oracle at the project's bar: `absorbed` and `uidx` bit-exact (an argmin may differ only where the two
values are within 1e-12 of the scale), values within 1e-12 of the value scale.

Grids: N = 5 (odd: the last node has no partner), 6 (even), 2 (a single pair).  Fiber counts: 1; 63 and 65 (lanes past the end, a
second tile); 200 (four tiles)."""
import dataclasses
import json
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
PARKED_K = (2, 4)
SWEEP_K = (2, 3, 4, 5)  # the two parked K, the rank-split K between them, and a node-split K as the control
PART_ENV, PARKED_ENV = "C3SC_FIBER_PARTITION", "C3SC_PAIR_PARKED"

PREDICATE_CHECKS = r"""
#include "launch_fpp.hpp"
#include "models.hpp"
using namespace c3sc;
#if FPP_NODE_SPLIT
// car7d at rank 10: the form at K = 2 and 4 only
static_assert(fpp_parked<Car7D, 10, 0>() == 0 && fpp_parked<Car7D, 10, 1>() == 0 && fpp_parked<Car7D, 10, 3>() == 0 &&
              fpp_parked<Car7D, 10, 5>() == 0 && fpp_parked<Car7D, 10, 6>() == 0, "car7d rank 10: K = 0, 1, 3, 5, 6 keep their form");
static_assert(fpp_parked<Car7D, 10, 2>() == 3 && fpp_parked<Car7D, 10, 4>() == FPP_PARKED_K4 && FPP_PARKED_K4 >= 1 && FPP_PARKED_K4 <= 2,
              "car7d rank 10: K = 2 parks three vectors, K = 4 one or two");
// the old predicates keep their values
static_assert(fpp_node_split<Car7D, 10, 0>() && fpp_node_split<Car7D, 10, 1>() && fpp_node_split<Car7D, 10, 5>() &&
              fpp_node_split<Car7D, 10, 6>() && !fpp_node_split<Car7D, 10, 2>() && !fpp_node_split<Car7D, 10, 3>() &&
              !fpp_node_split<Car7D, 10, 4>() && fpp_node_split_optout(7, 10, 4) && FPP_NODE_SPLIT_VGPRS == 140,
              "fpp_node_split, its opt-out list and its budget are unchanged");
// nothing else takes the form: ranks below 10, lqg6d, the direct-fold kernels
static_assert(fpp_parked<Car7D, 4, 0>() == 0 && fpp_parked<Car7D, 4, 2>() == 0 && fpp_parked<Car7D, 4, 3>() == 0 && fpp_parked<Car7D, 4, 4>() == 0 &&
              fpp_parked<Car7D, 4, 6>() == 0, "car7d rank 4");
static_assert(fpp_parked<LqgNd<6>, 8, 0>() == 0 && fpp_parked<LqgNd<6>, 8, 2>() == 0 && fpp_parked<LqgNd<6>, 8, 3>() == 0 &&
              fpp_parked<LqgNd<6>, 8, 5>() == 0, "lqg6d");
static_assert(fpp_parked<Dubins3D, 6, 0>() == 0 && fpp_parked<Dubins3D, 6, 1>() == 0 && fpp_parked<Dubins3D, 6, 2>() == 0, "dubins3d");
#define PARKED(K)                                                                                                                  \
    /* P + register-held = all folded vectors; six stay in registers at most, every parked one lies right of K */                  \
    static_assert(fpp_parked<Car7D, 10, K>() > 0 && fpp_parked<Car7D, 10, K>() < PairMap<Car7D, K>::nv(), "K = " #K);              \
    static_assert(PairMap<Car7D, K>::nv() - fpp_parked<Car7D, 10, K>() <= 6, "registers, K = " #K);                                \
    static_assert(PairMap<Car7D, K>::nv() - fpp_parked<Car7D, 10, K>() >= PairMap<Car7D, K>::SL::nv(), "parked slots right of K = " #K); \
    /* hand-over rows [0, (NV - P) RH) and L, R, VX, PX [0, px + rows) end below the homes: disjoint */                             \
    static_assert((PairMap<Car7D, K>::nv() - fpp_parked<Car7D, 10, K>()) * 5 <= fpp_parked_home_row<Car7D, 10, K>(), "hand-over, K = " #K); \
    static_assert(fpp_parked_px_row<10>() == 24 && fpp_parked_px_row<10>() + PairPark<Car7D, K>::rows() <= fpp_parked_home_row<Car7D, 10, K>(), \
                  "parked rows, K = " #K);                                                                                         \
    static_assert(fpp_parked_rows<Car7D, 10, K>() == fpp_parked_home_row<Car7D, 10, K>() + 10 * fpp_parked<Car7D, 10, K>(), "homes, K = " #K); \
    static_assert(fpp_tile_doubles<Car7D, 10, K>(true, true) == (size_t)fpp_parked_rows<Car7D, 10, K>() * 64, "launcher, K = " #K); \
    /* four workgroups in 160 KB with the tables of N = 41, nine candidates */                                                     \
    static_assert(4 * (fpp_tile_doubles<Car7D, 10, K>(true, true) + CandLds<Car7D>::doubles(9) + NodeLds<Car7D, K>::doubles(41)) * 8 <= 160 * 1024, \
                  "four workgroups, K = " #K);                                                                                     \
    /* the footprint does not move: below the rank-split rows and below the staged core image of the 41-node grid */               \
    static_assert(fpp_tile_doubles<Car7D, 10, K>(true, true) <= fpp_tile_doubles<Car7D, 10, K>(false), "rank-split rows, K = " #K); \
    static_assert(fpp_tile_doubles<Car7D, 10, K>(true, true) <= (size_t)41 * fpl_lds_stride(10 * 10), "staged image, K = " #K);
PARKED(2) PARKED(4)
static_assert(fpp_parked_rows<Car7D, 10, 2>() == 61 && fpp_parked_rows<Car7D, 10, 4>() == 31 + 10 * FPP_PARKED_K4, "rows as budgeted");
#endif
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_parked_predicate_and_lds(tmp_path):
    """Host-only: which instantiations take the form, that the old predicates did not move, and the row budget of a tile, as
    static_asserts on the constexpr functions the kernel and the launcher use (a syntax-only host pass over the headers)."""
    src = tmp_path / "parked_split.hip"
    src.write_text(PREDICATE_CHECKS)
    r = subprocess.run([HIPCC, "-std=c++20", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_resources_against_the_replaced_kernels():
    """the compiler's remarks of the build (pk_res/ for the new kernels): no more scratch and no more spilled VGPRs than the kernel
    each one stands in for, and the same static LDS"""
    new_p = os.path.join(CSRC, "pk_res", "kernel_resources.json")
    old_p = os.path.join(CSRC, "kernel_resources.json")
    assert os.path.exists(new_p) and os.path.exists(old_p), "the build keeps the resource tables next to the objects"
    new, old = json.load(open(new_p)), json.load(open(old_p))
    assert not [n for n in new if "_pk<" not in n], "the file of the parked kernels instantiates no kernel they replace"
    seen = 0
    for k in PARKED_K:
        for forced in ("false", "true"):
            for a, b in (("k_fiber_pair_pk", "k_fiber_pair"), ("k_fiber_pair_part_pk", "k_fiber_pair_part")):
                n, o = new[f"{a}<Car7D, 10, {k}, {forced}>"], old[f"{b}<Car7D, 10, {k}, {forced}>"]
                print(a, k, forced, {f: (o[f], n[f]) for f in ("vgprs", "vgpr_spill", "scratch_bytes_per_lane", "sgpr_spill", "static_lds_bytes")})
                assert n["scratch_bytes_per_lane"] <= o["scratch_bytes_per_lane"], (a, k, forced, o, n)
                assert n["vgpr_spill"] <= o["vgpr_spill"], (a, k, forced, o, n)
                assert n["static_lds_bytes"] == o["static_lds_bytes"], (a, k, forced, o, n)
                seen += 1
    assert seen == 8 and len(new) == 8
    assert not [n for n in old if "_pk<" in n], "the parked kernels keep out of the table of the earlier kernels"


def _engine(w, cores, cends=False):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    eng.set_variant(3)  # the fiber-pair kernel, forced
    eng.configure(w, cores)
    if cends:
        eng.set_consistent_ends(True)
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
    if ui is not None:  # argmin may only differ where the two values are within the bar
        bad = ui != ref_ui
        assert not bad.any() or np.abs(out - ref)[bad].max() <= REL_TOL * scale


def _kernel_ok(eng, k):
    assert eng.status() == 0
    assert eng.last_kernel() == f"k_fiber_pair<Car7D,10,K={k}>"  # the registry name does not change with the form


@pytest.fixture(scope="module", params=GRIDS, ids=[f"N{n}" for n in GRIDS])
def case(request, oracle):
    """engine + the oracle's answers for 200 fibers of every swept dimension, computed once and shared (read-only)"""
    w = wl.c4_car7d().scaled(ngrid=(request.param,) * 7, rank=10)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    return w, _engine(w, cores), {k: _ref(P, k, _fibers(w, k, max(COUNTS))) for k in SWEEP_K}


@pytest.mark.gpu
@pytest.mark.parametrize("F", COUNTS)
def test_parked_split_vs_oracle(case, F):
    """main sweep: K = 2, 4 (parked), 3 (rank split), 5 (node split) at every fiber count"""
    w, eng, refs = case
    assert PARKED_ENV not in os.environ and PART_ENV not in os.environ
    for k, (idx, ref, ref_ui, ref_ab) in refs.items():
        out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx[:F]))
        _kernel_ok(eng, k)
        _hold(w, k, out, ui, ab, ref[:F], ref_ui[:F], ref_ab[:F], f"F={F}")


@pytest.fixture(scope="module")
def base(oracle):
    w = wl.c4_car7d().scaled(ngrid=(6, 5, 6, 5, 6, 5, 6), rank=10)
    cores = wl.synth_cores(w)
    return w, cores


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARKED_K)
@pytest.mark.parametrize("bc", (wl.BC_PERIODIC, wl.BC_REFLECT, wl.BC_ABSORB), ids=("periodic", "reflect", "absorb"))
def test_boundary_in_dim_k(oracle, base, k, bc):
    """periodic (v[N-2] wraps to node 0: both wavefronts form it, each reading the homes), reflecting and absorbing ends of K"""
    w0, cores = base
    w = dataclasses.replace(w0, bc=tuple(bc if m == k else b for m, b in enumerate(w0.bc)))
    eng = _engine(w, cores)
    idx, ref, ref_ui, ref_ab = _ref(oracle.Problem(w, cores), k, _fibers(w, k, 65))
    out, ui, ab = eng.bellman_fibers_host(k, np.ascontiguousarray(idx))
    _kernel_ok(eng, k)
    _hold(w, k, out, ui, ab, ref, ref_ui, ref_ab, f"bc={bc}")


@pytest.fixture(scope="module")
def extra(oracle, base):
    w, cores = base
    P = oracle.Problem(w, cores)
    return w, _engine(w, cores), {k: _ref(P, k, _fibers(w, k, 65)) for k in PARKED_K}


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARKED_K)
def test_policy_evaluation(extra, k):
    """the FORCED instantiation: applying the oracle's own minimiser at every node must give the oracle's minimum"""
    w, eng, refs = extra
    idx, ref, ref_ui, ref_ab = refs[k]
    for F in (1, 65):
        out, ab = eng.policy_fibers_host(k, np.ascontiguousarray(idx[:F]), np.ascontiguousarray(ref_ui[:F]).astype(np.int32))
        _kernel_ok(eng, k)
        _hold(w, k, out, None, ab, ref[:F], ref_ui[:F], ref_ab[:F], f"forced F={F}")


def _with_env(fn, **env):
    """run fn() with the given variables set (None: unset); both switches are read at every launch"""
    saved = {n: os.environ.get(n) for n in env}
    try:
        for n, v in env.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v
        return fn()
    finally:
        for n, v in saved.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v


@pytest.mark.gpu
@pytest.mark.parametrize("k", PARKED_K)
def test_old_against_new(extra, k, capfd):
    """the same batch with C3SC_PAIR_PARKED=0: the rank-split kernels.  Flags equal, values within the bar of each other (another
    summation order inside a dot: no bit equality).  That the switch reaches the other kernels is read from the launcher's
    verbose line, which only a parked launch prints."""
    w, eng, refs = extra
    idx, ref, ref_ui, ref_ab = refs[k]
    run = lambda: eng.bellman_fibers_host(k, np.ascontiguousarray(idx))  # noqa: E731
    capfd.readouterr()
    new = _with_env(run, C3SC_PAIR_PARKED=None, C3SC_VERBOSE="1")
    said_new = capfd.readouterr().err
    old = _with_env(run, C3SC_PAIR_PARKED="0", C3SC_VERBOSE="1")
    said_old = capfd.readouterr().err
    _kernel_ok(eng, k)
    assert f"parked node split K={k}" in said_new and "parked node split" not in said_old
    print(said_new.strip())  # LDS bytes and workgroups per CU of the parked launch, as the occupancy query gives them
    _hold(w, k, new[0], new[1], new[2], ref, ref_ui, ref_ab, "parked")
    _hold(w, k, old[0], old[1], old[2], ref, ref_ui, ref_ab, "switched off")
    np.testing.assert_array_equal(new[2], old[2])
    scale = np.abs(ref).max()
    print(f"k={k} old against new: {np.abs(new[0] - old[0]).max() / scale:.3e} of the scale")
    assert np.abs(new[0] - old[0]).max() <= REL_TOL * scale
    bad = new[1] != old[1]
    assert not bad.any() or np.abs(new[0] - old[0])[bad].max() <= REL_TOL * scale


def _part_batch(w, k, F=300, seed=11):
    """F fibers, a third of them (at scattered positions) on an absorbing face of dimension 0"""
    idx = wl.synth_fibers(w, k, F).astype(np.int32)
    rng = np.random.default_rng(seed + 17 * k + w.ngrid[k])
    for m in (0, 1):  # both absorb: interior first
        idx[:, m] = 1 + idx[:, m] % (w.ngrid[m] - 2)
    dead = rng.permutation(F)[: F // 3]
    idx[dead[::2], 0] = 0
    idx[dead[1::2], 0] = w.ngrid[0] - 1
    idx[:, k] = 0
    return np.ascontiguousarray(idx)


@pytest.mark.gpu
@pytest.mark.parametrize("cends", (0, 1), ids=("literal", "consistent"))
@pytest.mark.parametrize("nk", (5, 6, 9, 10))
@pytest.mark.parametrize("k", PARKED_K)
def test_partitioned_path(oracle, k, nk, cends):
    """k_fiber_pair_part_pk behind the partition pre-pass, reflecting K: tiles of absorbed fibers under literal ends run only the
    first and the last trips of the node loop (the skip applies from T = N / 2 + 1 = 5 on and differs for odd and even T: N = 9,
    10 against 5, 6), under consistent ends none.  Bit-identical to the same batch with the pass off, held to the oracle, and
    the same bits in three launches."""
    w0 = wl.c4_car7d().scaled(ngrid=tuple(nk if m == k else 5 for m in range(7)), rank=10)
    w = dataclasses.replace(w0, bc=tuple(wl.BC_REFLECT if m == k else b for m, b in enumerate(w0.bc)))
    cores = wl.synth_cores(w)
    eng = _engine(w, cores, cends)
    P = oracle.Problem(w, cores, consistent_ends=bool(cends))
    idx = _part_batch(w, k)
    ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
    dead = (idx[:, 0] == 0) | (idx[:, 0] == w.ngrid[0] - 1)
    assert int(dead.sum()) == 100 and (ref_ab[dead][:, 1:-1] == 1).all()  # a third of the batch: more than one absorbed tile

    def run():
        n0 = eng.L.c3sc_hip_launch_count()
        r = eng.bellman_fibers_host(k, idx)
        return r + (eng.L.c3sc_hip_launch_count() - n0,)

    on = [_with_env(run, C3SC_FIBER_PARTITION="1") for _ in range(3)]
    off = _with_env(run, C3SC_FIBER_PARTITION="0")
    _kernel_ok(eng, k)
    assert off[3] == 1 and all(o[3] == 4 for o in on), "three partition launches in front of the kernel's one, or none"
    _hold(w, k, on[0][0], on[0][1], on[0][2], ref, ref_ui, ref_ab, f"cends={cends} partitioned")
    _hold(w, k, off[0], off[1], off[2], ref, ref_ui, ref_ab, f"cends={cends} pass off")
    for o in on:
        for a, b in zip(o[:3], off[:3]):
            np.testing.assert_array_equal(a, b)
