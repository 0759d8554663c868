"""Absorbed tiles of the pair kernel (fiber_partition.hpp; kernel_fiber_pair.hpp: dead_tile).

A fiber with a fixed index on an absorbing face is absorbed at every node.  A fiber-pair launch of a batch that can hold such
fibers is preceded by a stable partition on the device (live fibers first), the kernel's tiles read their fibers through it, and a
tile of absorbed fibers writes Model::boundcost without staging, folding or scanning -- except, under the literal end-point rule
with a reflecting or periodic varying dimension, the two end nodes, which still get their full backup.

Every case forces the pair variant, runs the batch with the pass on (C3SC_FIBER_PARTITION=1: every batch size) and off (=0) on
the same library, and holds
  * the run with the pass on to the oracle at the project's bar: `absorbed` bit-exact, `uidx` bit-exact (an argmin may differ on
    an exact tie only), values within 1e-12 of the value scale;
  * the two runs to each other: BIT-IDENTICAL values, uidx and flags for the undiscounted models (car7d, dubins3d); for the
    discounted one (lqg6d with absorbing faces) within the oracle bar, because its scan picks the form of the discount factor by
    wave vote and the partition changes a fiber's tile-mates;
  * every output row to be written: the outputs are pre-filled with NaN / a sentinel and none may remain.
That the pass ran (or did not) is read from c3sc_hip_launch_count: three partition launches in front of the kernel's one.

Batches: 200 fibers (four tiles, the last one partial) with hand-built face indices -- no dead fiber; every fiber dead; 130 live
(tiles 0, 1 live, tile 2 mixed, tile 3 dead); 128 live (nlive a multiple of 64); 136 live (64 dead); 256 fibers with 128 dead (F a
multiple of 64); F = 1 live and dead.  Varying dimensions: car7d K = 0 (absorbing), 5 (reflecting, node split), 3 (reflecting, rank
split), 2 (periodic, rank split); dubins3d K = 0 and 2 (direct fold).  N_K = 2, 3, 5, 6 at a grid of 5 (6 for dubins3d) in the
fixed dimensions, and N_K = 10, 13, 41: an absorbed tile under literal ends leaves the trips between the first and the last two
(three in the node split where T = N / 2 + 1 is even: the exchange rows alternate with the trip's parity) out of the node loop,
which starts at T = 5; 10 and 13 are one even and one odd T, 41 is the benchmark's.  Both end-point rules.  One case runs 2^19
fibers with the variable unset: the default threshold."""
import dataclasses
import os

import numpy as np
import pytest

from c3sc_amd import workloads as wl

REL_TOL = 1e-12
ENV = "C3SC_FIBER_PARTITION"
# (F, number of dead fibers)
BATCHES = {"none": (200, 0), "all": (200, 200), "mixed": (200, 70), "live128": (200, 72), "dead64": (200, 64), "f256": (256, 128),
           "one-live": (1, 0), "one-dead": (1, 1)}


def _engine(w, cores, cends):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    eng.set_variant(3)  # the fiber-pair kernel, forced
    eng.configure(w, cores)
    eng.set_consistent_ends(bool(cends))
    return eng


def _faces(w, k):
    return [m for m in range(w.dx) if m != k and w.bc[m] == wl.BC_ABSORB]


def _batch(w, k, F, ndead, seed=7):
    """F fibers of which exactly ndead (at scattered positions) have a fixed index on an absorbing face"""
    idx = wl.synth_fibers(w, k, F).astype(np.int32)
    rng = np.random.default_rng(seed + 131 * k + F)
    faces = _faces(w, k)
    for m in faces:  # everything live first: interior indices in the absorbing dimensions
        idx[:, m] = 1 + idx[:, m] % (w.ngrid[m] - 2)
    dead = rng.permutation(F)[:ndead]
    for n, f in enumerate(dead):
        m = faces[n % len(faces)]
        idx[f, m] = 0 if (n // len(faces)) % 2 == 0 else w.ngrid[m] - 1
    idx[:, k] = 0
    return np.ascontiguousarray(idx)


def _launch(eng, k, idx, mode, policy=None, want_uidx=True, want_absorbed=True):
    """one launch through the device API with pre-filled outputs; returns (out, ui, ab, launches).  mode: the value of the
    environment variable, None: unset"""
    import torch

    os.environ.pop(ENV, None)
    if mode is not None:
        os.environ[ENV] = mode
    try:
        dev = torch.device("cuda", 0)
        F, N = idx.shape[0], eng.ngrid[k]
        idx_t = torch.from_numpy(idx).to(dev)
        out_t = torch.full((F, N), float("nan"), dtype=torch.float64, device=dev)
        ui_t = torch.full((F, N), -77, dtype=torch.int32, device=dev) if want_uidx and policy is None else None
        ab_t = torch.full((F, N), -77, dtype=torch.int32, device=dev) if want_absorbed else None
        sp = torch.cuda.current_stream(dev).cuda_stream
        n0 = eng.L.c3sc_hip_launch_count()
        if policy is None:
            eng.bellman_fibers(k, idx_t, out_t, ui_t, ab_t, stream_ptr=sp)
        else:
            pol_t = torch.from_numpy(np.ascontiguousarray(policy, dtype=np.int32)).to(dev)
            eng._chk(eng.L.c3sc_hip_policy_fibers(eng.h, k, F, idx_t.data_ptr(), pol_t.data_ptr(), out_t.data_ptr(),
                                                  ab_t.data_ptr() if ab_t is not None else None, sp), "policy_fibers")
        launches = eng.L.c3sc_hip_launch_count() - n0
        torch.cuda.synchronize(dev)
        assert eng.status() == 0
        assert "k_fiber_pair" in eng.last_kernel()
        get = lambda t: None if t is None else t.cpu().numpy()
        return get(out_t), get(ui_t), get(ab_t), launches
    finally:
        os.environ.pop(ENV, None)


def _written(out, ui, ab):
    assert not np.isnan(out).any(), f"{int(np.isnan(out).sum())} values were never written"
    for a in (ui, ab):
        if a is not None:
            assert not (a == -77).any(), "an integer output row was never written"


def _hold(out, ui, ab, ref, ref_ui, ref_ab, what):
    scale = np.abs(ref).max()
    if ab is not None:
        np.testing.assert_array_equal(ab, ref_ab)
    err = np.abs(out - ref).max()
    print(f"{what}: err {err:.3e} scale {scale:.3e}")
    assert err <= REL_TOL * scale, f"{what}: err {err:.3e} scale {scale:.3e}"
    if ui is not None:  # argmin may only differ on exact ties
        bad = ui != ref_ui
        assert not bad.any() or np.abs(out - ref)[bad].max() <= REL_TOL * scale


def _check(eng, P, w, k, idx, what, bitwise=True, expect_pass=True, **kw):
    on = _launch(eng, k, idx, "1", **kw)
    off = _launch(eng, k, idx, "0", **kw)
    _written(*on[:3])
    _written(*off[:3])
    assert off[3] == 1, "the switch must turn the partition off"
    assert on[3] == (4 if expect_pass else 1), f"{what}: {on[3]} launches"
    ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
    _hold(on[0], on[1], on[2], ref, ref_ui, ref_ab, what)
    if bitwise:
        for a, b in zip(on[:3], off[:3]):
            if a is not None:
                np.testing.assert_array_equal(a, b)
    else:
        _hold(on[0], on[1], on[2], off[0], off[1], off[2], what + " (on against off)")
    return ref, ref_ui, ref_ab


def _car7d(k, nk, n=5):
    return wl.c4_car7d().scaled(ngrid=tuple(nk if m == k else n for m in range(7)), rank=10)


_cache = {}


def _setup(oracle, w, cends):
    key = (w.name, w.ngrid, w.bc, cends)
    if key not in _cache:
        cores = wl.synth_cores(w)
        _cache[key] = (_engine(w, cores, cends), oracle.Problem(w, cores, consistent_ends=bool(cends)))
    return _cache[key]


CAR_K = {0: "absorb", 5: "reflect-nodesplit", 3: "reflect-ranksplit", 2: "periodic-ranksplit"}


@pytest.mark.gpu
@pytest.mark.parametrize("cends", (0, 1))
@pytest.mark.parametrize("k", CAR_K, ids=CAR_K.values())
def test_car7d_batches(oracle, k, cends):
    """every batch composition at an even N; undiscounted: on and off bit-identical"""
    w = _car7d(k, 6)
    eng, P = _setup(oracle, w, cends)
    for name, (F, ndead) in BATCHES.items():
        _check(eng, P, w, k, _batch(w, k, F, ndead), f"car7d k={k} cends={cends} {name}")
    assert eng.last_kernel() == f"k_fiber_pair<Car7D,10,K={k}>"


@pytest.mark.gpu
@pytest.mark.parametrize("cends", (0, 1))
@pytest.mark.parametrize("nk", (2, 3, 5))
@pytest.mark.parametrize("k", CAR_K, ids=CAR_K.values())
def test_car7d_node_counts(oracle, k, nk, cends):
    """N_K = 2 and 3 (the four node indices 0, 1, N-2, N-1 overlap) and an odd N; mixed and all-dead batches"""
    w = _car7d(k, nk)
    eng, P = _setup(oracle, w, cends)
    for name in ("mixed", "all"):
        F, ndead = BATCHES[name]
        _check(eng, P, w, k, _batch(w, k, F, ndead), f"car7d k={k} N={nk} cends={cends} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("cends", (0, 1))
@pytest.mark.parametrize("nk", (10, 13, 41))
@pytest.mark.parametrize("k", (5, 3, 2), ids=[CAR_K[k] for k in (5, 3, 2)])
def test_car7d_long_fibers(oracle, k, nk, cends):
    """more than one trip of the node loop left out, in both parities of T = N / 2 + 1, and the benchmark's N = 41: the values
    the end nodes read (v[1], v[N-2]) and the exchange rows must survive the jump"""
    w = _car7d(k, nk)
    eng, P = _setup(oracle, w, cends)
    for name in ("mixed", "all"):
        F, ndead = BATCHES[name]
        _check(eng, P, w, k, _batch(w, k, F, ndead), f"car7d k={k} N={nk} cends={cends} {name}")


@pytest.mark.gpu
def test_default_threshold_runs_the_partition(oracle):
    """2^19 fibers with the variable unset: the pass runs by default (three launches more) and the values are bit for bit those
    of the run with the pass off; the small batches above hold the same code to the oracle"""
    k = 5
    w = _car7d(k, 13)
    eng, _ = _setup(oracle, w, 0)
    small = _batch(w, k, 4096, 1300)
    idx = np.ascontiguousarray(np.tile(small, (128, 1)))
    on = _launch(eng, k, idx, None)
    off = _launch(eng, k, idx, "0")
    assert on[3] == 4 and off[3] == 1
    _written(*on[:3])
    for a, b in zip(on[:3], off[:3]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("cends", (0, 1))
@pytest.mark.parametrize("k", (0, 2))
def test_dubins3d_direct_fold(oracle, k, cends):
    """a direct-fold kernel: K = 0 absorbing (y absorbs too), K = 2 periodic with both fixed dimensions absorbing"""
    w = wl.c2_dubins().scaled(ngrid=(6, 5, 7), rank=6)
    eng, P = _setup(oracle, w, cends)
    for name in ("none", "all", "mixed", "live128", "one-dead"):
        F, ndead = BATCHES[name]
        _check(eng, P, w, k, _batch(w, k, F, ndead), f"dubins3d k={k} cends={cends} {name}")
    assert eng.last_kernel() == f"k_fiber_pair<Dubins3D,6,K={k}>"


@pytest.mark.gpu
@pytest.mark.parametrize("cends", (0, 1))
@pytest.mark.parametrize("k", (5, 3, 0))
def test_policy_evaluation_and_optional_outputs(oracle, k, cends):
    """the FORCED instantiation (the oracle's own minimiser applied must give the oracle's minimum), and the minimising one with
    uidx / absorbed not requested"""
    w = _car7d(k, 6)
    eng, P = _setup(oracle, w, cends)
    idx = _batch(w, k, *BATCHES["mixed"])
    ref, ref_ui, ref_ab = _check(eng, P, w, k, idx, f"k={k} cends={cends} no uidx, no flags", want_uidx=False, want_absorbed=False)
    on = _launch(eng, k, idx, "1", policy=ref_ui)
    off = _launch(eng, k, idx, "0", policy=ref_ui)
    assert on[3] == 4 and off[3] == 1
    _written(*on[:3])
    _hold(on[0], None, on[2], ref, ref_ui, ref_ab, f"k={k} cends={cends} forced")
    np.testing.assert_array_equal(on[0], off[0])
    np.testing.assert_array_equal(on[2], off[2])


@pytest.mark.gpu
@pytest.mark.parametrize("cends", (0, 1))
@pytest.mark.parametrize("k", (2, 0))
def test_discounted_model_with_absorbing_faces(oracle, k, cends):
    """lqg6d (discount 0.1) with two faces set to absorb: the discounted scan votes per wave on the form of the discount factor,
    so on against off is held to the oracle bar, not to bit identity"""
    w0 = wl.c3_lqg6d().scaled(ngrid=(5, 5, 6, 5, 5, 5), rank=8)
    w = dataclasses.replace(w0, bc=(wl.BC_ABSORB, wl.BC_ABSORB) + w0.bc[2:])
    eng, P = _setup(oracle, w, cends)
    for name in ("mixed", "all", "live128"):
        F, ndead = BATCHES[name]
        _check(eng, P, w, k, _batch(w, k, F, ndead), f"lqg6d+faces k={k} cends={cends} {name}", bitwise=False)


@pytest.mark.gpu
def test_no_absorbing_dimension_launches_no_partition(oracle):
    """lqg6d reflects everywhere: no partition kernel is launched, the call's launch count is the kernel's one; the same for
    car7d K = 0 run on a batch below the default threshold with the variable unset"""
    import torch

    w = wl.c3_lqg6d().scaled(ngrid=(5,) * 6, rank=8)
    eng, P = _setup(oracle, w, 0)
    idx = np.ascontiguousarray(wl.synth_fibers(w, 2, 200).astype(np.int32))
    _check(eng, P, w, 2, idx, "lqg6d", bitwise=True, expect_pass=False)
    w = _car7d(5, 6)
    eng, P = _setup(oracle, w, 0)
    idx_t = torch.from_numpy(_batch(w, 5, 200, 70)).cuda()
    assert ENV not in os.environ
    n0 = eng.L.c3sc_hip_launch_count()
    eng.bellman_fibers(5, idx_t)
    torch.cuda.synchronize()
    assert eng.L.c3sc_hip_launch_count() - n0 == 1


@pytest.mark.gpu
@pytest.mark.parametrize("cends", (0, 1))
def test_bellman_fibers_all_streams(oracle, cends):
    """all seven varying dimensions of one batch in one call: three streams, each with its own partition scratch; every
    dimension's result is bit-identical to its single launch with the pass off"""
    import torch

    w = wl.c4_car7d().scaled(ngrid=(5, 6, 5, 6, 5, 6, 5), rank=10)
    eng, P = _setup(oracle, w, cends)
    ks = list(range(7))
    idx = [_batch(w, k, 200 + 8 * k, 70 + k) for k in ks]
    offs = [_launch(eng, k, idx[k], "0")[0] for k in ks]
    os.environ[ENV] = "1"
    try:
        idx_t = [torch.from_numpy(a).cuda() for a in idx]
        out_t = [torch.full((a.shape[0], w.ngrid[k]), float("nan"), dtype=torch.float64, device="cuda") for k, a in zip(ks, idx)]
        n0 = eng.L.c3sc_hip_launch_count()
        for _ in range(2):  # the second call reuses the scratch of the first
            eng.bellman_fibers_all(ks, idx_t, out_t)
        torch.cuda.synchronize()
        assert eng.L.c3sc_hip_launch_count() - n0 == 2 * 7 * 4
    finally:
        os.environ.pop(ENV, None)
    assert eng.status() == 0
    for k in ks:
        np.testing.assert_array_equal(out_t[k].cpu().numpy(), offs[k])
        ref = P.bellman_fibers(k, idx[k])[0]
        assert np.abs(offs[k] - ref).max() <= REL_TOL * np.abs(ref).max()
