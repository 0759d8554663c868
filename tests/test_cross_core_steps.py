"""The device-resident cross core steps (c3sc_amd/csrc/cross_device.hip) against a dense float64 reference (cross_reference.py).

tests/test_solver_loops.py holds the device path to its host twin (lu_maxvol in c3sc_cross.c) bit for bit; a mistake both
share, or a shape the adaptive solver never reaches, passes there.  Here the C-ABI is driven directly with CHOSEN per-bond ranks
and seeded index sets, and every step of the iteration is checked with numpy: nested distinct sets, an interpolatory core, maxvol
dominance, raw values of core 0, the memo's node count.

Dispatch of a core step (cross_iteration_impl; core_step, core_step_regs, core_step_global), m x n the step's matrix
(left-to-right: m = r_k N_k, n = r_{k+1}; right-to-left: m = N_k r_{k+1}, n = r_k), F N_k = r_k r_{k+1} N_k:
  copy        the last step of a half sweep (core 0 = the raw fiber values; the left-to-right step d-1 only evaluates)
  regs-1      F N_k 8 <= LDS_CAP_BYTES (132 KB), r_k, r_{k+1} <= 32, n <= 16, m <= 512: rows in registers, one per thread
  regs-2      the same with 512 < m <= 1024: two rows per thread
  lds         F N_k 8 <= 132 KB and r_k, r_{k+1} <= 32, but n > 16 or m > 1024: core_step<true>, the matrix in LDS
  global-NR   anything else: core_step_global<NR> on global scratch, NR = 32 / 40 / 48 the padding of n (a step may land here
              with n <= 16 when the OTHER rank exceeds 32); "panels" for m <= 2048 (register panels of the left-looking LU),
              "tall" beyond
The batched confirmation (c3sc_hip_cross_confirm) runs every step in LDS if all fit, otherwise every step on its own scratch
block as core_step_global<NR> with NR the padding of the LARGEST rank of the train.

Value functions are synth_cores at value rank 4 with consistent ends on.  Index-set tuples avoid the end nodes of absorbing dimensions: a
fiber through the node 0 or N - 1 of an absorbing dimension is constant, two such columns make a matrix singular, and every case
here is chosen so that all its matrices have full rank (cond(A[P]) at most a few 1e7, info[1] == 0).  For the same reason the rank-1 bond
sits in lqg6d (reflecting boundaries): behind a rank-1 bond of car7d the one pivot node lies on an absorbing face.
The singular matrices that production does factor are held in test_gpu_cross_singular_steps.py.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cross_reference as cr  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402
from cross_device_lib import SWAP_TOL, DeviceCross, interior_tuples, step_classes  # noqa: E402

pytestmark = pytest.mark.gpu

C3SC_ERR_ARG, C3SC_ERR_UNSUPPORTED = 1, 3


def _case(name, ngrid, ranks, seed):
    w = wl.WORKLOADS[name]().scaled(ngrid=ngrid, rank=4)
    cores = wl.synth_cores(w)
    d = w.dx
    rng = np.random.default_rng(seed)
    I = [interior_tuples(rng, w, range(k), ranks[k]) for k in range(d)]
    J = [interior_tuples(rng, w, range(k + 1, d), ranks[k + 1]) for k in range(d)]
    return w, cores, I, J


# (id, workload, grid, cross ranks, the dispatch classes the case is there for)
CASES = [
    ("regs-one-row", "car7d", (41,) * 7, (1, 10, 10, 10, 10, 10, 10, 1), {"regs-1"}),                 # 410 x 10
    ("regs-two-rows", "dubins3d", (101,) * 3, (1, 8, 8, 1), {"regs-2"}),                              # 808 x 8
    ("lds-17-columns-and-cap", "car7d", (41,) * 7, (1, 17, 24, 18, 24, 10, 10, 1), {"lds", "global-32-panels"}),
    # ^ 41 x 17 and 984 x 17 leave the register step; 17 x 24 x 41 x 8 = 133 824 B is just under the LDS cap, 18 x 24 x 41 x 8 =
    #   141 696 B just over (global scratch at ranks <= 32)
    ("global-nr-32-40-48", "car7d", (41,) * 7, (1, 32, 33, 40, 41, 48, 40, 1),
     {"global-32-panels", "global-40-panels", "global-48-panels"}),                                   # ranks 32 | 33, 40 | 41, 48
    ("global-tall", "dubins3d", (101,) * 3, (1, 24, 24, 1), {"global-32-tall"}),                      # 2424 x 24
    ("rank-1-bond", "lqg6d", (31,) * 6, (1, 8, 1, 8, 8, 8, 1), {"regs-1"}),                           # one-column matrices mid-train
    # the largest row count the registered Bellman kernels can feed: max_n = 128 (two nodes per lane) x rank 48 = 6144 rows
    # (MAXROWS = 8192 is not reachable through them)
    ("max-rows-6144", "dubins3d", (41, 128, 101), (1, 8, 48, 1), {"global-32-tall", "global-48-panels"}),
    # unequal grids: car7d with the overrunning confirm layout (1536-row steps at ranks 24 under a rank-33 train) and a 3-D case
    ("unequal-car7d", "car7d", (41, 41, 41, 64, 64, 41, 41), (1, 33, 33, 24, 24, 24, 24, 1), {"global-32-panels", "global-40-panels"}),
    ("unequal-dubins3d", "dubins3d", (101, 41, 41), (1, 24, 33, 1), {"lds", "global-32-panels", "global-40-panels"}),
]


def _print_report(cid, classes, rep):
    by = {}
    for s in rep["steps"]:
        c = classes[(s["dir"], s["k"])]
        b = by.setdefault(c, dict(res=0.0, dom=0.0, cond=0.0, shapes=set()))
        b["res"] = max(b["res"], s["residual"] or 0.0)
        b["dom"] = max(b["dom"], s["dominance"])
        b["cond"] = max(b["cond"], s["cond"])
        b["shapes"].add(f"{s['m']}x{s['n']}")
    for c, b in sorted(by.items()):
        print(f"{cid}: {c:18s} {sorted(b['shapes'])}: worst residual {b['res']:.2e}, dominance {b['dom']:.6f}, cond(A[P]) {b['cond']:.2e}")
    print(f"{cid}: core 0 vs oracle {rep['raw']:.2e}, {rep['nodes']} distinct nodes")


@pytest.mark.parametrize("cid,name,ngrid,ranks,want", CASES, ids=[c[0] for c in CASES])
def test_core_steps_against_the_dense_reference(oracle, cid, name, ngrid, ranks, want):
    w, cores, I, J = _case(name, ngrid, ranks, seed=7)
    classes = step_classes(w.ngrid, ranks)
    assert want <= set(classes.values()), f"case {cid} reaches {sorted(set(classes.values()))}, meant for {sorted(want)}"
    dev = DeviceCross(w, cores)
    try:
        rc = dev.setup(ranks, I, J)
        assert rc == 0, f"cross_setup: code {rc}: {dev.err()}"
        dev.iteration()
        gcores, gI, gJ, info = dev.fetch()
    finally:
        dev.close()
    P = oracle.Problem(w, cores, consistent_ends=True)
    rep = cr.check_iteration(P, ranks, J, gcores, gI, gJ, info, swap_tol=SWAP_TOL, label=cid)
    _print_report(cid, classes, rep)


def test_unsupported_layouts_are_refused_before_any_launch():
    """cross_setup / cross_confirm return their C3SC_ERR_* code and launch nothing."""
    from c3sc_amd.engine import load_library

    L = load_library()
    L.c3sc_hip_launch_count.restype = C.c_ulonglong

    def refused(w, ranks, code, what):
        dev = DeviceCross(w, wl.synth_cores(w))
        try:
            d = w.dx
            I = [np.zeros((ranks[k], k), dtype=np.int32) for k in range(d)]
            J = [np.zeros((ranks[k + 1], d - 1 - k), dtype=np.int32) for k in range(d)]
            n0 = L.c3sc_hip_launch_count()
            rc = dev.setup(ranks, I, J)
            assert rc == code, f"{what}: cross_setup returned {rc} ({dev.err()}), expected {code}"
            assert L.c3sc_hip_launch_count() == n0, f"{what}: something was launched"
            print(f"{what}: code {rc}: {dev.err()}")
        finally:
            dev.close()

    # r_1 N_0 = 3 x 2731 = 8193 rows: one more than the one-workgroup factorisation holds
    refused(wl.c1_lqg2d().scaled(ngrid=(2731, 5), rank=4), (1, 3, 1), C3SC_ERR_UNSUPPORTED, "8193 rows")
    refused(wl.c4_car7d().scaled(ngrid=(41,) * 7, rank=4), (1, 10, 10, 49, 10, 10, 10, 1), C3SC_ERR_UNSUPPORTED, "rank 49")
    refused(wl.c4_car7d().scaled(ngrid=(41,) * 7, rank=4), (2, 10, 10, 10, 10, 10, 10, 1), C3SC_ERR_ARG, "ranks[0] = 2")
    w = wl.c4_car7d().scaled(ngrid=(11,) * 7, rank=4)
    dev = DeviceCross(w, wl.synth_cores(w))
    try:
        ok = C.c_int(-1)
        n0 = L.c3sc_hip_launch_count()
        rc = L.c3sc_hip_cross_confirm(dev.h, C.byref(ok), None)
        assert rc == C3SC_ERR_ARG, f"cross_confirm before cross_setup returned {rc}"
        assert L.c3sc_hip_launch_count() == n0
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ the batched confirmation
CONFIRM_CASES = [
    ("unequal-car7d", "car7d", (41, 41, 41, 64, 64, 41, 41), (1, 33, 33, 24, 24, 24, 24, 1)),
    # every rank <= 32, but 24 x 18 x 41 exceeds the LDS cap: the all-global form of the confirmation at NR = 32
    ("all-global-ranks-le-32", "car7d", (41,) * 7, (1, 17, 24, 18, 24, 10, 10, 1)),
    # the benched layout, ranks 41 / 48 padded to 48; the first bond at 38: the nodes 0 and 40 of car7d's absorbing first
    # dimension give equal rows, so 41 x 41 would be singular
    ("bench-layout-41-48", "car7d", (41,) * 7, (1, 38, 48, 48, 48, 48, 41, 1)),
]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("cid,name,ngrid,ranks", CONFIRM_CASES, ids=[c[0] for c in CONFIRM_CASES])
def test_batched_confirmation_matches_the_sequential_iteration(oracle, cid, name, ngrid, ranks):
    """Contexts A and B, same set-up and history.  After every iteration that changed the sets A confirms and B iterates:
    confirmed must equal 'B's sets did not change', and a confirmed A holds B's cores and sets bit for bit.  A failed
    confirmation is followed by the sequential iteration on A too (same sets, warm pivots and memo epoch as B)."""
    w, cores, I, J = _case(name, ngrid, ranks, seed=11)
    A, B = DeviceCross(w, cores), DeviceCross(w, cores)
    P = oracle.Problem(w, cores, consistent_ends=True)
    outcomes = []
    try:
        for dev in (A, B):
            rc = dev.setup(ranks, I, J)
            assert rc == 0, f"cross_setup: code {rc}: {dev.err()}"
            dev.iteration()
        a, b = A.fetch(), B.fetch()
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2]), "A and B differ after the same iteration"
        prev = b
        for t in range(10):
            confirmed = A.confirm()
            B.iteration()
            b = B.fetch()
            unchanged = _same(b[1], prev[1]) and _same(b[2], prev[2])
            outcomes.append(confirmed)
            assert confirmed == unchanged, f"iteration {t + 2}: confirmed {confirmed}, but the sequential iteration " \
                                           f"{'kept' if unchanged else 'changed'} the index sets"
            if confirmed:
                a = A.fetch()
                for k in range(w.dx):
                    assert np.array_equal(a[0][k], b[0][k]), f"core {k}: confirmed core differs from the sequential one " \
                                                             f"(max {np.abs(a[0][k] - b[0][k]).max():.3e})"
                assert _same(a[1], b[1]) and _same(a[2], b[2]), "confirmed index sets differ from the sequential ones"
                assert b[3][1] == 0, "the sequential iteration flagged a rank-deficient matrix"
                rep = cr.check_iteration(P, ranks, prev[2], b[0], b[1], b[2], None, swap_tol=SWAP_TOL, label=cid)
                _print_report(cid, step_classes(w.ngrid, ranks), rep)
                break
            A.iteration()
            a = A.fetch()
            assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2]), "A and B differ after the same iteration"
            prev = b
        else:
            pytest.fail(f"{cid}: the index sets still change after 10 iterations")
    finally:
        A.close()
        B.close()
    print(f"{cid}: confirmations {outcomes}")
    # from random sets the second iteration still moves them: the first confirmation must fail, the last one succeeds
    assert outcomes[0] is False and outcomes[-1] is True, f"{cid}: confirmations {outcomes}"
