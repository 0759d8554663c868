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

pytestmark = pytest.mark.gpu

C3SC_ERR_ARG, C3SC_ERR_UNSUPPORTED = 1, 3
LDS_CAP_BYTES, MAXROWS = 132 * 1024, 8192
SWAP_TOL = 0.05
c_i32_p = C.POINTER(C.c_int32)
c_double_p = C.POINTER(C.c_double)


def _pad(n):
    return 32 if n <= 32 else 40 if n <= 40 else 48


def dispatch_class(r0, N, r1, direction, copy_only):
    """The kernel a step of the sequential iteration is launched with (cross_iteration_impl)."""
    if copy_only:
        return "copy"
    m, n = (r0 * N, r1) if direction == 0 else (N * r1, r0)
    if r0 * r1 * N * 8 <= LDS_CAP_BYTES and r0 <= 32 and r1 <= 32:
        if n <= 16 and m <= 1024:
            return "regs-1" if m <= 512 else "regs-2"
        return "lds"
    return f"global-{_pad(n)}-" + ("panels" if m <= 2048 else "tall")


def step_classes(ngrid, ranks):
    d = len(ngrid)
    out = {}
    for k in range(d):
        out[("lr", k)] = dispatch_class(ranks[k], ngrid[k], ranks[k + 1], 0, k == d - 1)
    for k in range(d - 1, -1, -1):
        out[("rl", k)] = dispatch_class(ranks[k], ngrid[k], ranks[k + 1], 1, k == 0)
    return out


def interior_tuples(rng, w, dims, r):
    """r distinct tuples over `dims`, entries of an absorbing dimension in 1 .. N - 2 (see the module docstring)"""
    lo = [1 if w.bc[m] == wl.BC_ABSORB else 0 for m in range(w.dx)]
    space = int(np.prod([w.ngrid[m] - 2 * lo[m] for m in dims])) if dims else 1
    assert r <= space, f"{r} distinct tuples over dims {list(dims)} do not exist"
    seen, out = set(), []
    while len(out) < r:
        t = tuple(int(rng.integers(lo[m], w.ngrid[m] - lo[m])) for m in dims)
        if t not in seen:
            seen.add(t)
            out.append(t)
    return np.array(out, dtype=np.int32).reshape(r, len(dims))


def _ptrs(arrs, ctype, ptype):
    keep = [np.ascontiguousarray(a, dtype=ctype).reshape(-1) if np.size(a) else np.zeros(1, dtype=ctype) for a in arrs]
    p = (ptype * len(keep))(*[a.ctypes.data_as(ptype) for a in keep])
    p._keep = keep
    return p


class DeviceCross:
    """One BellmanEngine context driven through c3sc_hip_cross_* (null stream)."""

    def __init__(self, w, cores):
        from c3sc_amd.engine import BellmanEngine

        self.eng = BellmanEngine(0)
        self.eng.configure(w, cores)
        self.eng.set_consistent_ends(True)
        self.L, self.h, self.w = self.eng.L, self.eng.h, w

    def err(self):
        msg = self.L.c3sc_hip_last_error(self.h)
        return msg.decode() if msg else ""

    def setup(self, ranks, I, J, new_sweep=1):
        self.ranks = [int(r) for r in ranks]
        rk = np.ascontiguousarray(ranks, dtype=np.uintp)
        return self.L.c3sc_hip_cross_setup(self.h, rk.ctypes.data_as(C.POINTER(C.c_size_t)), _ptrs(I, np.int32, c_i32_p),
                                           _ptrs(J, np.int32, c_i32_p), new_sweep)

    def iteration(self):
        rc = self.L.c3sc_hip_cross_iteration(self.h, 0, None)
        assert rc == 0, f"cross_iteration: code {rc}: {self.err()}"

    def confirm(self):
        ok = C.c_int(-1)
        rc = self.L.c3sc_hip_cross_confirm(self.h, C.byref(ok), None)
        assert rc == 0, f"cross_confirm: code {rc}: {self.err()}"
        return bool(ok.value)

    def fetch(self):
        d, N, r = self.w.dx, self.w.ngrid, self.ranks
        cores = [np.zeros(r[k] * N[k] * r[k + 1]) for k in range(d)]
        I = [np.zeros((r[k], k), dtype=np.int32) for k in range(d)]
        J = [np.zeros((r[k + 1], d - 1 - k), dtype=np.int32) for k in range(d)]
        pc, pI, pJ = _ptrs(cores, np.float64, c_double_p), _ptrs(I, np.int32, c_i32_p), _ptrs(J, np.int32, c_i32_p)
        info = (C.c_ulonglong * 4)()
        rc = self.L.c3sc_hip_cross_fetch(self.h, pc, pI, pJ, info, None)
        assert rc == 0, f"cross_fetch: code {rc}: {self.err()}"
        cores = [a.copy() for a in pc._keep]
        I = [pI._keep[k][: r[k] * k].reshape(r[k], k).copy() for k in range(d)]
        J = [pJ._keep[k][: r[k + 1] * (d - 1 - k)].reshape(r[k + 1], d - 1 - k).copy() for k in range(d)]
        return cores, I, J, list(info)

    def close(self):
        self.eng.close()


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
