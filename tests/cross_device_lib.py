"""What the tests of the device-resident cross core steps share (test_cross_core_steps.py, test_gpu_cross_singular_steps.py and
the CPU simulation of their cases in test_cross_reference.py): the dispatch class of every step of an iteration, seeded index
tuples, and one BellmanEngine context driven through the c3sc_hip_cross_* entry points."""
import ctypes as C
import time

import numpy as np

from c3sc_amd import workloads as wl

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
    """One BellmanEngine context driven through c3sc_hip_cross_* (null stream).  consistent_ends=False keeps the reference's
    literal end-point rule; variant forces a kernel family (C3SC_VARIANT_*), set before the value is uploaded."""

    def __init__(self, w, cores, consistent_ends=True, variant=None):
        from c3sc_amd.engine import BellmanEngine

        self.eng = BellmanEngine(0)
        if variant is not None:
            self.eng.set_variant(variant)
        self.eng.configure(w, cores)
        self.eng.set_consistent_ends(consistent_ends)
        self.L, self.h, self.w = self.eng.L, self.eng.h, w

    def err(self):
        msg = self.L.c3sc_hip_last_error(self.h)
        return msg.decode() if msg else ""

    def setup(self, ranks, I, J, new_sweep=1):
        self.ranks = [int(r) for r in ranks]
        rk = np.ascontiguousarray(ranks, dtype=np.uintp)
        self._setup_args = (rk.ctypes.data_as(C.POINTER(C.c_size_t)), _ptrs(I, np.int32, c_i32_p), _ptrs(J, np.int32, c_i32_p), new_sweep)
        self._setup_keep = rk
        return self.L.c3sc_hip_cross_setup(self.h, *self._setup_args)

    def setup_repeat(self, n, new_sweep=1):
        """the last set-up again, n times, without an iteration in between (n new memo epochs); returns the seconds it took"""
        args = self._setup_args[:-1] + (new_sweep,)
        t0 = time.perf_counter()
        for i in range(n):
            rc = self.L.c3sc_hip_cross_setup(self.h, *args)
            assert rc == 0, f"cross_setup {i} of {n}: code {rc}: {self.err()}"
        return time.perf_counter() - t0

    def upload_value(self, cores):
        """Another value function for the context.  It does NOT start a new generation of cached step values: call setup (with
        new_sweep=0 to stay in the memo epoch) before the next iteration, or a step that finds its list unchanged keeps the values
        it holds (c3sc_hip.h above c3sc_hip_cross_setup)."""
        self.eng.upload_value(self.w.ranks, cores)

    def grow_memo(self):
        rc = self.L.c3sc_hip_cross_grow_memo(self.h)
        assert rc == 0, f"cross_grow_memo: code {rc}: {self.err()}"

    def last_kernel(self):
        return self.eng.last_kernel()

    def iteration(self):
        rc = self.L.c3sc_hip_cross_iteration(self.h, 0, None)
        assert rc == 0, f"cross_iteration: code {rc}: {self.err()}"

    def iteration_pi(self, policy_engine, tag):
        """c3sc_hip_cross_iteration_pi with the greedy policy of policy_engine's value function (a DeviceCross or a BellmanEngine);
        returns the code: the caller asserts it."""
        return self.L.c3sc_hip_cross_iteration_pi(self.h, policy_engine.h, C.c_longlong(tag), None)

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
