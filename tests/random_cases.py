"""Seeded random cases of the Bellman fiber kernels and the checker that holds a device run of one to the CPU oracle -- TEST
INFRASTRUCTURE ONLY.  tests/test_random_cases.py holds this file without a GPU (generator, coverage, caps, planted faults),
tests/test_gpu_random_sweep.py runs the committed seeds on a device, tools/fuzz_parity.py walks seeds for as long as it is given.

case(family, seed) is a pure function of its arguments (np.random.default_rng([family id, seed]); no clock, no global state).
The domain is the one the tool was run on for four rounds: the eleven workloads of BASES, N >= 5 per dimension up to MAXN, bond
ranks 1 .. 20.  What a case draws:
  grid        every N from EDGE_N (5, 63, 64, 65, 127, 128 clipped to MAXN: one and two nodes per lane, the tile of the pair
              kernel) with probability 0.4, else uniform in 5 .. MAXN; for D >= 6 one dimension is drawn so and the others lie in
              5 .. 12; a batch of 257 fibers or more keeps every N <= 40 (the oracle's cost)
  ranks       the largest bond rank uniform over served_ranks (where every variant of the model finds a kernel; ten cases in a
              hundred: over 1 .. 20, where the pair and quad kernels refuse), then snapped one below a class (3, 7, 9, 11, 15, 19)
              for 30 in a hundred and onto a class of the model for 25; one bond holds it, the others are uniform below it
  batch       F from F_VALUES; the composition from COMPOSITIONS:
                random      uniform fibers, the all-zero and the all N - 1 fiber in front (the tool's batch)
                faces       a run of max(64, F / 2) consecutive fibers on a face of an absorbing dimension other than K, at a
                            random offset (whole tiles of the pair kernel are absorbed); the case has two absorbing dimensions
                repeats     F draws from F / 4 distinct fibers
                descending  the fibers sorted downwards by the indices next to K
  data        wl.synth_cores times U(0.5, 2) per core, or the signed class of fiber_kernel_cases.cores (synth_cores - 0.35);
              the value scale is fiber_kernel_cases.scale_of's
  candidates  the model's own list; 1 .. 11 random rows; exactly 64 random rows; 65 .. 150 random rows (the pair and quad
              kernels decline); a random list of more than two rows ends with a copy of its first row
  the rest    discount from {0, 0.1, 1.5} or the workload's own, consistent ends, boundary types per dimension, 0 .. 2 obstacle
              boxes, as the tool drew them
A draw the oracle refuses (a stationary candidate) or that breaks a cap is not redrawn at run time: its seed is not in SEEDS.
SEEDS is what `python tests/random_cases.py` prints: the seeds from 0 upwards that add to the coverage conditions of
tests/test_random_cases.py until all of them hold.

check() holds one launch: see its docstring.  predict() is the selection restatement of tests/test_fiber_kernel_cases.py (pick_rp,
find_kernel, the launchers' LDS arithmetic) applied to the case: the kernel name last_kernel() must report, or the refusal.

The forms leg (form_case, check_form; the section at the end of this file) does the same for the run-time compiled models of the
feature tests -- lqr_cd_jump, lqr_ic, lqgame -- against their numpy restatements.  Its two grid-dependent preconditions: the
horizon step is chosen per case from the reference's largest Q on the whole grid (Q delta / h^2 <= 0.8), and a draw with
correlation on whose grid breaks dominance is REDRAWN, deterministically, from the same stream; the DOMINANCE bit is still held
equal to the reference's prediction, which is then clear.

The selection restatement is imported from tests/test_fiber_kernel_cases.py as it stands there.

MAXN above 64 exists for lqg2d, dubins3d only (scar4d, rossler3d, tprob3d: 64); the other models' grids stay on one side."""
import dataclasses
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "tests")):  # as tests/conftest.py does, for the tool and for `python tests/random_cases.py`
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fiber_kernel_cases as T
import oracle_lib
import test_fiber_kernel_cases as S
from c3sc_amd import workloads as wl

BASES = ("lqg2d", "dubins3d", "lqg6d", "car7d", "quad10d", "scar4d", "rossler3d", "perch7d", "tprob3d", "skid5d", "cothrust6d")
FAMILIES = BASES
MAXN = {"lqg2d": 128, "dubins3d": 128, "lqg6d": 40, "car7d": 48, "quad10d": 28, "scar4d": 64, "rossler3d": 64, "perch7d": 40,
        "tprob3d": 64, "skid5d": 48, "cothrust6d": 40}
MAXR = 20
EDGE_N = (5, 63, 64, 65, 127, 128)
BELOW_CLASS = (3, 7, 9, 11, 15, 19)
F_VALUES = (1, 3, 4, 5, 63, 64, 65, 130, 257, 1025)
COMPOSITIONS = ("random", "faces", "repeats", "descending")
CAND_KINDS = ("own", "short", "64", "long")
AUTO, PER_WAVE, PAIR, QUAD = S.AUTO, S.PER_WAVE, S.PAIR, S.QUAD
VARIANT_NAME = {AUTO: "auto", PER_WAVE: "per-wave", PAIR: "pair", QUAD: "quad"}
PIN_MARGIN = 1e-9      # of the scale: the runner-up must lie this far from the minimum for the control to be compared
MAX_UNPINNED = 0.05    # of a case's live nodes (sim_kernel_cases.ODE_MAX_DROPPED)
MAX_REFUSED = 0.15     # of a (model, variant) leg's cases
STATUS_STATIONARY = 1  # C3SC_STATUS_STATIONARY
PREFILL = -77
KIND_FAMILY = {"C3SC_REG_FPW": "per-wave", "C3SC_REG_FPW_BOX": "per-wave", "C3SC_REG_FPP1": "pair", "C3SC_REG_FQ1": "quad",
               "C3SC_REG_FQD": "quad-duo", "REG_FQD_SB": "quad-duo", "C3SC_REG_STENCIL": "stencil"}
REFUSALS = ("no kernel instantiation for", "exceeds the 160 KB", "serves this call")  # launch_bellman's three answers

# registered pair / quad kernels that no case of the domain launches: name -> why
UNREACHED = {f"k_fiber_quad<Skid5D,16,K={k}>": "registered behind the duo kernel, which declines from N = 68 in another dimension on; MAXN is 48"
             for k in (0, 1, 3, 4)}


def model_id(family):
    return S.MODEL_ID[wl.WORKLOADS[family]().model]


def dim_of(family):
    return wl.WORKLOADS[family]().dx


def entries_of(family):
    m, d = model_id(family), dim_of(family)
    return [e for e in S.REG if e.model == m and e.d == d]


def legs(family):
    """the variants a case of the family runs: AUTO, the per-wave kernel, and the pair / quad variant where the registry holds one"""
    have = {e.variant for e in entries_of(family)}
    return tuple(v for v in (AUTO, PER_WAVE, PAIR, QUAD) if v == AUTO or v in have)


def served_ranks(family):
    """the largest bond ranks at which every leg of the family finds a kernel at the padded rank of its upload (K = 0 on the
    smallest grid: the launchers' LDS limits aside).  cothrust6d: 9 and 10 alone, the one class of its pair kernel"""
    m, d = model_id(family), dim_of(family)
    out = []
    for r in range(1, MAXR + 1):
        ok = True
        for v in legs(family):
            rp = S.pick_rp(S.REG, d, r, m, QUAD if v == QUAD else AUTO)
            e = S.find_kernel(S.REG, m, d, rp, 5, v, 0, 1)
            ok = ok and e is not None and e.rp == rp
        if ok:
            out.append(r)
    return out


class Refused:
    """what a launch answered instead of running: one of REFUSALS"""

    def __init__(self, reason):
        self.reason = reason

    def __repr__(self):
        return f"Refused({self.reason!r})"


def refusal_of(exc):
    """the Refused of a C3scHipError of launch_bellman, or None (the error is something else and not a refusal)"""
    msg = str(exc)
    if "(code 3): bellman_fibers: " not in msg:  # C3SC_ERR_UNSUPPORTED from the launch itself
        return None
    for r in REFUSALS:
        if r in msg:
            return Refused(r)
    return None


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    family: str
    seed: int
    ngrid: tuple
    ranks: tuple
    bc: tuple
    obstacles: tuple
    discount: float
    cand_kind: str
    cands: np.ndarray
    signed: bool
    core_seed: int
    core_mul: tuple
    cends: bool
    F: int
    comp: str
    stencil: bool
    policy: bool

    def __repr__(self):
        return (f"case({self.family!r}, {self.seed}): ngrid {self.ngrid} ranks {self.ranks} bc {self.bc} obstacles {len(self.obstacles)} "
                f"discount {self.discount} cands {self.cand_kind}/{len(self.cands)} {'signed' if self.signed else 'positive'} "
                f"cends {int(self.cends)} F {self.F} {self.comp} stencil {int(self.stencil)} policy {int(self.policy)}")

    def tobytes(self):
        parts = [repr((self.family, self.seed, self.ngrid, self.ranks, self.bc, self.obstacles, self.discount, self.cand_kind, self.signed,
                       self.core_seed, self.core_mul, self.cends, self.F, self.comp, self.stencil, self.policy)).encode(), self.cands.tobytes()]
        parts += [self.fibers(k).tobytes() for k in range(len(self.ngrid))]
        return b"|".join(parts)

    def workload(self):
        b = wl.WORKLOADS[self.family]()
        return wl.Workload(b.name, b.model, b.params, b.dx, b.du, b.lb, b.ub, self.ngrid, self.ranks, self.discount, self.bc,
                           [tuple(o) for o in self.obstacles], np.ascontiguousarray(self.cands))

    def cores(self, seed=None):
        """the case's value function; seed: another positive one on the same ranks (the policy's)"""
        cs = wl.synth_cores(self.workload(), seed=self.core_seed if seed is None else seed)
        if seed is not None:
            return cs
        return [c - 0.35 for c in cs] if self.signed else [c * m for c, m in zip(cs, self.core_mul)]

    def fibers(self, k, F=None, salt=0):
        """the batch along K = k (int32 [F, d]); F, salt: a batch of another size and stream (the stencil's and the policy's)"""
        d, ng = len(self.ngrid), np.array(self.ngrid)
        comp = self.comp if F is None else "random"
        F = self.F if F is None else F
        rng = np.random.default_rng([FAMILIES.index(self.family), self.seed, 1 + k, salt])
        idx = rng.integers(0, ng, size=(F, d))
        if comp == "random":
            if F >= 3:
                idx[0], idx[1] = 0, ng - 1
        elif comp == "faces":
            run = min(F, max(64, F // 2))
            at = int(rng.integers(0, F - run + 1))
            fs = [m for m in range(d) if m != k and self.bc[m] == wl.BC_ABSORB]
            m = np.array(fs)[rng.integers(0, len(fs), size=run)]
            idx[np.arange(at, at + run), m] = np.where(rng.integers(0, 2, size=run) == 1, ng[m] - 1, 0)
        elif comp == "repeats":
            idx = idx[rng.integers(0, max(1, F // 4), size=F)]
        elif comp == "descending":
            keys = [m for m in (k - 1, k + 1) if 0 <= m < d] + [m for m in range(d) if abs(m - k) > 1]
            order = np.lexsort([idx[:, m] for m in reversed(keys)])[::-1]  # the first key is the major one
            idx = idx[order]
        else:
            raise KeyError(comp)
        idx[:, k] = 0
        return np.ascontiguousarray(idx, dtype=np.int32)


def case(family, seed):
    fid = FAMILIES.index(family)
    rng = np.random.default_rng([fid, seed])
    b = wl.WORKLOADS[family]()
    d, maxn = b.dx, MAXN[family]
    F = int(rng.choice(F_VALUES))
    comp = str(rng.choice(COMPOSITIONS))
    cap = min(maxn, 40) if F >= 257 else maxn

    def draw_n():
        if rng.random() < 0.4:
            return int(min(int(rng.choice(EDGE_N)), cap))
        return int(rng.integers(5, cap + 1))

    if d >= 6:
        big = int(rng.integers(d))
        ngrid = tuple(draw_n() if m == big else int(rng.integers(5, 13)) for m in range(d))
    else:
        ngrid = tuple(draw_n() for _ in range(d))
    # ranks
    pool = list(range(1, MAXR + 1)) if rng.random() < 0.10 else served_ranks(family)
    rmax = int(rng.choice(pool))
    u = rng.random()
    classes = sorted({e.rp for e in entries_of(family)} & set(pool))
    below = [v for v in BELOW_CLASS if v in pool]
    if u < 0.30 and below:
        rmax = int(rng.choice(below))
    elif u < 0.55 and classes:
        rmax = int(rng.choice(classes))
    bonds = [int(rng.integers(1, rmax + 1)) for _ in range(d - 1)]
    bonds[int(rng.integers(d - 1))] = rmax
    ranks = (1,) + tuple(bonds) + (1,)
    # boundary, obstacles, discount
    bc = tuple(int(rng.choice([wl.BC_ABSORB, wl.BC_PERIODIC, wl.BC_REFLECT])) for _ in range(d)) if rng.random() < 0.7 else tuple(b.bc)
    if comp == "faces":  # every K needs an absorbing dimension other than itself
        bc = list(bc)
        for m in rng.permutation(d)[:2]:
            bc[int(m)] = wl.BC_ABSORB
        bc = tuple(bc)
    obstacles = []
    for _ in range(int(rng.integers(0, 3))):
        cen = tuple(float(rng.uniform(b.lb[m], b.ub[m])) for m in range(d))
        wid = tuple(float(rng.uniform(0.05, 0.8) * (b.ub[m] - b.lb[m])) for m in range(d))
        obstacles.append((cen, wid))
    discount = float(rng.choice([0.0, 0.1, 1.5])) if rng.random() < 0.5 else float(b.discount)
    # candidates
    u = rng.random()
    kind = "own" if u < 0.5 else "short" if u < 0.84 else "64" if u < 0.94 else "long"
    if F >= 257 and kind in ("64", "long"):
        kind = "short"
    if kind == "own":
        cands = np.array(b.cands, dtype=np.float64)
    else:
        U = {"short": int(rng.integers(1, 12)), "64": 64, "long": int(rng.integers(65, 151))}[kind]
        cands = rng.uniform(b.cands.min(axis=0), b.cands.max(axis=0), size=(U, b.du))
        if U > 2:
            cands[-1] = cands[0]
    signed = bool(rng.random() < 0.3)
    core_seed = int(rng.integers(1 << 30))
    core_mul = tuple(float(rng.uniform(0.5, 2.0)) for _ in range(d))
    cends = bool(rng.random() < 0.3)
    stencil = bool(rng.random() < 1.0 / 3.0)
    policy = bool(rng.random() < 0.5)
    return Case(family, int(seed), ngrid, ranks, bc, tuple(obstacles), discount, kind, np.ascontiguousarray(cands), signed, core_seed,
                core_mul, cends, F, comp, stencil, policy)


# ---------------------------------------------------------------------------------------------- selection, restated
def predict(c, variant, k):
    """(kernel name, None) that a launch of the case's batch along k must report under `variant`, or (None, the refusal of
    REFUSALS).  The quad variant runs on an engine of its own, whose upload pads the ranks to the quad kernels' classes."""
    upload = QUAD if variant == QUAD else AUTO
    e, _, declined = S.select(S.REG, model_id(c.family), len(c.ngrid), c.ranks, c.ngrid, upload, variant, k, len(c.cands), F=c.F)
    if e is not None:
        return e.name, None
    if not declined:
        return None, REFUSALS[0]
    last = S.launch(declined[-1], c.ngrid, k, len(c.cands))[0]
    return None, REFUSALS[1] if last == S.OOM else REFUSALS[2]


def predict_stencil(c, k):
    """the stencil kernel's name on the AUTO upload (c3sc_hip_stencil_fibers: model 0, AUTO, no batch size), or None"""
    d = len(c.ngrid)
    rp = S.pick_rp(S.REG, d, max(c.ranks), model_id(c.family), AUTO)
    e = S.find_kernel(S.REG, "0", d, rp, c.ngrid[k], AUTO, k)
    if e is None or e.rp != rp or S.launch(e, c.ngrid, k, 0)[0] != S.OK:
        return None
    return e.name


def family_of_kernel(name):
    by = {e.name: KIND_FAMILY[e.kind] for e in S.REG}
    return by[name]


# ------------------------------------------------------------------------------------------------------ reference
class Rejected(Exception):
    """the oracle does not accept the case (a stationary candidate)"""


@dataclasses.dataclass
class Ref:
    idx: np.ndarray
    ref: np.ndarray      # [F, N] the oracle's backup
    ui: np.ndarray       # [F, N] its argmin, -1 on absorbed nodes
    ab: np.ndarray       # [F, N] 1 boundary, -1 obstacle, 0 live
    Q: np.ndarray        # [F, N, U] every candidate's value
    scale: float
    pinned: np.ndarray   # [F, N] live and the best other control lies more than PIN_MARGIN of the scale above the minimum
    status: int          # the status word the device must report: STATIONARY only where the oracle skipped a candidate


_REF = {}


def problem(c, cores=None):
    return oracle_lib.Problem(c.workload(), c.cores() if cores is None else cores, consistent_ends=c.cends)


def reference(c, k):
    """the Ref of the case's batch along k (the last case's are kept)"""
    key = (c.family, c.seed)
    if _REF.get("key") != key:
        _REF.clear()
        _REF["key"] = key
        _REF["P"] = problem(c)
    if k not in _REF:
        P, w = _REF["P"], c.workload()
        idx = c.fibers(k)
        r = P.q_fibers(k, idx)
        if r is None:
            raise Rejected(repr(c))
        Q, ab = r
        live = ab == 0
        ui = np.where(live, Q.argmin(axis=-1), -1).astype(np.int32)  # the first of equal minima, as the oracle's strict '<'
        ref = Q.min(axis=-1)
        scale = T.scale_of(oracle_lib, w, c.cores(), k, idx, ref, c.signed)
        _, inv = np.unique(c.cands, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        same = inv[None, None, :] == inv[np.clip(ui, 0, None)][..., None]
        second = np.where(same, np.inf, Q).min(axis=-1)
        pinned = live & (second - ref > PIN_MARGIN * scale)
        # the oracle fails a batch with a stationary candidate (Rejected above): an accepted case skipped none
        _REF[k] = Ref(idx, ref, ui, ab, Q, float(scale), pinned, 0)
    return _REF[k]


def unpinned_share(c):
    live = sum(int((reference(c, k).ab == 0).sum()) for k in range(len(c.ngrid)))
    loose = sum(int(((reference(c, k).ab == 0) & ~reference(c, k).pinned).sum()) for k in range(len(c.ngrid)))
    return loose / max(live, 1)


# -------------------------------------------------------------------------------------------------------- the checker
def _worst(err, r):
    f, j = np.unravel_index(int(np.nanargmax(err)), err.shape)
    return f"worst node: fiber {f} {r.idx[f].tolist()} node {j}"


def check(c, variant, k, outputs, kernel_name, status, ref=None):
    """Holds one bellman_fibers launch of the case's batch along k under `variant`.  outputs: (values, uidx, absorbed) as the
    device left them in buffers pre-filled with NaN / PREFILL, or the Refused it answered with.  Raises AssertionError naming
    the case, the variant, k, the kernel and the worst node; returns ("ok", the largest error relative to the scale) or
    ("refused: <reason>", 0.0) for a refusal the restatement predicts.
      kernel    kernel_name equals predict()'s; a refusal is accepted only where predict() gives the same refusal
      coverage  every output finite and written
      flags     absorbed exact
      values    within fiber_kernel_cases.REL_TOL of the case's scale
      controls  on live nodes, cands[uidx] equals cands[the oracle's argmin] wherever the node is pinned; elsewhere the oracle's
                value of the device's choice lies within PIN_MARGIN of the scale of the minimum
      status    the oracle's prediction"""
    what = f"{c!r}\n  variant {VARIANT_NAME[variant]} k {k} kernel {kernel_name}"
    want, reason = predict(c, variant, k)
    if isinstance(outputs, Refused):
        assert want is None, f"{what}: refused ({outputs.reason}) where the restatement predicts {want}"
        assert outputs.reason == reason, f"{what}: refused with '{outputs.reason}', the restatement predicts '{reason}'"
        return f"refused: {reason}", 0.0
    assert want is not None, f"{what}: launched where the restatement predicts the refusal '{reason}'"
    assert kernel_name == want, f"{what}: the restatement predicts {want}"
    r = reference(c, k) if ref is None else ref
    out, ui, ab = outputs
    assert out.shape == ui.shape == ab.shape == r.ref.shape, f"{what}: shapes {out.shape} {ui.shape} {ab.shape}, the batch is {r.ref.shape}"
    unwritten = np.isnan(out) | (ui == PREFILL) | (ab == PREFILL)
    assert not unwritten.any(), f"{what}: {int(unwritten.sum())} nodes were never written; {_worst(unwritten.astype(float), r)}"
    assert np.isfinite(out).all(), f"{what}: {int((~np.isfinite(out)).sum())} values are not finite; {_worst(~np.isfinite(out) * 1.0, r)}"
    bad = ab != r.ab
    assert not bad.any(), f"{what}: {int(bad.sum())} absorbed flags differ; {_worst(bad.astype(float), r)}"
    err = np.abs(out - r.ref)
    assert err.max() <= T.REL_TOL * r.scale, f"{what}: value error {err.max():.3e}, scale {r.scale:.3e}; {_worst(err, r)}"
    live = r.ab == 0
    U = len(c.cands)
    oob = live & ((ui < 0) | (ui >= U))
    assert not oob.any(), f"{what}: {int(oob.sum())} live nodes have no candidate index in 0 .. {U - 1}; {_worst(oob.astype(float), r)}"
    uic = np.clip(ui, 0, U - 1)
    differs = live & (c.cands[uic] != c.cands[np.clip(r.ui, 0, U - 1)]).any(axis=-1)
    wrong = differs & r.pinned
    assert not wrong.any(), f"{what}: {int(wrong.sum())} pinned nodes took another control; {_worst(wrong.astype(float), r)}"
    gap = np.where(live, np.take_along_axis(r.Q, uic[..., None], axis=-1)[..., 0] - r.ref, 0.0)
    assert gap.max() <= PIN_MARGIN * r.scale, \
        f"{what}: the oracle's value of the device's control lies {gap.max():.3e} above the minimum, scale {r.scale:.3e}; {_worst(gap, r)}"
    assert status == r.status, f"{what}: status word {status}, the oracle predicts {r.status}"
    return "ok", float(err.max() / r.scale)


def check_stencil(c, k, idx, costs, ab, kernel_name, P):
    """the stencil kernel against P.stencil_fibers: flags exact, values within REL_TOL of the scale (max |ref|, for signed
    cores the stencil on |cores|), the kernel name predict_stencil's; returns the relative error"""
    what = f"{c!r}\n  stencil k {k} kernel {kernel_name}"
    assert kernel_name == predict_stencil(c, k), f"{what}: the restatement predicts {predict_stencil(c, k)}"
    ref, rab = P.stencil_fibers(k, idx)
    assert not np.isnan(costs).any() and not (ab == PREFILL).any(), f"{what}: nodes were never written"
    assert np.array_equal(ab, rab), f"{what}: {int((ab != rab).sum())} absorbed flags differ"
    scale = float(np.abs(ref).max())
    if c.signed:
        scale = max(scale, T.vabs(oracle_lib, c.workload(), c.cores(), k, idx))
    err = np.abs(costs - ref)
    f, j, s = np.unravel_index(int(err.argmax()), err.shape)
    assert err.max() <= T.REL_TOL * scale, f"{what}: error {err.max():.3e}, scale {scale:.3e}; worst: fiber {f} {idx[f].tolist()} node {j} entry {s}"
    return float(err.max() / scale)


# ----------------------------------------------------------------------------------------------------- device side
def launch_host(eng, k, idx):
    """bellman_fibers_host on buffers pre-filled with NaN / PREFILL: (values, uidx, absorbed), or the Refused the call answered"""
    from c3sc_amd.engine import C3scHipError

    F, N = idx.shape[0], eng.ngrid[k]
    out = np.full((F, N), np.nan)
    ui = np.full((F, N), PREFILL, dtype=np.int32)
    ab = np.full((F, N), PREFILL, dtype=np.int32)
    try:
        eng._chk(eng.L.c3sc_hip_bellman_fibers_host(eng.h, k, F, idx.ctypes.data, out.ctypes.data, ui.ctypes.data, ab.ctypes.data),
                 "bellman_fibers_host")
    except C3scHipError as e:
        r = refusal_of(e)
        if r is None:
            raise
        return r
    return out, ui, ab


class Tally:
    """what a sweep did: launches and the worst relative error per kernel family, refusals by reason"""

    def __init__(self):
        self.runs, self.worst, self.refused = {}, {}, {}

    def add(self, fam, err):
        self.runs[fam] = self.runs.get(fam, 0) + 1
        self.worst[fam] = max(self.worst.get(fam, 0.0), err)

    def lines(self):
        out = [f"{fam}: {self.runs[fam]} launches, worst relative error {self.worst[fam]:.3e}" for fam in sorted(self.runs)]
        out += [f"refused as predicted ({why}): {n}" for why, n in sorted(self.refused.items())] or ["refused as predicted: 0"]
        return out


def run_case(c, tally, partition_env=None, verbose=False):
    """every launch of one case on device 0, each through its checker: AUTO, per-wave and pair on one engine, the quad variant
    on its own, every k; the stencil kernel and policy evaluation where the case draws them.  partition_env(on): a context
    manager that sets C3SC_FIBER_PARTITION for one launch (a batch of 1025 fibers or more runs again under it and must not
    change a bit).  A failure raises AssertionError."""
    from c3sc_amd.engine import BellmanEngine

    w, cores, d = c.workload(), c.cores(), len(c.ngrid)
    say = print if verbose else (lambda *a: None)
    for k in range(d):
        reference(c, k)  # Rejected before anything runs on the device
    eng = BellmanEngine(0)
    eng.configure(w, cores)
    eng.set_consistent_ends(c.cends)
    eng_q = None
    if QUAD in legs(c.family):
        eng_q = BellmanEngine(0)
        eng_q.set_variant(QUAD)
        eng_q.configure(w, cores)
        eng_q.set_consistent_ends(c.cends)
    for variant in legs(c.family):
        e = eng_q if variant == QUAD else eng
        e.set_variant(variant)
        for k in range(d):
            r = reference(c, k)
            e.status()
            res = launch_host(e, k, r.idx)
            name = None if isinstance(res, Refused) else e.last_kernel()
            verdict, err = check(c, variant, k, res, name, 0 if isinstance(res, Refused) else e.status(), r)
            say(f"  {VARIANT_NAME[variant]} k {k}: {name} {verdict} {err:.3e}")
            if isinstance(res, Refused):
                tally.refused[res.reason] = tally.refused.get(res.reason, 0) + 1
                continue
            tally.add(family_of_kernel(name), err)
            if c.F >= 1025 and partition_env is not None:
                with partition_env("1"):
                    again = launch_host(e, k, r.idx)
                assert not isinstance(again, Refused) and e.last_kernel() == name and e.status() == 0, f"{c!r}\n  partitioned launch: {again}"
                for a, b in zip(res, again):
                    assert np.array_equal(a, b), f"{c!r}\n  variant {VARIANT_NAME[variant]} k {k} {name}: the partitioned launch differs"
    eng.set_variant(AUTO)
    P = _REF["P"]
    if c.stencil:
        for k in range(d):
            idx = c.fibers(k, F=30 if (c.seed + k) % 2 else 1, salt=1)
            costs, ab = eng.stencil_fibers_host(k, idx)
            err = check_stencil(c, k, idx, costs, ab, eng.last_kernel(), P)
            say(f"  stencil k {k}: {eng.last_kernel()} {err:.3e}")
            tally.add("stencil", err)
    if c.policy:  # the greedy policy of a second value function applied to this one; the oracle's own argmin is forced
        cores_pol = c.cores(seed=c.core_seed + 7919)
        pol_vf = oracle_lib.ValueF(w.ngrid, w.ranks, cores_pol)
        eng_pol = BellmanEngine(0)
        eng_pol.configure(w, cores_pol)
        eng_pol.set_consistent_ends(c.cends)
        P.pi_begin()
        P.pi_step_begin()
        for k in range(d):
            idx = c.fibers(k, F=40 if (c.seed + k) % 2 else 2, salt=2)
            ref, ref_ui = P.policy_fibers(pol_vf, k, idx)
            _, ui, _ = eng_pol.bellman_fibers_host(k, idx)
            out, _ = eng.policy_fibers_host(k, idx, np.where(ref_ui >= 0, ref_ui, ui).astype(np.int32))
            scale = float(np.abs(ref).max())
            if c.signed:
                scale = max(scale, T.vabs(oracle_lib, w, cores, k, idx))
            err = np.abs(out - ref)
            f, j = np.unravel_index(int(np.nanargmax(err)), err.shape)
            assert np.isfinite(out).all() and err.max() <= T.REL_TOL * scale, \
                f"{c!r}\n  policy k {k} kernel {eng.last_kernel()}: error {err.max():.3e}, scale {scale:.3e}; worst: fiber {f} {idx[f].tolist()} node {j}"
            say(f"  policy k {k}: {eng.last_kernel()} {err.max() / scale:.3e}")
            tally.add("policy (" + family_of_kernel(eng.last_kernel()) + ")", float(err.max() / scale))
        assert eng.status() == 0 and eng_pol.status() == 0
        eng_pol.close()
    eng.close()
    if eng_q is not None:
        eng_q.close()


# ------------------------------------------------------------------------------------------- the committed seed lists
SEEDS = {  # `python tests/random_cases.py` prints these lines
    "lqg2d": (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 14, 17, 30, 50),  # 15
    "dubins3d": (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14, 16, 20, 21),  # 15
    "lqg6d": (0, 2, 3, 4, 5, 6, 7, 8, 10, 15, 16, 17, 18, 21, 22),  # 15
    "car7d": (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 14, 17, 18, 21, 30),  # 15
    "quad10d": (2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 16, 17, 20, 22, 24, 25, 60),  # 17
    "scar4d": (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 41, 43, 61, 69, 92),  # 34
    "rossler3d": (0, 1, 2, 3, 4, 6, 7, 10, 11, 14, 15, 16, 17, 18, 101),  # 15
    "perch7d": (0, 1, 2, 3, 4, 6, 7, 8, 9, 12, 14, 18, 19, 22, 24, 55),  # 16
    "tprob3d": (0, 1, 2, 3, 4, 5, 6, 8, 9, 11, 13, 15, 18, 20, 24, 29),  # 16
    "skid5d": (0, 1, 2, 3, 4, 6, 7, 8, 10, 15, 16, 17, 29),  # 13
    "cothrust6d": (0, 1, 2, 3, 4, 6, 7, 10, 11, 16, 19, 20, 21, 25),  # 14
}


def acceptable(c):
    """the oracle accepts the case and at most MAX_UNPINNED of its live nodes are unpinned"""
    try:
        return unpinned_share(c) <= MAX_UNPINNED
    except Rejected:
        return False


def coverage_items(c):
    """what the case adds to the coverage conditions of tests/test_random_cases.py, as a set of hashable items; the items of a
    condition that asks for n cases carry a slot 0 .. n - 1 when counted (choose_seeds)"""
    d = len(c.ngrid)
    once = {("F", c.F), ("comp", c.comp), ("cands", c.cand_kind)}
    for n in c.ngrid:
        if MAXN[c.family] > 64:
            once.add(("side", n > 64))
    if c.F == 65 and c.comp in ("random", "descending") and all((c.fibers(k)[63] != c.fibers(k)[64]).any() for k in range(d)):
        once.add(("last of 65", True))  # the one fiber of a second pair tile is not a copy of its predecessor
    fams, names = set(), set()
    for v in legs(c.family):
        for k in range(d):
            name, _ = predict(c, v, k)
            if name:
                fams.add(family_of_kernel(name))
                if "pair" in name or "quad" in name:
                    names.add(name)
    if c.stencil and all(predict_stencil(c, k) for k in range(d)):
        fams.add("stencil")
    return once, fams, names


def refused_legs(c):
    """the variants of the case's legs with a refusal at some k"""
    return {v for v in legs(c.family) if any(predict(c, v, k)[0] is None for k in range(len(c.ngrid)))}


def needs(family):
    """the coverage conditions of a family as {item: cases wanted}"""
    want = {("F", f): 1 for f in F_VALUES}
    want.update({("comp", x): 1 for x in COMPOSITIONS})
    want.update({("cands", x): 1 for x in CAND_KINDS})
    want[("last of 65", True)] = 1
    if MAXN[family] > 64:
        want.update({("side", False): 1, ("side", True): 1})
    for e in entries_of(family):
        want[("family", KIND_FAMILY[e.kind])] = 5
        if e.variant in (PAIR, QUAD) and e.name not in UNREACHED:
            want[("kernel", e.name)] = 2
    want[("family", "stencil")] = 5
    return want


def choose_seeds(family, first=400, limit=4000):
    """Three passes over the seeds from 0 upwards, skipping what is not acceptable.  One: among the first `first` seeds, the
    cases without a predicted refusal that add to a coverage condition still open.  Two: for what is still open (the long
    candidate lists, the kernels of the ranks that another variant refuses), the cases with a refusal that add to it.  Three:
    further cases without a refusal, until no leg's refusals exceed MAX_REFUSED of the list."""
    want = needs(family)
    have = {k: 0 for k in want}
    seeds, refused, deferred = [], {v: 0 for v in legs(family)}, []
    done = lambda: all(have[i] >= want[i] for i in want)

    def gain(items):
        return [i for i in items if i in have and have[i] < want[i]]

    def items_of(c):
        once, fams, names = coverage_items(c)
        return list(once) + [("family", f) for f in fams] + [("kernel", n) for n in names]

    def take(s, items, rl):
        seeds.append(s)
        for i in items:
            if i in have:
                have[i] += 1
        for v in rl:
            refused[v] += 1

    for s in range(limit):
        if done() or (s >= first and deferred):
            break
        c = case(family, s)
        items, rl = items_of(c), refused_legs(c)
        if rl:
            deferred.append((s, items, rl))
        elif gain(items) and acceptable(c):
            take(s, items, rl)
    for s, items, rl in deferred:
        if not done() and gain(items) and acceptable(case(family, s)):
            take(s, items, rl)
    for s in range(limit):
        if all(n <= MAX_REFUSED * len(seeds) for n in refused.values()):
            break
        c = case(family, s)
        if s not in seeds and not refused_legs(c) and acceptable(c):
            take(s, items_of(c), ())
    missing = {i: (have[i], want[i]) for i in want if have[i] < want[i]}
    return sorted(seeds), missing


# ======================================================================================================= the forms leg
# The run-time compiled models of the feature tests, with their specs and names (a process compiles each once):
#   lqr_cd_jump (tests/test_gpu_corr.py)    horizon, stop, jump and correlation in any of the 16 combinations, class 4
#   lqr_ic      (tests/test_gpu_impulse.py) interventions, with and without jumps, classes 4 / 8 / 12
#   lqgame      (tests/test_gpu_game.py)    both orders, classes 4 / 8
# form_case(family, seed) draws a 2-D grid with both N in 5 .. 128 (EDGE_N with probability 0.4), boundary types per dimension,
# jump_lib's obstacle or none, discount 0.3 or 0, one bond rank of FORM_RANKS, k in {0, 1}, F in FORM_F and the switches.  The
# reference is the numpy restatement of each feature over backup_ref (corr_lib.corr_fibers, impulse_lib.impulse_fibers,
# game_lib.game_backup) on the ORACLE's stencil of the batch; the bound is theirs, 1e-12 max(1, |ref|) per node, the index is
# compared where the restatement's margin exceeds 1e-9.  Two preconditions are functions of the grid, taken from the reference
# over the WHOLE grid and all candidates:
#   horizon step   delta = 0.8 h^2 / max Q, rounded down to two digits: Q delta / h^2 <= 0.8 at every node, no CFL bit
#   dominance      a case with correlation on whose grid breaks dominance at some node is REDRAWN (the next draw of the same
#                  stream: still a pure function of family and seed); the DOMINANCE bit must then equal the reference's: clear
FORM_FAMILIES = ("lqr_cd_jump", "lqr_ic", "lqgame")
FORM_F = (1, 5, 37, 130)
FORM_RANKS = {"lqr_cd_jump": (3, 4), "lqr_ic": (3, 4, 7, 11), "lqgame": (3, 4, 7)}
FORM_CLASSES = {"lqr_cd_jump": (4,), "lqr_ic": (4, 8, 12), "lqgame": (4, 8)}
SWITCHES = ("horizon", "stop", "jump", "corr")
STATUS_CFL, STATUS_DOMINANCE = 2, 4
FORM_REL_TOL = 1e-12
U_LQ = np.linspace(-1.0, 1.0, 9).reshape(-1, 1)   # tests/test_gpu_game.py
W_LQ = np.linspace(-0.5, 0.5, 5).reshape(-1, 1)
GAME_BCOST, GAME_OCOST = 100.0, 0.0


@dataclasses.dataclass(frozen=True, eq=False)
class FormCase:
    family: str
    seed: int
    ngrid: tuple
    bc: tuple
    obstacle: bool
    discount: float
    rank: int
    k: int
    F: int
    core_seed: int
    switches: tuple   # lqr_cd_jump: (horizon, stop, jump, corr); lqr_ic: (False, False, jump, False); lqgame: all False
    delta: float      # the horizon step; 0.0 without the switch

    def __repr__(self):
        on = "+".join(s for s, v in zip(SWITCHES, self.switches) if v) or "none"
        return (f"form_case({self.family!r}, {self.seed}): ngrid {self.ngrid} bc {self.bc} obstacle {int(self.obstacle)} discount {self.discount} "
                f"rank {self.rank} k {self.k} F {self.F} switches {on} delta {self.delta}")

    def tobytes(self):
        return repr((self.family, self.seed, self.ngrid, self.bc, self.obstacle, self.discount, self.rank, self.k, self.F, self.core_seed,
                     self.switches, self.delta)).encode() + self.fibers().tobytes()

    @property
    def cls(self):
        return min(c for c in FORM_CLASSES[self.family] if c >= self.rank)

    def workload(self, mid=1000):
        import corr_lib as CL
        import game_lib as GL
        import impulse_lib as IL
        import jump_lib as JL

        obs = [JL.LQR_OBSTACLE] if self.obstacle else []
        ranks = (1, self.rank, 1)
        if self.family == "lqgame":
            return wl.Workload("lqgame", mid, GL.LQGAME_PRM, 2, 2, (-2.0, -2.0), (2.0, 2.0), self.ngrid, ranks, self.discount, self.bc, obs,
                               GL.product(U_LQ, W_LQ))
        base = CL.lqr_workload(mid, 4, self.discount, JL.LQR_PRM) if self.family == "lqr_cd_jump" else \
            IL.lqr_workload(mid, 4, self.discount, IL.lqr_cost_scale(self.cls))
        return dataclasses.replace(base, ngrid=self.ngrid, ranks=ranks, bc=self.bc, obstacles=obs)

    def cores(self):
        return wl.synth_cores(self.workload(), seed=self.core_seed)

    def fibers(self):
        rng = np.random.default_rng([len(FAMILIES) + FORM_FAMILIES.index(self.family), self.seed, 1])
        idx = rng.integers(0, np.array(self.ngrid), size=(self.F, 2))
        if self.F >= 3:
            idx[0], idx[1] = 0, np.array(self.ngrid) - 1
        idx[:, self.k] = 0
        return np.ascontiguousarray(idx, dtype=np.int32)

    def labels(self):
        """the launches of the case: both orders of the game, else one"""
        return ("minmax", "maxmin") if self.family == "lqgame" else ("",)

    def kernel(self):
        return f"k_fiber_per_wave<rtc:{self.family},{self.cls},{1 if self.ngrid[self.k] <= 64 else 2}>"


def _grid_nodes(w):
    i0, i1 = np.meshgrid(np.arange(w.ngrid[0]), np.arange(w.ngrid[1]), indexing="ij")
    ix = np.stack([i0.reshape(-1), i1.reshape(-1)], axis=-1)
    xg = w.xgrid()
    return ix, np.stack([xg[0][ix[:, 0]], xg[1][ix[:, 1]]], axis=-1)


def _grid_preconditions(c):
    """(max Q over every node of the grid and every candidate, dominance broken somewhere) of an lqr_cd_jump case, from the
    restatement's rates alone: Q is read off backup_ref.candidate_values in its explicit form with delta = h^2, beta = 0, on the
    stencil 'self = 1, neighbours = 0' against the all-zero stencil (value = g h^2 + 1 - Q against g h^2)"""
    import backup_ref as BR
    import corr_lib as CL
    import jump_lib as JL
    import stop_lib as SL

    w = c.workload()
    _, x = _grid_nodes(w)
    h2, t = BR.mca_constants(w)
    q0 = np.zeros(len(x))
    broken = False
    if c.switches[2]:
        q0 = q0 + h2 * JL.lqr_jumps(w.params, x)[0]
    if c.switches[3]:
        r, _ = CL.pair_rates(w, CL.lqr_jump_covar, CL.LQR_PAIRS, x)
        q0 = q0 - 2.0 * r.sum(axis=1)
        broken = bool(CL.dominance(w, SL.lqrn_host, CL.LQR_PAIRS, x, r).any())
    C = np.asarray(w.cands, dtype=np.float64)
    one = np.zeros((len(x), 5))
    one[:, 4] = 1.0
    v1 = BR.candidate_values(SL.lqrn_host, w.params, x, one, C, h2, t, 0.0, q0, None, h2)[0]
    v0 = BR.candidate_values(SL.lqrn_host, w.params, x, np.zeros((len(x), 5)), C, h2, t, 0.0, q0, None, h2)[0]
    return float((1.0 - (v1 - v0)).max()), broken


def form_case(family, seed):
    import backup_ref as BR

    fid = len(FAMILIES) + FORM_FAMILIES.index(family)
    rng = np.random.default_rng([fid, seed])
    while True:
        draw_n = lambda: int(rng.choice(EDGE_N)) if rng.random() < 0.4 else int(rng.integers(5, 129))
        ngrid = (draw_n(), draw_n())
        bc = tuple(int(rng.choice([wl.BC_ABSORB, wl.BC_PERIODIC, wl.BC_REFLECT])) for _ in range(2))
        obstacle = bool(rng.random() < 0.5)
        discount = float(rng.choice([0.3, 0.0]))
        rank = int(rng.choice(FORM_RANKS[family]))
        k = int(rng.integers(2))
        F = int(rng.choice(FORM_F))
        core_seed = int(rng.integers(1 << 30))
        sw = tuple(bool(b) for b in rng.integers(0, 2, size=4))
        if family == "lqr_ic":
            sw = (False, False, sw[2], False)
        elif family == "lqgame":
            sw = (False,) * 4
        c = FormCase(family, int(seed), ngrid, bc, obstacle, discount, rank, k, F, core_seed, sw, 0.0)
        if family != "lqr_cd_jump" or not (sw[0] or sw[3]):
            return c
        qmax, broken = _grid_preconditions(c)
        if broken:
            continue  # redrawn: the grid's aspect ratio breaks dominance
        if sw[0]:
            h2, _ = BR.mca_constants(c.workload())
            d = 0.8 * h2 / qmax
            e = int(np.floor(np.log10(d))) - 1
            c = dataclasses.replace(c, delta=float(np.floor(d / 10.0 ** e) * 10.0 ** e))
        return c


@dataclasses.dataclass
class FormRef:
    idx: np.ndarray
    ref: np.ndarray
    ui: np.ndarray
    ab: np.ndarray
    margin: np.ndarray
    status: int


_FREF = {}


def form_reference(c, label=""):
    """the FormRef of one launch of the case (the last case's are kept): the feature's numpy restatement on the oracle's stencil"""
    import corr_lib as CL
    import game_lib as GL
    import impulse_lib as IL
    import jump_lib as JL
    import stop_lib as SL

    key = (c.family, c.seed)
    if _FREF.get("key") != key:
        _FREF.clear()
        _FREF["key"] = key
        w, cores = c.workload(), c.cores()
        # the oracle's stencil needs the grid, the boundary and the train alone: any built-in model stands in for the compiled one
        P = oracle_lib.Problem(dataclasses.replace(w, model=wl.MODEL_LQGND, params=(2.0, 1.0, 1.0)), cores)
        idx = c.fibers()
        _FREF["stencil"] = (idx,) + P.stencil_fibers(c.k, idx)
    if label not in _FREF:
        w, cores = c.workload(), c.cores()
        idx, costs, ab = _FREF["stencil"]
        bcost, ocost = (lambda x: SL.lqrn_terminal(w.params, x)), (lambda x: np.full(len(x), 5.0))
        status = 0
        if c.family == "lqgame":
            out, ui, mg, stat = GL.game_backup(w, GL.lqgame_host, c.k, idx, costs, ab, U_LQ, W_LQ, label, GAME_BCOST, GAME_OCOST)
        elif c.family == "lqr_ic":
            out, ui, mg, stat, _ = IL.impulse_fibers(w, SL.lqrn_host, IL.lqr_impulses, JL.Train(w, cores), c.k, idx, costs, ab, bcost, ocost,
                                                     jumps=JL.lqr_jumps if c.switches[2] else None)
        else:
            hz, stop, jump, corr = c.switches
            out, ui, mg, stat, cfl, dom = CL.corr_fibers(w, SL.lqrn_host, CL.lqr_jump_covar, CL.LQR_PAIRS, CL.full_values(w, cores), c.k, idx, costs, ab,
                                                         bcost, ocost, c.delta if hz else None, (lambda x: SL.lqr_psi(w.params, x)) if stop else None,
                                                         jumps=JL.lqr_jumps if jump else None, interp=JL.Train(w, cores), with_corr=corr)
            status |= (STATUS_CFL if cfl.any() else 0) | (STATUS_DOMINANCE if dom.any() else 0)
        status |= STATUS_STATIONARY if np.asarray(stat).any() else 0
        _FREF[label] = FormRef(idx, out, np.asarray(ui), ab, mg, status)
    return _FREF[label]


def form_unpinned_share(c):
    n = m = 0
    for label in c.labels():
        r = form_reference(c, label)
        live = r.ab == 0
        n, m = n + int(live.sum()), m + int((live & ~(r.margin > PIN_MARGIN)).sum())
    return m / max(n, 1)


def check_form(c, label, outputs, kernel_name, status, ref=None):
    """one launch of a forms case: the kernel name, every output written, absorbed exact, values within FORM_REL_TOL max(1, |ref|)
    per node (the same non-finite entries), the index equal wherever the restatement's margin exceeds PIN_MARGIN and in range on
    every live node, the status word (STATIONARY, CFL, DOMINANCE) equal to the restatement's.  Returns the largest error relative
    to max(1, |ref|)"""
    what = f"{c!r}\n  {label or 'launch'} kernel {kernel_name}"
    assert not isinstance(outputs, Refused), f"{what}: refused ({outputs.reason}); the per-wave kernel of a compiled model serves every grid"
    assert kernel_name == c.kernel(), f"{what}: expected {c.kernel()}"
    r = form_reference(c, label) if ref is None else ref
    out, ui, ab = outputs
    assert out.shape == ui.shape == ab.shape == r.ref.shape, f"{what}: shapes"
    unwritten = np.isnan(out) | (ui == PREFILL) | (ab == PREFILL)
    assert not unwritten.any(), f"{what}: {int(unwritten.sum())} nodes were never written; {_worst(unwritten.astype(float), r)}"
    bad = ab != r.ab
    assert not bad.any(), f"{what}: {int(bad.sum())} absorbed flags differ; {_worst(bad.astype(float), r)}"
    fin = np.isfinite(r.ref)
    assert np.array_equal(fin, np.isfinite(out)) and np.array_equal(out[~fin], r.ref[~fin]), f"{what}: non-finite values differ"
    err = np.where(fin, np.abs(out - np.where(fin, r.ref, 0.0)) / np.maximum(1.0, np.abs(np.where(fin, r.ref, 0.0))), 0.0)
    assert err.max() <= FORM_REL_TOL, f"{what}: relative error {err.max():.3e}; {_worst(err, r)}"
    live = r.ab == 0
    none = live & (ui < 0) & (r.ui >= 0)
    assert not none.any(), f"{what}: {int(none.sum())} live nodes have no action; {_worst(none.astype(float), r)}"
    wrong = live & (r.margin > PIN_MARGIN) & (ui != r.ui)
    assert not wrong.any(), f"{what}: {int(wrong.sum())} pinned nodes took another action; {_worst(wrong.astype(float), r)}"
    assert status == r.status, f"{what}: status word {status}, the restatement predicts {r.status}"
    return float(err.max())


_FORM_IDS = {}


def compile_forms():
    """the three models with the specs and names of their feature tests"""
    import corr_lib as CL
    import game_lib as GL
    import impulse_lib as IL
    import jump_lib as JL
    from c3sc_amd import engine as E

    if not _FORM_IDS:
        _FORM_IDS["lqr_cd_jump"] = E.compile_model(CL.LQR_JUMP, 2, 2, ranks=(4,), name="lqr_cd_jump", horizon=True, stop=True, njump=JL.LQR_NJUMP,
                                                   corr_pairs=CL.LQR_PAIRS, **CL.LQR_MASKS)
        _FORM_IDS["lqr_ic"] = E.compile_model(IL.LQR_JUMP, 2, 2, ranks=(4, 8, 12), name="lqr_ic", njump=JL.LQR_NJUMP, nimpulse=IL.LQR_NIMPULSE,
                                              **IL.LQR_MASKS)
        _FORM_IDS["lqgame"] = E.compile_model(GL.LQGAME, 2, 2, ranks=(4, 8), name="lqgame", game=True, **GL.LQGAME_MASKS)
    return _FORM_IDS


def run_form_case(c, tally, verbose=False):
    from c3sc_amd.engine import BellmanEngine

    w = c.workload(compile_forms()[c.family])
    for label in c.labels():
        form_reference(c, label)
    eng = BellmanEngine(0)
    eng.configure(w, c.cores())
    hz, stop, jump, corr = c.switches
    if c.family == "lqr_cd_jump":
        if stop:
            eng.set_stopping(True)
        if hz:
            eng.set_horizon_step(c.delta)
        if jump:
            eng.set_jumps(True)
        if corr:
            eng.set_correlation(True)
    elif c.family == "lqr_ic":
        eng.set_jumps(jump)
        eng.set_impulses(True)
    for label in c.labels():
        if label:
            eng.set_game(U_LQ, W_LQ, label)
        r = form_reference(c, label)
        eng.status()
        res = launch_host(eng, c.k, r.idx)
        err = check_form(c, label, res, eng.last_kernel(), eng.status(), r)
        if verbose:
            print(f"  {label or 'launch'}: {eng.last_kernel()} {err:.3e}")
        tally.add("forms: " + c.family, err)
    eng.close()


FORM_SEEDS = {  # `python tests/random_cases.py lqr_cd_jump lqr_ic lqgame` prints these lines
    "lqr_cd_jump": (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 21, 27, 30, 33, 37, 38, 40, 41, 45, 50, 56, 57, 66, 87, 90, 96, 158),  # 32
    "lqr_ic": (0, 1, 2, 3, 5, 6, 8),  # 7
    "lqgame": (0, 1, 2, 3, 4, 5),  # 6
}


def form_items(c):
    side = c.ngrid[c.k] > 64
    return {("F", c.F), ("class", c.cls), ("switches", c.switches, side), ("side", side), ("k", c.k), ("discount", c.discount),
            ("obstacle", c.obstacle)}


def form_needs(family):
    import itertools

    want = {("F", f) for f in FORM_F} | {("class", x) for x in FORM_CLASSES[family]} | {("side", False), ("side", True), ("k", 0), ("k", 1)}
    want |= {("discount", 0.3), ("discount", 0.0), ("obstacle", False), ("obstacle", True)}
    if family == "lqr_cd_jump":
        want |= {("switches", s, side) for s in itertools.product((False, True), repeat=4) for side in (False, True)}
    elif family == "lqr_ic":
        want |= {("switches", (False, False, j, False), side) for j in (False, True) for side in (False, True)}
    return want


def form_acceptable(c):
    return form_unpinned_share(c) <= MAX_UNPINNED


def choose_form_seeds(family, limit=2000):
    want, have, seeds = form_needs(family), set(), []
    for s in range(limit):
        if want <= have:
            break
        c = form_case(family, s)
        if (form_items(c) & want) - have and form_acceptable(c):
            seeds.append(s)
            have |= form_items(c)
    return seeds, want - have


if __name__ == "__main__":
    oracle_lib.build()
    for fam in (sys.argv[1:] or FAMILIES + FORM_FAMILIES):
        seeds, missing = choose_seeds(fam) if fam in FAMILIES else choose_form_seeds(fam)
        print(f'    "{fam}": {tuple(seeds)},  # {len(seeds)}' + (f"  MISSING {missing}" if missing else ""), flush=True)
