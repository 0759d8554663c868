"""The numpy restatement of node_backup_box (c3sc_amd/csrc/kernel_common.hpp), the continuous-control minimiser, step for step
-- TEST INFRASTRUCTURE ONLY.  It shares no code with the kernels or with the host's box_minimize.

The algorithm, vectorised over P nodes (minimise):
  grid      dl = (ub - lb) / (G - 1); candidate c = 0 .. G^du - 1 decodes with control 0 fastest; a point is ub[i] where its digit is
            G - 1, else fma(gi, dl, lb) (one rounding: formed in exact rational arithmetic and rounded once); the take rule is the
            strict '<' from best = 1e301, starting at u = lb
  polish    `polish` rounds over i = 0 .. du - 1: the cell [max(lb, u_i - dl), min(ub, u_i + dl)], gr = 0.6180339887498949, two
            probes, 40 steps of the kernel's update of (lo, hi, x1, x2, f1, f2), xm = f1 < f2 ? x1 : x2, fm = min(f1, f2), taken
            only where fm < best; every round starts from the point the previous one left
  status    a node is stationary when ANY evaluated point (grid or golden-section probe) had Q < 1e-14

The objective (Objective) is NOT the device's: the oracle's model callbacks (drift, diagonal sigma, stage) at every node's own u,
as fiber_kernel_cases.model_tables calls them, then the arithmetic of backup_ref.candidate_values -- upwind thresholds +-1e-14, a
candidate with Q < 1e-14 is worth 1e300 and marks the node stationary, dt = h2 / Q, the self-loop 1 - Q / Q and exp(-beta dt).
Every dimension is evaluated at u: the kernel's hoist of the dimensions outside Model::UDEP_MASK to u = lb is not copied, so a
wrong mask shows.  The stencil V comes from oracle.Problem.stencil_fibers (fiber_setup); absorbed and obstacle nodes take the
oracle's costs and u = 0.

The trace.  Two double implementations of one objective differ by rounding (measured: BOX_MARGIN below), so a comparison of two
objective values that lie within thr = BOX_MARGIN * scale of each other may fall either way on the device: it is UNSURE.
  grid      unsure where the best value and the best value of a DIFFERENT point lie within thr (copies of one point, as a control
            with lb == ub makes them, are not runners-up): the device may start from another cell, the node is unpinned
  search    per (round, coordinate): the bracket [lo, hi] held at the first unsure comparison f1 < f2 (the final comparison for xm
            included), else the final bracket; the spread (max - min) of the reference objective at 17 evenly spaced points of that
            bracket; whether a probe was stationary.  The device's point of this search lies in that bracket whichever way the
            unsure comparisons fell.
  take      fm < best is unsure where |fm - best| <= thr, plus the search's spread where one of its comparisons was unsure (the
            device's fm may then be any value of the bracket).  A search whose take surely fails leaves no trace in the result:
            its spread does not count.  Where the take is unsure the gap |fm - best| counts as spread as well.
  interval  [ulo_i, uhi_i], where the device's u_i may lie: the grid point exactly; after a search of i the recorded bracket where
            the take is sure, unchanged where it surely fails, the hull of both where it is unsure.
  widening  the searches before the last round's search of i may have left the other coordinates anywhere in their intervals,
            which moves the minimiser along i.  The last round's search of i is run again with coordinate j at either end of its
            interval, for every j != i; with r(j, e) the recorded bracket of that run,
                ulo_i = lo_i - sum_j max_e max(0, lo_i - r(j, e).lo),   uhi_i = hi_i + sum_j max_e max(0, r(j, e).hi - hi_i)
            -- first order in the displacements, which are ~1e-7 of the box where the brackets are.
A node is PINNED where the grid is sure and the spread over every recorded bracket that can reach the result is at most
REL_TOL * scale / 2: whatever the device decided at unsure comparisons, its value lies within the tolerance.

fault= plants a mistake (FAULTS); tests/test_box_ref.py shows every one rejected on some row."""
import ctypes as C
import dataclasses
import os
import sys
from collections import namedtuple
from fractions import Fraction

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "tests")):  # as tests/conftest.py does, for `python tests/box_ref.py`
    if _p not in sys.path:
        sys.path.insert(0, _p)

import backup_ref as BR
import fiber_kernel_cases as T
from random_cases import MAX_UNPINNED  # of a row's live nodes: the project's cap

GR = 0.6180339887498949
STEPS = 40
NSAMPLE = 17
# |device objective - reference objective| at equal u, relative to the scale, measured on an MI355X over every row of
# tests/test_gpu_box_minimiser.py (policy_fibers_box_host on the returned controls): 9.35e-16 at worst (Cothrust6D at rank class 20,
# synth; 1e-16 .. 6e-16 on the other rows, 1e-18 on tprob3d, whose scale is its boundary cost of 100).  100 times that: a flip of a
# comparison by either side's rounding needs the two values within twice the noise.
BOX_MARGIN = 9.4e-14
STATUS_STATIONARY = 1

FAULTS = ("no_polish", "first_round", "coord0", "reverse", "half_cell", "no_clamp", "restart", "steps10", "always_take", "freeze",
          "grid_status")
# Dropped from the issue's list, still accepted by fault= so that the statement can be checked:
#   slowest      the tensor order with control 0 slowest.  A full tensor grid is the same SET of points in either order and every
#                point keeps its own value, so the order decides only exact ties between distinct points; the winner of a strict '<'
#                scan is otherwise the same, and with it everything downstream.  tests/test_box_ref.py asserts that it changes
#                nothing, to the bit, on the du = 3 rows.
# first_round, restart and half_cell show on few pinned nodes: they need a pinned minimiser that the second round moves, or one
# more than dl / 2 from its grid point, and most pinned minimisers sit on faces.  Coarse control grids on wide boxes show them on
# many pinned nodes (half_cell on 50 of 189 on lqg2d at grid = 2) but with a third or more of the nodes unpinned; under the cap
# the rows that show them are the `rounds` rows (grid = 2, found by a search for them) and tprob3d `polish1`: one pinned node per
# row, two or three rows per fault.
DROPPED_FAULTS = ("slowest",)


def model_eval(oracle, w, x, U):
    """(b [P, D], s [P, D], stage [P]) of the oracle's model callbacks at states x [P, D] and controls U [P, du]"""
    L = oracle.lib()
    x = np.ascontiguousarray(x, dtype=np.float64)
    U = np.ascontiguousarray(U, dtype=np.float64)
    P, D = x.shape
    du = U.shape[1]
    prm = np.zeros(8)
    prm[:len(w.params)] = w.params
    b, s, st = np.empty((P, D)), np.empty((P, D)), np.empty(P)
    vp, model = C.c_void_p, C.c_int(w.model)
    pa, xa, ua, ba, sa, ta = prm.ctypes.data, x.ctypes.data, U.ctypes.data, b.ctypes.data, s.ctypes.data, st.ctypes.data
    drift, diag, stage = L.orc_model_drift, L.orc_model_diff_diag, L.orc_model_stage
    pp = vp(pa)
    for p in range(P):
        xp, up = vp(xa + 8 * D * p), vp(ua + 8 * du * p)
        drift(model, pp, xp, up, vp(ba + 8 * D * p))
        diag(model, pp, xp, up, vp(sa + 8 * D * p))
        stage(model, pp, xp, up, vp(ta + 8 * p))
    return b, s, st


class Objective:
    """the backup of P nodes (states x [P, D], stencils V [P, 2D + 1]) as a function of each node's own control"""

    def __init__(self, oracle, w, x, V, freeze=None, freeze_at=None, reordered=False):
        """freeze, freeze_at: the planted wrong mask -- dimension `freeze` takes its drift and diffusion at u = freeze_at.
        reordered: the same formula with the sums in another order and a reciprocal for the divisions -- a second double
        implementation, as far from this one as the device's is (tests/test_box_ref.py runs the minimiser on it to see that the
        pinned nodes survive rounding)"""
        self.oracle, self.w, self.reordered = oracle, w, reordered
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.V = np.asarray(V, dtype=np.float64)
        self.P, self.D = self.x.shape
        self.h2, self.t = BR.mca_constants(w)
        self.freeze = freeze
        if freeze is not None:
            b0, s0, _ = model_eval(oracle, w, self.x, np.broadcast_to(np.asarray(freeze_at, dtype=np.float64), (self.P, w.du)))
            self.b0, self.s0 = b0[:, freeze], s0[:, freeze]
        self.evals = 0

    def __call__(self, U):
        """(value [P], stationary [P]) at the controls U [P, du]"""
        b, s, st = model_eval(self.oracle, self.w, self.x, U)
        if self.freeze is not None:
            b[:, self.freeze], s[:, self.freeze] = self.b0, self.s0
        self.evals += 1
        D, t, V = self.D, self.t, self.V
        Q, PV = np.zeros(self.P), np.zeros(self.P)
        for m in range(D):
            half = t[2 * m + 1] * (s[:, m] * s[:, m]) / 2.0
            tb = t[2 * m] * b[:, m]
            pm = np.where(b[:, m] < -1e-14, half - tb, half)
            pp = np.where(b[:, m] > 1e-14, half + tb, half)
            if self.reordered:
                Q = (Q + pm) + pp
                PV = (PV + pm * V[:, 2 * m]) + pp * V[:, 2 * m + 1]
            else:
                Q += pm + pp
                PV += pm * V[:, 2 * m] + pp * V[:, 2 * m + 1]
        bad = Q < 1e-14
        Qs = np.where(bad, 1.0, Q)
        dt = self.h2 / Qs
        if self.reordered:
            inv = 1.0 / Qs
            val = (self.h2 * inv) * st + np.exp(-self.w.discount * (self.h2 * inv)) * ((1.0 - Qs * inv) * V[:, 2 * D] + PV * inv)
            return np.where(bad, 1.0e300, val), bad
        val = dt * st + np.exp(-self.w.discount * dt) * (PV / Qs + (1.0 - Qs / Qs) * V[:, 2 * D])
        return np.where(bad, 1.0e300, val), bad

    def at(self, u):
        return self(np.broadcast_to(np.asarray(u, dtype=np.float64), (self.P, len(u))))


def grid_point(lb, ub, G, c, slowest=False):
    """candidate c of the tensor grid: control 0 takes the fastest digit (slowest: the planted order)"""
    du = len(lb)
    dl = (ub - lb) / (G - 1)
    u, rem = np.empty(du), c
    for i in (range(du - 1, -1, -1) if slowest else range(du)):
        gi = rem % G
        rem //= G
        u[i] = ub[i] if gi == G - 1 else float(Fraction(gi) * Fraction(float(dl[i])) + Fraction(float(lb[i])))  # fma: one rounding
    return u


@dataclasses.dataclass
class Search:
    xm: np.ndarray
    fm: np.ndarray
    lo: np.ndarray      # the recorded bracket
    hi: np.ndarray
    stat: np.ndarray
    rec: np.ndarray     # a comparison was unsure
    spread: np.ndarray = None


def line_search(obj, u0, i, lo, hi, thr, steps=STEPS, sample=True):
    """the kernel's golden-section search of coordinate i from the point u0 [P, du] in the cell [lo, hi] [P]"""
    u = np.array(u0, dtype=np.float64)
    lo, hi = lo.copy(), hi.copy()
    x1, x2 = hi - GR * (hi - lo), lo + GR * (hi - lo)
    u[:, i] = x1
    f1, s1 = obj(u)
    u[:, i] = x2
    f2, s2 = obj(u)
    stat = s1 | s2
    rec = np.zeros(len(lo), dtype=bool)
    rlo, rhi = lo.copy(), hi.copy()

    def note():
        nonlocal rec, rlo, rhi
        first = ~rec & (np.abs(f1 - f2) <= thr)
        rlo, rhi, rec = np.where(first, lo, rlo), np.where(first, hi, rhi), rec | first

    for _ in range(steps):
        note()
        left = f1 < f2  # keep [lo, x2]
        hi = np.where(left, x2, hi)
        lo = np.where(left, lo, x1)
        xn = np.where(left, hi - GR * (hi - lo), lo + GR * (hi - lo))
        u[:, i] = xn
        fn, sn = obj(u)
        stat |= sn
        x1, f1, x2, f2 = np.where(left, xn, x2), np.where(left, fn, f2), np.where(left, x1, xn), np.where(left, f1, fn)
    note()
    rlo, rhi = np.where(rec, rlo, lo), np.where(rec, rhi, hi)
    out = Search(np.where(f1 < f2, x1, x2), np.minimum(f1, f2), rlo, rhi, stat, rec)
    if sample:
        vals = []
        for a in np.linspace(0.0, 1.0, NSAMPLE):
            u[:, i] = rlo + a * (rhi - rlo)
            vals.append(obj(u)[0])
        vals = np.array(vals)
        out.spread = np.where((vals >= 1.0e300).any(axis=0), np.inf, vals.max(axis=0) - vals.min(axis=0))
    return out


@dataclasses.dataclass
class BoxRef:
    val: np.ndarray          # [P] the minimiser's value
    u: np.ndarray            # [P, du] its point
    grid_val: np.ndarray     # [P] the grid scan's best
    grid_u: np.ndarray       # [P, du] the winning grid point
    grid_c: np.ndarray       # [P] its candidate number
    grid_unsure: np.ndarray  # [P] a different point lies within thr of the best
    stat: np.ndarray         # [P] some evaluated point was stationary
    ulo: np.ndarray          # [P, du] where the device's u may lie (module docstring: interval, widening)
    uhi: np.ndarray
    spread: np.ndarray       # [P] the largest spread over the recorded brackets (0 without a search)
    searches: list           # per line search: dict(round, i, lo, hi, spread, stat, take, take_unsure)

    def pinned(self, tol):
        """[P]: the grid is sure and every recorded bracket's spread is at most tol / 2 (tol = REL_TOL * scale)"""
        return ~self.grid_unsure & (self.spread <= tol / 2.0)


def minimise(obj, lb, ub, G, polish, thr, fault=None, widen=True):
    """node_backup_box at the P nodes of obj; thr = BOX_MARGIN * scale; fault: one of FAULTS / DROPPED_FAULTS"""
    assert fault is None or fault in FAULTS + DROPPED_FAULTS, fault
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    P, du = obj.P, len(lb)
    dl = (ub - lb) / (G - 1)
    total = G ** du
    best = np.full(P, 1.0e301)
    u = np.tile(lb, (P, 1))
    cbest = np.full(P, -1)
    allv, pts = np.empty((P, total)), np.empty((total, du))
    stat = np.zeros(P, dtype=bool)
    for c in range(total):
        pts[c] = grid_point(lb, ub, G, c, slowest=fault == "slowest")
        v, bad = obj.at(pts[c])
        stat |= bad
        allv[:, c] = v
        take = v < best
        best = np.where(take, v, best)
        cbest = np.where(take, c, cbest)
        u = np.where(take[:, None], pts[c][None, :], u)
    other = (pts[None, :, :] != u[:, None, :]).any(axis=-1)  # [P, total]: a different point
    second = np.where(other, allv, np.inf).min(axis=1)
    grid_unsure = second - best <= thr
    grid_val, grid_u = best.copy(), u.copy()
    ulo, uhi = u.copy(), u.copy()
    spread = np.zeros(P)
    searches = []
    rounds = 0 if fault == "no_polish" else min(polish, 1) if fault == "first_round" else polish
    coords = [0] if fault == "coord0" else list(range(du - 1, -1, -1)) if fault == "reverse" else list(range(du))
    half = dl / 2.0 if fault == "half_cell" else dl
    steps = 10 if fault == "steps10" else STEPS
    pstat = np.zeros(P, dtype=bool)
    for r in range(rounds):
        if fault == "restart" and r == 1:
            best, u, ulo, uhi = grid_val.copy(), grid_u.copy(), grid_u.copy(), grid_u.copy()
        for i in coords:
            lo, hi = u[:, i] - half[i], u[:, i] + half[i]
            if fault != "no_clamp":
                lo, hi = np.maximum(lb[i], lo), np.minimum(ub[i], hi)
            s = line_search(obj, u, i, lo, hi, thr, steps)
            pstat |= s.stat
            wlo, whi = s.lo.copy(), s.hi.copy()
            if widen and r == rounds - 1:
                for j in range(du):
                    if j == i or not (uhi[:, j] > ulo[:, j]).any():
                        continue
                    dlo, dhi = np.zeros(P), np.zeros(P)
                    for end in (ulo[:, j], uhi[:, j]):
                        u2 = u.copy()
                        u2[:, j] = end
                        s2 = line_search(obj, u2, i, lo, hi, thr, steps, sample=False)
                        dlo, dhi = np.maximum(dlo, s.lo - s2.lo), np.maximum(dhi, s2.hi - s.hi)
                    wlo, whi = wlo - dlo, whi + dhi
            take = np.ones(P, dtype=bool) if fault == "always_take" else s.fm < best
            # the device's fm lies within the spread of the reference's where a comparison was unsure, else within thr of it
            room = thr + np.where(s.rec, s.spread, 0.0)
            tun = np.abs(s.fm - best) <= room
            if fault == "always_take":
                tun = np.zeros(P, dtype=bool)
            ulo[:, i] = np.where(tun, np.minimum(wlo, ulo[:, i]), np.where(take, wlo, ulo[:, i]))
            uhi[:, i] = np.where(tun, np.maximum(whi, uhi[:, i]), np.where(take, whi, uhi[:, i]))
            best0 = best
            best = np.where(take, s.fm, best)
            u[:, i] = np.where(take, s.xm, u[:, i])
            # what the search can cost: nothing where the take surely fails, the spread where it is surely made, and the gap between
            # the two outcomes as well where it is unsure
            spread = np.maximum(spread, np.where(tun, np.maximum(s.spread, np.abs(s.fm - best0)), np.where(take, s.spread, 0.0)))
            searches.append(dict(round=r, i=i, lo=s.lo, hi=s.hi, spread=s.spread, stat=s.stat, take=take, take_unsure=tun))
    if fault != "grid_status":
        stat = stat | pstat
    return BoxRef(best, u, grid_val, grid_u, cbest, grid_unsure, stat, ulo, uhi, spread, searches)


# ---------------------------------------------------------------------------------------------------- the nodes of fibers
@dataclasses.dataclass
class FiberRef:
    idx: np.ndarray
    ab: np.ndarray       # [F, N] the oracle's flags
    val: np.ndarray      # [F, N] absorbed nodes: the oracle's costs
    u: np.ndarray        # [F, N, du] absorbed nodes: 0
    box: BoxRef          # over the F * N nodes in fiber order (absorbed nodes: computed and to be ignored)
    scale: float
    obj: Objective

    @property
    def live(self):
        return self.ab == 0

    def of(self, a):
        """a per-node array of box reshaped to [F, N, ...]"""
        return a.reshape(self.ab.shape + a.shape[1:])

    @property
    def pinned(self):
        return self.live & self.of(self.box.pinned(T.REL_TOL * self.scale))

    @property
    def status(self):
        return STATUS_STATIONARY if (self.of(self.box.stat) & self.live).any() else 0


def fiber_setup(oracle, w, cs, k, idx):
    """(x [P, D], V [P, 2D + 1], ab [F, N], cost [F, N]) of the batch: states, the oracle's stencils and flags, and on absorbed
    nodes the oracle's boundary / obstacle cost"""
    L, dp = oracle.lib(), oracle.dp
    P = oracle.Problem(w, cs)
    V, ab = P.stencil_fibers(k, idx)
    x = BR.node_states(w, k, idx).reshape(-1, w.dx)
    prm = np.zeros(8)
    prm[:len(w.params)] = w.params
    cost = np.zeros(ab.size)
    v = C.c_double(0)
    for p in np.flatnonzero(ab.reshape(-1) != 0):
        fn = L.orc_model_boundcost if ab.reshape(-1)[p] == 1 else L.orc_model_obscost
        fn(w.model, dp(prm), dp(np.ascontiguousarray(x[p])), C.byref(v))
        cost[p] = v.value
    return x, V.reshape(-1, 2 * w.dx + 1), ab, cost.reshape(ab.shape)


def frozen_dim(w):
    """the control-dependent dimension the "freeze" fault takes out of the mask: the first of the model's set"""
    return T.udep(T.MODEL_OF[w.name])[0]


def fibers(oracle, w, cs, k, idx, lb, ub, G, polish, signed, fault=None, widen=True, margin=BOX_MARGIN, reordered=False):
    """the box minimiser on every node of the fibers idx along k (FiberRef).  The scale is fiber_kernel_cases.scale_of of the
    clean grid scan (the same for every fault)"""
    x, V, ab, cost = fiber_setup(oracle, w, cs, k, idx)
    clean = Objective(oracle, w, x, V)
    scan = np.full(len(x), np.inf)
    for c in range(G ** len(lb)):
        scan = np.minimum(scan, clean.at(grid_point(np.asarray(lb, float), np.asarray(ub, float), G, c))[0])
    live = ab == 0
    scale = T.scale_of(oracle, w, cs, k, idx, np.where(live, scan.reshape(ab.shape), cost), signed)
    obj = Objective(oracle, w, x, V, frozen_dim(w), lb) if fault == "freeze" else Objective(oracle, w, x, V, reordered=True) if reordered else clean
    box = minimise(obj, lb, ub, G, polish, margin * scale, fault, widen)
    val = np.where(live, box.val.reshape(ab.shape), cost)
    u = np.where(live[..., None], box.u.reshape(ab.shape + (len(lb),)), 0.0)
    return FiberRef(idx, ab, val, u, box, float(scale), clean)


# ---------------------------------------------------------------------------------------------------- the rows
@dataclasses.dataclass(frozen=True)
class Row:
    name: str        # the workload
    tag: str
    lb: tuple
    ub: tuple
    grid: int
    polish: int
    edge: bool = False
    mul: float = 1.0  # every core of fiber_kernel_cases.cores times this

    @property
    def id(self):
        return f"{self.name}-{self.tag}"


def example_grid(du):
    """the default resolution of the examples' set-up (c3opt_alloc of a line-search optimiser): 33 / 17 / 9 points for du = 1 / 2 / 3"""
    return {1: 33, 2: 17, 3: 9}[du]


def box_case(name, lowest=True, npl2=False):
    """the fpw_box row of fiber_kernel_cases.CASES of a model at its lowest / highest registered rank class"""
    rows = [c for c in T.CASES if c.family == "fpw_box" and c.name == name and (c.tag == "npl2") == npl2]
    return min(rows, key=lambda c: c.rp) if lowest else max(rows, key=lambda c: c.rp)


BOX_MODELS = tuple(n for n, _, box, _ in T.FPW_MODELS if box)
SETTING_MODELS = ("lqg2d", "tprob3d", "cothrust6d")  # du = 1, 3, 3
NFIB = 7
Spec = namedtuple("Spec", "case tag grid polish kind")  # kind: kernel, plain, edge (>= EDGE_SHARE of the live nodes on a face), fixed


def row_specs():
    """The rows without their boxes.
      kernel rows    every box model at its lowest and its highest registered rank class and the NPL = 2 lqg2d row: the small grid of
                     fiber_kernel_cases.BOX, two rounds
      settings rows  lqg2d, tprob3d, cothrust6d at their lowest class: polish 0 .. 3, grid = 2 (the cell is the whole box), an even
                     grid (0 is no grid point of a symmetric box, and the faces' neighbours are no round numbers), the grid of the
                     example's set-up, an asymmetric box, two edge rows, and one control with lb == ub (the last)
      rounds         LqgNd<6>, LqgNd<4> and Cothrust6D at their lowest class, grid = 2, two rounds, on boxes found by a search for
                     rows under the cap where the second round moves a pinned node (LqgNd<4> signed: one in the outer half cell)"""
    out = []
    for name in BOX_MODELS:
        g = T.BOX[name][2]
        for lowest in (True, False):
            case = box_case(name, lowest)
            if not any(sp.case is case for sp in out):
                out.append(Spec(case, f"rp{case.rp}", g, 2, "kernel"))
    case = box_case("lqg2d", True, npl2=True)
    out.append(Spec(case, f"rp{case.rp}-npl2", T.BOX["lqg2d"][2], 2, "kernel"))
    for name in SETTING_MODELS:
        case, g = box_case(name), T.BOX[name][2]
        out += [Spec(case, f"polish{p}", g, p, "plain") for p in (0, 1, 2, 3)]
        out += [Spec(case, "grid2", 2, 2, "plain"), Spec(case, "even", g + 1, 2, "plain"),
                Spec(case, "example", example_grid(len(T.BOX[name][0])), 2, "plain"), Spec(case, "asym", g, 2, "plain"),
                Spec(case, "edge", g, 2, "edge"), Spec(case, "edge2", g - 1, 1, "edge"), Spec(case, "fixed", g, 2, "fixed")]
    for name in ("lqg6d", "lqg4d", "cothrust6d"):  # where the second round moves a pinned node, or one lies in the outer half cell
        out.append(Spec(box_case(name), "rounds", 2, 2, "plain"))
    return out


def spec_key(sp):
    return f"{T.case_id(sp.case)}/{sp.tag}"


# The boxes and the cores.  Under BOX_MARGIN a node whose minimiser is a smooth interior minimum is unpinned more often than not.
# First round: an unsure comparison needs the minimum within thr / (0.47 a w) of the middle of a bracket of width w (a: the
# curvature), and it leaves the node unpinned while a w^2 is above the tolerance; summed over those steps (w shrinks by 0.618) the
# probability is ~ 3.4 BOX_MARGIN / (REL_TOL / 2) = 0.64.  From the second round on the first two probes lie symmetric about the
# point the first round found and differ by the odd part of the objective alone: on the fine grids of the examples that is below
# thr at 94 % of lqg2d's nodes (the recorded bracket is then the whole cell), on grids of 2 or 3 points at a quarter of them.  The nodes that are pinned are those whose decisions are all clear: the minimiser on a face of the box (the search
# runs into the face and its result is surely not taken) or at a kink of the upwind rates (both one-sided slopes are far above thr
# down to the last bracket).  So a row is BUILT on a sub-box [lb + a wd, lb + (a + b) wd] of the example's range and on cores scaled
# by `mul` (larger values against the same stage cost: fewer smooth interior minima), chosen per data class from the reference
# alone by choose() over the fixed list candidates() and grid_options(), among the entries that survives() accepts; `python tests/box_ref.py` prints the table.  A (row, data class) for which no
# entry of the list keeps the preconditions (row_ok) is NOT built; tests/test_box_ref.py holds the preconditions on every built row
# and checks that the rows not built are exactly those the table leaves out.
EDGE_SHARE = 0.10
MULS = (1.0, 4.0, 16.0, 64.0)
MIN_INTERIOR_PINNED = 1  # pinned live nodes that the polish moved off their grid point: the nodes on which a wrong polish shows
BOXES = {  # (row, signed) -> (lb, ub, mul, control grid)
    ('fpw_box-LqgNd4-4/rounds', False): ((-0.2, -0.2), (0.2, 0.2), 1.0, 2),
    ('fpw_box-LqgNd4-4/rounds', True): ((-0.2, -0.2), (0.1, 0.1), 8.0, 2),
    ('fpw_box-Cothrust6D-4/rounds', False): ((0.0, 0.0, 0.0), (0.45, 0.12, 0.12), 8.0, 2),
    ('fpw_box-Cothrust6D-4/rounds', True): ((0.45, 0.12, 0.12), (1.26, 0.336, 0.336), 256.0, 2),
    # from the wide list, and the three FACE_ONLY pairs
    ('fpw_box-Rossler3D-4/rp4', False): ((-3.6,), (-1.44,), 8.0, 9),
    ('fpw_box-Tprob3D-4/rp4', True): ((-4.5, -4.5, -4.5), (-1.8, -1.8, -1.8), 32.0, 5),
    ('fpw_box-Tprob3D-20/rp20', True): ((-1.5, -1.5, -1.5), (0.0, 0.0, 0.0), 32.0, 3),
    ('fpw_box-LqgNd4-4/rp4', False): ((0.7, 0.7), (1.0, 1.0), 2.0, 5),
    ('fpw_box-Cothrust6D-20/rp20', False): ((-1.05, -0.28, -0.28), (0.21, 0.056, 0.056), 0.25, 5),
    ('fpw_box-Tprob3D-4/polish2', True): ((-4.5, -4.5, -4.5), (-1.8, -1.8, -1.8), 32.0, 5),
    ('fpw_box-Tprob3D-4/polish3', True): ((-4.5, -4.5, -4.5), (-1.8, -1.8, -1.8), 32.0, 5),
    ('fpw_box-Tprob3D-4/grid2', True): ((-3.0, -3.0, -3.0), (-1.5, -1.5, -1.5), 32.0, 2),
    ('fpw_box-Tprob3D-4/asym', True): ((-4.5, -4.5, -4.5), (-1.8, -1.8, -1.8), 32.0, 5),
    ('fpw_box-Tprob3D-4/edge', True): ((-4.5, -4.5, -4.5), (-1.8, -1.8, -1.8), 32.0, 5),
    ('fpw_box-Cothrust6D-4/even', False): ((-0.45, -0.12, -0.12), (0.36, 0.096, 0.096), 2.0, 6),
    ('fpw_box-Cothrust6D-4/example', False): ((-1.05, -0.28, -0.28), (0.21, 0.056, 0.056), 0.25, 9),
    ('fpw_box-LqgNd6-4/rounds', True): ((-1.0, -1.0, -1.0), (0.0, 0.0, 0.0), 64.0, 2),
    ('fpw_box-Tprob3D-20/rp20', False): ((3.0, 3.0, 3.0), (4.5, 4.5, 4.5), 8.0, 5),
    ('fpw_box-Tprob3D-4/even', True): ((-5.0, -5.0, -5.0), (-3.5, -3.5, -3.5), 256.0, 6),
    ('fpw_box-Tprob3D-4/example', True): ((-5.0, -5.0, -5.0), (-3.5, -3.5, -3.5), 256.0, 9),
    # from the first list
    ('fpw_box-Perch7D-4/rp4', False): ((-6.283185307179586,), (6.283185307179586,), 1.0, 9),
    ('fpw_box-Perch7D-4/rp4', True): ((-6.283185307179586,), (6.283185307179586,), 1.0, 9),
    ('fpw_box-Perch7D-20/rp20', False): ((-6.283185307179586,), (0.0,), 1.0, 9),
    ('fpw_box-Perch7D-20/rp20', True): ((-6.283185307179586,), (6.283185307179586,), 1.0, 9),
    ('fpw_box-LqgNd6-4/rounds', False): ((-1.0, -1.0, -1.0), (-0.3, -0.3, -0.3), 4.0, 2),
    ('fpw_box-Rossler3D-4/rp4', True): ((-2.4,), (-0.8,), 64.0, 9),
    ('fpw_box-Rossler3D-20/rp20', False): ((-4.0,), (0.0,), 4.0, 9),
    ('fpw_box-Rossler3D-20/rp20', True): ((-2.4,), (-0.8,), 16.0, 9),
    ('fpw_box-Tprob3D-4/rp4', False): ((3.0, 3.0, 3.0), (5.0, 5.0, 5.0), 16.0, 3),
    ('fpw_box-LqgNd2-4/rp4', False): ((-1.0,), (-0.3,), 16.0, 9),
    ('fpw_box-LqgNd2-4/rp4', True): ((-0.6,), (-0.2,), 1.0, 9),
    ('fpw_box-LqgNd2-20/rp20', False): ((-0.8,), (-0.4,), 1.0, 9),
    ('fpw_box-LqgNd2-20/rp20', True): ((0.2,), (0.9,), 1.0, 9),
    ('fpw_box-LqgNd4-4/rp4', True): ((0.0, 0.0), (0.7, 0.7), 64.0, 5),
    ('fpw_box-LqgNd6-4/rp4', False): ((-0.6, -0.6, -0.6), (-0.2, -0.2, -0.2), 4.0, 5),
    ('fpw_box-LqgNd6-4/rp4', True): ((-1.0, -1.0, -1.0), (-0.3, -0.3, -0.3), 64.0, 5),
    ('fpw_box-LqgNd6-20/rp20', False): ((0.2, 0.2, 0.2), (0.6, 0.6, 0.6), 1.0, 5),
    ('fpw_box-LqgNd6-20/rp20', True): ((0.2, 0.2, 0.2), (0.9, 0.9, 0.9), 16.0, 3),
    ('fpw_box-Cothrust6D-4/rp4', False): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 3),
    ('fpw_box-Cothrust6D-4/rp4', True): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 5),
    ('fpw_box-Cothrust6D-20/rp20', True): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 5),
    ('fpw_box-LqgNd2-4-npl2/rp4-npl2', False): ((-0.8,), (-0.1,), 16.0, 9),
    ('fpw_box-LqgNd2-4-npl2/rp4-npl2', True): ((-0.8,), (-0.1,), 1.0, 9),
    ('fpw_box-LqgNd2-4/polish0', False): ((-1.0,), (1.0,), 1.0, 9),
    ('fpw_box-LqgNd2-4/polish0', True): ((-1.0,), (1.0,), 1.0, 9),
    ('fpw_box-LqgNd2-4/polish1', False): ((-1.0,), (0.0,), 16.0, 9),
    ('fpw_box-LqgNd2-4/polish1', True): ((0.2,), (0.9,), 1.0, 9),
    ('fpw_box-LqgNd2-4/polish2', False): ((-1.0,), (-0.3,), 16.0, 9),
    ('fpw_box-LqgNd2-4/polish2', True): ((-0.6,), (-0.2,), 1.0, 9),
    ('fpw_box-LqgNd2-4/polish3', False): ((-1.0,), (-0.3,), 16.0, 9),
    ('fpw_box-LqgNd2-4/polish3', True): ((-0.6,), (-0.2,), 1.0, 9),
    ('fpw_box-LqgNd2-4/grid2', False): ((0.0,), (1.0,), 16.0, 2),
    ('fpw_box-LqgNd2-4/grid2', True): ((-1.0,), (-0.3,), 4.0, 2),
    ('fpw_box-LqgNd2-4/even', False): ((-1.0,), (-0.3,), 1.0, 10),
    ('fpw_box-LqgNd2-4/even', True): ((-0.6,), (-0.2,), 1.0, 10),
    ('fpw_box-LqgNd2-4/example', False): ((-1.0,), (-0.3,), 1.0, 33),
    ('fpw_box-LqgNd2-4/example', True): ((-0.6,), (-0.2,), 1.0, 33),
    ('fpw_box-LqgNd2-4/asym', False): ((-1.0,), (-0.3,), 16.0, 9),
    ('fpw_box-LqgNd2-4/asym', True): ((-0.6,), (-0.2,), 1.0, 9),
    ('fpw_box-LqgNd2-4/edge', False): ((-1.0,), (-0.3,), 16.0, 9),
    ('fpw_box-LqgNd2-4/edge', True): ((-0.6,), (-0.2,), 1.0, 9),
    ('fpw_box-LqgNd2-4/edge2', False): ((0.0,), (1.0,), 16.0, 8),
    ('fpw_box-LqgNd2-4/edge2', True): ((-0.8,), (-0.4,), 16.0, 8),
    ('fpw_box-LqgNd2-4/fixed', False): ((-0.4,), (-0.4,), 1.0, 9),
    ('fpw_box-LqgNd2-4/fixed', True): ((-0.4,), (-0.4,), 1.0, 9),
    ('fpw_box-Tprob3D-4/polish0', False): ((-5.0, -5.0, -5.0), (5.0, 5.0, 5.0), 1.0, 5),
    ('fpw_box-Tprob3D-4/polish0', True): ((-5.0, -5.0, -5.0), (5.0, 5.0, 5.0), 1.0, 5),
    ('fpw_box-Tprob3D-4/polish1', False): ((0.0, 0.0, 0.0), (3.5, 3.5, 3.5), 16.0, 3),
    ('fpw_box-Tprob3D-4/polish1', True): ((-5.0, -5.0, -5.0), (-3.0, -3.0, -3.0), 64.0, 5),
    ('fpw_box-Tprob3D-4/polish2', False): ((3.0, 3.0, 3.0), (5.0, 5.0, 5.0), 16.0, 3),
    ('fpw_box-Tprob3D-4/polish3', False): ((3.0, 3.0, 3.0), (5.0, 5.0, 5.0), 16.0, 3),
    ('fpw_box-Tprob3D-4/grid2', False): ((-4.0, -4.0, -4.0), (-2.0, -2.0, -2.0), 16.0, 2),
    ('fpw_box-Tprob3D-4/even', False): ((-2.0, -2.0, -2.0), (0.0, 0.0, 0.0), 16.0, 6),
    ('fpw_box-Tprob3D-4/example', False): ((3.0, 3.0, 3.0), (5.0, 5.0, 5.0), 16.0, 9),
    ('fpw_box-Tprob3D-4/asym', False): ((3.0, 3.0, 3.0), (5.0, 5.0, 5.0), 16.0, 3),
    ('fpw_box-Tprob3D-4/edge', False): ((3.0, 3.0, 3.0), (5.0, 5.0, 5.0), 16.0, 3),
    ('fpw_box-Tprob3D-4/edge2', False): ((0.0, 0.0, 0.0), (3.5, 3.5, 3.5), 16.0, 3),
    ('fpw_box-Tprob3D-4/edge2', True): ((-5.0, -5.0, -5.0), (-3.0, -3.0, -3.0), 64.0, 4),
    ('fpw_box-Tprob3D-4/fixed', False): ((-2.0, -2.0, -2.0), (0.0, 0.0, -2.0), 4.0, 3),
    ('fpw_box-Tprob3D-4/fixed', True): ((3.0, 3.0, -2.0), (5.0, 5.0, -2.0), 64.0, 3),
    ('fpw_box-Cothrust6D-4/polish0', False): ((-1.5, -0.4, -0.4), (1.5, 0.4, 0.4), 1.0, 5),
    ('fpw_box-Cothrust6D-4/polish0', True): ((-1.5, -0.4, -0.4), (1.5, 0.4, 0.4), 1.0, 5),
    ('fpw_box-Cothrust6D-4/polish1', False): ((0.6, 0.16, 0.16), (1.2, 0.32, 0.32), 16.0, 5),
    ('fpw_box-Cothrust6D-4/polish1', True): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 5),
    ('fpw_box-Cothrust6D-4/polish2', False): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 3),
    ('fpw_box-Cothrust6D-4/polish2', True): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 5),
    ('fpw_box-Cothrust6D-4/polish3', False): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 3),
    ('fpw_box-Cothrust6D-4/polish3', True): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 5),
    ('fpw_box-Cothrust6D-4/grid2', False): ((0.6, 0.16, 0.16), (1.2, 0.32, 0.32), 4.0, 2),
    ('fpw_box-Cothrust6D-4/grid2', True): ((-0.6, -0.16, -0.16), (0.45, 0.12, 0.12), 16.0, 2),
    ('fpw_box-Cothrust6D-4/even', True): ((0.0, 0.0, 0.0), (0.6, 0.16, 0.16), 64.0, 6),
    ('fpw_box-Cothrust6D-4/example', True): ((-0.6, -0.16, -0.16), (0.45, 0.12, 0.12), 16.0, 9),
    ('fpw_box-Cothrust6D-4/asym', False): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 3),
    ('fpw_box-Cothrust6D-4/asym', True): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 5),
    ('fpw_box-Cothrust6D-4/edge', False): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 3),
    ('fpw_box-Cothrust6D-4/edge', True): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 5),
    ('fpw_box-Cothrust6D-4/edge2', False): ((0.3, 0.08, 0.08), (1.35, 0.36, 0.36), 1.0, 4),
    ('fpw_box-Cothrust6D-4/edge2', True): ((-0.6, -0.16, -0.16), (0.45, 0.12, 0.12), 1.0, 4),
    ('fpw_box-Cothrust6D-4/fixed', False): ((0.6, 0.16, -0.16), (1.2, 0.32, -0.16), 4.0, 3),
    ('fpw_box-Cothrust6D-4/fixed', True): ((-1.2, -0.32, -0.16), (0.3, 0.08, -0.16), 1.0, 5),
}


# rows of row_specs that run on neither data class: no entry of the list leaves a PINNED node that the polish moved while the cap holds
WHOLLY_MISSING = ()
# FACE ONLY: the (row, data class) pairs for which neither list of candidates() leaves a pinned node that the polish moved while the
# cap holds.  They run on the first entry that keeps the cap and hold the grid scan, the clamp, the take rule, the status bit and
# the kernel's name -- no coverage of the polish; tests/test_box_ref.py asserts that they have no pinned interior node (a row that
# gains one belongs in the table proper)
FACE_ONLY = {('fpw_box-Tprob3D-20/rp20', False), ('fpw_box-Tprob3D-4/even', True), ('fpw_box-Tprob3D-4/example', True)}


def grid_options(sp):
    """the control grids a row may take: its own; for a du >= 2 row that is not named for its grid also the coarse grid of 3 points
    (wide cells: second rounds whose first comparison is clear, minimisers far from their grid point)"""
    if sp.tag in ("grid2", "even", "example") or sp.polish == 0 or len(T.BOX[sp.case.name][0]) < 2:
        return (sp.grid,)
    return (sp.grid, 3)


def candidates(name, kind, wide=False):
    """the list a row's box and core scale are chosen from; wide: the longer list, walked for the pairs the first one leaves out"""
    lb, ub, _ = T.BOX[name]
    lb, ub = np.array(lb, dtype=np.float64), np.array(ub, dtype=np.float64)
    wd = ub - lb
    for b in ((0.85, 0.6, 0.42, 0.27, 0.15) if wide else (1.0, 0.7, 0.5, 0.35, 0.2)):
        for a in np.arange(0.0, 1.0 - b + 1e-9, 0.05 if wide else 0.1):
            lo, hi = np.round(lb + a * wd, 4), np.round(lb + (a + b) * wd, 4)
            if kind == "fixed":
                lo[-1] = hi[-1] = np.round(lb[-1] + 0.3 * wd[-1], 4)
            for mul in ((0.25, 2.0, 8.0, 32.0, 256.0) if wide else MULS):
                yield tuple(map(float, lo)), tuple(map(float, hi)), mul


def row_stats(ref, row):
    """of a FiberRef: live nodes, unpinned share, nodes whose minimiser is interior to a cell (the polish moved u off the grid
    point), those of them that are pinned, share of the live nodes whose best grid point is on a face of the box"""
    live, pin, b = ref.live, ref.pinned, ref.box
    free = np.array(row.ub) > np.array(row.lb)
    face = (((b.grid_u == np.array(row.lb)) | (b.grid_u == np.array(row.ub))) & free).any(axis=1).reshape(live.shape)
    moved = (b.u != b.grid_u).any(axis=1).reshape(live.shape)
    n = max(int(live.sum()), 1)
    return dict(live=int(live.sum()), free=bool(free.any()), unpinned=float((live & ~pin).sum() / n), interior=int((live & moved).sum()),
                interior_pinned=int((live & moved & pin).sum()), face=float((live & face).sum() / n))


# Perch7D's objective has no interior minimiser in u: on every box of candidates(), every grid and every core scale, on both data
# classes and both rank classes, the polish moves no live node (its control enters the drift alone, without a cost of its own: the
# minimum is at a face or a grid point).  Its two kernel rows run on the example's box (rank class 20, synth: on its lower half,
# where the grid scan is clear at every node) and hold the grid scan, the clamp and the take rule of its kernels; they are no coverage of the polish, and DESIGN.md 6.4 says so.
NO_INTERIOR = ("perch7d",)


def row_ok(sp, stats, face_only=False):
    """the preconditions of a row: the cap, pinned live nodes with an interior minimiser (where there is a polish; not on a
    face-only row), the edge rows' share"""
    return (stats["live"] > 0 and stats["unpinned"] <= MAX_UNPINNED
            and (sp.polish == 0 or not stats["free"] or face_only or sp.case.name in NO_INTERIOR
                 or stats["interior_pinned"] >= MIN_INTERIOR_PINNED)
            and (sp.kind != "edge" or stats["face"] >= EDGE_SHARE))


def make_row(sp, lo, hi, mul, grid=None):
    return Row(sp.case.name, sp.tag, tuple(lo), tuple(hi), grid or sp.grid, sp.polish, sp.kind == "edge", mul)


def survives(oracle, case, row, signed):
    """the minimiser on the re-ordered objective (Objective(reordered=True)) passes check_device against the reference of the row:
    the pinned rule bounds one search at a time, and a row on which a flipped comparison cascades through later searches is left out"""
    import contextlib
    import io

    ref = row_ref(oracle, case, row, signed)[3]
    other = row_ref(oracle, case, row, signed, widen=False, reordered=True)[3]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            check_device(ref, other.val, other.u, other.ab, other.status, row.lb, row.ub, row.polish)
    except AssertionError:
        return False
    return True


def choose(oracle, sp, signed, wide=False, face_only=False):
    """the entry of candidates() x grid_options() that keeps row_ok and survives() with the most pinned interior nodes (the first
    one with three, else the first of the best); None where there is none.  face_only: the first entry that keeps the cap"""
    best, score = None, -1
    for G in grid_options(sp):
        for lo, hi, mul in candidates(sp.case.name, sp.kind, wide):
            row = make_row(sp, lo, hi, mul, G)
            st = row_stats(row_ref(oracle, sp.case, row, signed, widen=False)[3], row)
            _REF.clear()
            if row_ok(sp, st, face_only) and st["interior_pinned"] > score and survives(oracle, sp.case, row, signed):
                best, score = (lo, hi, mul, G), st["interior_pinned"]
                if score >= 3 or sp.polish == 0 or face_only:
                    return best
    return best


def built_rows(kinds=None):
    """[(Case, Row, signed)] of the (row, data class) pairs of row_specs that BOXES holds.  Rows of one case and data class that
    come out as the same launch (box, grid, polish, cores) are ONE entry whose tag joins theirs with '+': the launch runs once and
    counts once"""
    out, at = [], {}
    for sp in row_specs():
        for signed in (False, True):
            key = (spec_key(sp), signed)
            if key in BOXES and (kinds is None or sp.kind in kinds):
                row = make_row(sp, *BOXES[key])
                same = (T.case_id(sp.case), row.lb, row.ub, row.grid, row.polish, row.mul, signed)
                if same in at:
                    c, r, sg = out[at[same]]
                    out[at[same]] = (c, dataclasses.replace(r, tag=r.tag + "+" + row.tag, edge=r.edge or row.edge), sg)
                else:
                    at[same] = len(out)
                    out.append((sp.case, row, signed))
    return out


def specs_of(case, row):
    """the specs a (possibly merged) row stands for"""
    by = {spec_key(sp): sp for sp in row_specs()}
    return [by[f"{T.case_id(case)}/{t}"] for t in row.tag.split("+")]


def not_built():
    return [(spec_key(sp), signed) for sp in row_specs() for signed in (False, True) if (spec_key(sp), signed) not in BOXES]


def kernel_rows():
    """the built rows that stand for a kernel row (a settings row that is the same launch is merged into it)"""
    return [r for r in built_rows() if any(sp.kind == "kernel" for sp in specs_of(r[0], r[1]))]


def setting_rows():
    return [r for r in built_rows() if not any(sp.kind == "kernel" for sp in specs_of(r[0], r[1]))]


def row_id(case, row, signed):
    return f"{T.case_id(case)}-{row.tag}-{'signed' if signed else 'synth'}"


def interior_fibers(w, k, F):
    """F seeded fibers along k with every fixed index off the faces (1 .. N - 2): Perch7D's batches, whose fibers of
    fiber_kernel_cases.fibers leave four live nodes in seven fibers (six fixed indices on grids of 5 .. 7 nodes)"""
    rng = np.random.default_rng(0xB0C5 + k)
    idx = rng.integers(1, np.array(w.ngrid) - 1, size=(F, w.dx))
    idx[:, k] = 0
    return np.ascontiguousarray(idx, dtype=np.int32)


def fibers_of(case):
    return interior_fibers if case.name == "perch7d" else T.fibers


def middle_k(case):
    return case.ks[len(case.ks) // 2]


_REF = {}


def row_ref(oracle, case, row, signed, fault=None, w=None, fib=None, margin=BOX_MARGIN, widen=True, reordered=False):
    """(workload, cores, k, FiberRef) of a row on its case's workload (or w), NFIB fibers (fiber_kernel_cases.fibers, or fib) along
    the middle k (memoised: the reference is computed once and shared)"""
    key = (T.case_id(case), row, signed, fault, None if w is None else (w.params, w.ngrid), None if fib is None else fib.__name__, margin, widen, reordered)
    if key not in _REF:
        w = w or T.workload(case)
        cs = [c * row.mul for c in T.cores(case, w, signed)]
        k = middle_k(case)
        idx = (fib or fibers_of(case))(w, k, NFIB)
        _REF[key] = (w, cs, k, fibers(oracle, w, cs, k, idx, row.lb, row.ub, row.grid, row.polish, signed, fault, widen, margin, reordered))
    return _REF[key]


# ---------------------------------------------------------------------------------------------------- the stationary rows
# LqgNd without diffusion (fiber_kernel_cases.stationary_workload: sigma = 0, a node at 0 on every axis): at a node with x1 = 0 the
# control u = 0 leaves every rate zero, Q < 1e-14.  Q vanishes only within 1e-14 of u = 0, and the box is one per launch, so a point
# is stationary either on the grid (0 is a grid point) or on a probe, never both in one launch; and the status word is one per
# launch.  Hence two launches:
#   grid    the example's box [-1, 1] on the odd grid: u = 0 is a grid point
#   probe   the box [-gr, 1 - gr] with grid = 2: the cell is the whole box, of width exactly 1 (1 - gr is exact, by Sterbenz), and
#           the second probe lo + gr (hi - lo) = -gr + gr is exactly 0; neither grid point is 0
STATIONARY = (Row("lqg2d", "stationary-grid", (-1.0,), (1.0,), 9, 2), Row("lqg2d", "stationary-probe", (-GR,), (1.0 - GR,), 2, 2))


def stationary_case():
    return box_case("lqg2d", True)


def stationary_workload(case):
    return T.stationary_workload(case)


def stationary_fibers(w, k, F):
    return T.fibers_through(w, k, F)


# ---------------------------------------------------------------------------------------------------- the device's side
def check_device(ref, out, uo, ab, status, lb, ub, polish, what=""):
    """Holds one bellman_fibers_box_host launch (values out [F, N], controls uo [F, N, du], flags ab, the status word) to the
    FiberRef.  Returns (worst value error on pinned nodes relative to the scale, unpinned share of the live nodes).
      flags     absorbed flags exact; absorbed values exact, their u = 0
      value     pinned live nodes: |out - ref| <= REL_TOL * scale
      u         pinned live nodes: ulo_i <= u_i <= uhi_i (module docstring: interval, widening); polish = 0: bit-equal to the grid
                point on every node whose grid scan is sure
      unpinned  out <= the reference's grid-scan value + REL_TOL * scale (the device's own rounding of the grid point's value: where
                the polish gains nothing it returns that value, one rounding of its own away from the reference's), u inside the box
      status    the STATIONARY bit equals the reference's"""
    lb, ub = np.asarray(lb), np.asarray(ub)
    tol = T.REL_TOL * ref.scale
    np.testing.assert_array_equal(ab, ref.ab, err_msg=f"{what}: absorbed flags")
    live, pin = ref.live, ref.pinned
    assert np.array_equal(out[~live], ref.val[~live]), f"{what}: absorbed values"
    assert not uo[~live].any(), f"{what}: u of absorbed nodes"
    err = np.abs(out - ref.val)
    worst = float(err[pin].max() / ref.scale) if pin.any() else 0.0
    unp = float((live & ~pin).sum() / max(int(live.sum()), 1))
    print(f"{what}: worst value error {worst:.2e} on {int(pin.sum())} pinned nodes, unpinned share {unp:.3f}")
    assert worst <= T.REL_TOL, f"{what}: value error {worst:.3e} of the scale {ref.scale:.3e} at node {np.unravel_index(np.where(pin, err, -1).argmax(), err.shape)}"
    ulo, uhi = ref.of(ref.box.ulo), ref.of(ref.box.uhi)
    outside = pin[..., None] & ((uo < ulo) | (uo > uhi))
    assert not outside.any(), (f"{what}: {int(outside.any(axis=-1).sum())} pinned nodes with u outside the recorded bracket; first "
                               f"{np.argwhere(outside)[0]}: u {uo[tuple(np.argwhere(outside)[0])]!r} not in "
                               f"[{ulo[tuple(np.argwhere(outside)[0])]!r}, {uhi[tuple(np.argwhere(outside)[0])]!r}]")
    if polish == 0:
        sure = live & ~ref.of(ref.box.grid_unsure)
        assert np.array_equal(uo[sure], ref.u[sure]), f"{what}: polish = 0, u is not the grid point"
    loose = live & ~pin
    gv = ref.of(ref.box.grid_val)
    assert (out[loose] <= gv[loose] + tol).all(), f"{what}: an unpinned node above the grid scan"
    assert ((uo[live] >= lb) & (uo[live] <= ub)).all(), f"{what}: u outside the box"
    assert (status & STATUS_STATIONARY) == ref.status, f"{what}: status word {status}, the reference's STATIONARY bit is {ref.status}"
    return worst, unp


if __name__ == "__main__":  # prints the lines of BOXES; `missing`: the pairs BOXES lacks, from the wide list, then face-only
    import multiprocessing as mp

    import oracle_lib

    oracle_lib.build()
    MISSING = "missing" in sys.argv
    KEYS = set(not_built())
    JOBS = [(i, signed) for i, sp in enumerate(row_specs()) for signed in (False, True) if not MISSING or (spec_key(sp), signed) in KEYS]

    def _one(job):
        sp = row_specs()[job[0]]
        if not MISSING:
            return (spec_key(sp), job[1]), choose(oracle_lib, sp, job[1]), ""
        box = choose(oracle_lib, sp, job[1], wide=True)
        if box:
            return (spec_key(sp), job[1]), box, "  # wide list"
        return (spec_key(sp), job[1]), choose(oracle_lib, sp, job[1], face_only=True), "  # FACE ONLY"

    with mp.Pool(8) as pool:
        for key, box, note in pool.imap(_one, JOBS):
            print(f"    {key!r}: {box},{note}" if box else f"    # {key!r}: no entry of the list keeps the preconditions", flush=True)
