"""The case table of the Bellman fiber kernels: every instantiation the C3SC_REG_FPW / _FPW_BOX / _FPP1 / _FQ1 / _FQD / REG_FQD_SB
/ _STENCIL lines of c3sc_amd/csrc/inst_*.hip register (k_fiber_per_wave, k_fiber_pair, k_fiber_quad, k_fiber_quad_duo) -- TEST
INFRASTRUCTURE ONLY.

A row names the workload, the grid, the bond ranks, the engine variant and the batch size that select its instantiations, the
varying dimensions it runs and, for each of them, the exact string eng.last_kernel() must then report.  One row per (family,
model or D, padded rank RP), plus rows marked by a tag: `npl2` (two nodes per lane: the varying N in 65 .. 128), `unstaged` (the
varying core exceeds FPW_MAX_LDS: the STAGED = false instantiation of the per-wave kernel), `behind-duo` (a grid on which the duo
launcher declines for LDS and the quad kernel registered behind it runs).

Families: fpw (the per-wave kernel's candidate-list form, C3SC_REG_FPW and C3SC_REG_FPW_BOX entries), fpw_box (the box minimiser of
the C3SC_REG_FPW_BOX entries, cmode 1), fpp (pair), fq (quad), fqd (duo; a row also names the quad kernel that serves a k the duo
form is not registered for), table (TableModel<D>), stencil (on-grid stencil, model 0).

Ranks: the largest bond rank lies above the model's next smaller class of the forced variant and below the class itself where the
class allows (3, 5, 7, 9, 11, 13 .. 15, 17 .. 19 for 4, 6, 8, 10, 12, 16, 20), so the padding columns of the cores are exercised;
bond ranks are unequal for D >= 3 (a D = 2 train has a single bond).  The variant is set BEFORE the value is uploaded: the padded
rank follows it (pick_rp in c3sc_hip.hip).

Batches: ragged against the kernel's tile (4 fibers per workgroup per-wave, 64 pair, 16 NWV quad, 8 NWV duo) and at least three
tiles for the pair / quad / duo families; rows 0, 1, 2 are the all-zero, all N-1 and all-1 fixed indices.

tests/test_fiber_kernel_cases.py holds the table to the registry (registered == table + UNREACHABLE) and to a restatement of the
selection logic and of the launchers' LDS arithmetic, and pins the reference below to the oracle; tests/test_gpu_fiber_kernels.py
runs every row on a device.

LDS arithmetic behind the tagged rows (doubles; the limit is 160 KiB = 20480 doubles; CW = doubles per candidate row):
  per-wave, staged:  4 (4 RP + 2 D RP + 64 NPL) + N_k ((k is an end ? RP : RP^2) | 1) + ncand CW
    RP 20, NPL 1: 401 N_k > ~19300 from N_k = 49 on (scar4d (12, 60, 10, 9), k = 1)
    RP 16, NPL 2: 257 N_k > ~19400 from N_k = 76 on (dubins3d (65, 128, 70), k = 1); NPL 1 stops at N = 64: 16448 + 4 WS fits
    RP 12: 145 x 128 + 992 = 19552: fits at every N <= 128 (a candidate list of ~190 rows would be needed): no row
    an end dimension (k = 0, d - 1; both dimensions of a 2-D problem) stages N RP doubles and always fits
  duo:  S (x 2 with two staging buffers) + (NWV/2) (16 N_k + 16 D + 128 D) + ncand CW,  S = max_{m != k} N_m (RP^2 + 2) (RP + 2 at ends)
  quad: S + NWV 16 (one pass ? 18 : N_k) + ncand CW;  one pass unless RP >= 16 and D >= 8
    Skid5D 16 (duo: one buffer, NWV 8; quad NWV 8): N_2 = 68: S = 17544; duo 17544 + 64 N_k + 2880 > 20480, quad 17544 + 2304 fits
    Perch7D 16 (duo: two buffers, NWV 8; quad NWV 4): N_m = 40: S = 10320; duo 20640 > 20480, quad 10320 + 1152 fits
    Chain<10> 16 (duo: two buffers, NWV 8; quad NWV 4, two passes): N_m = 30: S = 7740; duo 15480 + 5760 + 64 N_k > 20480, quad fits
  the big dimension's own k does not stage its core (the duo kernel runs there), so Perch7D and Chain<10> have a second row with
  the big dimension elsewhere."""
from collections import namedtuple

import numpy as np

from c3sc_amd import workloads as wl
from sim_kernel_cases import _chain

# kernel name -> why no (grid, ranks, variant, k) selects the registration.  Empty: every registration is selected by a row.
UNREACHABLE = {}

REL_TOL = 1e-12
# The bar of the project, |got - ref| <= REL_TOL * scale.  `synth` data (cores in 0.3 .. 0.4, no cancellation): scale = max |ref|
# over the batch.  Signed data (synth_cores - 0.35): max |ref| can be small against the terms that cancel, so
#   scale = max(max |ref|, max Vabs),  Vabs = the oracle's stencil (P.stencil_fibers) of the same fibers on |cores|.
# Derivation (the bound tests/offgrid_ref.py derived for the off-grid kernels, on grid nodes): a train value is d matrix-vector
# products of inner length <= r, so every computed value carries at most d r roundings of terms whose moduli sum to the same
# train on |cores|: |fl(V) - V| <= d r u Vabs + O(u^2), u = 2^-53.  The backup is dt stage + exp(-beta dt) sum_i p_i V_i over the
# 2d + 1 stencil nodes with probabilities p_i >= 0, sum_i p_i <= 1 (and exp(..) <= 1), so the value errors enter with weight at
# most one: <= d r u max Vabs, plus 2d + 3 roundings of the sum itself, each relative to a partial sum bounded by
# max(|ref|, max Vabs).  With d <= 10, r <= 20 that is (200 + 23) u = 2.5e-14 of the scale per side, 5e-14 between two double
# implementations that order the sums differently: a factor 20 below REL_TOL.  The measured errors are in DESIGN.md (4.8, coverage of
# the Bellman fiber kernels).
EPS_BOUND = (10 * 20 + 2 * 10 + 3) * 2.0 ** -53

PER_WAVE, PAIR, QUAD = 1, 3, 4  # C3SC_VARIANT_*
Case = namedtuple("Case", "family key rp tag name ngrid ranks variant nfib ks kernels opts")

MODEL_OF = {"lqg2d": "LqgNd<2>", "lqg4d": "LqgNd<4>", "lqg6d": "LqgNd<6>", "dubins3d": "Dubins3D", "car7d": "Car7D",
            "cothrust6d": "Cothrust6D", "chain2": "Chain<2>", "chain4": "Chain<4>", "quad10d": "Chain<10>", "rossler3d": "Rossler3D",
            "tprob3d": "Tprob3D", "perch7d": "Perch7D", "scar4d": "Scar4D", "skid5d": "Skid5D"}


def _lqg4d():
    ax = [-1.0, 0.0, 1.0]
    return wl.Workload("lqg4d", wl.MODEL_LQGND, (4.0, 1.0, 1.0), 4, 2, (-2.0,) * 4, (2.0,) * 4, (9,) * 4, wl.uniform_ranks(4, 4), 0.1,
                       (wl.BC_REFLECT,) * 4, [], np.array([(a, b) for a in ax for b in ax], dtype=np.float64))


def _base(name):
    if name in ("chain2", "chain4"):
        return _chain(int(name[-1]))
    if name == "lqg4d":
        return _lqg4d()
    return wl.WORKLOADS[name]()


def with_cands(w, cands):
    return wl.Workload(w.name, w.model, w.params, w.dx, w.du, w.lb, w.ub, w.ngrid, w.ranks, w.discount, w.bc, list(w.obstacles),
                       np.ascontiguousarray(np.asarray(cands, dtype=np.float64).reshape(-1, w.du)))


MAX_CANDS = 6  # a row's candidate list: this many rows of the workload's own list, evenly spread (first and last kept)


def workload(case):
    w = _base(case.name).scaled(ngrid=case.ngrid)
    w.ranks = tuple(case.ranks)
    n = min(w.ncand, case.opts.get("ncand", MAX_CANDS))
    if n < w.ncand:
        w = with_cands(w, w.cands[np.unique(np.round(np.linspace(0, w.ncand - 1, n)).astype(int))])
    return w


def cores(case, w, signed=False):
    """wl.synth_cores (positive, 0.3 .. 0.4), or the signed class synth_cores - 0.35 whose products cancel"""
    cs = wl.synth_cores(w, seed=case.opts.get("seed", 0xC35C))
    return [c - 0.35 for c in cs] if signed else cs


def fibers(w, k, F):
    """F fibers along k: seeded fixed indices; rows 0 / 1 / 2 are all zero, all N - 1, all 1 (faces, wrap-around, first interior)"""
    idx = wl.synth_fibers(w, k, F)
    idx[0, :] = 0
    idx[1, :] = np.array(w.ngrid) - 1
    idx[2, :] = 1
    idx[:, k] = 0
    return idx


def case_id(c):
    key = str(c.key).replace("<", "").replace(">", "")
    return f"{c.family}-{key}-{c.rp}" + (f"-{c.tag}" if c.tag else "")


def _ranks(d, hi):
    """bond ranks with maximum hi, unequal for d >= 3: hi, hi - 2, hi - 1, hi, ... (never below 1)"""
    bonds = [max(1, hi - (2 * i) % 3) for i in range(d - 1)]
    return (1,) + tuple(bonds) + (1,)


def _hi(rp, lower):
    """largest bond rank of a row: below the class where the next smaller class leaves room, else the class"""
    return rp - 1 if rp - 1 > lower else rp


def _mid(d):
    return tuple(sorted({0, d // 2, d - 1}))


GRIDS = {  # NPL = 1 grids: every N <= 64, unequal per dimension
    "dubins3d": (21, 17, 16), "lqg2d": (33, 27), "chain2": (17, 13), "chain4": (9, 7, 8, 6), "scar4d": (12, 11, 10, 9),
    "car7d": (9, 8, 10, 7, 6, 5, 11), "skid5d": (9, 8, 11, 7, 10), "quad10d": (5, 6, 5, 4, 5, 6, 5, 4, 5, 6), "rossler3d": (23, 40, 31),
    "tprob3d": (13, 11, 12), "lqg6d": (7, 8, 9, 6, 5, 7), "lqg4d": (9, 8, 7, 10), "perch7d": (6, 5, 7, 6, 5, 6, 5),
    "cothrust6d": (7, 8, 6, 9, 5, 7),
}
GRIDS2 = {"dubins3d": (128, 70, 65), "lqg2d": (65, 128)}  # NPL = 2 grids: every N in 65 .. 128
DIM_WORKLOAD = {2: "lqg2d", 3: "dubins3d", 4: "scar4d", 5: "skid5d", 6: "lqg6d", 7: "car7d", 10: "quad10d"}

# per-wave classes of each model (C3SC_REG_FPW / _FPW_BOX), `box`: C3SC_REG_FPW_BOX entries (both forms), `npl2`: classes with an
# NPL = 2 registration
FPW_MODELS = [
    # (workload, classes, box, npl2 classes)
    ("dubins3d", (4, 6, 8, 12, 16, 20), False, (4, 6, 8, 12, 16, 20)),
    ("chain2", (4,), False, ()),
    ("chain4", (4,), False, ()),
    ("scar4d", (4, 8, 12, 16, 20), False, ()),
    ("car7d", (4, 10, 12, 16, 20), False, ()),
    ("skid5d", (4, 8, 12, 16, 20), False, ()),
    ("quad10d", (4, 8, 12, 16, 20), False, ()),
    ("rossler3d", (4, 8, 12, 16, 20), True, ()),
    ("tprob3d", (4, 8, 12, 16, 20), True, ()),
    ("lqg2d", (4, 8, 12, 20), True, (4, 8, 12, 20)),
    ("lqg4d", (4,), True, ()),
    ("lqg6d", (4, 8, 12, 16, 20), True, ()),
    ("perch7d", (4, 8, 12, 16, 20), True, ()),
    ("cothrust6d", (4, 8, 10, 12, 16, 20), True, ()),
]
# the control box of each model's example (tests/test_gpu_parity.py::test_continuous_control_box_minimiser) and a small grid whose
# spacing is exact in binary where the box allows
BOX = {
    "lqg2d": ([-1.0], [1.0], 9), "lqg4d": ([-1.0] * 2, [1.0] * 2, 5), "lqg6d": ([-1.0] * 3, [1.0] * 3, 5),
    "rossler3d": ([-4.0], [4.0], 9), "perch7d": ([-2.0 * np.pi], [2.0 * np.pi], 9), "tprob3d": ([-5.0] * 3, [5.0] * 3, 5),
    "cothrust6d": ([-1.5, -0.4, -0.4], [1.5, 0.4, 0.4], 5),
}


def _rows():
    rows = []

    def add(family, key, rp, tag, name, ngrid, ranks, variant, nfib, ks, fmt, **opts):
        kernels = {k: (fmt[k] if isinstance(fmt, dict) else fmt.replace("{k}", str(k))) for k in ks}
        assert len(ranks) == len(ngrid) + 1 and ranks[0] == 1 and ranks[-1] == 1
        rows.append(Case(family, str(key), rp, tag, name, tuple(ngrid), tuple(ranks), variant, nfib, tuple(ks), kernels, opts))

    # ------------------------------------------------------------------------------------------ per-wave, candidate lists
    for name, classes, box, npl2 in FPW_MODELS:
        model, d = MODEL_OF[name], len(GRIDS[name])
        for i, rp in enumerate(classes):
            hi = _hi(rp, classes[i - 1] if i else 0)
            add("fpw", model, rp, "", name, GRIDS[name], _ranks(d, hi), PER_WAVE, 23, _mid(d), f"k_fiber_per_wave<{model},{rp},1>")
            if rp in npl2:  # (at rank 20 the middle dimension's 65 nodes x 401 doubles are never staged)
                add("fpw", model, rp, "npl2", name, GRIDS2[name], _ranks(d, hi), PER_WAVE, 23, _mid(d), f"k_fiber_per_wave<{model},{rp},2>",
                    unstaged=(1,) if (d, rp) == (3, 20) else ())
            if box:
                lb, ub, g = BOX[name]
                add("fpw_box", model, rp, "", name, GRIDS[name], _ranks(d, hi), PER_WAVE, 7, _mid(d), f"k_fiber_per_wave<{model},{rp},1>",
                    lb=lb, ub=ub, grid=g)
                if rp in npl2:
                    add("fpw_box", model, rp, "npl2", name, GRIDS2[name], _ranks(d, hi), PER_WAVE, 7, _mid(d),
                        f"k_fiber_per_wave<{model},{rp},2>", lb=lb, ub=ub, grid=g)
    # the varying core exceeds FPW_MAX_LDS (module docstring): the STAGED = false instantiation, one row per rank class it reaches.
    # last_kernel() reports the same string for both instantiations, so that these rows take the L2-read path is asserted on the
    # CPU side only, by the restatement of fpw_geometry in tests/test_fiber_kernel_cases.py (launch); the device run checks values.
    add("fpw", "Scar4D", 20, "unstaged", "scar4d", (12, 60, 10, 9), _ranks(4, 19), PER_WAVE, 23, (1,), "k_fiber_per_wave<Scar4D,20,1>", unstaged=(1,))
    add("fpw", "Dubins3D", 16, "npl2-unstaged", "dubins3d", (65, 128, 70), _ranks(3, 15), PER_WAVE, 23, (1,), "k_fiber_per_wave<Dubins3D,16,2>", unstaged=(1,))

    # ------------------------------------------------------------------------------------------------------------ pair
    for name, classes, nc in (("car7d", (4, 10), 0), ("lqg6d", (4, 8), 0), ("dubins3d", (4, 6, 8), 0), ("rossler3d", (4, 8), 0),
                              ("scar4d", (4, 8), 0), ("lqg2d", (4,), 0), ("cothrust6d", (10,), 64)):
        model, d = MODEL_OF[name], len(GRIDS[name])
        for i, rp in enumerate(classes):
            hi = _hi(rp, classes[i - 1] if i else (8 if name == "cothrust6d" else 0))
            opts = dict(ncand=nc) if nc else {}  # cothrust6d keeps its 64 candidates: the longest list the pair kernel serves
            add("fpp", model, rp, "", name, GRIDS[name], _ranks(d, hi), PAIR, 150, range(d), f"k_fiber_pair<{model},{rp},K={{k}}>", **opts)
    add("fpp", "Dubins3D", 6, "n128", "dubins3d", (128, 65, 101), _ranks(3, 5), PAIR, 150, range(3), "k_fiber_pair<Dubins3D,6,K={k}>")

    # ------------------------------------------------------------------------------------------------------------ quad
    for name, classes, nwv in (("car7d", (4, 12), 8), ("quad10d", (4,), 8), ("scar4d", (8, 20), 8), ("lqg6d", (8,), 8)):
        model, d = MODEL_OF[name], len(GRIDS[name])
        for i, rp in enumerate(classes):
            hi = _hi(rp, classes[i - 1] if i else 0)
            add("fq", model, rp, "", name, GRIDS[name], _ranks(d, hi), QUAD, 2 * 16 * nwv + 14, range(d), f"k_fiber_quad<{model},{rp},K={{k}}>")
    # duo kernels (tile 8 NWV = 64 fibers); Skid5D has no duo form at k = 2: the quad kernel answers there
    add("fqd", "Chain<10>", 16, "", "quad10d", GRIDS["quad10d"], _ranks(10, 15), QUAD, 150, range(10), "k_fiber_quad_duo<Chain<10>,16,K={k}>")
    add("fqd", "Perch7D", 16, "", "perch7d", GRIDS["perch7d"], _ranks(7, 15), QUAD, 150, range(7), "k_fiber_quad_duo<Perch7D,16,K={k}>")
    add("fqd", "Skid5D", 16, "", "skid5d", GRIDS["skid5d"], _ranks(5, 15), QUAD, 270, range(5),
        {k: ("k_fiber_quad<Skid5D,16,K=2>" if k == 2 else f"k_fiber_quad_duo<Skid5D,16,K={k}>") for k in range(5)})
    # the quad kernels behind them, after the duo launcher declined (module docstring); quad tiles: 16 NWV fibers
    add("fq", "Skid5D", 16, "behind-duo", "skid5d", (5, 6, 68, 5, 6), _ranks(5, 15), QUAD, 270, range(5), "k_fiber_quad<Skid5D,16,K={k}>")
    add("fq", "Perch7D", 16, "behind-duo", "perch7d", (6, 5, 7, 40, 5, 6, 5), _ranks(7, 15), QUAD, 142, (0, 1, 2, 4, 5, 6), "k_fiber_quad<Perch7D,16,K={k}>")
    add("fq", "Perch7D", 16, "behind-duo-k3", "perch7d", (6, 5, 40, 6, 5, 6, 5), _ranks(7, 15), QUAD, 142, (3,), "k_fiber_quad<Perch7D,16,K={k}>")
    add("fq", "Chain<10>", 16, "behind-duo", "quad10d", (5, 6, 30, 4, 5, 6, 5, 4, 5, 6), _ranks(10, 15), QUAD, 142,
        (0, 1, 3, 4, 5, 6, 7, 8, 9), "k_fiber_quad<Chain<10>,16,K={k}>")
    add("fq", "Chain<10>", 16, "behind-duo-k2", "quad10d", (5, 6, 5, 4, 5, 30, 5, 4, 5, 6), _ranks(10, 15), QUAD, 142, (2,), "k_fiber_quad<Chain<10>,16,K={k}>")

    # ------------------------------------------------------------------------------------------------- TableModel<D>
    # the context's model is the workload's own (its classes give the padded rank); the tables come from the oracle's callbacks
    for d, classes, npl2 in ((2, (4, 8, 12, 20), True), (3, (4, 6, 8, 12, 16), True), (4, (4, 8, 20), False), (6, (4, 8), False),
                             (7, (4, 10), False), (10, (4, 16), False)):
        name = DIM_WORKLOAD[d]
        own = sorted({c.rp for c in rows if c.family == "fpw" and c.name == name})
        for rp in classes:
            hi = _hi(rp, max([c for c in own if c < rp], default=0))
            add("table", f"TableModel<{d}>", rp, "", name, GRIDS[name], _ranks(d, hi), 0, 7, _mid(d), f"k_fiber_per_wave<TableModel<{d}>,{rp},1>", ncand=4)
            if npl2:
                add("table", f"TableModel<{d}>", rp, "npl2", name, GRIDS2[name], _ranks(d, hi), 0, 7, _mid(d),
                    f"k_fiber_per_wave<TableModel<{d}>,{rp},2>", ncand=3)

    # ------------------------------------------------------------------------------------------------ on-grid stencil
    for d, classes, npl2 in ((2, (4, 8, 12, 20), True), (3, (4, 6, 8, 12, 16, 20), True), (4, (4, 8, 12, 16, 20), False),
                             (5, (4, 8, 12, 16, 20), False), (6, (4, 8, 12, 16, 20), False), (7, (4, 10, 12, 16, 20), False),
                             (10, (4, 8, 12, 16, 20), False)):
        name = DIM_WORKLOAD[d]
        for i, rp in enumerate(classes):
            hi = _hi(rp, classes[i - 1] if i else 0)
            add("stencil", d, rp, "", name, GRIDS[name], _ranks(d, hi), 0, 23, _mid(d), f"k_fiber_per_wave<stencil,{d},{rp},1>")
            if npl2:
                add("stencil", d, rp, "npl2", name, GRIDS2[name], _ranks(d, hi), 0, 23, _mid(d), f"k_fiber_per_wave<stencil,{d},{rp},2>",
                    unstaged=(1,) if (d, rp) == (3, 20) else ())
    add("stencil", 3, 20, "unstaged", "dubins3d", (21, 60, 16), _ranks(3, 19), 0, 23, (1,), "k_fiber_per_wave<stencil,3,20,1>", unstaged=(1,))
    return rows


CASES = _rows()
LIST_FAMILIES = ("fpw", "fpp", "fq", "fqd")  # rows with a candidate list that the minimising and the FORCED form run on
TILE = {"fpw": 4, "fpw_box": 4, "table": 4, "stencil": 4, "fpp": 64}  # fibers per tile; quad: 16 NWV, duo: 8 NWV (NWV = 8 or 4)


# ------------------------------------------------------------------------------------------------------------ reference
def q_table(oracle, w, cs, k, idx):
    """Q[fiber, node, c]: the oracle's backup with candidate c alone (one oracle run per candidate on a workload whose candidate
    list is that single control), and the flags of each run.  Q.min(-1) is the Bellman backup; a policy's value is a gather."""
    F, N = len(idx), w.ngrid[k]
    Q = np.empty((F, N, w.ncand))
    flags = np.empty((w.ncand, F, N), dtype=np.int32)
    for c in range(w.ncand):
        P = oracle.Problem(with_cands(w, w.cands[c:c + 1]), cs)
        Q[:, :, c], _, flags[c] = P.bellman_fibers(k, idx)
    return Q, flags


def vabs(oracle, w, cs, k, idx):
    """max over the batch of the oracle's stencil of the same fibers on |cores| (the signed class's scale)"""
    P = oracle.Problem(w, [np.abs(c) for c in cs])
    v, _ = P.stencil_fibers(k, idx)
    return float(np.abs(v).max())


def scale_of(oracle, w, cs, k, idx, ref, signed):
    s = float(np.abs(ref).max())
    return max(s, vabs(oracle, w, cs, k, idx)) if signed else s


def model_tables(oracle, w, k, idx):
    """(tables (F, N, U, 2d+1), costs2 (F, N, 2)) of c3sc_hip_bellman_fibers_tables from the oracle's model callbacks"""
    import ctypes as C

    L = oracle.lib()
    dp = oracle.dp
    xg = w.xgrid()
    d, N, S = w.dx, w.ngrid[k], 2 * w.dx + 1
    prm = np.zeros(8)
    prm[:len(w.params)] = w.params
    tables = np.zeros((len(idx), N, w.ncand, S))
    costs2 = np.zeros((len(idx), N, 2))
    b, sg, st = np.zeros(d), np.zeros(d), C.c_double(0)
    for f, row in enumerate(idx):
        for j in range(N):
            x = np.array([xg[m][j] if m == k else xg[m][row[m]] for m in range(d)])
            bc, oc = C.c_double(0), C.c_double(0)
            L.orc_model_boundcost(w.model, dp(prm), dp(x), C.byref(bc))
            L.orc_model_obscost(w.model, dp(prm), dp(x), C.byref(oc))
            costs2[f, j] = (bc.value, oc.value)
            for c in range(w.ncand):
                u = np.ascontiguousarray(w.cands[c])
                L.orc_model_drift(w.model, dp(prm), dp(x), dp(u), dp(b))
                L.orc_model_diff_diag(w.model, dp(prm), dp(x), dp(u), dp(sg))
                L.orc_model_stage(w.model, dp(prm), dp(x), dp(u), C.byref(st))
                tables[f, j, c, :d] = b
                tables[f, j, c, d:2 * d] = sg
                tables[f, j, c, 2 * d] = st.value
    return tables, costs2


def box_grid(lb, ub, G):
    """the tensor grid of controls the box minimiser scans (kernel_common.hpp): G points per control, the first control fastest"""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    du = len(lb)
    dl = (ub - lb) / (G - 1)
    out = np.empty((G ** du, du))
    for c in range(G ** du):
        rem = c
        for i in range(du):
            gi = rem % G
            rem //= G
            out[c, i] = ub[i] if gi == G - 1 else lb[i] + gi * dl[i]
    return out
