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
runs every row on a device, at the discount of its example and at the discounts of the regimes defined below (one per scan body of
node_backup), and the LqgNd / Chain rows on inputs with stationary candidates.

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
# implementations that order the sums differently: a factor 20 below REL_TOL.  The discount factor adds its own term when beta is
# the regime's and not the example's: the device forms exp(x), x = -beta dt, by a polynomial (exp_tiny: truncation below
# 2^-56; exp_small: degree 7 below 2^-7) or by the device libm, the oracle by the host libm, each within an ulp or two of exp(x),
# i.e. 4 u between them; x itself carries the two roundings of dt = h2 / Q and of the product, 2 u |x|, which exp turns into
# 2 u |x| e^x <= 2 u / e < u of the factor.  The factor multiplies the cost-to-go, which the scale bounds, so the term is 5 u of the
# scale.  The measured errors are in DESIGN.md (4.8, coverage of the Bellman fiber kernels).
EPS_BOUND = (10 * 20 + 2 * 10 + 3 + 5) * 2.0 ** -53

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
    want = case.opts.get("ncand", MAX_CANDS)
    if want > w.ncand and case.opts.get("spread"):  # a list longer than the model's own: evenly spaced inside its control range
        lo, hi = w.cands.min(axis=0), w.cands.max(axis=0)
        return with_cands(w, lo + (hi - lo) * np.linspace(0.0, 1.0, want)[:, None])
    n = min(w.ncand, want)
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
    # classes that only one model of the dimension has -- Cothrust6D's 10 (LqgNd<6> has none), Perch7D's 8 (Car7D has none): found
    # missing by the random sweep (tests/random_cases.py: case('cothrust6d', 0), bond ranks 9 and 10, and case('perch7d', 18), bond
    # ranks 5 .. 8, whose stencil launches were refused before the registrations)
    add("stencil", 6, 10, "", "cothrust6d", GRIDS["cothrust6d"], _ranks(6, 9), 0, 23, _mid(6), "k_fiber_per_wave<stencil,6,10,1>")
    add("stencil", 7, 8, "", "perch7d", GRIDS["perch7d"], _ranks(7, 7), 0, 23, _mid(7), "k_fiber_per_wave<stencil,7,8,1>")
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


# ------------------------------------------------------------------------------------------------------- discount regimes
# node_backup (c3sc_amd/csrc/kernel_common.hpp) compiles several candidate scans into every kernel and picks one per node, by wave
# votes on the run-time discount beta:
#   beta == 0                            the fraction scan (cross-multiplied comparison, one division for the winner)
#   SPLIT kernels (per-wave, pair)       q0ok = no lane with Q0 < 1e-14;  x0 = beta h2 / Q0 per lane
#     q0ok, every x0 < 2^-10             E0        exp_tiny (degree 4)
#     q0ok, every x0 < 2^-7              E1        exp_small (degree 7)
#     q0ok otherwise                     E2        exp_discount: exp_small where every lane's beta dt_c < 2^-7, else libm exp
#     not q0ok                           E2+CHECK  the same with the stationary test
#   !SPLIT kernels (quad, duo)           E3        one body with the stationary test; the same three forms chosen inside, all_tiny and
#                                                  all_small without q0ok (a lane with Q0 = 0 fails both votes)
# Q0 is the sum of the upwind rates of the dimensions outside the model's control-dependent set, restated here from models.hpp
# (tests/test_fiber_kernel_cases.py holds the table to every UDEP_MASK line); Chain<DIM> and LqgNd<DIM> are formulas in DIM.
UDEP = {"Dubins3D": (2,), "Scar4D": (2, 3), "Car7D": (5, 6), "Rossler3D": (1,), "Tprob3D": (0, 1, 2), "Perch7D": (3, 4, 5, 6),
        "Skid5D": (3, 4), "Cothrust6D": (3, 4, 5), "TableModel": (), "NoModel": (),
        "LqgNd": lambda dim: tuple(range(1, dim, 2)),  # odd dimensions are driven by a control
        "Chain": lambda dim: (dim - 1,)}


def udep(mtype):
    """the control-dependent dimensions of a model type string such as "Car7D" or "LqgNd<6>" """
    base, _, arg = mtype.partition("<")
    v = UDEP[base]
    return tuple(v(int(arg.rstrip(">")))) if callable(v) else v


REGIMES = ("zero", "tiny", "small", "libm", "mixed", "vote")
SPLIT = {"fpw": True, "fpp": True, "fq": False, "fqd": False}  # node_backup's SPLIT argument in the family's kernel
# the bodies a SPLIT setting compiles: name, or name + "+CHECK" where the stationary test is compiled in and a stationary lane
# (SPLIT) or candidate (fraction) is in the batch.  The fraction scan and E3 always carry the test.
BODIES = {True: ("fraction", "E0", "E1", "E2-poly", "E2-libm", "E2-poly+CHECK", "E2-libm+CHECK"),
          False: ("fraction", "E3-tiny", "E3-small", "E3-poly", "E3-libm")}
# body -> (families, why no row of theirs reaches it).  Empty: every family reaches every body its SPLIT setting compiles.
UNREACHABLE_BODIES = {}

NodePieces = namedtuple("NodePieces", "dt r0 prob stage h2")


def node_pieces(oracle, w, k, idx, mtype=None):
    """Per node of every fiber (absorbed nodes included: their lanes take part in the wave votes) and per candidate, from the
    oracle's pieces: orc_model_drift / _diff_diag / _stage and transition_assemble.
      dt[f, j, c]   = h2 / Q_c, nan where transition_assemble returns 1 (Q_c < 1e-14: a stationary candidate)
      r0[f, j]      = h2 / Q0 from transition_assemble on the drift and diffusion with the control-dependent dimensions zeroed,
                      inf where that returns 1 (Q0 < 1e-14)
      prob[f, j, c] = the 2d + 1 transition probabilities, stage[f, j, c] the stage cost"""
    import ctypes as C

    L, dp = oracle.lib(), oracle.dp
    mtype = mtype or MODEL_OF[w.name]
    P = oracle.Problem(w)
    h2, tv = P.h2(), P.tvec()
    xg = w.xgrid()
    d, N, S, F = w.dx, w.ngrid[k], 2 * w.dx + 1, len(idx)
    keep = np.array([m not in udep(mtype) for m in range(d)], dtype=np.float64)
    prm = np.zeros(8)
    prm[:len(w.params)] = w.params
    cands = np.ascontiguousarray(w.cands, dtype=np.float64)
    dt = np.full((F, N, w.ncand), np.nan)
    r0 = np.full((F, N), np.inf)
    prob = np.full((F, N, w.ncand, S), np.nan)
    stage = np.zeros((F, N, w.ncand))
    x, b, sg, b0, diff, p1, st, dtv = np.zeros(d), np.zeros(d), np.zeros(d), np.zeros(d), np.zeros(d * d), np.zeros(S), C.c_double(0), C.c_double(0)
    diag = diff[::d + 1]  # a view of the diagonal
    args = (C.c_size_t(d), C.c_size_t(w.du), C.c_size_t(d), C.c_double(h2), dp(tv))
    pprm, px, pb, psg, pb0, pdiff, pp1, pst, pdt = dp(prm), dp(x), dp(b), dp(sg), dp(b0), dp(diff), dp(p1), C.byref(st), C.byref(dtv)
    for f, row in enumerate(idx):
        for m in range(d):
            x[m] = xg[m][row[m]]
        for j in range(N):
            x[k] = xg[k][j]
            for c in range(w.ncand):
                pu = dp(cands[c])
                L.orc_model_drift(w.model, pprm, px, pu, pb)
                L.orc_model_diff_diag(w.model, pprm, px, pu, psg)
                L.orc_model_stage(w.model, pprm, px, pu, pst)
                stage[f, j, c] = st.value
                diag[:] = sg
                if L.orc_transition_assemble(*args, pb, None, pdiff, None, pp1, None, pdt, None, None) == 0:
                    dt[f, j, c] = dtv.value
                    prob[f, j, c] = p1
                if c == 0:  # the control-independent share: the same call on the other dimensions alone
                    b0[:] = b * keep
                    diag[:] = sg * keep
                    if L.orc_transition_assemble(*args, pb0, None, pdiff, None, pp1, None, pdt, None, None) == 0:
                        r0[f, j] = dtv.value
    return NodePieces(dt, r0, prob, stage, h2)


_PIECES = {}


def row_pieces(oracle, case, w=None, fib=None):
    """{k: (dt, r0)} of a row's batches (memoised per row, candidate list and batch: the regimes of a row share them)"""
    w = w or workload(case)
    fib = fib or fibers
    key = (case_id(case), w.ngrid, w.params, w.cands.tobytes(), fib.__name__)
    if key not in _PIECES:
        mtype = MODEL_OF[case.name]
        out = {}
        for k in case.ks:
            p = node_pieces(oracle, w, k, fib(w, k, case.nfib), mtype)
            out[k] = (p.dt, p.r0)
        _PIECES[key] = out
    return _PIECES[key]


def regime_betas(oracle, case, w=None, fib=None):
    """The discounts of a row, from the oracle's own dt and r0 over all of the row's k (never a literal).  R is r0 where
    it is finite and the node's largest dt where it is not; the factors of two keep every vote clear of rounding.
      zero   0                     the fraction scan
      tiny   2^-11 / max R         beta r0 <= 2^-11 < 2^-10 on every lane: all_tiny wherever q0ok holds
      small  2^-8 / max R          beta r0 <= 2^-8 < 2^-7 on every lane: all_small; = 2^-8 > 2^-10 on the maximising node
      libm   2^-6 / min dt         beta dt_c >= 2^-6 > 2^-7 for every candidate of every lane (and r0 >= dt_c): exp() runs
      mixed  2^-7 / median dt      the batch straddles 2^-7
      vote   2^-7 / sqrt(max R m)  m = min over the candidates of the largest dt_c of the batch (m <= max R: a candidate only adds
                                   rates).  Where m < max R the lane of the largest r0 fails all_small while the candidate that
                                   attains m passes the per-candidate vote in every wave: exp_discount's polynomial arm"""
    pc = row_pieces(oracle, case, w, fib)
    dts = np.concatenate([dt[np.isfinite(dt)] for dt, _ in pc.values()])
    R = np.concatenate([np.where(np.isfinite(r0), r0, np.nanmax(np.where(np.isfinite(dt), dt, -np.inf), axis=-1)).ravel()
                        for dt, r0 in pc.values()])
    assert np.isfinite(R).all() and (dts > 0).all()
    m = min(max(np.nanmax(dt[..., c]) for dt, _ in pc.values()) for c in range(next(iter(pc.values()))[0].shape[-1]))
    assert m <= R.max()
    return {"zero": 0.0, "tiny": 2.0 ** -11 / R.max(), "small": 2.0 ** -8 / R.max(), "libm": 2.0 ** -6 / dts.min(),
            "mixed": 2.0 ** -7 / float(np.median(dts)), "vote": 2.0 ** -7 / float(np.sqrt(R.max() * m))}


def bodies_of(split, dt, r0, beta):
    """The set of scan bodies a batch with these dt[f, j, c] and r0[f, j] reaches at discount beta, from batch-wide inequalities
    alone (which lanes share a wave is not modelled).  A body is listed when some wave must take it whatever its lanes are:
      the wave that holds a lane with r0 = inf takes the CHECK body (SPLIT) / fails all_tiny and all_small (E3);
      where every lane of the batch passes a vote, every wave passes it; the wave that holds the lane with the largest r0 fails
      every vote that lane fails; a candidate whose beta dt_c is below 2^-7 on every lane of the batch passes the per-candidate
      vote in every wave, one that is at or above it on every lane fails it in every wave.
    Bodies that only some arrangement of lanes would reach are left out."""
    valid = np.isfinite(dt)
    if beta == 0.0:
        return {"fraction"}
    fin = np.isfinite(r0)
    x0 = beta * np.where(fin, r0, np.inf)
    xc = beta * np.where(valid, dt, np.nan)
    cmax = np.nanmax(np.where(valid, xc, -np.inf).reshape(-1, dt.shape[-1]), axis=0)  # per candidate, over the batch
    cmin = np.nanmin(np.where(valid, xc, np.inf).reshape(-1, dt.shape[-1]), axis=0)
    vote = set()  # what exp_discount does in a wave that reaches it
    if (cmax < 2.0 ** -7).any():
        vote.add("poly")
    if (cmin >= 2.0 ** -7).any():
        vote.add("libm")
    out = set()
    if split:
        if not fin.all():
            out |= {f"E2-{v}+CHECK" for v in vote}
        if fin.all():  # every wave has q0ok
            if (x0 < 2.0 ** -10).all():
                out.add("E0")
            elif (x0 < 2.0 ** -7).all():
                out.add("E1")  # the wave of the largest r0; others may take E0
            else:
                out |= {f"E2-{v}" for v in vote}  # the wave of the largest r0
        return out
    if (x0 < 2.0 ** -10).all():
        out.add("E3-tiny")
    elif (x0 < 2.0 ** -7).all():
        out.add("E3-small")
    else:
        out |= {f"E3-{v}" for v in vote}
    return out


def scan_bodies(oracle, case, k, beta, w=None, fib=None):
    dt, r0 = row_pieces(oracle, case, w, fib)[k]
    return bodies_of(SPLIT[case.family], dt, r0, beta)


# ------------------------------------------------------------------------------------------- the skip-and-flag path
# The oracle fails a whole fiber on a stationary candidate (rc 101), so Q[f, j, c] is built from its pieces: the stencil of
# P.stencil_fibers, node_pieces above and bellmanrhs; an invalid candidate is nan.  Inputs: LqgNd and Chain with the diffusion
# switched off (sigma = 0 in both parameters), on a grid with a node at 0 on every axis that is another equation's drift, and a
# candidate list that holds u = 0: there every rate vanishes.  Rossler3D cannot: its third equation's drift 0.1 + x2 (x0 - 14) and
# its first, -x1 - x2, vanish together only off the grid nodes of its box, and its diffusion parameters are shared with them.
STATIONARY_ROWS = (("fpw", "LqgNd<2>", 4, ""), ("fpw", "LqgNd<4>", 4, ""), ("fpw", "LqgNd<6>", 8, ""), ("fpw", "Chain<2>", 4, ""),
                   ("fpw", "Chain<4>", 4, ""), ("fpp", "LqgNd<2>", 4, ""), ("fpp", "LqgNd<6>", 4, ""), ("fpp", "LqgNd<6>", 8, ""),
                   ("fq", "LqgNd<6>", 8, ""))


STATIONARY_REGIMES = ("zero", "tiny", "libm")  # tiny: the polynomial arm of the CHECK body on the pair kernels too


def stationary_cases():
    return [c for c in CASES if (c.family, c.key, c.rp, c.tag) in STATIONARY_ROWS]


def stationary_workload(case):
    """the row's workload without diffusion, every N made odd (a node at 0: the boxes are symmetric), u = 0 as the candidate list's
    third entry"""
    w = workload(case)
    ngrid = tuple(n | 1 for n in w.ngrid)
    cands = w.cands[(w.cands != 0.0).any(axis=1)]  # u = 0 sits at position 2, once
    cands = np.insert(cands, 2, 0.0, axis=0) if len(cands) < w.ncand else np.concatenate([cands[:2], cands[:1] * 0.0, cands[3:]])
    assert len({tuple(c) for c in cands}) == len(cands)
    params = (w.params[0], 0.0, 0.0) + tuple(w.params[3:])
    w2 = wl.Workload(w.name, w.model, params, w.dx, w.du, w.lb, w.ub, ngrid, w.ranks, w.discount, w.bc, [], cands)
    for g, n in zip(w2.xgrid(), ngrid):
        assert g[n // 2] == 0.0
    return w2


def fibers_through(w, k, F):
    """F fibers along k, every fixed index at the centre node on a third of them (rows 0, 3, 6, ..: the stationary nodes lie there)"""
    idx = fibers(w, k, F)
    idx[::3] = np.array(w.ngrid) // 2
    idx[:, k] = 0
    return idx


def fibers_clear(w, k, F):
    """F fibers along k with no fixed index at its centre node"""
    idx = fibers(w, k, F)
    mid = np.array(w.ngrid) // 2
    idx = np.where(idx == mid, idx + 1, idx).astype(idx.dtype)
    idx[:, k] = 0
    return idx


def zero_axes(mtype):
    """the coordinates that must vanish for u = 0 to be stationary without diffusion: another equation's drift"""
    d = int(mtype.partition("<")[2].rstrip(">"))
    return tuple(range(1, d, 2)) if mtype.startswith("LqgNd") else tuple(range(1, d))


def q_pieces(oracle, w, cs, k, idx, mtype):
    """(Q[f, j, c], flags, status): bellmanrhs on the oracle's stencil and node_pieces; nan where the candidate is stationary;
    absorbed nodes carry the model's cost in every column.  status: a live node has an invalid candidate."""
    import ctypes as C

    L, dp = oracle.lib(), oracle.dp
    P = oracle.Problem(w, cs)
    V, ab = P.stencil_fibers(k, idx)
    p = node_pieces(oracle, w, k, idx, mtype)
    F, N, U = p.dt.shape
    Q = np.full((F, N, U), np.nan)
    xg = w.xgrid()
    prm = np.zeros(8)
    prm[:len(w.params)] = w.params
    d = w.dx
    for f in range(F):
        for j in range(N):
            if ab[f, j] != 0:
                x = np.array([xg[m][j] if m == k else xg[m][idx[f][m]] for m in range(d)])
                v = C.c_double(0)
                (L.orc_model_boundcost if ab[f, j] == 1 else L.orc_model_obscost)(w.model, dp(prm), dp(x), C.byref(v))
                Q[f, j] = v.value
                continue
            for c in range(U):
                if np.isfinite(p.dt[f, j, c]):
                    Q[f, j, c], _ = oracle.bellmanrhs(d, w.du, p.stage[f, j, c], w.discount, p.prob[f, j, c], p.dt[f, j, c], V[f, j])
    live = ab == 0
    return Q, ab, bool((np.isnan(Q).any(axis=-1) & live).any())
