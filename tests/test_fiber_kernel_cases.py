"""CPU side of the Bellman fiber kernel tests (tests/test_gpu_fiber_kernels.py): the case table covers the registry, every row
selects the kernel it claims under a restatement of pick_rp / find_kernel and of the launchers' LDS arithmetic, and the
per-candidate table Q that the GPU tests compare against is pinned to the oracle.  Nothing here needs a GPU."""
import glob
import os
import re
from collections import Counter, namedtuple

import numpy as np
import pytest

import fiber_kernel_cases as T
from c3sc_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")

AUTO, PER_WAVE, PAIR, QUAD = 0, 1, 3, 4
Entry = namedtuple("Entry", "kind model mtype d rp npl variant max_n k nwv dbuf name file order")
REG_KINDS = ("C3SC_REG_FPW_BOX", "C3SC_REG_FPW", "C3SC_REG_FPP1", "C3SC_REG_FQ1", "C3SC_REG_FQD", "REG_FQD_SB", "C3SC_REG_STENCIL")
EXPECTED = {"C3SC_REG_FPW": 61, "C3SC_REG_FPW_BOX": 35, "C3SC_REG_FPP1": 57, "C3SC_REG_FQ1": 60, "C3SC_REG_FQD": 17, "REG_FQD_SB": 4,
            "C3SC_REG_STENCIL": 47}
HELPERS = {"REG7P", "REG7Q", "REG10Q", "REG10QD", "REG4Q", "REG6Q", "REG3P", "REG3R", "REG4P", "REG6P"}


def _dim_of(mtype):
    m = re.search(r"<(\d+)>$", mtype) or re.search(r"(\d+)D$", mtype)
    return int(m.group(1))


def _entry(kind, args, file, order):
    a = [t.strip() for t in args.split(",")]
    if kind == "C3SC_REG_STENCIL":  # (DIM, RP, NPL)
        d, rp, npl = int(a[0]), int(a[1]), int(a[2])
        return Entry(kind, "0", "stencil", d, rp, npl, PER_WAVE, 64 * npl, -1, 0, False, f"k_fiber_per_wave<stencil,{d},{rp},{npl}>", file, order)
    if kind in ("C3SC_REG_FPW", "C3SC_REG_FPW_BOX"):  # (MODEL_ID, RP, NPL, Model)
        mtype, rp, npl = ",".join(a[3:]), int(a[1]), int(a[2])
        return Entry(kind, a[0], mtype, _dim_of(mtype), rp, npl, PER_WAVE, 64 * npl, -1, 0, False, f"k_fiber_per_wave<{mtype},{rp},{npl}>", file, order)
    if kind == "C3SC_REG_FPP1":  # (MODEL_ID, RP, K, Model)
        mtype, rp, k = ",".join(a[3:]), int(a[1]), int(a[2])
        return Entry(kind, a[0], mtype, _dim_of(mtype), rp, 0, PAIR, 128, k, 0, False, f"k_fiber_pair<{mtype},{rp},K={k}>", file, order)
    mtype, rp, k, nwv = ",".join(a[4:]), int(a[1]), int(a[2]), int(a[3])  # (MODEL_ID, RP, K, NWV, Model)
    if kind == "C3SC_REG_FQ1":
        return Entry(kind, a[0], mtype, _dim_of(mtype), rp, 0, QUAD, 128, k, nwv, False, f"k_fiber_quad<{mtype},{rp},K={k}>", file, order)
    return Entry(kind, a[0], mtype, _dim_of(mtype), rp, 0, QUAD, 128, k, nwv, kind == "C3SC_REG_FQD",
                 f"k_fiber_quad_duo<{mtype},{rp},K={k}>", file, order)


_DEFINE = re.compile(r"^#define\s+(\w+)\(([^)]*)\)((?:.*\\\n)*.*)\n", re.M)
_CALL = re.compile(r"\b(" + "|".join(REG_KINDS) + r"|REG\w+)\(([^()]*)\)")


def registrations():
    """every Bellman fiber registration of inst_*.hip in registration order per file, read as text: the C3SC_REG_* lines and the
    lines of the file-local helper macros (REG7P .. REG6P), expanded; REG_FQD_SB is the file-local single-buffer duo registration"""
    out = []
    files = sorted(f for f in glob.glob(os.path.join(CSRC, "inst_*.hip")) if "rollout" not in os.path.basename(f))
    assert files
    seen_helpers = set()
    for f in files:
        src = open(f).read()
        helpers = {}
        for name, params, body in _DEFINE.findall(src):
            if name == "REG_FQD_SB":
                assert "launch_fq_duo<__VA_ARGS__, RP, K, NWV, false>" in body and '"k_fiber_quad_duo<"' in body
            elif name.startswith("REG"):
                helpers[name] = ([p.strip() for p in params.split(",")], body)
        seen_helpers |= set(helpers)
        text = _DEFINE.sub("\n", src)
        text = re.sub(r"//.*", "", text)
        for name, args in _CALL.findall(text):
            if name in helpers:
                params, body = helpers[name]
                vals = [t.strip() for t in args.split(",")]
                assert len(vals) == len(params), (f, name, args)
                for p, v in zip(params, vals):
                    body = re.sub(r"\b%s\b" % p, v, body)
                for kind, a2 in _CALL.findall(body):
                    assert kind in REG_KINDS, (f, name, kind)
                    out.append(_entry(kind, a2, os.path.basename(f), len(out)))
            else:
                assert name in REG_KINDS, (f, name)
                out.append(_entry(name, args, os.path.basename(f), len(out)))
    assert seen_helpers == HELPERS, seen_helpers ^ HELPERS
    return out


REG = registrations()


def test_registry_parse_counts():
    """the expansion of the C3SC_REG_* lines, helper macros included: 281 registrations with distinct kernel names"""
    assert dict(Counter(e.kind for e in REG)) == EXPECTED
    assert len(REG) == 281
    names = [e.name for e in REG]
    assert len(names) == len(set(names)), [n for n, c in Counter(names).items() if c > 1]
    # ties that first-registered-wins decides (same model, dimension, rank, variant, nodes per lane, k) sit in one file: the order
    # of static initialisers across translation units does not matter
    groups = {}
    for e in REG:
        groups.setdefault((e.model, e.d, e.rp, e.variant, e.npl, e.k), []).append(e)
    for g in groups.values():
        assert len({e.file for e in g}) == 1, g


def test_every_model_class_has_a_stencil_kernel():
    """stencil_fibers looks the model-independent kernel up at the padded rank of the upload, which pick_rp takes from the
    MODEL's classes: every (dimension, padded rank, nodes per lane) some model has a Bellman kernel at has a stencil kernel too
    (Cothrust6D's class 10 and Perch7D's class 8 had none: the random sweep's stencil launches were refused there)"""
    stencil = {(e.d, e.rp, e.npl) for e in REG if e.kind == "C3SC_REG_STENCIL"}
    for e in REG:
        if e.kind in ("C3SC_REG_FPW", "C3SC_REG_FPW_BOX") and not e.mtype.startswith("TableModel"):
            assert (e.d, e.rp, e.npl) in stencil, e.name
        elif e.kind != "C3SC_REG_STENCIL" and not e.mtype.startswith("TableModel"):
            assert (e.d, e.rp, 1) in stencil, e.name


def test_case_table_covers_the_registry():
    """registered == table + UNREACHABLE: every registration is named by a row for some k (the C3SC_REG_FPW_BOX entries by a row of
    both forms), no row names a kernel that is not registered, no two rows share an id"""
    ids = [T.case_id(c) for c in T.CASES]
    assert len(ids) == len(set(ids)), [i for i, n in Counter(ids).items() if n > 1]
    registered = {e.name for e in REG}
    unreachable = set(T.UNREACHABLE)
    claimed = {n for c in T.CASES for n in c.kernels.values()}
    assert not (claimed & unreachable)
    missing = registered - claimed - unreachable
    stale = (claimed | unreachable) - registered
    assert not missing, f"registered and neither in tests/fiber_kernel_cases.py nor on its UNREACHABLE list: {sorted(missing)}"
    assert not stale, f"in the case table or on UNREACHABLE and not registered: {sorted(stale)}"
    for why in T.UNREACHABLE.values():
        assert isinstance(why, str) and why.strip()
    by_family = lambda *fam: {n for c in T.CASES if c.family in fam for n in c.kernels.values()}
    kind = lambda *k: {e.name for e in REG if e.kind in k}
    table_names = {e.name for e in REG if e.mtype.startswith("TableModel")}
    assert by_family("fpw_box") | unreachable >= kind("C3SC_REG_FPW_BOX") and by_family("fpw_box") <= kind("C3SC_REG_FPW_BOX")
    assert by_family("fpw") | unreachable >= kind("C3SC_REG_FPW", "C3SC_REG_FPW_BOX") - table_names
    assert by_family("table") | unreachable >= table_names and by_family("table") <= table_names
    assert by_family("stencil") | unreachable >= kind("C3SC_REG_STENCIL")
    assert by_family("fpp") | unreachable >= kind("C3SC_REG_FPP1")
    assert by_family("fq", "fqd") | unreachable >= kind("C3SC_REG_FQ1", "C3SC_REG_FQD", "REG_FQD_SB")
    assert by_family("fqd") | unreachable >= kind("C3SC_REG_FQD", "REG_FQD_SB")
    # the quad kernels behind a duo kernel are named by a row in which the duo launcher declined
    behind = {e.name for e in REG if e.kind == "C3SC_REG_FQ1" and any(o.variant == QUAD and o.kind != "C3SC_REG_FQ1" and
                                                                      (o.model, o.d, o.rp, o.k) == (e.model, e.d, e.rp, e.k) for o in REG)}
    assert len(behind) == 4 + 7 + 10
    assert {n for c in T.CASES if c.tag.startswith("behind-duo") for n in c.kernels.values()} >= behind


# ------------------------------------------------------------------------------------ the selection logic, restated
def pick_rp(reg, d, maxrank, model, variant):
    """c3sc_hip.hip pick_rp: the smallest padded rank >= maxrank among the entries of the forced variant and the model, else of
    the model, else of the dimension"""
    def smallest(pred):
        r = [e.rp for e in reg if e.d == d and e.rp >= maxrank and pred(e)]
        return min(r) if r else 0
    rp = 0
    if variant != AUTO:
        rp = smallest(lambda e: e.variant == variant and (model == "0" or e.model == model))
    if not rp and model != "0":
        rp = smallest(lambda e: e.model == model)
    return rp or smallest(lambda e: True)


SMALL_BATCH_FIBERS = 16384


def find_kernel(reg, model, d, rank_needed, N, variant, k, F=None, skip=()):
    """c3sc_hip.hip find_kernel: model, dimension, rp >= rank_needed, max_n >= N, k, the variant filter; then the smallest rp, the
    preference order of the variants (per-wave first for small AUTO batches, else pair, quad, per-wave), fewer nodes per lane;
    the first registered wins a tie"""
    small = variant == AUTO and F is not None and F < SMALL_BATCH_FIBERS
    order = [PER_WAVE, PAIR, QUAD] if small else [PAIR, QUAD, PER_WAVE]
    pref = lambda v: order.index(v) if v in order else 3
    best = None
    for e in reg:
        if e.model != model or e.d != d or e.rp < rank_needed or e.max_n < N or e in skip:
            continue
        if e.k >= 0 and e.k != k:
            continue
        if variant != AUTO and e.variant != variant:
            continue
        if (best is None or e.rp < best.rp or (e.rp == best.rp and pref(e.variant) < pref(best.variant)) or
                (e.rp == best.rp and e.variant == best.variant and e.npl < best.npl)):
            best = e
    return best


# doubles per candidate row in LDS, CandLds<Model>::CW = DU + max(NCF, 1) + 2 max(NUC, 1) + 1 (kernel_common.hpp), from models.hpp:
# (DU, NCF, bits of UCONST_MASK)
def cand_row(mtype):
    d = _dim_of(mtype)
    du, ncf, nuc = {"Dubins3D": (1, 0, 1), "Scar4D": (2, 1, 1), "Car7D": (2, 0, 2), "Rossler3D": (1, 0, 0), "Tprob3D": (3, 0, 0),
                    "Perch7D": (1, 0, 1), "Skid5D": (1, 0, 0), "Cothrust6D": (3, 3, 3)}.get(mtype, (None, 0, 0))
    if mtype.startswith("LqgNd"):
        du, ncf, nuc = d // 2, 0, d // 2
    elif mtype.startswith("Chain"):
        du, ncf, nuc = 1, 0, 1
    return du + max(ncf, 1) + 2 * max(nuc, 1) + 1


LDS_LIMIT = 160 * 1024  # bytes
OK, OOM, UNSUPPORTED = "ok", "out of memory", "not supported"


def launch(e, ngrid, k, ncand, cmode=0):
    """what the entry's launcher answers before it launches (launch_fpw.hpp, launch_fpp.hpp, launch_fq.hpp), and whether the
    per-wave kernel stages its varying core: (OK | OOM | UNSUPPORTED, staged)"""
    d, rp, N = e.d, e.rp, ngrid[k]
    if e.variant == PER_WAVE:
        if cmode == 1 and e.kind != "C3SC_REG_FPW_BOX":
            return UNSUPPORTED, None
        cand = 0 if e.kind == "C3SC_REG_STENCIL" or e.mtype.startswith("TableModel") else ncand * cand_row(e.mtype)
        ws = 4 * rp + 2 * d * rp + 64 * e.npl
        edge = k == 0 or k == d - 1
        staged = (4 * ws + N * ((rp if edge else rp * rp) | 1) + cand) * 8
        if staged <= LDS_LIMIT:
            return OK, True
        return (OK, False) if rp >= 12 else (OOM, None)
    if e.variant == PAIR:
        return (UNSUPPORTED if ncand > 64 else OK), None
    if cmode == 1 or ncand > 64:
        return UNSUPPORTED, None
    stage = max(ngrid[m] * ((rp if m in (0, d - 1) else rp * rp) + 2) for m in range(d) if m != k)
    stage = (stage + 1) & ~1
    if e.kind == "C3SC_REG_FQ1":
        onepass = not (rp >= 16 and d >= 8)
        doubles = stage + e.nwv * (18 if onepass else N) * 16
    else:
        half = e.nwv // 2
        doubles = stage * (2 if e.dbuf else 1) + half * N * 16 + half * 2 * d * 8 + half * 2 * d * 64
    doubles += ncand * cand_row(e.mtype)
    return (OOM if doubles * 8 > LDS_LIMIT else OK), None


def select(reg, model, d, ranks, ngrid, upload_variant, variant, k, ncand, F=None, cmode=0, lookup_model=None):
    """launch_bellman restated: the padded rank of the upload, then the best entry that does not decline.  Returns (entry or None,
    staged, the entries that declined)."""
    rp = pick_rp(reg, d, max(ranks), model, upload_variant)
    declined = []
    while True:
        e = find_kernel(reg, lookup_model or model, d, rp, ngrid[k], variant, k, F, declined)
        if e is None or e.rp != rp:
            return None, None, declined
        ans, staged = launch(e, ngrid, k, ncand, cmode)
        if ans == OK:
            return e, staged, declined
        declined.append(e)


def _E(kind, model, d, rp, npl, variant, max_n, k, name, nwv=0, dbuf=False):
    return Entry(kind, model, "Car7D", d, rp, npl, variant, max_n, k, nwv, dbuf, name, "x", 0)


def test_selection_restatement_rules():
    """the rules of pick_rp and find_kernel one by one, on a hand-made registry"""
    reg = [
        _E("C3SC_REG_FPW", "M", 7, 4, 2, PER_WAVE, 128, -1, "w4n2"),
        _E("C3SC_REG_FPW", "M", 7, 4, 1, PER_WAVE, 64, -1, "w4n1"),
        _E("C3SC_REG_FPW", "M", 7, 10, 1, PER_WAVE, 64, -1, "w10"),
        _E("C3SC_REG_FPW", "M", 7, 12, 1, PER_WAVE, 64, -1, "w12"),
        _E("C3SC_REG_FPP1", "M", 7, 4, 0, PAIR, 128, 2, "p4k2"),
        _E("C3SC_REG_FPP1", "M", 7, 10, 0, PAIR, 128, 2, "p10k2"),
        _E("C3SC_REG_FQD", "M", 7, 12, 0, QUAD, 128, 2, "d12k2", 8, True),
        _E("C3SC_REG_FQ1", "M", 7, 12, 0, QUAD, 128, 2, "q12k2", 8),
        _E("C3SC_REG_FQ1", "M", 7, 4, 0, QUAD, 128, 2, "q4k2", 8),
        _E("C3SC_REG_FPW", "O", 7, 8, 1, PER_WAVE, 64, -1, "other8"),
        _E("C3SC_REG_STENCIL", "0", 7, 6, 1, PER_WAVE, 64, -1, "st6"),
    ]
    # pick_rp: the forced variant's own classes first, then the model's, then the dimension's
    assert pick_rp(reg, 7, 9, "M", AUTO) == 10 and pick_rp(reg, 7, 9, "M", QUAD) == 12 and pick_rp(reg, 7, 9, "M", PAIR) == 10
    assert pick_rp(reg, 7, 11, "M", PAIR) == 12  # no pair class holds 11: the model's
    assert pick_rp(reg, 7, 5, "X", AUTO) == 6 and pick_rp(reg, 7, 5, "0", AUTO) == 6 and pick_rp(reg, 7, 13, "M", AUTO) == 0
    name = lambda *a, **kw: getattr(find_kernel(reg, *a, **kw), "name", None)
    assert name("M", 7, 4, 20, PER_WAVE, 2) == "w4n1"      # the variant filter; fewer nodes per lane wins the tie
    assert name("M", 7, 4, 65, PER_WAVE, 2) == "w4n2"      # max_n
    assert name("M", 7, 4, 129, AUTO, 2) is None
    assert name("M", 7, 4, 20, PAIR, 2) == "p4k2" and name("M", 7, 4, 20, PAIR, 3) is None  # k
    assert name("M", 7, 5, 20, AUTO, 2) == "p10k2"         # the smallest rp at or above the rank needed
    assert name("M", 7, 4, 20, AUTO, 2) == "p4k2" and name("M", 7, 4, 20, AUTO, 2, F=100) == "w4n1"  # the preference orders
    assert name("M", 7, 4, 20, AUTO, 3) == "w4n1" and name("M", 7, 12, 20, AUTO, 2) == "d12k2"       # quad before per-wave
    assert name("M", 7, 12, 20, QUAD, 2) == "d12k2"        # the first registered wins
    assert name("M", 7, 12, 20, QUAD, 2, skip=[reg[6]]) == "q12k2" and name("M", 7, 12, 20, AUTO, 2, skip=reg[6:8]) == "w12"
    assert name("0", 7, 6, 20, AUTO, 0) == "st6" and name("O", 7, 4, 20, AUTO, 0) == "other8"
    # the launchers: a list of more than 64 candidates, the box mode, the LDS limits
    assert launch(reg[4], (9,) * 7, 2, 65)[0] == UNSUPPORTED and launch(reg[7], (9,) * 7, 2, 65)[0] == UNSUPPORTED
    assert launch(reg[0], (9,) * 7, 2, 9, cmode=1)[0] == UNSUPPORTED and launch(reg[7], (9,) * 7, 2, 9, cmode=1)[0] == UNSUPPORTED
    assert launch(reg[3], (9, 9, 64, 9, 9, 9, 9), 2, 9) == (OK, True) and launch(reg[2], (9, 9, 128, 9, 9, 9, 9), 1, 9) == (OK, True)
    big = _E("C3SC_REG_FPW", "M", 7, 20, 1, PER_WAVE, 64, -1, "w20")
    assert launch(big, (9, 9, 64, 9, 9, 9, 9), 2, 9) == (OK, False) and launch(big, (64, 9, 9, 9, 9, 9, 9), 0, 9) == (OK, True)
    # rank 12 at d = 7: one buffer of 69 nodes x 146 fits the quad kernel, two buffers do not fit the duo kernel
    assert launch(reg[6], (9, 69, 9, 9, 9, 9, 9), 2, 9)[0] == OOM and launch(reg[7], (9, 69, 9, 9, 9, 9, 9), 2, 9)[0] == OK


MODEL_ID = {wl.MODEL_DUBINS3D: "C3SC_MODEL_DUBINS3D", wl.MODEL_SCAR4D: "C3SC_MODEL_SCAR4D", wl.MODEL_CAR7D: "C3SC_MODEL_CAR7D",
            wl.MODEL_LQGND: "C3SC_MODEL_LQGND", wl.MODEL_CHAIN: "C3SC_MODEL_CHAIN", wl.MODEL_ROSSLER3D: "C3SC_MODEL_ROSSLER3D",
            wl.MODEL_TPROB3D: "C3SC_MODEL_TPROB3D", wl.MODEL_PERCH7D: "C3SC_MODEL_PERCH7D", wl.MODEL_SKID5D: "C3SC_MODEL_SKID5D",
            wl.MODEL_COTHRUST6D: "C3SC_MODEL_COTHRUST6D"}
TILES = {"C3SC_REG_FPW": 4, "C3SC_REG_FPW_BOX": 4, "C3SC_REG_STENCIL": 4, "C3SC_REG_FPP1": 64}


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_row_selects_the_kernel_it_claims(case):
    """every row's (grid, ranks, variant, k) selects the kernel name the row claims, with the staging and the declines its tag
    says; its ranks, grid and batch follow the table's rules"""
    w = T.workload(case)
    d = w.dx
    model = MODEL_ID[w.model]
    assert case.family in ("table", "stencil") or case.key == T.MODEL_OF[case.name]
    lookup = {"table": "C3SC_MODEL_TABLE", "stencil": "0"}.get(case.family)
    cmode = 1 if case.family == "fpw_box" else 0
    assert case.ks and set(case.ks) <= set(range(d)) and set(case.kernels) == set(case.ks)
    if case.family in ("fpp", "fq", "fqd"):  # K-specific families run every k (a tagged row and its sibling share them)
        sib = [c for c in T.CASES if (c.family, c.key, c.rp) == (case.family, case.key, case.rp) and c.tag[:10] == case.tag[:10]]
        assert sorted(k for c in sib for k in c.ks) == list(range(d))
    for k in case.ks:
        # the box call looks the per-wave kernel up itself; the table and stencil calls look up AUTO without a batch size.  The
        # box launch keeps the context's candidate list in its LDS arithmetic (fill_args: A.ncand = c->ncand).
        variant = PER_WAVE if cmode else (AUTO if lookup else case.variant)
        e, staged, declined = select(REG, model, d, case.ranks, case.ngrid, case.variant, variant, k, w.ncand,
                                     F=None if lookup or cmode else case.nfib, cmode=cmode, lookup_model=lookup)
        assert e is not None, (k, [x.name for x in declined])
        assert e.name == case.kernels[k], (k, e.name, case.kernels[k], [x.name for x in declined])
        assert e.rp == case.rp
        if e.variant == PER_WAVE:
            assert staged == (k not in case.opts.get("unstaged", ())), (k, staged)
            assert (case.ngrid[k] > 64) == (e.npl == 2)
        if cmode:  # the box test's round trip: a second engine, the list kernel on one candidate per node of the batch
            e2, staged2, declined2 = select(REG, model, d, case.ranks, case.ngrid, case.variant, case.variant, k,
                                            case.nfib * case.ngrid[k], F=case.nfib)
            assert e2 is e and staged2 == staged and not declined2, (k, getattr(e2, "name", None), staged2)
        has_duo = any(o.kind in ("C3SC_REG_FQD", "REG_FQD_SB") and (o.model, o.d, o.rp, o.k) == (model, d, case.rp, k) for o in REG)
        if case.tag.startswith("behind-duo") and has_duo:
            assert [x.kind for x in declined] in (["C3SC_REG_FQD"], ["REG_FQD_SB"]), [x.name for x in declined]
            assert launch(declined[0], case.ngrid, k, w.ncand)[0] == OOM
        else:
            assert not declined, [x.name for x in declined]
        tile = TILES.get(e.kind) or (16 * e.nwv if e.kind == "C3SC_REG_FQ1" else 8 * e.nwv)
        assert case.nfib % tile != 0  # ragged against the tile
        if e.variant != PER_WAVE:
            assert case.nfib > 2 * tile, (case.nfib, tile)  # at least three tiles: two full ones and a ragged third
    # ranks: the largest above the next smaller class of the upload's variant and below the class where it allows; unequal bonds
    classes = sorted({e.rp for e in REG if e.d == d and e.model == model and (case.variant == AUTO or e.variant == case.variant)})
    assert case.rp in classes or case.family in ("table", "stencil")
    lower = max([c for c in sorted({e.rp for e in REG if e.d == d and e.model == model}) if c < case.rp], default=0) \
        if case.variant == AUTO else max([c for c in classes if c < case.rp], default=0)
    assert lower < max(case.ranks) <= case.rp
    assert max(case.ranks) < case.rp or case.rp - 1 <= lower
    assert d < 3 or len(set(case.ranks[1:-1])) > 1
    if case.tag.startswith("npl2") or case.tag == "n128":
        assert all(65 <= case.ngrid[k] <= 128 for k in case.ks)
    elif case.family in ("fpw", "fpw_box", "table", "stencil"):
        assert all(case.ngrid[k] <= 64 for k in case.ks)
    if cmode == 0 and case.family not in ("table", "stencil"):
        assert 2 <= w.ncand <= 64


def test_table_spans_the_edges():
    npl2 = [n for c in T.CASES if c.tag == "npl2" for n in c.ngrid]
    assert 65 in npl2 and 128 in npl2
    for rp in (16, 20):  # the STAGED = false instantiation of the per-wave kernel, both rank classes a grid reaches it at
        assert any(c.opts.get("unstaged") and c.rp == rp and c.family == "fpw" for c in T.CASES)
    assert {len(c.ngrid) for c in T.CASES if c.family == "table"} == {2, 3, 4, 6, 7, 10}
    assert {c.name for c in T.CASES if c.family == "stencil" and len(c.ngrid) in (5, 10)} == {"skid5d", "quad10d"}
    assert T.EPS_BOUND * 2 < T.REL_TOL / 10


# ------------------------------------------------------------------------------------ the reference, pinned to the oracle
Q_ROWS = [c for c in T.CASES if c.family in T.LIST_FAMILIES + ("table",)]


@pytest.mark.parametrize("signed", [False, True], ids=["synth", "signed"])
@pytest.mark.parametrize("case", Q_ROWS, ids=T.case_id)
def test_q_table_is_the_oracles_backup(oracle, case, signed):
    """the per-candidate table: Q.min over the candidates equals the oracle's Bellman backup to 1e-14 of the batch scale on live
    nodes for every k the row runs, every single-candidate run has the full run's flags on every node, and the oracle's
    argmin attains the minimum.  A pin of the construction on the first min(nfib, 40) fibers of each batch; the GPU file builds Q for
    the whole batch."""
    w = T.workload(case)
    cs = T.cores(case, w, signed)
    P = oracle.Problem(w, cs)
    for k in case.ks:
        idx = T.fibers(w, k, min(case.nfib, 40))
        ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
        Q, flags = T.q_table(oracle, w, cs, k, idx)
        for c in range(w.ncand):
            assert np.array_equal(flags[c], ref_ab)
        live = ref_ab == 0
        assert live.any()
        scale = np.abs(ref).max()
        qmin = Q.min(axis=-1)
        assert np.abs(qmin - ref)[live].max() <= 1e-14 * scale
        assert np.array_equal(qmin[~live], ref[~live])
        at = np.take_along_axis(Q, np.clip(ref_ui, 0, w.ncand - 1)[..., None], axis=-1)[..., 0]
        assert (ref_ui[live] >= 0).all() and (ref_ui[live] < w.ncand).all()
        assert np.abs(at - qmin)[live].max() <= 1e-14 * scale
        if signed:
            assert T.vabs(oracle, w, cs, k, idx) > 0.0


# ------------------------------------------------------------------------------------------------ discount regimes
def test_udep_table_matches_models_hpp():
    """T.UDEP restates every UDEP_MASK line of models.hpp; Chain<DIM> and LqgNd<DIM> as formulas, compared at every registered DIM"""
    src = re.sub(r"//.*", "", open(os.path.join(CSRC, "models.hpp")).read())
    found, name, templ, prev = {}, None, False, ""
    for line in src.splitlines():
        m = re.match(r"struct\s+(\w+)\s*\{", line)  # a top-level struct (nested ones are indented)
        if m:
            name, templ = m.group(1), bool(re.match(r"template\s*<int DIM>", prev))
        m = re.search(r"UDEP_MASK\s*=\s*([^;,]+)[;,]", line)
        if m:
            assert name and name not in found, line
            found[name] = (templ, re.sub(r"(0x[0-9A-Fa-f]+|\d+)u\b", r"\1", m.group(1)).strip())
        prev = line if line.strip() else prev
    assert len(re.findall(r"UDEP_MASK\s*=", src)) == len(found)
    assert set(found) == set(T.UDEP), set(found) ^ set(T.UDEP)
    dims = {"LqgNd": (2, 4, 6), "Chain": (2, 4, 10), "TableModel": (2, 3, 4, 6, 7, 10), "NoModel": (2, 3, 4, 5, 6, 7, 10)}
    for name, (templ, expr) in found.items():
        for dim in dims.get(name, (None,)):
            assert templ == (dim is not None), name
            mask = eval(expr, {"__builtins__": {}}, {"DIM": dim})
            want = T.udep(name if dim is None else f"{name}<{dim}>")
            assert mask == sum(1 << m for m in want), (name, dim, hex(mask), want)
    for c in T.CASES:  # every row's model has an entry
        if c.family not in ("table", "stencil"):
            T.udep(c.key)


def test_bodies_of_on_hand_made_batches():
    """the batch-wide inequalities one by one"""
    dt = np.array([[[1.0, 0.5], [0.25, 0.125]]])
    r0 = np.array([[2.0, 0.5]])
    B = lambda split, beta, r=r0, t=dt: T.bodies_of(split, t, r, beta)
    assert B(True, 0.0) == B(False, 0.0) == {"fraction"}
    assert B(True, 2.0 ** -12) == {"E0"} and B(False, 2.0 ** -12) == {"E3-tiny"}
    assert B(True, 2.0 ** -11) == {"E1"} and B(False, 2.0 ** -9) == {"E3-small"}  # 2^-11 x 2 = 2^-10 fails all_tiny
    assert B(True, 2.0 ** -8) == {"E2-poly"}  # the lane with r0 = 2 fails all_small; every dt <= 1 passes the candidate vote
    assert B(True, 2.0 ** -7) == {"E2-poly"} and B(False, 2.0 ** -7) == {"E3-poly"}  # candidate 1 passes everywhere, candidate 0 is split
    assert B(True, 2.0 ** -4) == {"E2-libm"} and B(False, 2.0 ** -4) == {"E3-libm"}
    rinf = np.array([[np.inf, 0.5]])
    assert B(True, 2.0 ** -12, rinf) == {"E2-poly+CHECK"} and B(True, 2.0 ** -4, rinf) == {"E2-libm+CHECK"}
    assert B(False, 2.0 ** -12, rinf) == {"E3-poly"}  # a lane with Q0 = 0 fails all_tiny and all_small
    dtn = dt.copy()
    dtn[0, 0, 0] = np.nan  # an invalid candidate takes no part in the inequalities
    assert B(True, 2.0 ** -4, rinf, dtn) == {"E2-libm+CHECK"}


LIST_ROWS = [c for c in T.CASES if c.family in T.LIST_FAMILIES]


@pytest.mark.parametrize("case", LIST_ROWS, ids=T.case_id)
def test_regime_implies_body(oracle, case):
    """the named regime implies the named body, for every k of the row, from the oracle's dt and r0"""
    beta = T.regime_betas(oracle, case)
    assert set(beta) == set(T.REGIMES)
    split = T.SPLIT[case.family]
    pc = T.row_pieces(oracle, case)
    any_inf = any(np.isinf(r0).any() for _, r0 in pc.values())
    all_inf = all(np.isinf(r0).all() for _, r0 in pc.values())
    assert any_inf == all_inf == (case.key == "Tprob3D")  # a row's own batch has no stationary lane, Tprob3D's nothing else
    B = {r: {k: T.scan_bodies(oracle, case, k, beta[r]) for k in case.ks} for r in T.REGIMES}
    union = {r: set().union(*B[r].values()) for r in T.REGIMES}
    for k in case.ks:
        dt, r0 = pc[k]
        assert np.isfinite(dt).all()
        assert B["zero"][k] == {"fraction"}
        if not split:
            assert B["tiny"][k] == {"E3-tiny"} and B["libm"][k] == {"E3-libm"} and B["small"][k] <= {"E3-tiny", "E3-small"}
        elif all_inf:
            assert B["tiny"][k] == B["small"][k] == {"E2-poly+CHECK"} and B["libm"][k] == {"E2-libm+CHECK"}
        else:
            assert B["tiny"][k] == {"E0"} and B["libm"][k] == {"E2-libm"} and B["small"][k] <= {"E0", "E1"}
        assert B["small"][k]
    # the k that holds the row's largest r0 fails all_tiny in `small`
    assert ("E3-small" if not split else "E2-poly+CHECK" if all_inf else "E1") in union["small"]
    dts = np.concatenate([dt.ravel() for dt, _ in pc.values()])
    assert beta["mixed"] * dts.min() < 2.0 ** -7 <= beta["mixed"] * dts.max()  # the batch straddles the threshold
    assert 0.0 < beta["tiny"] < beta["small"] < beta["libm"]


def _stationary_bodies(oracle, case):
    w = T.stationary_workload(case)
    beta = T.regime_betas(oracle, case, w, T.fibers_through)
    return {r: set().union(*[T.scan_bodies(oracle, case, k, beta[r], w, T.fibers_through) for k in case.ks]) for r in T.STATIONARY_REGIMES}


def test_every_family_reaches_every_body(oracle):
    """over the table and the regimes, every family reaches every body its SPLIT setting compiles, up to UNREACHABLE_BODIES; the
    CHECK bodies are reached by rows other than Tprob3D's (the stationary inputs)"""
    reached = {f: set() for f in T.LIST_FAMILIES}
    check_rows = set()
    for case in LIST_ROWS:
        beta = T.regime_betas(oracle, case)
        for r in T.REGIMES:
            for k in case.ks:
                b = T.scan_bodies(oracle, case, k, beta[r])
                reached[case.family] |= b
                if any(x.endswith("+CHECK") for x in b):
                    check_rows.add(case.key)
    for case in T.stationary_cases():
        for r, b in _stationary_bodies(oracle, case).items():
            reached[case.family] |= b
            if any(x.endswith("+CHECK") for x in b):
                check_rows.add(T.case_id(case))
    for fam, got in reached.items():
        want = set(T.BODIES[T.SPLIT[fam]])
        assert got <= want
        missing = want - got - {b for b, (fams, why) in T.UNREACHABLE_BODIES.items() if fam in fams}
        assert not missing, (fam, sorted(missing))
    for b, (fams, why) in T.UNREACHABLE_BODIES.items():
        assert isinstance(why, str) and why.strip()
        for fam in fams:
            assert b in T.BODIES[T.SPLIT[fam]] and b not in reached[fam], (b, fam)  # a stale entry
    assert check_rows - {"Tprob3D"}, check_rows
    assert {c.family for c in T.stationary_cases()} == {"fpw", "fpp", "fq"} and len(T.stationary_cases()) == len(T.STATIONARY_ROWS)


@pytest.mark.parametrize("case", T.stationary_cases(), ids=T.case_id)
def test_stationary_reference_is_pinned_to_q_table(oracle, case):
    """Q built from the oracle's pieces (T.q_pieces) equals T.q_table to 1e-14 of the batch scale on a batch without a stationary
    node, flags included; on the batch through the centre nodes it has invalid candidates exactly where every coordinate of
    T.zero_axes vanishes, only at u = 0, the oracle fails those fibers with 101, and every node keeps a valid candidate"""
    import ctypes as C

    w = T.stationary_workload(case)
    cs = T.cores(case, w)
    mtype = T.MODEL_OF[case.name]
    za = T.zero_axes(mtype)
    xg = w.xgrid()
    assert (w.cands[2] == 0.0).all()
    for k in case.ks:
        n = min(case.nfib, 12)
        if any(m != k for m in za):
            idx = T.fibers_clear(w, k, n)
            Q, ab, bad = T.q_pieces(oracle, w, cs, k, idx, mtype)
            Qt, flags = T.q_table(oracle, w, cs, k, idx)
            assert not bad and not np.isnan(Q).any()
            assert np.array_equal(flags[0], ab)
            assert np.abs(Q - Qt).max() <= 1e-14 * np.abs(Qt).max()
        idx = T.fibers_through(w, k, n)
        Q, ab, bad = T.q_pieces(oracle, w, cs, k, idx, mtype)
        x = np.stack([np.broadcast_to(xg[m][:, None] if m == k else xg[m][idx[:, m]][None, :], (w.ngrid[k], n)).T for m in range(w.dx)], -1)
        want = (x[..., list(za)] == 0.0).all(axis=-1) & (ab == 0)
        assert want.any() and bad
        assert np.array_equal(np.isnan(Q[..., 2]), want)
        assert not np.isnan(np.delete(Q, 2, axis=-1)).any()
        P = oracle.Problem(w, cs)
        o, u = np.zeros((1, w.ngrid[k])), np.zeros((1, w.ngrid[k]), dtype=np.int32)
        f = int(np.argmax(want.any(axis=1)))
        row = np.ascontiguousarray(idx[f:f + 1], dtype=np.int32)
        assert P.L.orc_bellman_fibers(P.h, C.c_size_t(k), C.c_size_t(1), oracle.ip(row), oracle.dp(o), oracle.ip(u), None) == 101
