"""tests/box_ref.py, the numpy restatement of the continuous-control minimiser, held without a GPU: its objective to the oracle's
per-candidate values, its grid scan to the oracle's Bellman backup over the same grid, the whole minimiser to the host's
box_minimize (c3opt_minimize of libc3sc.so, loaded through facade_lib as the simulate tests load it); the preconditions of
tests/test_gpu_box_minimiser.py on the reference alone (the cap on unpinned nodes, interior minimisers, the edge rows' share); and
every planted fault rejected on some row by the GPU test's own criterion."""
import ctypes as C

import numpy as np
import pytest

import box_ref as B
import fiber_kernel_cases as T

DATA = [False, True]
DATA_IDS = ["synth", "signed"]
ROWS = B.built_rows()
ROW_IDS = [B.row_id(*r) for r in ROWS]


def _lowest(name):
    case = B.box_case(name)
    w = T.workload(case)
    return case, w, B.middle_k(case)


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("name", B.BOX_MODELS)
def test_objective_is_the_oracles_candidate_value(oracle, name, signed):
    """the restatement's objective on an explicit candidate list (the small grid of the example's box) equals
    oracle.Problem.q_fibers to 1e-13 of the scale at every live node"""
    case, w, k = _lowest(name)
    lb, ub, G = T.BOX[name]
    cs = T.cores(case, w, signed)
    idx = T.fibers(w, k, B.NFIB)
    cands = T.box_grid(lb, ub, G)
    wscan = T.with_cands(w, cands)
    Q, ab = oracle.Problem(wscan, cs).q_fibers(k, idx)
    x, V, ab2, _ = B.fiber_setup(oracle, w, cs, k, idx)
    assert np.array_equal(ab, ab2)
    obj = B.Objective(oracle, w, x, V)
    mine = np.stack([obj.at(c)[0] for c in cands], axis=-1).reshape(Q.shape)
    live = ab == 0
    scale = T.scale_of(oracle, wscan, cs, k, idx, Q.min(axis=-1), signed)
    err = float(np.abs(mine - Q)[live].max() / scale)
    print(f"{name}: objective against q_fibers {err:.2e} of the scale")
    assert live.any() and err <= 1e-13


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("name", B.BOX_MODELS)
def test_grid_scan_is_the_oracles_backup(oracle, name, signed):
    """polish = 0 against Problem.bellman_fibers on fiber_kernel_cases.box_grid: the same winning grid point at every live node,
    the points of the grid themselves box_grid's to an ulp of the box width, the absorbed nodes' costs exactly the oracle's, and the value the
    objective's at that point -- which the test above holds to the oracle's to 1e-13 of the scale; the two are separate
    implementations of the arithmetic (the oracle's transition_assemble and bellmanrhs), so the last bits may differ"""
    case, w, k = _lowest(name)
    lb, ub, G = T.BOX[name]
    cs = T.cores(case, w, signed)
    idx = T.fibers(w, k, B.NFIB)
    cands = T.box_grid(lb, ub, G)
    ulp = 2.0 ** -52 * (np.array(ub) - np.array(lb))  # box_grid rounds gi dl and then the sum, the kernel's fma once
    for c in range(len(cands)):
        assert (np.abs(B.grid_point(np.array(lb, float), np.array(ub, float), G, c) - cands[c]) <= ulp).all()
    scan, ui, ab = oracle.Problem(T.with_cands(w, cands), cs).bellman_fibers(k, idx)
    ref = B.fibers(oracle, w, cs, k, idx, lb, ub, G, 0, signed)
    live = ab == 0
    assert np.array_equal(ref.ab, ab) and np.array_equal(ref.val[~live], scan[~live]) and not ref.u[~live].any()
    sure = live & ~ref.of(ref.box.grid_unsure)
    assert sure.sum() >= 0.9 * live.sum()
    assert np.array_equal(ref.of(ref.box.grid_c)[sure], ui[sure])
    assert (np.abs(ref.u[sure] - cands[ui[sure]]) <= ulp).all()
    assert np.abs(ref.val - scan)[live].max() <= 1e-13 * ref.scale
    assert not ref.box.searches and np.array_equal(ref.box.u, ref.box.grid_u)


# ------------------------------------------------------------------------------------------------ the host's minimiser
OBJ = C.CFUNCTYPE(C.c_double, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
dpp = C.POINTER(C.c_double)


def _host_minimise(obj, lb, ub, G, polish, nodes):
    """c3opt_minimize of a line-search c3Opt (the examples' set-up: box bounds, c3opt_set_box_search) on the reference objective
    of one node at a time: (values, points)"""
    import facade_lib

    L = facade_lib.lib()
    L.c3opt_alloc.argtypes = [C.c_int, C.c_size_t]
    L.c3opt_add_objective.argtypes = [C.c_void_p, OBJ, C.c_void_p]
    L.c3opt_minimize.argtypes = [C.c_void_p, dpp, dpp]
    L.c3opt_set_box_search.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
    L.c3opt_add_lb.argtypes = L.c3opt_add_ub.argtypes = [C.c_void_p, dpp]
    L.c3opt_free.argtypes = [C.c_void_p]
    du = len(lb)
    lo, hi = np.array(lb, dtype=np.float64), np.array(ub, dtype=np.float64)
    vals, pts = np.empty(len(nodes)), np.empty((len(nodes), du))
    for n, p in enumerate(nodes):
        one = B.Objective(obj.oracle, obj.w, obj.x[p:p + 1], obj.V[p:p + 1])
        f = OBJ(lambda d, u, g, a: float(one(np.array([[u[i] for i in range(d)]]))[0][0]))
        opt = C.c_void_p(L.c3opt_alloc(0, du))  # BFGS: the box minimiser
        L.c3opt_add_lb(opt, lo.ctypes.data_as(dpp))
        L.c3opt_add_ub(opt, hi.ctypes.data_as(dpp))
        L.c3opt_set_box_search(opt, G, polish)
        L.c3opt_add_objective(opt, f, None)
        x, v = np.zeros(du), C.c_double(0.0)
        assert L.c3opt_minimize(opt, x.ctypes.data_as(dpp), C.byref(v)) == 0
        vals[n], pts[n] = v.value, x
        L.c3opt_free(opt)
    return vals, pts


HOST_ROWS = [r for r in B.setting_rows() if r[1].name in ("lqg2d", "tprob3d") and r[1].tag in ("polish2", "polish3", "edge", "even", "fixed")]


@pytest.mark.parametrize("case,row,signed", HOST_ROWS, ids=[B.row_id(*r) for r in HOST_ROWS])
def test_host_box_minimize_follows_the_restatement(oracle, case, row, signed):
    """the host's box_minimize (c3sc_support.c) over the SAME objective callback: its decisions are the restatement's, so the
    value agrees to 1e-12 of the scale (in fact to the bit: asserted too) and u lies in the recorded interval, at every live node
    of up to 40 spread over the batch"""
    w, cs, k, ref = B.row_ref(oracle, case, row, signed)
    live = np.flatnonzero(ref.live.reshape(-1))
    nodes = live[np.unique(np.round(np.linspace(0, len(live) - 1, 40)).astype(int))]
    vals, pts = _host_minimise(ref.obj, row.lb, row.ub, row.grid, row.polish, nodes)
    b = ref.box
    assert np.abs(vals - b.val[nodes]).max() <= T.REL_TOL * ref.scale
    assert ((pts >= b.ulo[nodes]) & (pts <= b.uhi[nodes])).all()
    assert np.array_equal(vals, b.val[nodes]) and np.array_equal(pts, b.u[nodes])


# ------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("case,row,signed", ROWS, ids=ROW_IDS)
def test_rows_keep_the_preconditions(oracle, case, row, signed):
    """on the reference alone (box_ref.row_ok): at most MAX_UNPINNED of a row's live nodes are unpinned; a row with a polish and a
    free control has at least MIN_INTERIOR_PINNED PINNED live nodes whose minimiser is interior to a cell (the polish moved them off
    their grid point: the nodes on which a wrong polish shows); an edge row has at least EDGE_SHARE of its live nodes with the best
    grid point on a face"""
    st = B.row_stats(B.row_ref(oracle, case, row, signed)[3], row)
    print(f"{B.row_id(case, row, signed)}: box {row.lb} .. {row.ub}, grid {row.grid}, cores x {row.mul}: {st}")
    assert st["unpinned"] <= B.MAX_UNPINNED, st
    for sp in B.specs_of(case, row):
        face_only = (B.spec_key(sp), signed) in B.FACE_ONLY
        if face_only or case.name in B.NO_INTERIOR:  # the exemption is honest: such a row has no pinned node that the polish moved
            assert st["interior_pinned"] == 0, st
            assert case.name not in B.NO_INTERIOR or st["interior"] == 0, st
        else:
            assert row.polish == 0 or not st["free"] or st["interior_pinned"] >= B.MIN_INTERIOR_PINNED, st
        assert B.row_ok(sp, st, face_only), (B.spec_key(sp), st)


def test_rows_not_built_are_the_ones_listed():
    """every (row, data class) of box_ref.row_specs is either built or listed by not_built(); the count is the one DESIGN.md 6.4
    records, so that a row cannot leave silently"""
    assert sum(len(r.tag.split("+")) for _, r, _ in B.built_rows()) + len(B.not_built()) == 2 * len(B.row_specs())
    assert len(B.not_built()) == 0 and len(B.FACE_ONLY) == 3
    built = {(T.case_id(c), t) for c, r, _ in ROWS for t in r.tag.split("+")}
    for sp in B.row_specs():  # every row of the issue's list runs on at least one data class, but for the ones named here
        if (T.case_id(sp.case), sp.tag) not in built:
            assert B.spec_key(sp) in B.WHOLLY_MISSING, B.spec_key(sp)


# ------------------------------------------------------------------------------------------------ planted faults
def _differs(clean, faulty):
    """the GPU test's criterion on the clean reference's pinned nodes: a value more than REL_TOL of the scale away, or a u_i outside
    the recorded interval"""
    pin = clean.pinned
    val = np.abs(faulty.val - clean.val) > T.REL_TOL * clean.scale
    ulo, uhi = clean.of(clean.box.ulo), clean.of(clean.box.uhi)
    out = ((faulty.u < ulo) | (faulty.u > uhi)).any(axis=-1)
    return int((pin & (val | out)).sum())


# fault -> the built rows (box_ref.row_id) on which it is looked for, found by walking every built row once; at least one must show it
FAULT_ROWS = {
    "no_polish": ("fpw_box-LqgNd2-4-edge2-signed", "fpw_box-Cothrust6D-4-edge2-signed", "fpw_box-Tprob3D-4-polish1+edge2-synth"),
    "first_round": ("fpw_box-LqgNd6-4-rounds-synth", "fpw_box-LqgNd4-4-rounds-synth", "fpw_box-Cothrust6D-4-rounds-synth",
                    "fpw_box-Cothrust6D-4-rounds-signed"),
    "restart": ("fpw_box-LqgNd6-4-rounds-synth", "fpw_box-LqgNd4-4-rounds-synth", "fpw_box-Cothrust6D-4-rounds-synth",
                "fpw_box-Cothrust6D-4-rounds-signed"),
    "coord0": ("fpw_box-Cothrust6D-4-polish1-synth", "fpw_box-Tprob3D-4-polish1+edge2-synth"),
    "reverse": ("fpw_box-Tprob3D-4-polish1+edge2-synth",),
    "half_cell": ("fpw_box-Tprob3D-4-polish1+edge2-synth", "fpw_box-LqgNd4-4-rounds-signed"),
    "no_clamp": ("fpw_box-LqgNd2-4-edge2-signed", "fpw_box-Rossler3D-20-rp20-synth"),
    "steps10": ("fpw_box-LqgNd2-4-edge2-signed", "fpw_box-Cothrust6D-4-grid2-synth"),
    "always_take": ("fpw_box-Rossler3D-4-rp4-signed", "fpw_box-LqgNd2-4-grid2-signed"),
    "freeze": ("fpw_box-LqgNd2-4-polish0-synth", "fpw_box-Tprob3D-4-polish0-synth", "fpw_box-Cothrust6D-4-polish0-synth",
               "fpw_box-Rossler3D-20-rp20-synth"),
}


@pytest.mark.parametrize("fault", [f for f in B.FAULTS if f != "grid_status"])
def test_planted_fault_is_rejected_on_some_row(oracle, fault):
    """every row of FAULT_ROWS[fault] is a built row, and on each of them the faulty reference differs from the clean one on pinned
    nodes by the device test's criterion"""
    seen = {}
    by_id = {B.row_id(*r): r for r in ROWS}
    for rid in FAULT_ROWS[fault]:
        case, row, signed = by_id[rid]
        clean = B.row_ref(oracle, case, row, signed)[3]
        faulty = B.row_ref(oracle, case, row, signed, fault=fault, widen=False)[3]
        seen[rid] = _differs(clean, faulty)
    print(f"{fault}: pinned nodes that differ, per row: {seen}")
    assert seen and all(seen.values()), seen


def test_status_fault_is_rejected_on_the_probe_row(oracle):
    """the status bit from grid points alone: clear on the probe row, where the restatement sets it; equal on the grid row"""
    case = B.stationary_case()
    w = B.stationary_workload(case)
    grid_row, probe_row = B.STATIONARY
    for signed in DATA:
        for row, differs in ((grid_row, False), (probe_row, True)):
            clean = B.row_ref(oracle, case, row, signed, w=w, fib=B.stationary_fibers)[3]
            faulty = B.row_ref(oracle, case, row, signed, fault="grid_status", w=w, fib=B.stationary_fibers, widen=False)[3]
            assert clean.status == B.STATUS_STATIONARY
            assert (faulty.status != clean.status) == differs
        # on the probe row no grid point is stationary at any node, and the stationary probe is never the result
        assert not (clean.of(clean.box.grid_val)[clean.live] >= 1e299).any() and (clean.val[clean.live] < 1e299).all()


def test_dropped_fault_changes_nothing(oracle):
    """the tensor order with control 0 slowest (box_ref.DROPPED_FAULTS): the same values and points, to the bit, on the du = 3
    rows"""
    n = 0
    for case, row, signed in B.setting_rows():
        if len(row.lb) == 3 and row.polish > 0 and not np.allclose(np.array(row.lb), -np.array(row.ub)):
            clean = B.row_ref(oracle, case, row, signed)[3]
            faulty = B.row_ref(oracle, case, row, signed, fault="slowest", widen=False)[3]
            assert np.array_equal(clean.val, faulty.val) and np.array_equal(clean.u, faulty.u)
            n += 1
    assert n >= 4


# ------------------------------------------------------------------------------------------------ the pinned nodes survive rounding
@pytest.mark.parametrize("case,row,signed", ROWS, ids=ROW_IDS)
def test_pinned_nodes_survive_another_rounding(oracle, case, row, signed):
    """the minimiser run on a second double implementation of the same objective (Objective(reordered=True): other summation order,
    a reciprocal for the divisions -- as far from the reference as the device is) passes the GPU test's own checks against the
    reference: pinned values within REL_TOL of the scale, u inside the interval, unpinned values not above the grid scan"""
    w, cs, k, ref = B.row_ref(oracle, case, row, signed)
    other = B.row_ref(oracle, case, row, signed, widen=False, reordered=True)[3]
    noise = np.abs(other.obj(ref.box.u)[0] - ref.box.val)[ref.live.reshape(-1)].max() / ref.scale
    assert noise <= B.BOX_MARGIN / 50, noise  # the stand-in is no noisier than the margin allows for
    B.check_device(ref, other.val, other.u, other.ab, other.status, row.lb, row.ub, row.polish, B.row_id(case, row, signed))
