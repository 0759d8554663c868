"""The rank-deficient cases of the cross core steps: one table for the CPU simulation (test_cross_reference.py) and the GPU run
(test_gpu_cross_singular_steps.py).

Where deficiency can come from.  car7d and dubins3d absorb on dimensions 0 and 1 only, and under consistent ends a fiber through
a node with x_0 or x_1 on a face is the constant boundcost.  A right set J[k] covers the dimensions k+1 .. d-1, so only J[0] can
carry a face index (in dimension 1); behind it constancy travels through the LEFT sets:
  square first bond   r_1 = N_0: the N_0 x N_0 matrix of step 0 has the equal rows 0 and N_0 - 1, I[1] is every node, and the
                      right-to-left step 1 has the two equal constant columns a = 0 and a = N_0 - 1
  face columns        `faces` tuples of J[0] with x_1 on a face: that many equal constant columns in the left-to-right step 0
  few distinct rows   the rows (a, j) of the left-to-right step 1 with a or j on a face are all the same constant row: at most
                      (N_0 - 2)(N_1 - 2) + 1 different rows; a bond r_2 above that count is deficient, I[2] then holds face
                      tuples, the right-to-left step 2 has that many equal constant columns and the left-to-right step 2 as
                      many blocks of equal rows
  rank-1 bond         the one pivot of a one-column step is the largest entry, the boundcost: I[2] is one face tuple and the
                      left-to-right step 2 is exactly constant
"""
import numpy as np

from c3sc_amd import workloads as wl

# id, workload, grid, cross ranks, tuples of J[0] on a face of dimension 1 ("all": every one), dispatch classes the case is there
# for, dispatch classes that must SEE a deficient matrix (a step of that class with a pivot ratio <= 1e-12 by the restatement),
# dispatch classes that must see an EXACTLY CONSTANT matrix (the tie rule: the only place where the order of equal keys shows)
SINGULAR_CASES = [
    ("square-first-bond", "car7d", (7,) * 7, (1, 7, 8, 8, 8, 8, 7, 1), 0, {"regs-1"}, {"regs-1"}, set()),
    ("face-columns-regs2", "dubins3d", (8, 65, 9), (1, 8, 8, 1), 2, {"regs-2"}, {"regs-1", "regs-2"}, set()),
    ("face-columns-lds", "car7d", (5, 5, 9, 9, 9, 9, 9), (1, 5, 17, 17, 17, 17, 9, 1), 2, {"lds"}, {"lds"}, set()),
    ("global-40-48", "car7d", (7,) * 7, (1, 7, 33, 41, 41, 33, 7, 1), 2,
     {"global-32-panels", "global-40-panels", "global-48-panels"}, {"global-32-panels", "global-40-panels"}, set()),
    ("global-48", "car7d", (7,) * 7, (1, 7, 41, 41, 41, 33, 7, 1), 2, {"global-48-panels"}, {"global-32-panels", "global-48-panels"}, set()),
    ("global-32-le32", "dubins3d", (24, 31, 31), (1, 24, 24, 1), 2, {"global-32-panels"}, {"global-32-panels"}, set()),
    ("tall", "dubins3d", (24, 101, 24), (1, 24, 24, 1), 2, {"global-32-tall"}, {"global-32-tall"}, set()),
    ("rank-1-face", "car7d", (7,) * 7, (1, 4, 1, 4, 4, 4, 4, 1), 0, {"regs-1"}, {"regs-1"}, {"regs-1"}),
    ("all-constant", "car7d", (7,) * 7, (1, 4, 4, 4, 4, 4, 4, 1), "all", {"regs-1"}, {"regs-1"}, {"regs-1"}),
    # behind a rank-1 bond on a face every matrix is exactly constant: one such train per remaining form, so that each form's tie
    # order is held (r_3 <= 7: the step behind the bond has N_2 = 7 rows)
    ("rank-1-face-lds", "car7d", (7,) * 7, (1, 4, 1, 7, 17, 17, 7, 1), 0, {"lds"}, {"lds"}, {"lds"}),
    ("rank-1-face-global", "car7d", (7,) * 7, (1, 4, 1, 7, 33, 41, 7, 1), 0,
     {"global-32-panels", "global-40-panels", "global-48-panels"}, {"global-32-panels", "global-40-panels", "global-48-panels"},
     {"global-32-panels", "global-40-panels", "global-48-panels"}),
    ("rank-1-face-regs2", "dubins3d", (9, 65, 9), (1, 1, 8, 1), 0, {"regs-2"}, {"regs-1"}, {"regs-2"}),      # 520 x 1: one column, constant but of full rank
    ("rank-1-face-tall", "dubins3d", (9, 101, 33), (1, 1, 33, 1), 0, {"global-32-tall"}, {"global-40-panels"}, {"global-32-tall"}),  # 3333 x 1
]
# the well-conditioned control (test_cross_core_steps.py: regs-one-row) at a small grid: interior tuples only, flag 0
CONTROL_CASE = ("control-regs-one-row", "car7d", (11,) * 7, (1, 6, 6, 6, 6, 6, 6, 1), 0, {"regs-1"}, set(), set())
# The cases of the batched confirmation's A / B protocol, each with a seed at which the restated algorithm reaches index sets that
# stop changing (after 4, 4, 4 and 4 iterations).  Under exact deficiency that is not a given: the rows picked in exactly zero
# columns follow the row order and the warm rows, and from other seeds (face-columns-lds at 11, 3, 13; global-40-48 at 7, 5) the
# iteration settles into a cycle of two sets instead -- nothing a confirmation could ever confirm.
CONFIRM_SEEDS = (("square-first-bond", 11), ("face-columns-lds", 7), ("global-40-48", 13), ("control-regs-one-row", 7))


def by_id(cid):
    return next(c for c in SINGULAR_CASES + [CONTROL_CASE] if c[0] == cid)


def seeded_tuples(rng, w, dims, r, faces=0, interior=True):
    """r distinct tuples over `dims`.  The first `faces` of them ("all": every one) carry the node 0 or N - 1 (in turn) of the first
    absorbing dimension of `dims`, if there is one; the others stay off the faces of absorbing dimensions (interior=True) or
    go anywhere."""
    dims = list(dims)
    absorbing = [m for m in dims if w.bc[m] == wl.BC_ABSORB]
    nface = (r if faces == "all" else int(faces)) if absorbing else 0
    lo = {m: 1 if (interior and w.bc[m] == wl.BC_ABSORB) else 0 for m in dims}
    seen, out = set(), []
    tries = 0
    while len(out) < r:
        t = [int(rng.integers(lo[m], w.ngrid[m] - lo[m])) for m in dims]
        if len(out) < nface:
            t[dims.index(absorbing[0])] = 0 if len(out) % 2 == 0 else w.ngrid[absorbing[0]] - 1
        t = tuple(t)
        tries += 1
        assert tries < 100000, f"{r} distinct tuples over dims {dims} do not exist"
        if t not in seen:
            seen.add(t)
            out.append(t)
    return np.array(out, dtype=np.int32).reshape(r, len(dims))


def make_case(case, seed=7):
    """(workload, value cores, I, J): synth_cores at value rank 4; J placed as the table says; I -- only the warm hint of the first
    iteration, every left set is produced -- any distinct tuples."""
    _, name, ngrid, ranks, faces = case[:5]
    w = wl.WORKLOADS[name]().scaled(ngrid=ngrid, rank=4)
    cores = wl.synth_cores(w)
    d = w.dx
    rng = np.random.default_rng(seed)
    I = [seeded_tuples(rng, w, range(k), ranks[k], interior=False) for k in range(d)]
    J = [seeded_tuples(rng, w, range(k + 1, d), ranks[k + 1], faces=faces) for k in range(d)]
    return w, cores, I, J


def summarise(cid, classes, rep):
    """Per dispatch class of one checked iteration: shapes, worst span residual, worst interpolation residual, worst max |B|,
    smallest and largest pivot ratio on either side of the threshold, exact zero pivots, swaps; as lines to print."""
    by = {}
    for s in rep["steps"]:
        b = by.setdefault(classes[(s["dir"], s["k"])], dict(span=0.0, res=0.0, big=0.0, below=0.0, above=np.inf, zeros=0, const=0,
                                                           swaps=0, deficient=0, shapes=set()))
        b["span"] = max(b["span"], s["span"])
        b["res"] = max(b["res"], s["residual"] or 0.0)
        b["big"] = max(b["big"], s["maxB"] or 0.0)
        if s["ratio"] <= 1e-12:
            b["below"] = max(b["below"], s["ratio"])
            b["deficient"] += 1
        else:
            b["above"] = min(b["above"], s["ratio"])
        b["zeros"] += s["zero_pivots"]
        b["const"] += int(s["constant"])
        b["swaps"] += s["swaps"]
        b["shapes"].add(f"{s['m']}x{s['n']}")
    lines = [f"{cid}: {c:17s} {sorted(b['shapes'])}: span {b['span']:.1e}, interpolation {b['res']:.1e}, max|B| {b['big']:.6f}, "
             f"{b['deficient']} deficient steps (worst ratio below {b['below']:.1e}, above {b['above']:.1e}), {b['zeros']} exact zero pivots, "
             f"{b['const']} constant matrices, {b['swaps']} swaps" for c, b in sorted(by.items())]
    lines.append(f"{cid}: flag {rep['flag']}, core 0 vs oracle {rep['raw']:.1e}, {rep['nodes']} distinct nodes")
    return lines, by
