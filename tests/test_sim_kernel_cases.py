"""CPU side of the closed-loop kernel tests (tests/test_gpu_sim_kernels.py): the case table covers the registry, the
extended-precision reference of the off-grid stencil agrees with the oracle on everything the GPU tests feed it, and the
reference side of the k_rollout_ode lock-step keeps its drop share.  Nothing here needs a GPU."""
import glob
import os
import re

import numpy as np
import pytest

import offgrid_ref as R
import sim_kernel_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")
REG = re.compile(r"^\s*C3SC_REG_(ROLLOUT_ODE|ROLLOUT|STENCIL_POINTS)\(([^)]*)\)", re.M)
FAMILY = {"ROLLOUT": "rollout", "ROLLOUT_ODE": "ode", "STENCIL_POINTS": "stencil"}


def _registered():
    """(family, model or D, RP) of every C3SC_REG_ROLLOUT / _STENCIL_POINTS / _ROLLOUT_ODE line, read as text"""
    out = []
    files = sorted(glob.glob(os.path.join(CSRC, "inst_rollout*.hip")))
    assert files
    for f in files:
        for kind, args in REG.findall(open(f).read()):
            a = [t.strip() for t in args.split(",")]
            if kind == "STENCIL_POINTS":  # (DIM, RP)
                out.append(("stencil", a[0], int(a[1])))
            else:  # (MODEL_ID, RP, BOX, Model...): the model's type may hold a comma-free template argument
                out.append((FAMILY[kind], ",".join(a[3:]), int(a[1])))
    return out


def test_case_table_covers_the_registry():
    reg = _registered()
    assert len(reg) == len(set(reg)), "an instantiation is registered twice"
    assert len(reg) >= 64
    table = [(c.family, c.key, c.rp) for c in S.CASES]
    assert len(table) == len(set(table)), "two rows of the case table select the same instantiation"
    unreachable = set(S.UNREACHABLE)
    assert not (set(table) & unreachable)
    missing = set(reg) - set(table) - unreachable
    stale = (set(table) | unreachable) - set(reg)
    assert not missing, f"registered and neither in tests/sim_kernel_cases.py nor on its UNREACHABLE list: {sorted(missing)}"
    assert not stale, f"in the case table or on UNREACHABLE and not registered: {sorted(stale)}"
    for why in S.UNREACHABLE.values():
        assert isinstance(why, str) and why.strip()


# Bellman classes of the models the table uses: the fiber-kernel registrations (C3SC_REG_FPW / FPW_BOX / FPP1 / FQ1 / FQD, the
# last three through the REG..P / REG..Q helper macros), read as text like the lines above
def _bellman_classes():
    text = {f: open(f).read() for f in glob.glob(os.path.join(CSRC, "inst_*.hip"))}
    cls = {}
    for src in text.values():
        helpers = {}  # helper macro -> model type, from "#define REG7P(RP) \ C3SC_REG_FPP1(C3SC_MODEL_CAR7D, RP, 0, Car7D) ..."
        for name, body in re.findall(r"#define\s+(REG\w+)\(RP[^)]*\)((?:.*\\\n)*.*)", src):
            m = re.search(r"C3SC_REG_F\w+\(C3SC_MODEL_\w+,\s*RP,\s*\w+,(?:\s*NWV,)?\s*([\w<>]+)\)", body)
            if m:
                helpers[name] = m.group(1)
        for name, rp in re.findall(r"^(REG\w+)\((\d+)", src, re.M):
            if name in helpers:
                cls.setdefault(helpers[name], set()).add(int(rp))
        for rp, rest in re.findall(r"^C3SC_REG_F(?:PW|PW_BOX|PP1|Q1|QD)\(C3SC_MODEL_\w+,\s*(\d+),([^)]*)\)", src, re.M):
            cls.setdefault(rest.split(",")[-1].strip(), set()).add(int(rp))
    return cls


MODEL_OF = {"lqg2d": "LqgNd<2>", "lqg6d": "LqgNd<6>", "dubins3d": "Dubins3D", "car7d": "Car7D", "cothrust6d": "Cothrust6D",
            "chain2": "Chain<2>", "chain4": "Chain<4>", "rossler3d": "Rossler3D", "tprob3d": "Tprob3D", "perch7d": "Perch7D",
            "scar4d": "Scar4D", "skid5d": "Skid5D"}


def test_case_ranks_select_their_instantiation():
    """pick_rp restated: the smallest Bellman class of the row's model at or above its largest bond rank is the row's RP"""
    cls = _bellman_classes()
    for c in S.CASES:
        model = MODEL_OF[c.name]
        assert model in cls, model
        if c.family != "stencil":
            assert c.key == model
        assert min(r for r in cls[model] if r >= max(c.ranks)) == c.rp, (c.kernel, sorted(cls[model]), c.ranks)
    for fam in ("stencil", "rollout", "ode"):  # unequal bond ranks in one row per family and dimension (D >= 3)
        for d in sorted({len(c.ngrid) for c in S.CASES if c.family == fam and len(c.ngrid) >= 3}):
            assert any(len(set(c.ranks[1:-1])) > 1 for c in S.CASES if c.family == fam and len(c.ngrid) == d), (fam, d)
    used = {n for c in S.STENCIL for n in c.ngrid}
    assert {2, 3, 5, 33, 128} <= used


# ------------------------------------------------------------------------- the reference against the oracle, on the CPU
def _oracle_stencil_full(oracle, P, w, x):
    from test_gpu_simulate import _oracle_stencil, _oracle_value

    want, ab = _oracle_stencil(oracle, P, w, x)
    if ab == 0:  # the host routine leaves entry 2d to its caller
        want[2 * w.dx] = _oracle_value(oracle, P, w, x)
    return want, ab


@pytest.mark.parametrize("signed", [False, True], ids=["synth", "signed"])
@pytest.mark.parametrize("case", S.STENCIL, ids=S.case_id)
def test_longdouble_reference_agrees_with_oracle(oracle, case, signed):
    """every (grid, ranks, boundary, obstacle) configuration and every point the GPU stencil test uses: the longdouble
    reference and the oracle's double restatement of the host code agree to TOL of Vabs, with identical flags"""
    w = S.workload(case)
    cs = S.cores(case, w, signed)
    P = oracle.Problem(w, cs)
    for m in range(w.dx):  # both sides on the same grid bits
        assert np.array_equal(P.xgrid(m), w.xgrid()[m])
    ref = R.OffgridRef(w, cs)
    X = S.stencil_points(w)
    worst, nobs = 0.0, 0
    for i, x in enumerate(X):
        V, Vabs, flag = ref.stencil(x)
        want, ab = _oracle_stencil_full(oracle, P, w, x)
        assert flag == ab, (i, x)
        nobs += flag != 0
        err = R.rel_err(want, V, Vabs)
        worst = max(worst, float(err.max()))
        assert (err <= R.TOL).all(), (i, x, want, V, Vabs)
        if not signed:
            assert np.array_equal(V, Vabs)
    if w.obstacles:
        assert nobs > 0
    print(f"{case.kernel} {'signed' if signed else 'synth'}: {len(X)} points, worst |oracle - ref| / Vabs = {worst:.2e}")


def test_reference_constelm_is_the_nearer_node():
    """CONSTELM: the reference's value is the product of the core slices at the nearer node of each cell (ties to the right)"""
    case = S.STENCIL[5]
    w = S.workload(case)
    cs = S.cores(case, w, True)
    ref = R.OffgridRef(w, cs)
    xg = w.xgrid()
    for x in S.stencil_points(w):
        v = np.ones(1, dtype=R.LD)
        for m in range(w.dx):
            g = xg[m]
            xc = min(max(x[m], g[0]), g[-1])
            d = np.abs(g - xc)
            j = int(np.argmin(d))
            if j + 1 < len(g) and d[j + 1] == d[j]:
                j += 1
            v = v @ ref.G[m][j]
        got, _ = ref.value(x, constelm=True)
        assert float(got) == pytest.approx(float(v[0]), rel=1e-15)


# --------------------------------------------------------------------------- the k_rollout_ode reference keeps its caps
@pytest.mark.parametrize("case", S.ODE, ids=S.case_id)
def test_ode_reference_drop_share(oracle, case):
    """the caps of the k_rollout_ode lock-step are conditions on the reference alone (host loop over the oracle's controller and
    its margins): at most 5 % of the start states dropped for a stage margin <= 1e-9, at least 50 % left to check"""
    n = case.opts["n"]
    for method in S.ODE_METHODS:
        w, cs, x0, rows = S.ode_reference(oracle, case, method)
        stopped = sum(r is None for r in rows)
        dropped = sum(r is not None and r[3] <= S.MARGIN_TOL for r in rows)
        checked = n - stopped - dropped
        print(f"{case.kernel} {method}: {checked} to check, {dropped} dropped ({100.0 * dropped / n:.1f} %), {stopped} start in an obstacle")
        assert dropped <= S.ODE_MAX_DROPPED * n and checked >= S.ODE_MIN_CHECKED * n
