"""The case table of the closed-loop kernels: one row per registered instantiation of k_stencil_points<D,RP>,
k_rollout<Model,RP> and k_rollout_ode<Model,RP> (c3sc_amd/csrc/inst_rollout*.hip) -- TEST INFRASTRUCTURE ONLY.

A row names the workload, the grid and the bond ranks that select the instantiation, and the string eng.last_kernel() must
then report.  The padded rank is the smallest Bellman class of the model at or above the largest bond rank (pick_rp in
c3sc_hip.hip), and the closed-loop kernels need an instantiation of exactly that padded rank (find_sim_kernel), so a row's
largest bond rank lies above the model's next smaller class; it is below the class itself wherever the class allows (11, 13,
17 for 12, 16, 20), so that the padding of the cores is exercised, and one row per family and dimension has unequal bond
ranks.  (A D = 2 train has a single bond.)

Bellman classes per model, from the C3SC_REG_FPW* / FPP1 / FQ* lines: Dubins3D 4 6 8 12 16 20; LqgNd<2> 4 8 12 20; LqgNd<6> 4 8
12 16 20; Car7D 4 10 12 16 20; Cothrust6D 4 8 10 12 16 20; Chain<2>, Chain<4> 4; Rossler3D, Tprob3D, Perch7D, Scar4D, Skid5D 4 8
12 16 20.

tests/test_sim_kernel_cases.py holds the table to the registry: registered == table + UNREACHABLE."""
from collections import namedtuple

import numpy as np

from c3sc_amd import workloads as wl

# (family, model or D, RP) of registered instantiations that no value function can select, each with the reason.  Empty: every
# closed-loop instantiation sits on a Bellman class of its model.  (The converse gap exists and is an error path, not an
# instantiation: Cothrust6D bond ranks 9 and 10 pad to the pair kernel's class 10, where no rollout is registered;
# test_gpu_simulate.py::test_last_kernel_and_unsupported_requests pins the "unsupported" answer.)
UNREACHABLE = {}

Case = namedtuple("Case", "family key rp name ngrid ranks kernel opts")


def _case(family, key, rp, name, ngrid, ranks, **opts):
    kernel = {"stencil": "k_stencil_points<%s,%d>", "rollout": "k_rollout<%s,%d>", "ode": "k_rollout_ode<%s,%d>"}[family] % (key, rp)
    assert len(ranks) == len(ngrid) + 1 and ranks[0] == 1 and ranks[-1] == 1
    return Case(family, str(key), rp, name, tuple(ngrid), tuple(ranks), kernel, opts)


def _chain(d):
    return wl.Workload(f"chain{d}", wl.MODEL_CHAIN, (float(d), 1.0, 1.0, 1.0), d, 1, (-2.0,) * d, (2.0,) * d, (9,) * d,
                       wl.uniform_ranks(d, 4), 0.1, (wl.BC_REFLECT,) * d, [], np.array([[-1.0], [0.0], [1.0]]))


def workload(case):
    w0 = _chain(int(case.name[-1])) if case.name.startswith("chain") else wl.WORKLOADS[case.name]()
    w = w0.scaled(ngrid=case.ngrid)
    w.ranks = tuple(case.ranks)
    if case.opts.get("bc") is not None:
        w.bc = tuple(case.opts["bc"])
    return w


def cores(case, w, signed=False):
    """full-rank data: wl.synth_cores (positive, 0.3 .. 0.4), or the signed class synth_cores - 0.35 whose products cancel"""
    cs = wl.synth_cores(w, seed=case.opts.get("seed", 0xC35C))
    return [c - 0.35 for c in cs] if signed else cs


def case_id(c):
    return c.kernel.replace("k_", "").replace("<", "-").replace(">", "").replace(",", "-")


# ----------------------------------------------------------------------------------------------------- k_stencil_points
# grids with unequal N per dimension, N from {2, 3, 5, 33, 128} mixed within a grid (2 <= N <= 4096 is what set_grid accepts):
# at N = 2 the bisection runs no round and a spacing spans the domain, at N = 3 the two cells share their only interior node.
# D = 2: lqg2d (reflecting); the 12 row with absorbing / periodic faces.  D = 3: dubins3d (absorbing, absorbing, periodic, an
# obstacle).  D = 6: lqg6d (reflecting) and cothrust6d (reflecting, an obstacle).  D = 7: car7d (absorbing, periodic,
# reflecting, an obstacle).
STENCIL = [
    _case("stencil", 2, 4, "lqg2d", (33, 5), (1, 3, 1)),
    _case("stencil", 2, 8, "lqg2d", (2, 128), (1, 7, 1)),
    _case("stencil", 2, 12, "lqg2d", (3, 33), (1, 11, 1), bc=(wl.BC_ABSORB, wl.BC_PERIODIC)),
    _case("stencil", 2, 20, "lqg2d", (128, 3), (1, 17, 1)),
    _case("stencil", 3, 4, "dubins3d", (33, 5, 3), (1, 3, 2, 1)),
    _case("stencil", 3, 6, "dubins3d", (21, 17, 16), (1, 5, 3, 1)),
    _case("stencil", 3, 8, "dubins3d", (2, 128, 5), (1, 7, 5, 1)),
    _case("stencil", 3, 12, "dubins3d", (128, 3, 33), (1, 11, 9, 1)),
    _case("stencil", 3, 16, "dubins3d", (5, 2, 128), (1, 13, 15, 1)),
    _case("stencil", 3, 20, "dubins3d", (33, 33, 2), (1, 17, 19, 1)),
    _case("stencil", 6, 4, "cothrust6d", (5, 3, 33, 2, 5, 9), (1, 3, 2, 3, 1, 3, 1)),
    _case("stencil", 6, 8, "lqg6d", (3, 128, 5, 2, 33, 5), (1, 5, 7, 3, 7, 2, 1)),
    _case("stencil", 6, 12, "cothrust6d", (33, 5, 2, 3, 128, 5), (1, 3, 11, 7, 9, 5, 1)),
    _case("stencil", 6, 16, "lqg6d", (5, 33, 3, 5, 2, 3), (1, 13, 5, 13, 8, 15, 1)),
    _case("stencil", 6, 20, "cothrust6d", (2, 5, 5, 33, 3, 5), (1, 17, 17, 19, 17, 17, 1)),
    _case("stencil", 7, 4, "car7d", (5, 33, 3, 2, 5, 3, 128), (1, 3, 3, 2, 3, 1, 3, 1)),
    _case("stencil", 7, 10, "car7d", (33, 5, 128, 3, 2, 5, 3), (1, 3, 9, 7, 8, 5, 9, 1)),
    _case("stencil", 7, 12, "car7d", (3, 2, 5, 33, 5, 128, 5), (1, 3, 11, 7, 12, 5, 9, 1)),
    _case("stencil", 7, 16, "car7d", (5, 5, 33, 5, 3, 2, 3), (1, 13, 5, 13, 9, 13, 4, 1)),
    _case("stencil", 7, 20, "car7d", (2, 3, 5, 5, 33, 5, 5), (1, 17, 17, 17, 13, 17, 17, 1)),
]
CONSTELM_DIMS = ("2", "3", "7")  # the D = 2, 3 and 7 rows run once more as a CONSTELM value function


def stencil_points(w, n=40, seed=17):
    """the point set of test_gpu_simulate._points (interior points, points outside the domain, on / beside / across each face,
    obstacle interiors and faces) and, where the interior / left / right tests of the stencil sit on equality: points exactly on
    grid nodes and exactly one spacing from lb and from ub (and one ulp either side of those)"""
    from test_gpu_simulate import _points

    pts = list(_points(w, n, seed))
    rng = np.random.default_rng(seed + 1)
    lo, hi = np.array(w.lb), np.array(w.ub)
    xg = w.xgrid()
    for m in range(w.dx):
        g = xg[m]
        N, h = len(g), g[1] - g[0]
        special = [g[j] for j in sorted({0, 1, N // 2, N - 2, N - 1})]
        for e in (g[0] + h, g[N - 1] - h):
            special += [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]
        for v in special:
            p = lo + (hi - lo) * rng.uniform(0.1, 0.9, w.dx)
            p[m] = v
            pts.append(p)
    for _ in range(4):  # whole grid nodes
        pts.append(np.array([xg[m][rng.integers(0, w.ngrid[m])] for m in range(w.dx)]))
    pts.append(np.array([g[0] for g in xg]))
    pts.append(np.array([g[-1] for g in xg]))
    return np.ascontiguousarray(pts, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- k_rollout
# small grids (8 .. 12 nodes per dimension for D >= 6); n trajectories x K steps; `top`: the model's top class, run twice more
# (steps_per_launch < K, and split with traj_offset)
_RO = dict(n=128, K=24)
_G3, _G2 = (21, 17, 16), (25, 23)
_G7, _G6 = (9, 8, 10, 8, 9, 11, 12), (10, 9, 8, 12, 11, 10)
ROLLOUT = [
    _case("rollout", "Dubins3D", 4, "dubins3d", _G3, (1, 3, 3, 1), wrap=True, dt=0.05, **_RO),
    _case("rollout", "Dubins3D", 6, "dubins3d", _G3, (1, 5, 4, 1), wrap=True, dt=0.05, **_RO),
    _case("rollout", "Dubins3D", 8, "dubins3d", _G3, (1, 7, 5, 1), wrap=True, dt=0.05, **_RO),
    _case("rollout", "Dubins3D", 12, "dubins3d", _G3, (1, 11, 9, 1), wrap=True, dt=0.05, **_RO),
    _case("rollout", "Dubins3D", 16, "dubins3d", _G3, (1, 13, 15, 1), wrap=True, dt=0.05, **_RO),
    _case("rollout", "Dubins3D", 20, "dubins3d", _G3, (1, 17, 19, 1), wrap=True, dt=0.05, top=True, **_RO),
    _case("rollout", "LqgNd<2>", 4, "lqg2d", _G2, (1, 3, 1), wrap=False, dt=0.02, **_RO),
    _case("rollout", "LqgNd<2>", 8, "lqg2d", _G2, (1, 7, 1), wrap=False, dt=0.02, **_RO),
    _case("rollout", "LqgNd<2>", 12, "lqg2d", _G2, (1, 11, 1), wrap=False, dt=0.02, **_RO),
    _case("rollout", "LqgNd<2>", 20, "lqg2d", _G2, (1, 17, 1), wrap=False, dt=0.02, top=True, **_RO),
    _case("rollout", "Car7D", 4, "car7d", _G7, (1, 3, 3, 2, 3, 1, 3, 1), wrap=False, dt=0.02, **_RO),
    _case("rollout", "Car7D", 10, "car7d", _G7, (1, 3, 9, 7, 8, 5, 9, 1), wrap=False, dt=0.02, **_RO),
    _case("rollout", "Car7D", 12, "car7d", _G7, (1, 3, 11, 7, 12, 5, 9, 1), wrap=False, dt=0.02, **_RO),
    _case("rollout", "Car7D", 16, "car7d", _G7, (1, 13, 5, 13, 9, 13, 4, 1), wrap=False, dt=0.02, **_RO),
    _case("rollout", "Car7D", 20, "car7d", _G7, (1, 17, 17, 17, 13, 17, 17, 1), wrap=False, dt=0.02, top=True, **_RO),
    _case("rollout", "Cothrust6D", 4, "cothrust6d", _G6, (1, 3, 2, 3, 1, 3, 1), wrap=False, dt=0.01, **_RO),
    _case("rollout", "Cothrust6D", 8, "cothrust6d", _G6, (1, 5, 7, 3, 7, 2, 1), wrap=False, dt=0.01, **_RO),
    _case("rollout", "Cothrust6D", 12, "cothrust6d", _G6, (1, 3, 11, 7, 9, 5, 1), wrap=False, dt=0.01, **_RO),
    _case("rollout", "Cothrust6D", 16, "cothrust6d", _G6, (1, 13, 5, 13, 8, 15, 1), wrap=False, dt=0.01, **_RO),
    _case("rollout", "Cothrust6D", 20, "cothrust6d", _G6, (1, 17, 17, 19, 17, 17, 1), wrap=False, dt=0.01, top=True, **_RO),
]

# ------------------------------------------------------------------------------------------------------------ k_rollout_ode
# the grids of test_gpu_integrate's smooth-core lock-step (15 nodes per dimension up to D = 4, 8 above, 9 for the chains); n
# start states, one outer step of two substeps, both methods
_ODE = dict(n=128)


def _g(d):
    return (15,) * d if d <= 4 else (8,) * d


ODE = [
    _case("ode", "Dubins3D", 4, "dubins3d", _g(3), (1, 3, 2, 1), **_ODE),
    _case("ode", "Dubins3D", 6, "dubins3d", _g(3), (1, 5, 4, 1), **_ODE),
    _case("ode", "Dubins3D", 8, "dubins3d", _g(3), (1, 7, 5, 1), **_ODE),
    _case("ode", "LqgNd<2>", 4, "lqg2d", _g(2), (1, 3, 1), **_ODE),
    _case("ode", "LqgNd<2>", 8, "lqg2d", _g(2), (1, 7, 1), **_ODE),
    _case("ode", "LqgNd<2>", 20, "lqg2d", _g(2), (1, 17, 1), **_ODE),
    _case("ode", "Chain<2>", 4, "chain2", (9,) * 2, (1, 3, 1), **_ODE),
    _case("ode", "Chain<4>", 4, "chain4", (9,) * 4, (1, 3, 4, 2, 1), **_ODE),
    _case("ode", "Rossler3D", 4, "rossler3d", _g(3), (1, 3, 2, 1), **_ODE),
    _case("ode", "Rossler3D", 8, "rossler3d", _g(3), (1, 7, 5, 1), **_ODE),
    _case("ode", "Tprob3D", 4, "tprob3d", _g(3), (1, 3, 2, 1), **_ODE),
    _case("ode", "Tprob3D", 12, "tprob3d", _g(3), (1, 11, 9, 1), **_ODE),
    _case("ode", "Perch7D", 4, "perch7d", _g(7), (1, 3, 3, 2, 3, 1, 3, 1), **_ODE),
    _case("ode", "Perch7D", 16, "perch7d", _g(7), (1, 13, 5, 13, 9, 13, 4, 1), **_ODE),
    _case("ode", "Cothrust6D", 4, "cothrust6d", _g(6), (1, 3, 2, 3, 1, 3, 1), **_ODE),
    _case("ode", "Cothrust6D", 8, "cothrust6d", _g(6), (1, 5, 7, 3, 7, 2, 1), **_ODE),
    _case("ode", "Car7D", 4, "car7d", _g(7), (1, 3, 3, 2, 3, 1, 3, 1), **_ODE),
    _case("ode", "Car7D", 10, "car7d", _g(7), (1, 3, 9, 7, 8, 5, 9, 1), **_ODE),
    _case("ode", "Scar4D", 4, "scar4d", _g(4), (1, 3, 4, 2, 1), **_ODE),
    _case("ode", "Scar4D", 20, "scar4d", _g(4), (1, 17, 19, 13, 1), **_ODE),
    _case("ode", "Skid5D", 4, "skid5d", _g(5), (1, 3, 4, 2, 3, 1), **_ODE),
    _case("ode", "Skid5D", 16, "skid5d", _g(5), (1, 13, 15, 9, 13, 1), **_ODE),
    _case("ode", "LqgNd<6>", 4, "lqg6d", _g(6), (1, 3, 2, 3, 1, 3, 1), **_ODE),
    _case("ode", "LqgNd<6>", 8, "lqg6d", _g(6), (1, 5, 7, 3, 7, 2, 1), **_ODE),
]
ODE_DT_OUT = 0.02
ODE_METHODS = ("forward-euler", "rk4")
MARGIN_TOL = 1e-9      # states with a controller margin at or below it are dropped / may differ in the control
ODE_MAX_DROPPED = 0.05  # of n, per (case, method)
ODE_MIN_CHECKED = 0.5

CASES = STENCIL + ROLLOUT + ODE


def ode_reference(oracle, case, method):
    """the reference side of the k_rollout_ode lock-step, all on the CPU: per start state None (inside an obstacle: nothing to
    integrate) or (end state, first control, cost, smallest stage margin) of test_gpu_integrate._host_loop over the oracle's
    controller.  Returns (w, cores, x0, rows)."""
    from test_gpu_integrate import _host_loop, _oracle_ctl
    from test_gpu_simulate import _margins, _oracle_fns, _x0

    w = workload(case)
    cs = cores(case, w)
    P = oracle.Problem(w, cs)
    fn = _oracle_fns(oracle, w)
    margin = _margins(oracle, w, cs)
    wrap = any(b == wl.BC_PERIODIC for b in w.bc)
    ctl = _oracle_ctl(oracle, P, w, wrap)
    x0 = _x0(w, case.opts["n"], 41)
    rows = []
    for x in x0:
        if P.bound.in_obstacle(x) == 1:
            rows.append(None)
            continue
        traj, U, J, mins = _host_loop(fn, ctl, x, 1, ODE_DT_OUT, ODE_DT_OUT / 2, w.discount, method, margin=margin)
        rows.append((traj[-1], U[0], J, float(mins[-1])))
    return w, cs, x0, rows
