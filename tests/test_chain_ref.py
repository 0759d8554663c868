"""The numpy restatement of the approximating Markov chain (tests/chain_ref.py) on its own, no GPU: the reference keeps its
caps on every case of tests/chain_cases.py, `check` rejects planted faults, the Bellman identity holds at every live node, and on
the 2-D case the walk's certificate agrees with the exact policy cost from a linear solve over the whole grid."""
import numpy as np
import pytest

import chain_cases as cc
import chain_ref
from c3sc_amd import workloads as wl

MAX_UNSURE = 0.025


@pytest.fixture(scope="module")
def refs(oracle):
    made = {}

    def get(case, beta, signed):
        key = (cc.case_id(case), beta, signed)
        if key not in made:
            w = cc.workload(case, beta)
            R = chain_ref.ChainRef(w, cc.cores(case, w, signed))
            node0 = cc.start_nodes(w)
            unif = np.random.default_rng(cc.SEED + 2).random((len(node0), cc.NSTEPS))
            made[key] = (w, R, R.walk(node0, cc.NSTEPS, unif), dict(R.stats))
        return made[key]

    return get


def _grid(case):
    return [(case, b, s) for b in cc.discounts(case) for s in (False, True)]


ALL = [p for c in cc.CASES for p in _grid(c)]
IDS = [f"{cc.case_id(c)}-beta{b}-{'signed' if s else 'positive'}" for c, b, s in ALL]


@pytest.mark.parametrize("case,beta,signed", ALL, ids=IDS)
def test_reference_keeps_its_caps(refs, case, beta, signed):
    w, R, run, st = refs(case, beta, signed)
    n = len(run["node0"])
    assert st["unsure"] <= MAX_UNSURE * st["steps"], st
    assert st["outcomes"] == set(range(2 * w.dx)), sorted(st["outcomes"])
    assert st["alive_mid"] >= n / 2, st
    if wl.BC_REFLECT in w.bc:
        assert st["selfloop"] >= 1
    if wl.BC_PERIODIC in w.bc:
        assert st["seam"] >= 1
    if wl.BC_ABSORB in w.bc:
        flags = np.array([R.node(run["traj"][i, e]).flag for i, e in enumerate(run["exit"]) if e >= 0])
        assert (flags == 1).any() and (flags == -1).any(), "an absorbing exit and an obstacle exit"
    out = R.check(run)  # the reference's own run passes its own replay
    assert out["steps"] == st["steps"]


@pytest.mark.parametrize("case", [cc.CASES[0], cc.CASES[2]], ids=cc.case_id)
def test_identity_and_probabilities(refs, case):
    """value = stage dt + exp(-beta dt) sum_k P_k V_k at every live node (the residue 1 - sum P multiplies the node's own value,
    as in bellmanrhs), P >= 0 and sums to 1"""
    for beta in cc.discounts(case):
        w, R, _, _ = refs(case, beta, False)
        for ix in cc.all_nodes(w):
            nd = R.node(ix)
            assert nd.flag == R.flag_rule(ix)
            if nd.flag != 0:
                continue
            t = R.transitions(nd)
            assert (t.P >= 0.0).all() and abs(t.P.sum() - 1.0) <= 1e-14
            rhs = t.stage * t.dt + np.exp(-beta * t.dt) * (t.P @ nd.V[:2 * w.dx] + (1.0 - t.P.sum()) * nd.V[2 * w.dx])
            assert abs(nd.value - rhs) <= 1e-12 * max(1.0, abs(rhs)), (tuple(ix), nd.value, rhs)
            for m in range(w.dx):  # the stencil is the function train at the index rule's neighbours
                lo, hi = chain_ref.neighbours(int(ix[m]), w.ngrid[m], w.bc[m])
                for side, j in ((0, lo), (1, hi)):
                    y = list(ix)
                    y[m] = j
                    assert abs(nd.V[2 * m + side] - R.node(y).V[2 * w.dx]) <= 1e-12 * max(1.0, abs(nd.V[2 * m + side]))


FAULTS = ["swap_order", "dt_other", "disc_first", "seam_swap", "prec_reversed"]


@pytest.mark.parametrize("fault", FAULTS)
def test_check_rejects_planted_faults(refs, fault):
    case = cc.CASES[2]  # dubins3d: a periodic seam, a face-and-obstacle line
    beta = 0.1
    w, R, run, _ = refs(case, beta, False)
    bad = R.walk(run["node0"], cc.NSTEPS, run["uniform"], fault=fault)
    with pytest.raises(AssertionError):
        R.check(bad)


def test_check_rejects_the_wrong_comparison_on_ties(refs):
    """uniforms exactly on a cumulative probability: '<' moves on to the next outcome, '<=' does not; a strict replay tells"""
    case = cc.CASES[0]
    w, R, run, _ = refs(case, 0.1, False)
    node0 = run["node0"][:32]
    unif = np.zeros((32, 1))
    for i, ix in enumerate(node0):
        t = R.transitions(R.node(ix))
        unif[i, 0] = np.cumsum(t.P)[i % (2 * w.dx - 1)]
    good = R.walk(node0, 1, unif)
    R.check(good, strict=True)
    bad = R.walk(node0, 1, unif, fault="le_sampler")
    with pytest.raises(AssertionError):
        R.check(bad, strict=True)


def exact_policy_cost(R, w):
    """J^pi on the whole grid of a 2-D case: (I - diag(gamma) P) J = g dt, absorbed and obstacle nodes at their cost"""
    nodes = cc.all_nodes(w)
    index = {tuple(ix): i for i, ix in enumerate(nodes)}
    n = len(nodes)
    A, b = np.eye(n), np.zeros(n)
    for i, ix in enumerate(nodes):
        nd = R.node(ix)
        if nd.flag != 0:
            b[i] = nd.value
            continue
        t = R.transitions(nd)
        g = np.exp(-w.discount * t.dt)
        b[i] = t.stage * t.dt
        for k in range(2 * w.dx):
            A[i, index[R.move(tuple(ix), k)]] -= g * t.P[k]
        A[i, i] -= g * (1.0 - t.P.sum())  # the rounding residue stays at the node
    return nodes, np.linalg.solve(A, b).reshape(w.ngrid)


def stat_problem():
    case = cc.CASES[0]
    w = cc.workload(case, 0.1)
    return case, w, cc.cores(case, w, False)


def certificate(R, w, run, Jpi):
    """per start node: (mean, standard error) of J_n + D_n J^pi(xi_n) over its lanes; an exited lane has paid everything"""
    ns = len(cc.STAT_STARTS)
    tail = np.array([Jpi[tuple(ix)] for ix in run["node"]])
    est = run["cost"] + np.where(run["exit"] == -1, run["disc"] * tail, 0.0)
    groups = [est[s::ns] for s in range(ns)]  # lane i starts at STAT_STARTS[i % ns]
    return np.array([g.mean() for g in groups]), np.array([g.std(ddof=1) / np.sqrt(len(g)) for g in groups])


def stat_start_nodes():
    return np.array([cc.STAT_STARTS[i % len(cc.STAT_STARTS)] for i in range(cc.STAT_NTRAJ)], dtype=np.int32)


def test_certificate_against_the_exact_policy_cost(oracle):
    case, w, cores = stat_problem()
    R = chain_ref.ChainRef(w, cores)
    _, Jpi = exact_policy_cost(R, w)
    node0 = stat_start_nodes()
    unif = R.uniforms(cc.STAT_SEED, 0, len(node0), cc.STAT_NSTEPS)
    run = R.walk(node0, cc.STAT_NSTEPS, unif)
    mean, se = certificate(R, w, run, Jpi)
    for s, start in enumerate(cc.STAT_STARTS):
        assert abs(mean[s] - Jpi[start]) <= 4.0 * se[s] + 1e-9, (start, mean[s], Jpi[start], se[s])
