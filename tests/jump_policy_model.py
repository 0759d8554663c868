"""Policy iteration on jump diffusions at step level: a numpy stand-in for what c3sc_hip_cross_iteration_pi computes when both
contexts are in jump mode (c3sc_hip_set_jumps), and the cases that hold the device to it -- numpy only.

JumpPolicyProblem has the interface cross_reference.check_iteration and simulate_iteration take in place of the oracle (.w and
.bellman_fibers) and the rules of cross_memo_model.PolicyMemoProblem: per live node the greedy candidate of the POLICY train, the
first one stored stays for a policy tag; the value is that candidate's backup on the context's OWN train; absorbed and obstacle
nodes are never stored; a batch is refused (CaseRefused) unless best and second-best of the policy train differ by GAP_TOL of
the scale at every stored node.  The per-candidate values are backup_ref's (candidate_values with the jump terms of jump_lib.jump_terms, the
targets read from jump_lib.Train): no oracle run has a jump term.  The 2d + 1 stencil values and the flags are the oracle's
(Problem.stencil_fibers under consistent ends), which reads the grid, the boundary types and the train, and no model.

The scenario is cross_memo_model.scenario_policy's (run_policy_scenario); JumpSimDevice runs it on the CPU, clean and with one
mistake planted at a time (FAULTS); tests/test_gpu_jump_policy.py runs it on the MI355X."""
from __future__ import annotations

import dataclasses

import numpy as np

import backup_ref as BR
import cross_memo_model as mm
import cross_singular_cases as sc
import jump_lib as JL
import stop_lib as SL
from c3sc_amd import workloads as wl

FAULTS = ("policy-without-jumps", "policy-tag-not-reset")
OBSCOST = 5.0  # obscost of both LQR sources


class JumpPolicyProblem:
    """policy_jumps=False plants the first mistake: the greedy candidate is taken from the jump-free operator."""

    def __init__(self, oracle, w, host, jumps, value_cores, policy_cores, policy_jumps=True):
        self.oracle, self.w, self.host, self.jumps, self.policy_jumps = oracle, w, host, jumps, policy_jumps
        self.bcost = lambda x: SL.lqrn_terminal(w.params, x)
        self.ocost = lambda x: np.full(len(x), OBSCOST)
        self.value = oracle.Problem(w, value_cores, consistent_ends=True)
        self.value_train = JL.Train(w, value_cores)
        self.set_policy(policy_cores)
        self.memo = {}
        self.stores = self.hits = self.policy_differing = 0
        self.live = set()

    def set_policy(self, policy_cores):
        self.policy_cores = policy_cores
        self.policy = self.oracle.Problem(self.w, policy_cores, consistent_ends=True)
        self.policy_train = JL.Train(self.w, policy_cores)

    def new_tag(self):
        self.memo.clear()
        self.live = set()

    def candidate(self, node, greedy):
        if node in self.memo:
            return self.memo[node], True
        self.memo[node] = greedy
        self.stores += 1
        return greedy, False

    def q_table(self, problem, train, k, idx, with_jumps=True):
        """(Q [F, N, nc] of every candidate with the jump term, flags [F, N], x [F * N, D])"""
        w = self.w
        costs, ab = problem.stencil_fibers(k, idx)
        h2, t = BR.mca_constants(w)
        x = BR.node_states(w, k, idx).reshape(-1, w.dx)
        if with_jumps:
            jrate, J = JL.jump_terms(w, self.jumps, train, x, self.bcost, self.ocost)
        else:
            jrate, J = np.zeros(len(x)), np.zeros(len(x))
        vals, stat, _ = BR.candidate_values(self.host, w.params, x, costs.reshape(-1, 2 * w.dx + 1), np.asarray(w.cands, dtype=np.float64),
                                            h2, t, w.discount, jrate, jrate * J)
        assert not np.isnan(vals).any() and not stat.any(), "sigma > 0: no candidate is skipped"
        return vals.reshape(ab.shape + (w.ncand,)), ab, x

    def bellman_fibers(self, k, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        Q, ab, x = self.q_table(self.value, self.value_train, k, idx)
        Qp, abp, _ = self.q_table(self.policy, self.policy_train, k, idx, self.policy_jumps)
        assert np.array_equal(ab, abp)
        greedy = np.argmin(Qp, axis=-1).astype(np.int32)  # the first of equal minima
        ids = mm.node_ids(self.w, k, idx)
        free = ab == 0
        if self.w.ncand > 1 and np.any(free):
            srt = np.sort(Qp, axis=-1)
            gap = float(((srt[..., 1] - srt[..., 0])[free]).min() / np.abs(Qp).max())
            if not gap >= mm.GAP_TOL:
                raise mm.CaseRefused(f"core step {k}: best and second-best Q of the policy value function are {gap:.3e} of the scale "
                                     f"apart at a stored node: the greedy candidate is not pinned, the case is refused")
        scale = float(np.abs(Q).max())
        flat = ab.reshape(-1)
        out = np.where(flat == 1, self.bcost(x), np.where(flat == -1, self.ocost(x), 0.0)).reshape(ab.shape)
        uidx = np.full(ab.shape, -1, dtype=np.int32)
        for f in range(ab.shape[0]):
            for j in range(ab.shape[1]):
                if not free[f, j]:
                    continue
                node, g = int(ids[f, j]), int(greedy[f, j])
                self.live.add(node)
                c, hit = self.candidate(node, g)
                out[f, j], uidx[f, j] = Q[f, j, c], c
                if hit:
                    self.hits += 1
                    if c != g and abs(Q[f, j, c] - Q[f, j, g]) > mm.POLICY_TOL * scale:
                        self.policy_differing += 1
        return out, uidx, ab


# ------------------------------------------------------------------------------------------------ the cases
# id, model, value rank, cross ranks, seed of the index tuples (cross_singular_cases.seeded_tuples, left sets first);
# V = synth_cores, P1 / P2 = cross_memo_model.value_b with the seeds POLICY_SEEDS
CASES = [
    ("lqr-21x70", "lqr", 4, (1, 5, 1), 11),         # the ragged grid: absorbing and periodic dimension, the obstacle
    ("lqr3-5x16x5", "lqr3", 4, (1, 4, 4, 1), 7),    # absorbing, periodic, reflecting: a node is reached from three directions
]
# tuples of seed 11 move the sets of the 2-D case in the second call of tag 7 (75 new nodes on the stand-in; with seed 7 none); the
# 3-D case's second call moves no set with any of the seeds 7 .. 31: all hits, as for dubins3d in cross_memo_model
CASES_WITH_NEW_NODES = ("lqr-21x70",)
POLICY_SEEDS = (0xBEEF, 0xF00D)
DISCOUNT = 0.3


def workload(case, mid=0):
    if case[1] == "lqr":
        return JL.lqr_workload(mid, case[2], DISCOUNT), JL.lqr_jumps
    w = JL.lqr3_workload(mid, ranks=wl.uniform_ranks(3, case[2]), discount=DISCOUNT)
    return dataclasses.replace(w, ngrid=(5, 16, 5)), JL.lqr3_jumps


def make_case(case, mid=0):
    """(workload, numpy jump model, V, P1, P2, cross ranks, I, J)"""
    w, jumps = workload(case, mid)
    ranks, seed = case[3], case[4]
    rng = np.random.default_rng(seed)
    d = w.dx
    I = [sc.seeded_tuples(rng, w, range(k), ranks[k], interior=False) for k in range(d)]
    J = [sc.seeded_tuples(rng, w, range(k + 1, d), ranks[k + 1]) for k in range(d)]
    return w, jumps, wl.synth_cores(w), mm.value_b(w, POLICY_SEEDS[0]), mm.value_b(w, POLICY_SEEDS[1]), ranks, I, J


def scenario(make, oracle, case, mid=0):
    """cross_memo_model.scenario_policy on a jump case; make(w, cores) gives a context in jump mode"""
    w, jumps, V, P1, P2, ranks, I, J = make_case(case, mid)
    model = JumpPolicyProblem(oracle, w, SL.lqrn_host, jumps, V, P1)
    return mm.run_policy_scenario(make, w, V, P1, P2, ranks, I, J, model, f"{case[0]} jump policy",
                                  new_nodes=case[0] in CASES_WITH_NEW_NODES)


# ------------------------------------------------------------------------------------------------ the numpy stand-in
class JumpSimDevice(mm.SimDevice):
    """cross_memo_model.SimDevice whose policy pass is JumpPolicyProblem; `fault` plants one of FAULTS"""

    def __init__(self, oracle, w, cores, jumps, fault=None):
        super().__init__(oracle, w, cores, fault=fault if fault == "policy-tag-not-reset" else None)
        self.policy_model = lambda orc, ww, vc, pc, ce: JumpPolicyProblem(orc, ww, SL.lqrn_host, jumps, vc, pc,
                                                                          policy_jumps=fault != "policy-without-jumps")
