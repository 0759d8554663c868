"""A first-value-stays model of the device node memo, and the step-level cases that hold the memo to it -- numpy only.

The device-resident cross iteration keeps a node memo (memo_merge in kernel_common.hpp, the epilogue of k_fiber_per_wave,
k_cross_memo / k_cross_memo_rehash in cross_device.hip): an open-addressing table keyed by sweep epoch and node id in which the
first value that reaches a node stays.  Under consistent ends with ONE value function a hit returns what the lane would have
computed anyway, so nothing of the memo shows.  It shows when
  the value function changes inside an epoch   (a hit must return T_A although the lane computed T_B),
  the ends are literal                         (a node's value depends on the direction of the fiber that reached it first),
  the policy value function changes inside a policy iteration (a hit must keep the first greedy candidate).

MemoProblem / PolicyMemoProblem wrap the oracle (anything with .w and .bellman_fibers) in a dict, node id -> first value, and
are what cross_reference.check_iteration and simulate_iteration take in place of the plain oracle: both only call those two
members, in the device's own order of core steps (left-to-right 0 .. d-1, right-to-left d-1 .. 0; a list asked for twice is one
batch whose second reading is all hits).  One batch never holds a node twice (distinct tuples, one varying dimension), so
within a batch the order of the merge does not matter.

SimDevice is the numpy stand-in for cross_device_lib.DeviceCross with the same methods: the restated iteration
(simulate_iteration(restatement=True)) over a model of its own, with the table's capacity, growth, epochs and their wrap, and
the policy tag.  The scenario_* functions below are the cases, written once against that interface: tests/test_gpu_cross_memo.py
runs them on the MI355X, tests/test_cross_memo_model.py on SimDevice -- clean, and with one mistake planted at a time (FAULTS).
"""
from __future__ import annotations

import os

import numpy as np

import cross_reference as cr
import cross_singular_cases as sc
import fiber_kernel_cases as fk
from c3sc_amd import workloads as wl

AUTO, PAIR, QUAD = 0, 3, 4                      # C3SC_VARIANT_*
FAMILY = {AUTO: "fiber_per_wave", PAIR: "fiber_pair", QUAD: "fiber_quad"}  # what c3sc_hip_last_kernel must name
C3SC_ERR_UNSUPPORTED = 3
POLICY_NEEDS_PER_WAVE = "the policy pass needs the fiber-per-wave kernel"
EPOCH_MAX = 0x7FFF                              # the key's 15-bit epoch field, all ones
SEE_TOL = 1e-9                                  # of the scale: a hit whose stored value differs from the current one by more
TWO_VALUE_TOL, POLICY_TOL = 1e-3, 1e-6          # admission thresholds of the cases, of the scale
GAP_TOL = 1e-9                                  # of the scale: best and second-best Q of the policy value function (argmin ties
                                                # are unpinned)


class CaseRefused(AssertionError):
    """a case that does not meet its admission condition: nothing could be seen with it"""


def node_ids(w, k, idx):
    """[F, N_k] mixed-radix ids of the nodes of the fibers idx along k, the strides check_iteration and cross_setup use"""
    d, N = w.dx, list(w.ngrid)
    strides = np.ones(d, dtype=np.int64)
    for m in range(d - 2, -1, -1):
        strides[m] = strides[m + 1] * N[m + 1]
    fixed = np.array(idx, dtype=np.int64)
    fixed[:, k] = 0
    return (fixed @ strides)[:, None] + np.arange(N[k], dtype=np.int64)[None, :] * strides[k]


class MemoProblem:
    """First value stays.  `problem` may be switched between iterations without clearing the dict (value function A, then B, in
    one epoch: switch), the dict is cleared for a new epoch (new_epoch).  Counts: stores, hits, and per hit the difference between
    the stored and the current value relative to the batch's scale (hit_diffs; differing(tol) counts those above tol);
    conflicts: the distinct nodes with a hit that differs by more than SEE_TOL."""

    def __init__(self, problem, memo=None, capacity=None):
        self.problem, self.w = problem, problem.w
        self.memo = {} if memo is None else memo
        self.capacity = capacity      # None: unbounded; else a miss is stored only while fewer entries are held (a full table)
        self.stores = self.hits = 0
        self.overflow = 0
        self.hit_diffs, self.conflicts = [], set()

    def switch(self, problem):
        self.problem = problem

    def new_epoch(self):
        self.memo.clear()

    def stored_ids(self):
        return np.array(sorted(self.memo), dtype=np.int64)

    def differing(self, tol):
        return int(np.sum(np.asarray(self.hit_diffs) > tol))

    # the one place a planted mistake overrides
    def lookup(self, node, own):
        """(value returned, hit) for a node whose lane computed `own`"""
        if node in self.memo:
            return self.memo[node], True
        if self.capacity is None or len(self.memo) < self.capacity:
            self.memo[node] = own
            self.stores += 1
        else:
            self.overflow = 1
        return own, False

    def bellman_fibers(self, k, idx):
        vals, ui, ab = self.problem.bellman_fibers(k, idx)
        ids = node_ids(self.w, k, idx)
        scale = float(np.abs(vals).max())
        out = vals.copy()
        for f in range(vals.shape[0]):
            for j in range(vals.shape[1]):
                node, own = int(ids[f, j]), float(vals[f, j])
                had = self.memo.get(node)
                out[f, j], hit = self.lookup(node, own)
                if hit:
                    self.hits += 1
                    diff = abs(had - own) / scale
                    self.hit_diffs.append(diff)
                    if diff > SEE_TOL:
                        self.conflicts.add(node)
        return out, ui, ab


class _ConsistentOracle:
    """fiber_kernel_cases.q_table builds oracle.Problem(w, cores): the same with the end-point rule of the case"""

    def __init__(self, oracle, consistent_ends):
        self.Problem = lambda w, cores: oracle.Problem(w, cores, consistent_ends=consistent_ends)


class PolicyMemoProblem:
    """The policy memo (memo_mode == 1 in the epilogue of k_fiber_per_wave is the authority): per live, non-absorbed node the
    greedy candidate index of the POLICY value function, first one stays for the whole policy iteration; the value returned is
    that candidate's backup on the context's OWN value function (a gather from fiber_kernel_cases.q_table).  Absorbed and obstacle
    nodes keep the oracle's value and are never stored.  Every batch is admitted only if best and second-best Q of the policy
    value function differ by GAP_TOL of the scale at every node that is stored.  Counts: stores, hits, policy_differing = hits
    whose stored candidate is not the current greedy one while the two Q entries differ by more than POLICY_TOL of the scale."""

    def __init__(self, oracle, w, value_cores, policy_cores, consistent_ends=True, memo=None):
        assert w.ncand <= fk.MAX_CANDS, f"{w.ncand} candidates: at most {fk.MAX_CANDS}"
        self.oracle, self.w, self.ce = oracle, w, consistent_ends
        self.shim = _ConsistentOracle(oracle, consistent_ends)
        self.value_cores = value_cores
        self.value = oracle.Problem(w, value_cores, consistent_ends=consistent_ends)
        self.set_policy(policy_cores)
        self.memo = {} if memo is None else memo
        self.stores = self.hits = self.policy_differing = 0
        self.live = set()  # every live, non-absorbed node seen since the last new_tag

    def set_policy(self, policy_cores):
        self.policy_cores = policy_cores
        self.policy = self.oracle.Problem(self.w, policy_cores, consistent_ends=self.ce)

    def new_tag(self):
        self.memo.clear()
        self.live = set()

    def candidate(self, node, greedy):
        """(candidate index used, hit) -- the one place a planted mistake overrides"""
        if node in self.memo:
            return self.memo[node], True
        self.memo[node] = greedy
        self.stores += 1
        return greedy, False

    def bellman_fibers(self, k, idx):
        own, _, _ = self.value.bellman_fibers(k, idx)
        _, greedy, ab = self.policy.bellman_fibers(k, idx)
        Q, _ = fk.q_table(self.shim, self.w, self.value_cores, k, idx)
        Qp, _ = fk.q_table(self.shim, self.w, self.policy_cores, k, idx)
        ids = node_ids(self.w, k, idx)
        free = ab == 0
        if self.w.ncand > 1 and np.any(free):
            srt = np.sort(Qp, axis=-1)
            gap = float(((srt[..., 1] - srt[..., 0])[free]).min() / np.abs(Qp).max())
            if not gap >= GAP_TOL:
                raise CaseRefused(f"core step {k}: best and second-best Q of the policy value function are {gap:.3e} of the scale "
                                  f"apart at a stored node: the greedy candidate is not pinned, the case is refused")
        scale = float(np.abs(Q).max())
        out = own.copy()
        uidx = greedy.copy()
        for f in range(own.shape[0]):
            for j in range(own.shape[1]):
                if not free[f, j]:
                    continue
                node, g = int(ids[f, j]), int(greedy[f, j])
                self.live.add(node)
                c, hit = self.candidate(node, g)
                out[f, j], uidx[f, j] = Q[f, j, c], c
                if hit:
                    self.hits += 1
                    if c != g and abs(Q[f, j, c] - Q[f, j, g]) > POLICY_TOL * scale:
                        self.policy_differing += 1
        return out, uidx, ab


# ------------------------------------------------------------------------------------------------ the cases
# value rank 4, tuples from cross_singular_cases.seeded_tuples with default_rng(seed) (left sets first, any tuples: only the warm
# hint of the first iteration), A = synth_cores(w), B = 3 synth_cores(w, seed=0xBEEF) core by core
TWO_VALUE_CASES = [  # consistent ends; J off the absorbing faces
    ("dubins3d-12-13-9", "dubins3d", (12, 13, 9), (1, 5, 5, 1), 7),
    ("car7d-7", "car7d", (7,) * 7, (1, 4, 5, 5, 5, 5, 4, 1), 7),
]
LITERAL_CASES = [    # literal ends; two tuples of J[0] on a face, the others anywhere
    ("dubins3d-8-9-9-seed7", "dubins3d", (8, 9, 9), (1, 8, 8, 1), 7),
    ("dubins3d-8-9-9-seed11", "dubins3d", (8, 9, 9), (1, 8, 8, 1), 11),
    ("car7d-5-seed7", "car7d", (5,) * 7, (1, 5, 6, 6, 6, 6, 5, 1), 7),
]
VARIANTS = {"dubins3d": (AUTO, PAIR), "car7d": (AUTO, PAIR, QUAD)}  # the forced families registered for the model at rank 4


def _workload(name, ngrid, max_cands=None):
    w = wl.WORKLOADS[name]().scaled(ngrid=ngrid, rank=4)
    if max_cands is not None and w.ncand > max_cands:  # fiber_kernel_cases.workload's rule: evenly spread, first and last kept
        w = fk.with_cands(w, w.cands[np.unique(np.round(np.linspace(0, w.ncand - 1, max_cands)).astype(int))])
    return w


def value_b(w, seed=0xBEEF):
    return [3.0 * c for c in wl.synth_cores(w, seed=seed)]


def make_case(case, literal=False, max_cands=None):
    """(workload, A, B, ranks, I, J)"""
    _, name, ngrid, ranks, seed = case
    w = _workload(name, ngrid, max_cands)
    rng = np.random.default_rng(seed)
    d = w.dx
    I = [sc.seeded_tuples(rng, w, range(k), ranks[k], interior=False) for k in range(d)]
    if literal:
        J = [sc.seeded_tuples(rng, w, range(k + 1, d), ranks[k + 1], faces=2, interior=False) for k in range(d)]
    else:
        J = [sc.seeded_tuples(rng, w, range(k + 1, d), ranks[k + 1]) for k in range(d)]
    return w, wl.synth_cores(w), value_b(w), ranks, I, J


def same_bits(a, b):
    """cores, I and J of two fetches are bit-identical"""
    return all(x.tobytes() == y.tobytes() for part in (0, 1, 2) for x, y in zip(a[part], b[part]))


def _setup(dev, ranks, I, J, new_sweep):
    rc = dev.setup(ranks, I, J, new_sweep)
    assert rc == 0, f"cross_setup: code {rc}: {dev.err()}"


def _family(dev, variant):
    if variant is not None:
        assert FAMILY[variant] in dev.last_kernel(), f"variant {variant}: the iteration ran {dev.last_kernel()}"


def _path(variant):
    return "k_cross_memo pass" if variant in (PAIR, QUAD) else "per-wave epilogue"


# ------------------------------------------------------------------------------------------------ the scenarios
def scenario_replay(make, case, variant=None, grow=0):
    """(a) and (e): an iteration under A; `grow` doublings of the table; B uploaded; the same iteration again from the same sets
    in the same epoch.  Every node is a hit, so the second fetch is the first bit for bit and nothing is stored."""
    w, A, B, ranks, I, J = make_case(case)
    dev = make(w, A, variant=variant)
    try:
        _setup(dev, ranks, I, J, 1)
        dev.iteration()
        first = dev.fetch()
        _family(dev, variant)
        for _ in range(grow):
            dev.grow_memo()
        dev.upload_value(B)
        _setup(dev, ranks, I, J, 0)
        dev.iteration()
        second = dev.fetch()
    finally:
        dev.close()
    print(f"{case[0]} replay ({_path(variant)}, {grow} doublings): info {first[3]} then {second[3]}")
    assert first[3][0] > 0 and first[3][3] == 0, f"first iteration: info {first[3]}"
    assert same_bits(first, second), "the replay under another value function differs from the first iteration: a hit did not return the stored value"
    assert second[3][0] == 0, f"the replay stored {second[3][0]} nodes: every node was stored before"
    assert second[3][3] == 0, f"the replay reports overflow {second[3][3]}"
    return first, second


def scenario_continue_and_new_epoch(make, oracle, case, variant=None):
    """(b) and (c): A; B from the sets A's iteration returned, same epoch -- held to the model loaded with iteration 1's nodes;
    then a new epoch under B -- held to the plain oracle, full count."""
    w, A, B, ranks, I, J = make_case(case)
    dev = make(w, A, variant=variant)
    try:
        _setup(dev, ranks, I, J, 1)
        dev.iteration()
        f1 = dev.fetch()
        _family(dev, variant)
        dev.upload_value(B)
        _setup(dev, ranks, f1[1], f1[2], 0)
        dev.iteration()
        f2 = dev.fetch()
        _family(dev, variant)
        _setup(dev, ranks, f2[1], f2[2], 1)
        dev.iteration()
        f3 = dev.fetch()
    finally:
        dev.close()
    PA, PB = (oracle.Problem(w, c, consistent_ends=True) for c in (A, B))
    model = MemoProblem(PA)
    label = f"{case[0]} ({_path(variant)})"
    rep1 = cr.check_iteration(model, ranks, J, *f1, swap_tol=0.05, label=f"{label} iteration 1 under A")
    stored, hits1 = model.stored_ids(), model.hits
    model.switch(PB)
    rep2 = cr.check_iteration(model, ranks, f1[2], *f2, swap_tol=0.05, label=f"{label} iteration 2 under B, same epoch", stored=stored)
    seen = model.differing(TWO_VALUE_TOL)
    print(f"{label}: iteration 1 {rep1['nodes']} nodes, {hits1} hits; iteration 2 {rep2['nodes']} new nodes, {model.hits - hits1} hits, "
          f"{seen} with |T_A - T_B| > {TWO_VALUE_TOL} of the scale (largest {max(model.hit_diffs):.3g}); worst residual "
          f"{max(s['residual'] or 0.0 for s in rep1['steps'] + rep2['steps']):.1e}, dominance "
          f"{max(s['dominance'] for s in rep1['steps'] + rep2['steps']):.6f}, cond(A[P]) {max(s['cond'] for s in rep1['steps'] + rep2['steps']):.1e}, "
          f"core 0 {max(rep1['raw'], rep2['raw']):.1e}")
    if seen < 100:
        raise CaseRefused(f"{label}: {seen} hits whose T_A and T_B differ by more than {TWO_VALUE_TOL} of the scale, 100 wanted")
    assert f2[3][3] == 0 and f3[3][3] == 0, f"overflow reported: {f2[3]}, {f3[3]}"
    rep3 = cr.check_iteration(PB, ranks, f2[2], *f3, swap_tol=0.05, label=f"{label} new epoch under B")
    print(f"{label}: new epoch {rep3['nodes']} nodes")
    return rep1, rep2, rep3


def scenario_literal(make, oracle, case, variant=None):
    """(d): literal ends.  One iteration already reaches nodes from two directions that disagree; the first value stays.  The
    same device result must FAIL the plain literal oracle, or the pass would say nothing."""
    w, A, _, ranks, I, J = make_case(case, literal=True)
    dev = make(w, A, consistent_ends=False, variant=variant)
    try:
        _setup(dev, ranks, I, J, 1)
        dev.iteration()
        f1 = dev.fetch()
        _family(dev, variant)
    finally:
        dev.close()
    P = oracle.Problem(w, A, consistent_ends=False)
    model = MemoProblem(P)
    label = f"{case[0]} literal ({_path(variant)})"
    rep = cr.check_iteration(model, ranks, J, *f1, swap_tol=0.05, label=label, allow_deficient=True, I_in=I)
    print(f"{label}: {rep['nodes']} nodes, {model.hits} hits, {len(model.conflicts)} conflicting nodes (largest difference "
          f"{max(model.hit_diffs):.3g} of the scale); span {max(s['span'] for s in rep['steps']):.1e}, interpolation "
          f"{max(s['residual'] or 0.0 for s in rep['steps']):.1e}, max|B| {max(s['maxB'] or 0.0 for s in rep['steps']):.6f}, core 0 {rep['raw']:.1e}")
    if len(model.conflicts) < 2:
        raise CaseRefused(f"{label}: {len(model.conflicts)} conflicting nodes inside the iteration, 2 wanted")
    try:
        cr.check_iteration(P, ranks, J, *f1, swap_tol=0.05, label=label + " plain oracle", allow_deficient=True, I_in=I)
    except cr.CrossCheckError as e:
        print(f"{label}: the plain literal oracle fails as it must: {e}")
    else:
        raise AssertionError(f"{label}: the result also passes the plain literal oracle: the memo is not visible in this case")
    return rep


def scenario_overflow(make, oracle, case, slots):
    """(f): a table of `slots` < distinct nodes.  A miss probes every slot, so the overflow is raised only with every slot taken:
    exactly `slots` stores.  Values that found no room are correct fiber values.  After a doubling the replay stores the rest."""
    w, A, _, ranks, I, J = make_case(case)
    dev = make(w, A)
    try:
        _setup(dev, ranks, I, J, 1)
        dev.iteration()
        f1 = dev.fetch()
        dev.grow_memo()
        _setup(dev, ranks, I, J, 0)
        dev.iteration()
        f2 = dev.fetch()
        _setup(dev, ranks, I, J, 0)
        dev.iteration()
        f3 = dev.fetch()
    finally:
        dev.close()
    P = oracle.Problem(w, A, consistent_ends=True)
    label = f"{case[0]} overflow at {slots} slots"
    print(f"{label}: info {f1[3]}, after the doubling {f2[3]}, third {f3[3]}")
    assert f1[3][3] == 1, f"{label}: info[3] = {f1[3][3]} with {slots} slots"
    assert f1[3][0] == slots, f"{label}: {f1[3][0]} nodes stored in a table of {slots} slots that overflowed"
    assert f1[3][1] == 0, f"{label}: info[1] = {f1[3][1]}"
    rep1 = cr.check_iteration(P, ranks, J, f1[0], f1[1], f1[2], None, swap_tol=0.05, label=label)
    ids1 = rep1["stored"]
    assert len(ids1) > slots, f"{label}: the iteration holds {len(ids1)} distinct nodes only"
    assert f2[3][3] == 0, f"{label}: info[3] = {f2[3][3]} after the doubling"
    rep2 = cr.check_iteration(P, ranks, J, f2[0], f2[1], f2[2], None, swap_tol=0.05, label=label + " replay")
    ids2 = rep2["stored"]
    if all(x.tobytes() == y.tobytes() for part in (1, 2) for x, y in zip(f1[part], f2[part])):
        print(f"{label}: the replay kept the sets: {len(ids1)} distinct nodes, {len(ids1) - slots} left to store")
        assert f2[3][0] == len(ids1) - slots, f"{label}: the replay stored {f2[3][0]} nodes, {len(ids1)} - {slots} were left"
        assert same_bits(f2, f3) and f3[3][0] == 0 and f3[3][3] == 0, f"{label}: the third replay: info {f3[3]}"
    else:  # a node that found no room kept the value of each direction that reached it; now the first one stays: a last-bit pivot flip
        print(f"{label}: the replay moved the sets: bounds only")
        lo = max(len(np.setdiff1d(ids2, ids1)), len(ids2) - slots)
        hi = len(ids2) - (slots - len(np.setdiff1d(ids1, ids2)))
        assert lo <= f2[3][0] <= hi, f"{label}: the replay stored {f2[3][0]} nodes, expected {lo} .. {hi}"
    return rep1, rep2


WRAP_OTHER_SEED = 23   # the tuples of the iteration at epoch 0x7FFF: another seed, so that it visits few nodes of the first one
WRAP_STALE_NODES = 100  # admission: nodes of the iteration after the wrap that hold an epoch-1 entry of A nothing has overwritten


def scenario_epoch_wrap(make, oracle, case):
    """(g): epoch 1 under A from the case's sets; set-ups without iterations up to 0x7FFE; B at 0x7FFF (the epoch field all
    ones) from the tuples of ANOTHER seed; then the wrap, and B again from the case's sets at what is epoch 1 once more.

    The slot of a node depends on its id alone and a slot of another epoch is claimed in place, so an iteration overwrites the
    older entries of every node it visits.  The nodes of the first iteration that the one at 0x7FFF did not visit still hold
    their key (1, n) with T_A when the epoch becomes 1 again: without the clear of the wrap they are hits, T_A comes back under
    B and fewer nodes are stored.  So the iteration after the wrap is held to the plain oracle on B with the full count, and to
    a fresh context's iteration bit for bit; admitted only with WRAP_STALE_NODES such nodes.  Last, a further epoch from the
    sets of the 0x7FFF iteration reproduces that iteration bit for bit (the epoch after the wrap works like any other)."""
    w, A, B, ranks, I, J = make_case(case)
    _, _, _, _, I2, J2 = make_case(case[:4] + (WRAP_OTHER_SEED,))
    dev, fresh = make(w, A), make(w, B)
    try:
        _setup(dev, ranks, I, J, 1)
        dev.iteration()
        f0 = dev.fetch()
        seconds = dev.setup_repeat(EPOCH_MAX - 2)
        dev.upload_value(B)
        _setup(dev, ranks, I2, J2, 1)
        dev.iteration()
        R = dev.fetch()
        _setup(dev, ranks, I, J, 1)
        dev.iteration()
        W = dev.fetch()
        _setup(dev, ranks, I2, J2, 1)
        dev.iteration()
        R2 = dev.fetch()
        _setup(fresh, ranks, I, J, 1)
        fresh.iteration()
        S = fresh.fetch()
    finally:
        dev.close()
        fresh.close()
    label = f"{case[0]} epoch wrap"
    print(f"{label}: {EPOCH_MAX - 2} set-ups in {seconds:.2f} s; info {f0[3]}, at 0x7FFF {R[3]}, after the wrap {W[3]}, one epoch on {R2[3]}, "
          f"a fresh context {S[3]}")
    PA, PB = (oracle.Problem(w, c, consistent_ends=True) for c in (A, B))
    ids0 = cr.check_iteration(PA, ranks, J, *f0, swap_tol=0.05, label=label + " at epoch 1 under A")["stored"]
    repR = cr.check_iteration(PB, ranks, J2, *R, swap_tol=0.05, label=label + " at epoch 0x7FFF")
    repS = cr.check_iteration(PB, ranks, J, *S, swap_tol=0.05, label=label + " a fresh context under B")
    stale = np.setdiff1d(np.intersect1d(repS["stored"], ids0), repR["stored"])
    print(f"{label}: {len(ids0)} nodes at epoch 1, {len(repR['stored'])} at 0x7FFF, {len(repS['stored'])} after the wrap, {len(stale)} of them "
          f"still hold their entry of epoch 1")
    if len(stale) < WRAP_STALE_NODES:
        raise CaseRefused(f"{label}: {len(stale)} nodes after the wrap hold an entry of epoch 1 that nothing overwrote, {WRAP_STALE_NODES} wanted")
    repW = cr.check_iteration(PB, ranks, J, *W, swap_tol=0.05, label=label + " after the wrap")
    assert same_bits(W, S) and W[3][0] == S[3][0] and W[3][3] == 0, \
        f"{label}: the iteration after the wrap differs from a fresh context's (info {W[3]} against {S[3]}): entries of an older epoch came alive"
    assert same_bits(R, R2), f"{label}: one epoch after the wrap the iteration of epoch 0x7FFF is not reproduced"
    assert R2[3][0] == R[3][0] and R2[3][3] == 0, f"{label}: info {R2[3]} one epoch after the wrap, {R[3]} at 0x7FFF"
    return repW, seconds


POLICY_CASES = [  # id, workload, grid, cross ranks, seed; V = synth_cores, P1 / P2 below
    ("dubins3d-12-13-9", "dubins3d", (12, 13, 9), (1, 5, 5, 1), 7),
    ("car7d-7", "car7d", (7,) * 7, (1, 4, 5, 5, 5, 5, 4, 1), 7),
]


POLICY_CASES_WITH_NEW_NODES = ("car7d-7",)  # dubins3d's second call moves no set: all hits


def policy_values(w):
    """P1, P2: two policy value functions whose greedy candidates differ at many nodes"""
    return value_b(w, seed=0xBEEF), value_b(w, seed=0xF00D)


def scenario_policy(make, oracle, case):
    """(h): c3sc_hip_cross_iteration_pi.  Tag 7 under P1; P2 uploaded, tag 7 again from the sets returned (stored nodes keep P1's
    candidate, new nodes take P2's); tag 8 (every node takes P2's)."""
    w, V, _, ranks, I, J = make_case(case, max_cands=fk.MAX_CANDS)
    P1, P2 = policy_values(w)
    return run_policy_scenario(make, w, V, P1, P2, ranks, I, J, PolicyMemoProblem(oracle, w, V, P1), f"{case[0]} policy",
                               new_nodes=case[0] in POLICY_CASES_WITH_NEW_NODES)


def run_policy_scenario(make, w, V, P1, P2, ranks, I, J, model, label, new_nodes=False):
    """the three calls of (h) on contexts from make(w, cores), each held to `model` -- a policy memo model under V and P1 with
    set_policy, new_tag and the counts of PolicyMemoProblem (tests/jump_policy_model.py has the one of jump mode).  new_nodes: the
    second call of tag 7 must store nodes.  The reports carry the model's counts of their call."""
    ev, pol = make(w, V), make(w, P1)
    try:
        _setup(ev, ranks, I, J, 1)
        rc = ev.iteration_pi(pol, 7)
        assert rc == 0, f"cross_iteration_pi: code {rc}: {ev.err()}"
        f1 = ev.fetch()
        _family(pol, AUTO)
        pol.upload_value(P2)
        _setup(ev, ranks, f1[1], f1[2], 0)
        rc = ev.iteration_pi(pol, 7)
        assert rc == 0, f"cross_iteration_pi: code {rc}: {ev.err()}"
        f2 = ev.fetch()
        _family(pol, AUTO)
        _setup(ev, ranks, f2[1], f2[2], 0)
        rc = ev.iteration_pi(pol, 8)
        assert rc == 0, f"cross_iteration_pi: code {rc}: {ev.err()}"
        f3 = ev.fetch()
        _family(pol, AUTO)
    finally:
        ev.close()
        pol.close()
    reps = []
    for t, (J0, got, what) in enumerate(((J, f1, "tag 7 under P1"), (f1[2], f2, "tag 7 under P2"), (f2[2], f3, "tag 8 under P2"))):
        if t == 1:
            model.set_policy(P2)
        if t == 2:
            model.new_tag()
        s0, h0, d0 = model.stores, model.hits, model.policy_differing
        rep = cr.check_iteration(model, ranks, J0, got[0], got[1], got[2], None, swap_tol=0.05, label=f"{label} {what}")
        rep["policies_stored"], rep["hits"], rep["policy_differing"] = model.stores - s0, model.hits - h0, model.policy_differing - d0
        reps.append(rep)
        print(f"{label} {what}: info {got[3]}; model {model.stores - s0} policies stored, {model.hits - h0} hits, {model.policy_differing - d0} "
              f"of them at nodes where P1 and P2 choose differently; worst residual {max(s['residual'] or 0.0 for s in rep['steps']):.1e}, "
              f"core 0 {rep['raw']:.1e}")
        assert got[3][0] == model.stores - s0, f"{label} {what}: info[0] = {got[3][0]}, the model stored {model.stores - s0} policies"
        assert got[3][1] == 0 and got[3][3] == 0, f"{label} {what}: info {got[3]}"
        if t == 1:
            hits, seen = model.hits - h0, model.policy_differing - d0
            if not (hits > 0 and seen >= 0.1 * hits):
                raise CaseRefused(f"{label}: {seen} of {hits} hits at nodes where the greedy candidate differs: 10 % wanted")
            if new_nodes and not got[3][0] > 0:  # 'new nodes take P2's' needs new nodes
                raise CaseRefused(f"{label} {what}: no new node in the second call of tag 7")
        if t == 2:
            assert got[3][0] == len(model.live), f"{label} {what}: info[0] = {got[3][0]}, {len(model.live)} live nodes"
    return reps


def scenario_policy_refuses_the_pair_kernel(make, case):
    w, V, _, ranks, I, J = make_case(case, max_cands=fk.MAX_CANDS)
    P1, _ = policy_values(w)
    ev, pol = make(w, V), make(w, P1, variant=PAIR)
    try:
        _setup(ev, ranks, I, J, 1)
        rc = ev.iteration_pi(pol, 7)
        msg = ev.err()
    finally:
        ev.close()
        pol.close()
    assert rc == C3SC_ERR_UNSUPPORTED, f"cross_iteration_pi with a forced pair kernel: code {rc} ({msg})"
    assert POLICY_NEEDS_PER_WAVE in msg, msg


# ------------------------------------------------------------------------------------------------ the numpy stand-in
FAULTS = ("no-memo", "last-value-stays", "epoch-not-cleared", "growth-drops-every-seventh", "hit-returns-next-id", "wrap-not-cleared",
          "policy-tag-not-reset")


class _FaultyMemo(MemoProblem):
    def __init__(self, problem, fault, **kw):
        super().__init__(problem, **kw)
        self.fault = fault

    def lookup(self, node, own):
        if node in self.memo:
            if self.fault == "no-memo":
                return own, True
            if self.fault == "last-value-stays":
                self.memo[node] = own
                return own, True
            if self.fault == "hit-returns-next-id":
                return self.memo.get(node + 1, own), True
        return super().lookup(node, own)


class SimDevice:
    """cross_device_lib.DeviceCross in numpy: the restated iteration over a memo model; `fault` plants one mistake (FAULTS)."""

    policy_model = PolicyMemoProblem  # bound here: a test that blinds the CHECKING model by name leaves the stand-in's own alone

    def __init__(self, oracle, w, cores, consistent_ends=True, variant=None, fault=None):
        self.oracle, self.w, self.ce, self.variant, self.fault = oracle, w, consistent_ends, variant, fault
        self.cores = cores
        self.mp = _FaultyMemo(oracle.Problem(w, cores, consistent_ends=consistent_ends), fault, capacity=0)
        self.epoch, self.tag, self.pm, self.archive = 0, None, None, {}
        self.taken = 0          # stores handed out by earlier fetches
        self.msg, self.flag = "", 0

    def err(self):
        return self.msg

    def last_kernel(self):
        return f"sim<{FAMILY[self.variant or AUTO]}>"

    def _new_epoch(self):
        """A slot of another epoch is free, but its key and value stay in the table until the node is stored again (the slot
        follows from the node id alone, and a free slot is claimed in place; two nodes in one probe chain are not modelled):
        `archive` is node -> (epoch, value) of what the slots still hold."""
        if self.fault == "epoch-not-cleared":
            self.epoch = self.epoch % EPOCH_MAX + 1
            return
        for node, value in self.mp.memo.items():
            self.archive[node] = (self.epoch, value)
        self.mp.memo.clear()
        self.epoch += 1
        if self.epoch > EPOCH_MAX:  # the wrap really clears
            self.epoch = 1
            if self.fault == "wrap-not-cleared":
                self.mp.memo.update({node: value for node, (epoch, value) in self.archive.items() if epoch == 1})
            self.archive = {}

    def setup(self, ranks, I, J, new_sweep=1):
        self.ranks, self.I, self.J = [int(r) for r in ranks], [np.array(a) for a in I], [np.array(a) for a in J]
        nodes = sum(self.ranks[k] * self.ranks[k + 1] * self.w.ngrid[k] for k in range(self.w.dx))
        want = 1 << int(os.environ.get("C3SC_MEMO_MIN_LOG2", "16"))
        while want < int(os.environ.get("C3SC_MEMO_SCALE", "32")) * nodes:
            want <<= 1
        self.mp.capacity = max(self.mp.capacity, want)
        if new_sweep or self.epoch == 0:
            self._new_epoch()
        return 0

    def setup_repeat(self, n, new_sweep=1):
        for _ in range(n):
            self.setup(self.ranks, self.I, self.J, new_sweep)
        return 0.0

    def upload_value(self, cores):
        self.cores = cores
        self.mp.switch(self.oracle.Problem(self.w, cores, consistent_ends=self.ce))

    def grow_memo(self):
        self.mp.capacity *= 2
        if self.fault == "growth-drops-every-seventh":
            for node in sorted(self.mp.memo)[::7]:
                del self.mp.memo[node]

    def _iterate(self, problem):
        ratios = []
        self.out = cr.simulate_iteration(problem, self.ranks, self.J, restatement=True, I_in=self.I, ratios=ratios)
        self.I, self.J = self.out[1], self.out[2]
        self.flag |= int(any(r <= cr.DEFICIENT_RATIO for r in ratios))

    def iteration(self):
        self._iterate(self.mp)

    def iteration_pi(self, policy, tag):
        if policy.variant in (PAIR, QUAD):
            self.msg = "cross_iteration_pi: " + POLICY_NEEDS_PER_WAVE
            return C3SC_ERR_UNSUPPORTED
        if self.pm is None:
            self.pm = self.policy_model(self.oracle, self.w, self.cores, policy.cores, self.ce)
        self.pm.set_policy(policy.cores)
        if tag != self.tag and not (self.fault == "policy-tag-not-reset" and self.tag is not None):
            self.pm.new_tag()
        self.tag = tag
        self.counted = self.pm
        self._iterate(self.pm)
        return 0

    def fetch(self):
        src = getattr(self, "counted", self.mp)
        info = [src.stores - self.taken, self.flag, 0, getattr(src, "overflow", 0)]
        self.taken, self.flag = src.stores, 0
        if src is self.mp:
            self.mp.overflow = 0
        cores, I, J = self.out
        return [np.array(c, dtype=np.float64) for c in cores], [np.array(a, dtype=np.int32) for a in I], [np.array(a, dtype=np.int32) for a in J], info

    def close(self):
        pass
