"""A numpy restatement of the approximating Markov chain (c3sc_hip_chain_transitions / c3sc_hip_simulate_chain)
-- TEST INFRASTRUCTURE ONLY.

Built from the oracle's pieces through oracle_lib, with Problem(w, cores, consistent_ends=True): the stencil of a node from
stencil_fibers, the decision and the candidates' values from bellman_fibers / q_fibers, drift, diagonal diffusion and stage cost
from the oracle's model functions, the probabilities and dt from transition_assemble (the reference's own routine).  `walk` is
this file's own loop with the Philox twin; `check` replays a run's saved nodes in lock-step from the run's own xi_s.

A node is looked up through the fiber along dimension 0 that holds it; fibers are computed once and kept.

Rules of `check`: a decision whose runner-up lies within MARGIN_TOL of the best candidate is unsure -- any candidate within the
margin is accepted and the replay goes on with the run's; a sample with |v C - c_k| <= SAMPLE_TOL C for some k is unsure in the
same way (either side of that k is accepted).  Everything else is held exactly (node, uidx, exit word) or to
TOL max(1, |.|) (J, D, T, vend, P, dt, value).
"""
import ctypes as C

import numpy as np

import oracle_lib
from c3sc_amd import workloads as wl

MARGIN_TOL = 1e-9
SAMPLE_TOL = 1e-12
TOL = 1e-12


def stuck_word(s):
    """the exit word of a walk frozen at a stuck node at step s (C3SC_CHAIN_STUCK)"""
    return -(int(s) + 2)


def neighbours(i, n, bc):
    """(lo, hi) of index i on n nodes under the fixed-dimension index rule (nodeutil.c:513-566): an absorbing face and a
    reflecting end name the node itself, the periodic seam is n - 2 / 1"""
    if i == 0:
        return (i, i) if bc == wl.BC_ABSORB else ((i, i + 1) if bc == wl.BC_REFLECT else (n - 2, i + 1))
    if i == n - 1:
        return (i, i) if bc == wl.BC_ABSORB else ((i - 1, i) if bc == wl.BC_REFLECT else (i - 1, 1))
    return i - 1, i + 1


class Node:
    __slots__ = ("ix", "flag", "V", "value", "ui", "Q", "x")


class Trans:
    __slots__ = ("ui", "stage", "dt", "P", "C", "stuck")


class ChainRef:
    def __init__(self, w, cores):
        self.w = w
        self.P = oracle_lib.Problem(w, cores, consistent_ends=True)
        self.L = oracle_lib.lib()
        self.xg = w.xgrid()
        self.h2 = self.P.h2()
        self.tvec = self.P.tvec()
        self.prm = oracle_lib.f64(list(w.params) if len(w.params) else [0.0])
        self._fibers = {}
        self._nodes = {}
        self._trans = {}

    # ---- one node
    def _fiber(self, ix):
        key = tuple(int(v) for v in ix[1:])
        f = self._fibers.get(key)
        if f is None:
            idx = np.array([[0] + list(key)], dtype=np.int32)
            V, ab_s = self.P.stencil_fibers(0, idx)
            val, ui, ab = self.P.bellman_fibers(0, idx)
            q = self.P.q_fibers(0, idx)
            assert (ab_s == ab).all()
            f = (V[0], val[0], ui[0], ab[0], None if q is None else q[0][0])
            self._fibers[key] = f
        return f

    def node(self, ix):
        key = tuple(int(v) for v in ix)
        nd = self._nodes.get(key)
        if nd is None:
            nd = self._nodes[key] = self._node(key)
        return nd

    def _node(self, ix):
        V, val, ui, ab, q = self._fiber(ix)
        j = int(ix[0])
        nd = Node()
        nd.ix = tuple(int(v) for v in ix)
        nd.flag = int(ab[j])
        nd.V = V[j]
        nd.value = float(val[j])
        nd.ui = int(ui[j])
        nd.Q = None if q is None else q[j]
        nd.x = np.array([self.xg[m][nd.ix[m]] for m in range(self.w.dx)])
        return nd

    def flag_rule(self, ix):
        """the flag by the rule itself: 1 on an absorbing face, else -1 inside an obstacle, else 0 (checked against the oracle)"""
        w = self.w
        if any(w.bc[m] == wl.BC_ABSORB and ix[m] in (0, w.ngrid[m] - 1) for m in range(w.dx)):
            return 1
        x = [self.xg[m][ix[m]] for m in range(w.dx)]
        return -1 if self.P.bound.in_obstacle(x) else 0

    def acceptable(self, nd):
        """the candidates within MARGIN_TOL of the best at a live node"""
        if nd.Q is None:
            return {nd.ui}
        best = nd.Q[nd.ui]
        return {c for c in range(self.w.ncand) if nd.Q[c] - best <= MARGIN_TOL * max(1.0, abs(best))}

    def transitions(self, nd, ui=None):
        """stage, dt and the 2d probabilities of candidate ui (default: the oracle's winner) at the live node nd"""
        ui = nd.ui if ui is None else int(ui)
        key = (nd.ix, ui)
        t = self._trans.get(key)
        if t is not None:
            return t
        w, L = self.w, self.L
        u = np.ascontiguousarray(w.cands[ui], dtype=np.float64)
        b, sg, st = np.zeros(w.dx), np.zeros(w.dx), C.c_double(0)
        assert L.orc_model_drift(w.model, oracle_lib.dp(self.prm), oracle_lib.dp(nd.x), oracle_lib.dp(u), oracle_lib.dp(b)) == 0
        assert L.orc_model_diff_diag(w.model, oracle_lib.dp(self.prm), oracle_lib.dp(nd.x), oracle_lib.dp(u), oracle_lib.dp(sg)) == 0
        assert L.orc_model_stage(w.model, oracle_lib.dp(self.prm), oracle_lib.dp(nd.x), oracle_lib.dp(u), C.byref(st)) == 0
        res, prob, dt, _, _ = oracle_lib.transition_assemble(w.dx, w.du, w.dw, self.h2, self.tvec, b, np.diag(sg).ravel())
        t = Trans()
        t.ui, t.stage, t.stuck = ui, st.value, res != 0
        t.dt = 0.0 if t.stuck else dt
        t.P = np.zeros(2 * w.dx) if t.stuck else prob[:2 * w.dx].copy()
        t.C = 0.0 if t.stuck else self.h2 / dt
        self._trans[key] = t
        return t

    def move(self, ix, k, fault=None):
        m, side = k >> 1, k & 1
        n, bc = self.w.ngrid[m], self.w.bc[m]
        nb = neighbours(ix[m], n, bc)
        if fault == "seam_swap" and bc == wl.BC_PERIODIC and ix[m] in (0, n - 1):
            nb = (nb[1], nb[0])
        out = list(ix)
        out[m] = nb[side]
        return tuple(out)

    @staticmethod
    def pick(v, P, fault=None):
        """(outcome, unsure): the first k with v < c_k (c = the running sum of P; v C < c_k C), else the last k with P_k > 0"""
        order = list(range(len(P)))
        if fault == "swap_order":
            order = [k ^ 1 for k in order]
        cum, out, unsure = 0.0, -1, False
        for k in order:
            cum += P[k]
            unsure = unsure or abs(v - cum) <= SAMPLE_TOL
            hit = (v <= cum) if fault == "le_sampler" else (v < cum)
            if out < 0 and hit:
                out = k
        if out < 0:
            out = max(k for k in order if P[k] > 0.0)
        return out, unsure

    def uniforms(self, seed, traj0, n, nsteps):
        """the Philox twin: u0 of c3sc_hip_jump_uniforms(seed, traj0 + i, s)"""
        from c3sc_amd import engine

        return np.array([[engine.jump_uniforms(seed, traj0 + i, s)[0] for s in range(nsteps)] for i in range(n)]).reshape(n, nsteps)

    # ---- the reference's own walk: a run in the layout of BellmanEngine.simulate_chain(save_every=1)
    def walk(self, node0, nsteps, uniform, fault=None):
        node0 = np.asarray(node0, dtype=np.int32)
        n, d, beta = len(node0), self.w.dx, self.w.discount
        run = {"node0": node0.copy(), "uniform": np.asarray(uniform, dtype=np.float64), "nsteps": nsteps,
               "cost": np.zeros(n), "disc": np.ones(n), "time": np.zeros(n), "vend": np.zeros(n),
               "node": np.zeros((n, d), np.int32), "exit": np.full(n, -1, np.int64),
               "traj": np.zeros((n, nsteps + 1, d), np.int32), "uidx": np.full((n, nsteps), -1, np.int32)}
        self.stats = {"unsure": 0, "steps": 0, "outcomes": set(), "selfloop": 0, "seam": 0, "alive_mid": 0}
        for i in range(n):
            ix = tuple(int(v) for v in node0[i])
            J, D, T, ex = 0.0, 1.0, 0.0, -1
            run["traj"][i, 0] = ix
            for s in range(nsteps + 1):
                nd = self.node(ix)
                flag = nd.flag
                if fault == "prec_reversed" and self.P.bound.in_obstacle(nd.x):
                    flag = -1
                if ex == -1 and flag != 0:
                    J += D * self._endcost(nd, flag)
                    ex = s
                if s == nsteps:
                    run["vend"][i] = nd.V[2 * d]
                    break
                if ex == -1:
                    t = self.transitions(nd)
                    if t.stuck:
                        ex = stuck_word(s)
                if ex == -1:
                    if s == nsteps // 2:
                        self.stats["alive_mid"] += 1
                    run["uidx"][i, s] = t.ui
                    dt = t.dt
                    if fault == "dt_other":
                        dt = self.transitions(nd, (t.ui + 1) % self.w.ncand).dt
                    g = np.exp(-beta * dt)
                    if fault == "disc_first":
                        D *= g
                    J += D * t.stage * dt
                    T += dt
                    if fault != "disc_first":
                        D *= g
                    k, unsure = self.pick(run["uniform"][i, s], t.P, fault)
                    nx = self.move(ix, k, fault)
                    self.stats["steps"] += 1
                    self.stats["unsure"] += int(unsure) + int(len(self.acceptable(nd)) > 1)
                    self.stats["outcomes"].add(k)
                    self.stats["selfloop"] += int(nx == ix)
                    m = k >> 1
                    self.stats["seam"] += int(self.w.bc[m] == wl.BC_PERIODIC and abs(nx[m] - ix[m]) > 1)
                    ix = nx
                run["traj"][i, s + 1] = ix
            run["cost"][i], run["disc"][i], run["time"][i], run["exit"][i], run["node"][i] = J, D, T, ex, ix
        return run

    def _endcost(self, nd, flag):
        c = C.c_double(0)
        f = self.L.orc_model_boundcost if flag == 1 else self.L.orc_model_obscost
        assert f(self.w.model, oracle_lib.dp(self.prm), oracle_lib.dp(nd.x), C.byref(c)) == 0
        return c.value

    # ---- lock-step replay of a run from its own nodes
    def check(self, run, strict=False):
        """Replays every lane from run["traj"] (save_every = 1) and returns {"unsure": .., "steps": ..}; raises AssertionError
        at the first difference.  strict: no sample is unsure (for runs whose uniforms sit exactly on a c_k)."""
        n, nsteps, d, beta = len(run["node0"]), run["nsteps"], self.w.dx, self.w.discount
        traj, uidx, unif = np.asarray(run["traj"]), np.asarray(run["uidx"]), np.asarray(run["uniform"])
        assert traj.shape == (n, nsteps + 1, d) and uidx.shape == (n, nsteps)
        unsure_n = steps = 0

        def close(a, b, what, i):
            assert abs(a - b) <= TOL * max(1.0, abs(b)), f"lane {i}: {what} {a!r} != {b!r}"

        for i in range(n):
            assert tuple(traj[i, 0]) == tuple(run["node0"][i]), f"lane {i}: row 0 is not the start node"
            J, D, T, ex = 0.0, 1.0, 0.0, -1
            for s in range(nsteps + 1):
                ix = tuple(int(v) for v in traj[i, s])
                nd = self.node(ix)
                assert nd.flag == self.flag_rule(ix)
                if ex == -1 and nd.flag != 0:
                    J += D * self._endcost(nd, nd.flag)
                    ex = s
                if s == nsteps:
                    close(run["vend"][i], nd.V[2 * d], "vend", i)
                    break
                t = None
                if ex == -1:
                    ok = self.acceptable(nd)
                    ui = int(uidx[i, s])
                    if ui not in ok and self.transitions(nd).stuck:
                        ex = stuck_word(s)
                    else:
                        assert ui in ok, f"lane {i} step {s}: candidate {ui}, the reference accepts {sorted(ok)}"
                        unsure_n += int(len(ok) > 1)
                        t = self.transitions(nd, ui)
                        if t.stuck:
                            ex = stuck_word(s)
                if ex != -1:
                    assert uidx[i, s] == -1, f"lane {i} step {s}: a frozen lane reports candidate {uidx[i, s]}"
                    assert tuple(traj[i, s + 1]) == ix, f"lane {i} step {s}: a frozen lane moved"
                    continue
                steps += 1
                J += D * t.stage * t.dt
                T += t.dt
                D *= np.exp(-beta * t.dt)
                k, unsure = self.pick(unif[i, s], t.P)
                unsure = unsure and not strict
                nxt = tuple(int(v) for v in traj[i, s + 1])
                if unsure:
                    unsure_n += 1
                    c = np.concatenate(([0.0], np.cumsum(t.P)))  # outcome kk owns [c_kk, c_kk+1): every owner within the tolerance
                    allowed = {self.move(ix, kk) for kk in range(2 * d)
                               if t.P[kk] > 0.0 and c[kk] - SAMPLE_TOL <= unif[i, s] <= c[kk + 1] + SAMPLE_TOL} | {self.move(ix, k)}
                    assert nxt in allowed, f"lane {i} step {s}: node {nxt} after an unsure sample, allowed {allowed}"
                else:
                    assert nxt == self.move(ix, k), f"lane {i} step {s}: node {nxt}, the reference moves to {self.move(ix, k)} (outcome {k})"
            close(run["cost"][i], J, "J", i)
            close(run["disc"][i], D, "D", i)
            close(run["time"][i], T, "T", i)
            assert int(run["exit"][i]) == ex, f"lane {i}: exit word {int(run['exit'][i])}, the reference has {ex}"
            assert tuple(run["node"][i]) == tuple(traj[i, nsteps]), f"lane {i}: final node"
        return {"unsure": unsure_n, "steps": steps}

    # ---- the transitions call against the reference
    def check_transitions(self, nodes, res):
        """res: the arrays of chain_transitions for `nodes`; returns the number of unsure decisions"""
        d, unsure_n = self.w.dx, 0
        for i, ixv in enumerate(np.asarray(nodes)):
            ix = tuple(int(v) for v in ixv)
            nd = self.node(ix)
            assert int(res["flag"][i]) == nd.flag == self.flag_rule(ix), f"node {ix}: flag"
            assert abs(res["value"][i] - nd.value) <= TOL * max(1.0, abs(nd.value)), f"node {ix}: value {res['value'][i]!r} != {nd.value!r}"
            ui = int(res["uidx"][i])
            if nd.flag != 0 or self.transitions(nd).stuck and ui == -1:
                assert ui == -1 and res["dt"][i] == 0.0 and (res["P"][i] == 0.0).all(), f"node {ix}: a node the chain does not leave"
                if nd.flag != 0:
                    assert res["stage"][i] == res["value"][i]
                continue
            ok = self.acceptable(nd)
            assert ui in ok, f"node {ix}: candidate {ui}, the reference accepts {sorted(ok)}"
            unsure_n += int(len(ok) > 1)
            t = self.transitions(nd, ui)
            assert abs(res["stage"][i] - t.stage) <= TOL * max(1.0, abs(t.stage)), f"node {ix}: stage"
            assert abs(res["dt"][i] - t.dt) <= TOL * max(1.0, abs(t.dt)), f"node {ix}: dt"
            assert np.abs(res["P"][i] - t.P).max() <= TOL, f"node {ix}: P"
            assert (res["P"][i] >= 0.0).all() and abs(res["P"][i].sum() - 1.0) <= 4e-16 * 2 * d
        return unsure_n

    def reference_transitions(self, nodes):
        """the reference's own answer in chain_transitions' layout"""
        nodes = np.asarray(nodes, dtype=np.int32)
        n, d = len(nodes), self.w.dx
        res = {"uidx": np.full(n, -1, np.int32), "value": np.zeros(n), "stage": np.zeros(n), "dt": np.zeros(n),
               "P": np.zeros((n, 2 * d)), "flag": np.zeros(n, np.int32)}
        for i, ix in enumerate(nodes):
            nd = self.node(ix)
            res["flag"][i], res["value"][i], res["stage"][i] = nd.flag, nd.value, nd.value
            if nd.flag == 0:
                t = self.transitions(nd)
                res["stage"][i] = t.stage
                if not t.stuck:
                    res["uidx"][i], res["dt"][i], res["P"][i] = t.ui, t.dt, t.P
        return res
