"""The numpy restatement of one trip of k_rollout's step loop (kernel_rollout.hpp), once, for every form the rollouts are offered
in (form_offered(form, FORM_ROLLOUT): plain, game, every subset of {horizon, stop, jump}, impulse, impulse + jump) -- TEST
INFRASTRUCTURE ONLY.  It never calls the device; the Philox twins engine.normals and engine.jump_uniforms are
host functions.  The backup is not re-derived: the candidates' values and the decision are backup_ref's (game_lib.minmax for the
game), the Poisson term and the compound-Poisson increment jump_lib's, the interventions impulse_lib's, the interpolant
jump_lib.Train with offgrid_ref's neighbour rule (tests/test_rollout_ref.py pins the float64 stencil here to OffgridRef).

A form is a frozenset of "horizon", "stop", "jump", "impulse", "game": data, not code.  A Ctx carries what a call of
c3sc_hip_simulate carries: the workload, the value function (one train, or the stack V_0 .. V_N in horizon mode), the switches'
callables and the arguments of the call.

    step(form, ctx, k, x, alive)   one trip of the loop for a batch of states, in the kernel's order: exit test at x, wrap,
                                   stencil, the terms of the form at xin, the decision, the outcome of the action, the next state
    rollout(form, ctx, fault=)     the reference's own closed loop (it follows its own decisions); fault: a planted mistake, for
                                   the tests of check itself (FAULTS)
    check(form, ctx, run)          the lock-step comparison of a run's saved outputs: every step is fed the run's own x_k

ROWS is the table tests/test_gpu_rollout_forms.py runs on the device and tests/test_rollout_ref.py holds to its preconditions."""
import dataclasses
import zlib
from collections import namedtuple

import numpy as np

import backup_ref as BR
import game_lib as GL
import impulse_lib as IL
import jump_lib as JL
import stop_lib as SL
from sim_kernel_cases import MARGIN_TOL

TOL = 1e-12  # states, costs and terminal values: |got - ref| <= TOL max(1, |ref|) (jump_lib.replay's and impulse_lib.replay's callers)
FORM_NAMES = ("horizon", "stop", "jump", "impulse", "game")
# a planted mistake per name; the feature a row needs for the mistake to show (None: every row)
FAULTS = {
    "nojump": "jump_decides",    # the controller runs without the jump term
    "jump_at_x": "jump_reads_seam",  # the jump term is taken at x instead of the wrapped xin
    "jump_norule": "jump_decides",  # the jump target value ignores the obstacle / face rule
    "psi_at_x": "stop",          # psi is taken at x instead of xin
    "impulse_pays_stage": "impulse",  # an intervention step also pays the stage cost
    "impulse_at_x": "impulse",   # an intervention is applied at x instead of xin
    "stage_k": "horizon",        # the controller of step k reads stage k instead of k + 1
    "no_terminal": "horizon",    # the terminal value is missing
    "le": "stop",                # '<=' for '<' between the stop action and the scan
    "index": "impulse",          # the action index nc + m for nc + 1 + m
    "exit_after": None,          # the exit test comes after the step instead of before it
    "uniform_key": "jump",       # the uniforms are keyed by i instead of traj_offset + i
    "u_stopped": "stop",         # the saved control of a stopped lane is left non-zero
}


@dataclasses.dataclass
class Ctx:
    w: object                 # the workload (params final: psi's constant, the intervention costs)
    C: np.ndarray             # the candidate list [nc, du] (the game: product(U, W), pair order)
    host: object              # (prm, x, u) -> (drift, sigma, stage)
    bcost: object
    ocost: object
    trains: list              # [Train]: the uploaded value; horizon: V_0 .. V_N
    ranks: list               # per train: the rank list
    cores: list               # per train: the cores as uploaded
    dt: float
    N: int
    x0: np.ndarray
    wrap: bool = False
    constelm: bool = False
    seed: int = 0
    traj_offset: int = 0
    noise: object = None      # [n, N, D] given normals, or None: Philox(seed)
    jumps: object = None
    impulses: object = None
    psi: object = None
    game: object = None       # (U, W, order)
    tie_psi: bool = False     # the tests of the '<=' fault: psi equals the scan's result exactly on every other lane

    def normals(self):
        if self.noise is not None:
            return self.noise
        if getattr(self, "_xi", None) is None:
            from c3sc_amd import engine as E

            self._xi = E.normals(self.seed, self.traj_offset, len(self.x0), 0, self.N, self.w.dx)
        return self._xi


def has_feature(form, feature, spec="lqr_jd"):
    """whether a planted fault of this feature can show in a run of the form.  jump_decides: the jump term reaches the decision.
    In the explicit scheme of horizon mode every candidate's value is g delta + exp(-beta delta) (V + (delta / h^2) (PV - Q V)),
    and the jump term adds the same h2 lambda to every Q and the same h2 lambda J to every PV: a constant over the candidates.
    It moves the scan's value against psi or an intervention, never the scan's argmin, so in horizon rows without the stop action
    no output of a rollout depends on the controller's jump term (the compound-Poisson increment is another matter)"""
    if feature is None:
        return True
    if feature == "jump_reads_seam":
        # ... and the jump term differs between x and xin.  The 3-D marks are shifts with constant weights and a rate that reads
        # the reflecting coordinate, and targets are wrapped: wrap(x + d) is wrap(wrap(x) + d), so the term is the same to
        # rounding.  The 2-D model's weights and its mark 2 read the periodic coordinate.  In the impulse rows an intervention
        # is applied at xin and returns the lane into [lb, ub): too few steps see xin != x for a decision to turn on it
        return spec == "lqr_jd" and has_feature(form, "jump_decides")
    if feature == "jump_decides":
        return "jump" in form and ("horizon" not in form or "stop" in form)
    return feature in form


def make_form(*names):
    f = frozenset(names)
    assert f <= set(FORM_NAMES), names
    return f


# ---------------------------------------------------------------------------------------------------- the pieces of a step
def in_obstacle(w, x):
    inobs = np.zeros(len(x), dtype=bool)
    for c, wd in w.obstacles:
        lo, hi = np.array(c) - np.array(wd) / 2.0, np.array(c) + np.array(wd) / 2.0
        inobs |= np.all((x >= lo) & (x <= hi), axis=1)  # closed boxes
    return inobs


def beyond_faces(w, x):
    from c3sc_amd import workloads as wl

    out = np.zeros(len(x), dtype=bool)
    for m, g in enumerate(w.xgrid()):
        if w.bc[m] == wl.BC_ABSORB:
            out |= (x[:, m] < g[0]) | (x[:, m] > g[-1])
    return out


def stencil(w, tr, x, constelm=False):
    """(V [P, 2D+1], ab [P]) of offgrid_stencil at the states x [P, D] in float64: offgrid_ref.OffgridRef's neighbour rule,
    vectorised; every point is evaluated on its own by jump_lib.Train.value"""
    from c3sc_amd import workloads as wl

    P, D = x.shape
    V = np.empty((P, 2 * D + 1))
    V[:, 2 * D] = tr.value(x, constelm)
    for m in range(D):
        g = tr.g[m]
        lb, ub, h, xm = g[0], g[-1], g[1] - g[0], x[:, m]
        interior = ((xm + h) < ub) & ((xm - h) > lb)
        left = ~interior & ((xm - h) <= lb)
        right = ~interior & ~left
        if w.bc[m] == wl.BC_PERIODIC:
            yl_b = np.where(xm > lb, ub - (h - (xm - lb)), (ub - (lb - xm)) - h)
            yr_b = np.where(xm < ub, lb + (h - (ub - xm)), (lb + (xm - ub)) + h)
        else:
            yl_b, yr_b = np.full(P, lb), np.full(P, ub)
        for e, y in ((0, np.where(left, yl_b, xm - h)), (1, np.where(right, yr_b, xm + h))):
            p = np.array(x, dtype=np.float64)
            p[:, m] = y
            V[:, 2 * m + e] = tr.value(p, constelm)
    inobs = in_obstacle(w, x)
    V[inobs] = V[inobs, 2 * D][:, None]
    return V, np.where(inobs, -1, 0)


Step = namedtuple("Step", "gone inobs xin ui margin near act u pay xnext stopped iv mark alive cfl")


def step(form, ctx, k, x, alive, fault=None, act=None):
    """one trip of k_rollout's loop at the states x [n, D]; alive [n]: the lanes still running before it.  act [n]: the action
    to apply in place of the decision (check's accepted one).  Returns a Step: gone / inobs (the exit test's verdict), xin, the
    decision ui with its margin and the actions within MARGIN_TOL of the best, near [n, nc + 1 + M] (column = action index; the game: [n, nc]),
    the action applied, the saved control row u, the discounted amount paid in this step, the next state, who stopped, who
    intervened, the jump mark of the step (-1: none) and the lanes still running after it"""
    w, C, n = ctx.w, ctx.C, len(x)
    nc, beta, dt = len(C), w.discount, ctx.dt
    disc = np.exp(-beta * (k * dt))
    # 1. the exit test at x itself: the obstacle first, then the absorbing faces
    inobs, out = in_obstacle(w, x), beyond_faces(w, x)
    gone = alive & (inobs | out)
    if fault == "exit_after":
        gone = np.zeros(n, dtype=bool)
    pay = np.where(gone, disc * np.where(inobs, ctx.ocost(x), ctx.bcost(x)), 0.0)
    live = alive & ~gone
    # 2. the state the controller sees
    xin = JL.wrap(w, x) if ctx.wrap else x
    # 3. the stencil of the value function the controller reads
    stage = 0
    if "horizon" in form:
        stage = k if fault == "stage_k" else k + 1
    tr = ctx.trains[stage]
    V, ab = stencil(w, tr, xin, ctx.constelm)
    # 4. the terms of the form
    h2, t = BR.mca_constants(w)
    q0 = pv0 = c = psi = None
    if "jump" in form and fault != "nojump":
        xj = x if fault == "jump_at_x" else xin
        if fault == "jump_norule":
            lam, pi, y = ctx.jumps(w.params, xj)
            q0, J = h2 * lam, np.zeros(n)
            for m in range(pi.shape[1]):
                J = J + pi[:, m] * tr.value(JL.wrap(w, y[:, m]), ctx.constelm)
        else:
            q0, J = JL.jump_terms(w, ctx.jumps, tr, xj, ctx.bcost, ctx.ocost, ctx.constelm)
        pv0 = q0 * J
    if "impulse" in form:
        c = IL.impulse_values(w, ctx.impulses, tr, xin, ctx.bcost, ctx.ocost, ctx.constelm)
    # 5. the decision
    vals, _, cfl = BR.candidate_values(ctx.host, w.params, xin, V, C, h2, t, beta, q0, pv0, dt if "horizon" in form else None)
    xpsi = x if fault == "psi_at_x" else xin
    if "stop" in form:
        psi = ctx.psi(xpsi)
        if ctx.tie_psi:
            cont = np.where(np.isnan(vals), np.inf, vals).min(axis=1)
            psi = np.where(np.arange(n) % 2 == 0, cont, psi)
    if "game" in form:
        U, W, order = ctx.game
        best, ui, mg = GL.minmax(vals.reshape(n, len(U), len(W)), order)
        allv = np.where(np.isnan(vals), np.inf, vals)
        near = np.abs(allv - best[:, None]) <= MARGIN_TOL * np.maximum(1.0, np.abs(best))[:, None]
    else:
        best, ui, mg = BR.backup(vals, psi, c, fault=fault if fault in ("index", "le") and c is not None else None)
        if fault == "le" and psi is not None:
            cont = np.where(np.isnan(vals), np.inf, vals).min(axis=1)
            ui = np.where(psi <= cont, nc, ui)
        M = 0 if c is None else c.shape[1]
        allv = np.full((n, nc + 1 + M), np.inf)
        allv[:, :nc] = np.where(np.isnan(vals), np.inf, vals)
        if psi is not None:
            allv[:, nc] = psi
        if c is not None:
            allv[:, nc + 1:] = c
        near = allv <= (best + MARGIN_TOL * np.maximum(1.0, np.abs(best)))[:, None]
    ui = np.where(ab != 0, -1, ui)  # the wrapped image lies inside an obstacle: no action, u = 0
    a = ui if act is None else np.where(act == -2, ui, act)
    # 6. the outcome of the action
    ar = np.arange(n)
    stopped = live & (a == nc) & ("stop" in form)
    iv = live & (a > nc) & ("impulse" in form)
    mk_iv = np.clip(a - nc - 1, 0, None)
    if fault == "index":  # the faulted kernel decodes nc + m: intervention m - 1, and nothing for nc itself
        iv = live & (a > nc)
    cont_l = live & ~stopped & ~iv
    is_c = cont_l & (a >= 0) & (a < nc)
    u = np.where(is_c[:, None], C[np.clip(a, 0, nc - 1)], 0.0)
    b, sg, stg = ctx.host(w.params, x, u)
    pay = pay + np.where(stopped, disc * (psi if psi is not None else 0.0), 0.0)
    xnext = np.array(x, dtype=np.float64)
    if "impulse" in form:
        kk, yy = ctx.impulses(w.params, x if fault == "impulse_at_x" else xin)
        mk_iv = np.clip(mk_iv, 0, kk.shape[1] - 1)
        pay = pay + np.where(iv, disc * np.where(iv, kk[ar, mk_iv], 0.0), 0.0)
        if fault == "impulse_pays_stage":
            pay = pay + np.where(iv, disc * stg * dt, 0.0)
    pay = pay + np.where(cont_l, disc * stg * dt, 0.0)
    # 7. the next state of a continuing lane
    acc = x + b * dt
    acc = acc + sg * np.sqrt(dt) * ctx.normals()[:, k]
    mark = np.full(n, -1)
    if "jump" in form:
        trajs = (0 if fault == "uniform_key" else ctx.traj_offset) + np.arange(n)
        ev, mk, inc = JL.step_jumps(w, ctx.jumps, x, ctx.seed, trajs, k, dt)
        acc = acc + inc
        mark = np.where(cont_l, mk, -1)
    if "impulse" in form:
        acc = np.where(iv[:, None], yy[ar, mk_iv], acc)
    xnext = np.where((live & ~stopped)[:, None], acc, x)
    u_saved = u
    if fault == "u_stopped":
        cbest = np.argmin(np.where(np.isnan(vals), np.inf, vals), axis=1)
        u_saved = np.where(stopped[:, None], C[cbest], u)
    alive2 = live & ~stopped
    if fault == "exit_after":  # the faulted order: the test runs on the state the step produced, under this step's index
        g2 = alive2 & (in_obstacle(w, xnext) | beyond_faces(w, xnext))
        pay = pay + np.where(g2, disc * np.where(in_obstacle(w, xnext), ctx.ocost(xnext), ctx.bcost(xnext)), 0.0)
        gone, alive2 = g2, alive2 & ~g2
    return Step(gone, inobs, xin, ui, mg, near, a, u_saved, pay, xnext, stopped, iv, mark, alive2, bool((cfl.any(axis=1) & live & (ab == 0)).any()))


def terminal(form, ctx, x, alive, fault=None):
    """the launch with s1 == nsteps: the exit test of x_N, the discounted V_N(x_N) of the lanes still running (horizon), V_end.
    Returns (gone, inobs, pay, vend)"""
    w = ctx.w
    dend = np.exp(-w.discount * (ctx.N * ctx.dt))
    inobs = in_obstacle(w, x)
    gone = alive & (inobs | beyond_faces(w, x))
    if fault == "exit_after":
        gone = np.zeros(len(x), dtype=bool)
    pay = np.where(gone, dend * np.where(inobs, ctx.ocost(x), ctx.bcost(x)), 0.0)
    xin = JL.wrap(w, x) if ctx.wrap else x
    vend = ctx.trains[ctx.N if "horizon" in form else 0].value(xin, ctx.constelm)
    if "horizon" in form and fault != "no_terminal":
        pay = pay + np.where(alive & ~gone, dend * vend, 0.0)
    return gone, inobs, pay, vend


# ---------------------------------------------------------------------------------------------------- the log of a run
class Log:
    """what happened at every step of a run: the action of every live lane (-9: not live), its margin, the jump mark, the exits"""

    def __init__(self, n, N, nc):
        self.n, self.N, self.nc = n, N, nc
        self.act = np.full((n, N), -9)
        self.margin = np.full((n, N), np.inf)
        self.mark = np.full((n, N), -1)
        self.iv = np.zeros((n, N), dtype=bool)
        self.wrapped = np.zeros((n, N), dtype=bool)
        self.exit_step = np.full(n, -1)
        self.exit_obs = np.zeros(n, dtype=bool)
        self.unsure = 0
        self.cfl = False

    def add(self, k, s, x, alive):
        self.cfl |= s.cfl
        live = alive & ~s.gone
        self.act[live, k] = s.act[live]
        self.margin[live, k] = s.margin[live]
        self.mark[:, k] = s.mark
        self.iv[:, k] = s.iv
        self.wrapped[:, k] = live & np.any(s.xin != x, axis=1)
        self.exited(k, s.gone, s.inobs)

    def exited(self, k, gone, inobs):
        self.exit_step[gone] = k
        self.exit_obs[gone] = inobs[gone]

    def counts(self):
        """checked and unsure decisions, occurrences of every action kind, jump events per mark, exits by kind"""
        nc, act = self.nc, self.act
        live = act != -9
        c = {"checked": int(live.sum()), "unsure": int(self.unsure if self.unsure else (live & (self.margin <= MARGIN_TOL)).sum()),
             "stop0": int((act[:, 0] == nc).sum()), "stop_later": int((act[:, 1:] == nc).sum()),
             "candidates": int(len(np.unique(act[(act >= 0) & (act < nc)]))),
             "impulses": [int((act == nc + 1 + m).sum()) for m in range(max(0, int(act.max()) - nc))],
             "jumps": [int((self.mark == m).sum()) for m in range(int(self.mark.max()) + 1)],
             "wrapped": int(self.wrapped.sum()), "cfl": bool(self.cfl), "alive_mid": int(live[:, self.N // 2].sum()),
             "exit_face": 0, "exit_obstacle": 0, "exit_obstacle0": 0, "exit_jump_face": 0, "exit_jump_obstacle": 0, "exit_impulse": 0}
        for i in np.nonzero(self.exit_step >= 0)[0]:
            k, obs = self.exit_step[i], self.exit_obs[i]
            if k > 0 and self.mark[i, k - 1] >= 0:
                c["exit_jump_obstacle" if obs else "exit_jump_face"] += 1
            elif k > 0 and self.iv[i, k - 1]:
                c["exit_impulse"] += 1
            else:
                c["exit_obstacle" if obs else "exit_face"] += 1
                c["exit_obstacle0"] += int(obs and k == 0)
        return c


# ---------------------------------------------------------------------------------------------------- the closed loop
def rollout(form, ctx, x0=None, fault=None):
    """the reference's own closed loop from x0 (ctx.x0): (run, log); run holds traj [n, N + 1, D], u [n, N, du], cost [n],
    exit [n] (k: exited at step k, -(k + 2): stopped at step k, -1: running), vend [n], xfinal [n, D] as simulate returns them
    with save_every = 1"""
    x = np.array(ctx.x0 if x0 is None else x0, dtype=np.float64)
    n, N = len(x), ctx.N
    traj, u = np.zeros((n, N + 1, x.shape[1])), np.zeros((n, N, ctx.C.shape[1]))
    J, ex, alive = np.zeros(n), np.full(n, -1, dtype=np.int64), np.ones(n, dtype=bool)
    log = Log(n, N, len(ctx.C))
    traj[:, 0] = x
    for k in range(N):
        s = step(form, ctx, k, x, alive, fault)
        log.add(k, s, x, alive)
        J = J + s.pay
        ex[s.gone] = k
        ex[s.stopped] = -(k + 2)
        u[:, k] = s.u
        x, alive = s.xnext, s.alive
        traj[:, k + 1] = x
    gone, inobs, pay, vend = terminal(form, ctx, x, alive, fault)
    log.exited(N, gone, inobs)
    ex[gone] = N
    return {"traj": traj, "u": u, "cost": J + pay, "exit": ex, "vend": vend, "xfinal": x}, log


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def check(form, ctx, run, strict=False):
    """the lock-step comparison of a run (rollout's dict, or simulate's with save_every = 1): at every step the run's own x_k
    goes through step.  Where the decision's margin exceeds MARGIN_TOL the run's action must be the reference's; at or below it
    the run's action is accepted if it is one of the actions within the margin, the replay goes on with it and the step counts
    as unsure.  strict: every decision must be the reference's own (a run of the same arithmetic: rollout's).  Returns
    (counts, mismatches, errors): counts as Log.counts, the list of what did not agree (empty: accepted), and the largest
    relative state, cost and V_end errors"""
    traj, u, cost, ex, vend, xfinal = (_np(run[q]) for q in ("traj", "u", "cost", "exit", "vend", "xfinal"))
    n, N, C = traj.shape[0], ctx.N, ctx.C
    nc = len(C)
    bad = []
    J, exr, alive = np.zeros(n), np.full(n, -1, dtype=np.int64), np.ones(n, dtype=bool)
    log = Log(n, N, nc)
    err = {"state": 0.0, "cost": 0.0, "vend": 0.0}

    def note(what, k, lanes):
        if lanes.any():
            bad.append(f"step {k}: {what} on lanes {np.nonzero(lanes)[0][:8].tolist()}")

    for k in range(N):
        x = traj[:, k]
        s = step(form, ctx, k, x, alive)
        live = alive & ~s.gone
        sure = live & ((s.margin > MARGIN_TOL) | strict)
        # the action the run took, as its outputs show it
        r_stop = ex == -(k + 2)
        eq = (u[:, k][:, None, :] == C[None]).all(axis=-1)
        r_act = np.where(eq.any(axis=1), eq.argmax(axis=1), -1)
        zero = (u[:, k] == 0.0).all(axis=1)
        if "impulse" in form:
            kk, yy = ctx.impulses(ctx.w.params, s.xin)
            for m in range(kk.shape[1] - 1, -1, -1):
                hit = zero & np.isfinite(kk[:, m]) & (np.abs(traj[:, k + 1] - yy[:, m]).max(axis=1) <= TOL) & s.near[:, nc + 1 + m]
                r_act = np.where(hit & (~sure | (s.ui == nc + 1 + m)), nc + 1 + m, r_act)
        r_act = np.where(r_stop, nc, r_act)
        note("the action is not the reference's", k, sure & (r_act != s.ui))
        unsure = live & ~sure
        ok = unsure & (((r_act >= 0) & s.near[np.arange(n), np.clip(r_act, 0, s.near.shape[1] - 1)]) | (r_act == s.ui))
        note("the action is not within the margin", k, unsure & ~ok)
        log.unsure += int(unsure.sum())
        acc = np.where(ok, r_act, s.ui)
        if (acc != s.ui).any():
            s = step(form, ctx, k, x, alive, act=acc)
        note("a stop decodes at another step", k, live & (r_stop != s.stopped))
        note("the saved control is not the action's row", k, ~(u[:, k] == s.u).all(axis=1))
        if "impulse" in form:
            note("an intervention's next state is not y_m(xin)", k, s.iv & (np.abs(traj[:, k + 1] - s.xnext).max(axis=1) > TOL))
        e = np.abs(traj[:, k + 1] - s.xnext) / np.maximum(1.0, np.abs(s.xnext))
        err["state"] = max(err["state"], float(e.max()))
        note("the next state differs", k, (e > TOL).any(axis=1))
        log.add(k, s, x, alive)
        J = J + s.pay
        exr[s.gone] = k
        exr[s.stopped] = -(k + 2)
        alive = s.alive
        if bad and len(bad) > 8:
            break
    if not bad:
        gone, inobs, pay, r_vend = terminal(form, ctx, traj[:, N], alive)
        log.exited(N, gone, inobs)
        exr[gone] = N
        J = J + pay
        note("exit codes differ", N, ex != exr)
        for name, got, ref in (("cost", cost, J), ("vend", vend, r_vend)):
            e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
            err[name] = float(e.max())
            note(name + " differs", N, e > TOL)
        note("xfinal differs", N, (np.abs(xfinal - traj[:, N]) > TOL * np.maximum(1.0, np.abs(traj[:, N]))).any(axis=1))
    return log.counts(), bad, err


# ---------------------------------------------------------------------------------------------------- the table
# spec: the device model of a row, by the name its source is compiled under in the neighbours' tests (one compile per process).
# SPECS[spec] = (compile arguments for engine.compile_model, without ranks); classes: the rank classes the row's model needs
def specs():
    return {
        "lqr_jd": dict(source=JL.LQR, d=2, du=2, horizon=True, stop=True, njump=JL.LQR_NJUMP, **JL.LQR_MASKS),
        "lqr3_jd": dict(source=JL.LQR3, d=3, du=3, horizon=True, stop=True, njump=JL.LQR3_NJUMP, **JL.LQR3_MASKS),
        "lqr_ic": dict(source=IL.LQR_JUMP, d=2, du=2, njump=JL.LQR_NJUMP, nimpulse=IL.LQR_NIMPULSE, **IL.LQR_MASKS),
        "lqr3_ic": dict(source=IL.LQR3, d=3, du=3, njump=JL.LQR3_NJUMP, nimpulse=IL.LQR3_NIMPULSE, **IL.LQR3_MASKS),
        "lqgame": dict(source=GL.LQGAME, d=2, du=2, game=True, **GL.LQGAME_MASKS),
    }


# the compile of a spec as its home test has it (name, ranks); lqr3_jd has no class 4 there: the rows that need it compile the
# same spec once more under the name lqr3_jd_c4 with both classes
COMPILED = {"lqr_jd": ("lqr_jd", (4, 8, 12)), "lqr3_jd": ("lqr3_jd", (12,)), "lqr3_jd_c4": ("lqr3_jd_c4", (4, 12)),
            "lqr_ic": ("lqr_ic", (4, 8, 12)), "lqr3_ic": ("lqr3_ic", (4, 12)), "lqgame": ("lqgame", (4, 8))}

Row = namedtuple("Row", "id spec model form bonds rp noise n N dt opts")
BETA = 0.3
DT2, DT2_H = 0.02, 0.01     # 2-D: the neighbours' rollout step; horizon rows: LQR_DELTA of test_gpu_jump.py, inside the CFL rule
DT3, DT3_H = 0.02, 0.004    # 3-D: LQR3_DELTA of test_gpu_jump.py in horizon rows
N2, N3, NLANES = 24, 16, 300
OFFSET = 1000               # traj_offset of every row: the uniforms' key is traj_offset + i
# psi's constant sits where about this share of the live start states stops at step 0 (psi below the continuation value there);
# the others may stop later.  In horizon rows every stage is another seeded train, so every step draws the share afresh
STOP_SHARE, STOP_SHARE_H = 0.2, 0.1
STACK_COMMON = 0.8
HORIZON_R = 0.1
LQR3_K = {12: IL.LQR3_K, 4: 0.03}  # the 3-D intervention cost scale per class: at bonds (3, 4) the train's node-to-node variation is
                                    # about 0.4 of that at (11, 9), and so is the scale at which interventions compete with the candidates
STOP_C1_H = 0.001           # psi = c0 + c1 |x|^2 in horizon rows: nearly flat.  There the jump term moves the continuation value by
                            # delta lambda (J - V) only, a few 1e-4 at most nodes, and it flips the stop decision only where psi is
                            # that close to the continuation value: with the model's c1 = 0.5 psi sweeps through the train's few
                            # per cent of variation within a fraction of a cell, and fewer than 0.1 % of the decisions depend on
                            # the jump term; with a flat psi the train's own variation decides, and more than 1 % do
LQR_IC_S = {4: 0.068, 12: 0.2}  # the boundary cost's s of the 2-D impulse rows per class (make_ctx says why)
HSJ_LAM0 = {2: 8.0, 3: 25.0}             # lam0 of the horizon + stop + jump rows by dimension: lambda delta <= 0.12 (2-D) and 0.11 (3-D) on top of the Q delta / h^2
                            # < 0.75 of the neighbours' cases stays inside the CFL rule (the rows assert it), and the jump term then
                            # decides more than 1 % of the stop decisions
U_LQ, W_LQ = np.linspace(-1.0, 1.0, 9).reshape(-1, 1), np.linspace(-0.5, 0.5, 5).reshape(-1, 1)  # test_gpu_game.py's lists


def _rows():
    rows = []

    def add(spec, names, bonds, rp, noise, model=None, **opts):
        form = make_form(*names)
        d = len(bonds) - 1
        dt = (DT2_H if d == 2 else DT3_H) if "horizon" in form else (DT2 if d == 2 else DT3)
        rid = "-".join([spec] + [q for q in FORM_NAMES if q in form] + [f"c{rp}", noise] + [a if opts[a] is True else str(opts[a]) for a in sorted(opts)])
        rows.append(Row(rid, spec, model or spec, form, tuple(bonds), rp, noise, NLANES, N2 if d == 2 else N3, dt, opts))

    for rp, bond in ((4, 3), (12, 11)):
        for noise in ("seed", "zero"):
            for mask in range(8):
                add("lqr_jd", [q for b, q in enumerate(("horizon", "stop", "jump")) if mask >> b & 1], (1, bond, 1), rp, noise)
            add("lqr_ic", ["impulse"], (1, bond, 1), rp, noise)
            add("lqr_ic", ["impulse", "jump"], (1, bond, 1), rp, noise)
    for order, noise in (("minmax", "seed"), ("maxmin", "zero"), ("minmax", "zero"), ("maxmin", "seed")):
        add("lqgame", ["game"], (1, 3, 1), 4, noise, order=order)
    for rp, bonds, noise in ((12, (1, 11, 9, 1), "seed"), (4, (1, 3, 4, 1), "zero")):
        model = "lqr3_jd" if rp == 12 else "lqr3_jd_c4"
        add("lqr3_jd", ["horizon", "stop", "jump"], bonds, rp, noise, model=model)
        add("lqr3_jd", ["jump"], bonds, rp, noise, model=model)
        add("lqr3_ic", ["impulse", "jump"], bonds, rp, noise)
    # a stack whose stages alternate between bond 3 (class 4) and bond 11 (class 12): every step launches its stage's own kernel
    add("lqr_jd", ["horizon", "stop", "jump"], (1, 11, 1), 12, "seed", mixed=True)
    # CONSTELM reaches jump_term and impulse_term through S.constelm
    add("lqr_jd", ["jump"], (1, 3, 1), 4, "seed", constelm=True)
    add("lqr_ic", ["impulse"], (1, 11, 1), 12, "seed", constelm=True)
    return rows


ROWS = _rows()
# launch cut and batch split: the forms whose state crosses the cut in ex's stop encoding and in the uniforms' key
CUT_ROWS = [r for r in ROWS if r.id in ("lqr_jd-stop-c4-seed", "lqr_jd-stop-jump-c4-seed", "lqr_ic-jump-impulse-c12-seed")]


def assert_occurrences(row, c):
    """the occurrence counts a row's run must show (Log.counts), on the reference's closed loop and on the device's own run"""
    form, d = row.form, len(row.bonds) - 1
    assert c["candidates"] >= 3, c
    assert not c["cfl"], "a horizon row leaves the CFL rule"
    assert c["alive_mid"] >= row.n // 2, c
    if "stop" in form:
        assert c["stop0"] >= 3 and c["stop_later"] >= 3, c
    if "impulse" in form:
        assert len(c["impulses"]) == (3 if d == 2 else 2) and min(c["impulses"]) >= 3, c
        if d == 2:  # the 3-D interventions move along the periodic and the reflecting dimension only
            assert c["exit_impulse"] >= 1, c
    if "jump" in form:
        assert len(c["jumps"]) == (3 if d == 2 else 2) and min(c["jumps"]) >= 3, c
        assert c["exit_jump_face"] + c["exit_jump_obstacle"] >= 1, c


def _x0(w, row, rng):
    """start states: most of the box, and lanes placed where the kernel's branches are: beside the absorbing face of dim 0 (a
    step, a mark-0 jump or intervention 1 leaves), inside the obstacle (exit at step 0), beside and beyond the periodic seam
    (xin != x), beside the reflecting face"""
    from c3sc_amd import workloads as wl

    n, d = row.n, w.dx
    lo, hi = np.array(w.lb), np.array(w.ub)
    x = lo + (hi - lo) * rng.uniform(0.04, 0.96, (n, d))
    x[:30, 0] = rng.uniform(hi[0] - 0.5, hi[0] - 0.005, 30)
    x[30:34, 0] = rng.uniform(lo[0] + 0.001, lo[0] + 0.02, 4)
    x[34:36, 0] = lo[0] - rng.uniform(0.01, 0.2, 2)  # a start beyond the face: the exit test of step 0
    for c, wd in w.obstacles[:1]:
        x[36:44] = np.array(c) + (rng.uniform(-0.4, 0.4, (8, d))) * np.array(wd)
        x[44:70] = np.array(c) + (rng.uniform(-1.0, 1.0, (26, d))) * np.array(wd)  # around it: a mark-2 jump lands inside
    for m in range(d):
        if w.bc[m] == wl.BC_PERIODIC:
            x[70:84, m] = rng.uniform(hi[m] - 0.03, hi[m] + 0.4, 14)
            x[84:92, m] = rng.uniform(lo[m] - 0.4, lo[m] + 0.03, 8)
        if w.bc[m] == wl.BC_REFLECT:
            x[92:100, m] = rng.uniform(hi[m] - 0.05, hi[m] + 0.05, 8)
    if row.spec == "lqr_ic":  # the lanes beside the face leave by intervention 1 before a jump can take them: more lanes from which
        c, wd = w.obstacles[0]  # a mark-2 jump lands inside the obstacle
        x[100:160] = np.array(c) + (rng.uniform(-1.0, 1.0, (60, d))) * np.array(wd)
    if d == 3:  # few events per lane in the short 3-D runs: more lanes from which a mark-0 jump leaves through the face
        x[100:160, 0] = rng.uniform(hi[0] - 0.6, hi[0] - 0.005, 60)
    for m in range(d):  # a whole period beyond the seam, near the origin otherwise: where psi is low at xin and high at x itself
        if w.bc[m] == wl.BC_PERIODIC:
            x[160:166] = rng.uniform(-0.4, 0.4, (6, d))
            x[160:166, m] += hi[m] - lo[m]
    return np.ascontiguousarray(x)


def make_ctx(row, mid=0):
    """the Ctx of a row: workload, trains, start states and constants, all from the CPU.  mid: the device model's id (the GPU
    test's; the reference does not read it)"""
    from c3sc_amd import workloads as wl

    form, d = row.form, len(row.bonds) - 1
    rng = np.random.default_rng(zlib.crc32(row.id.encode()))
    kw = {}
    if row.spec == "lqgame":
        w = wl.Workload("lqgame", mid, GL.LQGAME_PRM, 2, 2, (-2.0, -2.0), (2.0, 2.0), (21, 19), tuple(row.bonds), 0.1,
                        (wl.BC_ABSORB, wl.BC_REFLECT), [((0.9, -0.9), (0.5, 0.6))], GL.product(U_LQ, W_LQ))
        host, bcost, ocost = GL.lqgame_host, (lambda x: np.full(len(x), 100.0)), (lambda x: np.zeros(len(x)))
        kw["game"] = (U_LQ, W_LQ, row.opts["order"])
    else:
        if row.spec == "lqr_jd":
            w = JL.lqr_workload(mid, row.bonds[1], BETA)
        elif row.spec == "lqr3_jd":
            w = JL.lqr3_workload(mid, row.bonds, BETA)
        elif row.spec == "lqr_ic":
            # the boundary is cheap (test_gpu_impulse.py has s = 0.02): the controller of a lane beside the face does choose the
            # intervention that leaves.  Here s sits where leaving pays for about half of those lanes (K + s |y|^2 against the
            # train's level, |y|^2 between 4.4 and 8): the others stay, and a mark-0 jump takes some of them out.  The cost scale
            # follows the train's level, about 0.12 per unit of bond rank
            w = IL.lqr_workload(mid, row.bonds[1], BETA, IL.lqr_cost_scale(row.rp) * row.bonds[1] / row.rp)
            w = dataclasses.replace(w, params=w.params[:3] + (LQR_IC_S[row.rp],) + w.params[4:])
        else:
            w = IL.lqr3_workload(mid, row.bonds, BETA, LQR3_K[row.rp])
            w = dataclasses.replace(w, params=w.params[:3] + (0.02,) + w.params[4:])
        host, ocost = SL.lqrn_host, (lambda x: np.full(len(x), 5.0))
        if "jump" in form or row.spec.endswith("_jd"):
            kw["jumps"] = JL.lqr_jumps if d == 2 else JL.lqr3_jumps
        if "impulse" in form:
            kw["impulses"] = IL.lqr_impulses if d == 2 else IL.lqr3_impulses
    if {"horizon", "stop", "jump"} <= form:
        w = dataclasses.replace(w, params=w.params[:3] + (0.02,) + w.params[4:6] + (HSJ_LAM0[d],) + w.params[7:])
    if "horizon" in form and row.spec != "lqgame":
        # r = 0.1: in the explicit scheme the control cost r u^2 delta meets a gradient term of about 0.17 |u| delta at bond rank 3,
        # and with r = 1 nearly every lane takes the smallest |u|; at 0.1 the minimiser moves through the list
        w = dataclasses.replace(w, params=w.params[:2] + (HORIZON_R,) + w.params[3:])
    x0 = _x0(w, row, rng)
    nst = row.N + 1 if "horizon" in form else 1
    ranks, cores, trains = [], [], []
    for s in range(nst):
        bonds = row.bonds
        if row.opts.get("mixed") and s % 2 == 0:
            bonds = (1, 3, 1)
        ws = dataclasses.replace(w, ranks=tuple(bonds))
        cs = wl.synth_cores(ws, seed=0xC35C + 97 * s)
        if "horizon" in form:
            # a stack of another seed per stage, over a common part: independent stages would draw every lane's stop decision
            # afresh at every step.  The stages still differ by a fifth of the train's variation, far above any rounding
            cs = [STACK_COMMON * b + (1.0 - STACK_COMMON) * q for b, q in zip(wl.synth_cores(ws), cs)]
        tr = JL.Train(ws, cs)
        if "horizon" in form and "stop" in form and s > 0:
            # a nearly flat psi against trains of different seeds: every stage is scaled to stage 1's mean level at the start
            # states, or a stage whose level sits a per cent higher would stop every lane at once
            lvl = tr.value(np.clip(x0, w.lb, w.ub)).mean()
            level = lvl if s == 1 else level
            cs = [cs[0] * (level / lvl)] + list(cs[1:])
            tr = JL.Train(ws, cs)
        ranks.append(tuple(bonds))
        cores.append(cs)
        trains.append(tr)
    if row.spec != "lqgame":
        bcost = lambda x, w=w: SL.lqrn_terminal(w.params, x)
    ctx = Ctx(w=w, C=np.asarray(w.cands, dtype=np.float64), host=host, bcost=bcost, ocost=ocost, trains=trains, ranks=ranks,
              cores=cores, dt=row.dt, N=row.N, x0=x0, wrap=any(b == wl.BC_PERIODIC for b in w.bc), constelm=bool(row.opts.get("constelm")),
              seed=2024 + 7 * row.rp, traj_offset=OFFSET, noise=np.zeros((row.n, row.N, d)) if row.noise == "zero" else None, **kw)
    if "stop" in form:
        # psi = c0 + c1 |x|^2 with c0 at the 1 - STOP_SHARE quantile of the continuation values at the start states (the controller of step 0)
        if "horizon" in form:
            ctx.w = w = dataclasses.replace(w, params=w.params[:5] + (STOP_C1_H,) + w.params[6:])
        xin = JL.wrap(w, x0) if ctx.wrap else x0
        live = ~in_obstacle(w, x0) & ~beyond_faces(w, x0) & ~in_obstacle(w, xin)
        v = np.unique(_continuation(form, ctx, x0)[live] - w.params[5] * (xin[live] ** 2).sum(-1))
        q = int((1.0 - (STOP_SHARE_H if "horizon" in form else STOP_SHARE)) * len(v))
        c0 = float(0.5 * (v[q - 1] + v[q]))  # between two lanes' values: psi ties with no continuation value
        w = dataclasses.replace(w, params=w.params[:4] + (c0,) + w.params[5:])
        ctx.w = w
        ctx.psi = lambda x, w=w: SL.lqr_psi(w.params, x)
        if "horizon" not in form:
            # lanes on a ring just outside psi's level set at the train's median level: the drift alone (zero normals) carries
            # few lanes across it in 24 steps, and these stop a few steps into the run
            cont = _continuation(form, ctx, x0)[live]
            r = np.sqrt(max(0.05, (np.median(cont) - c0) / w.params[5]))
            ang = rng.uniform(0.0, 2.0 * np.pi, 30)
            x0[170:200] = (r + rng.uniform(0.0, 0.06, 30))[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    return ctx


def _continuation(form, ctx, x):
    """the scan's result at the controller's input of step 0: the smallest candidate value (with the jump term where the form has it)"""
    w = ctx.w
    xin = JL.wrap(w, x) if ctx.wrap else x
    tr = ctx.trains[1 if "horizon" in form else 0]
    V, _ = stencil(w, tr, xin, ctx.constelm)
    h2, t = BR.mca_constants(w)
    q0 = pv0 = None
    if "jump" in form:
        q0, J = JL.jump_terms(w, ctx.jumps, tr, xin, ctx.bcost, ctx.ocost, ctx.constelm)
        pv0 = q0 * J
    vals, _, _ = BR.candidate_values(ctx.host, w.params, xin, V, ctx.C, h2, t, w.discount, q0, pv0, ctx.dt if "horizon" in form else None)
    return np.nanmin(vals, axis=1)
