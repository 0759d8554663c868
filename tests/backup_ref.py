"""The numpy restatement of node_backup, once, for every form of the Bellman backup.  It shares no code with the
kernels; horizon_lib, stop_lib, jump_lib, impulse_lib, corr_lib and game_lib add the terms of their feature and call it.

How the arguments map to the form bits:
    FORM_HORIZON   delta (candidate_values): the explicit scheme g delta + exp(-beta delta) (V_self + (delta / h^2) (PV - Q V_self));
                   no candidate is skipped (Q = 0 is "stay"), Q delta / h^2 > 1 flags CFL.  Without it dt = h2 / Q,
                   value = dt g + exp(-beta dt) (PV / Q + (1 - Q / Q) V_self), and Q < 1e-14 skips the candidate (NaN, stationary).
    FORM_JUMP      q0 += h2 lambda, pv0 += h2 lambda J   the Poisson term (jump_lib.jump_terms; the caller forms the product)
    FORM_CORR      q0 += cq, pv0 += cpv                  the pairs' correction (corr_lib.corr_terms)
    FORM_STOP      psi (backup): the stop action, index nc, after the candidates
    FORM_IMPULSE   c [P, M] (backup): the interventions, index nc + 1 + m, after the candidates; never with psi (form_offered)
    FORM_GAME      the candidate list product(U, W) and game_lib.minmax as the decision (`decide`), with nothing else
Every candidate's Q and PV start at zero, take q0 and pv0, then the upwind rates of each dimension with the +-1e-14 dead zone.

fibers() wraps the two for the nodes of a batch of fibers (absorbed nodes pay the boundary or obstacle cost), sweeps() for the
whole grid of a 2-D workload, and loop_backup() states the same rule as a per-node, per-candidate Python loop (loop_decide:
the decision alone, on given values)."""
import numpy as np


def mca_constants(w):
    """(h2, t) as BellmanEngine.configure sets them"""
    xg = w.xgrid()
    hs = [g[1] - g[0] for g in xg]
    hmin = min([w.ub[0] - w.lb[0]] + hs)
    h2 = hmin * hmin
    t = []
    for h in hs:
        t += [h2 / h, h2 / h / h]
    return h2, t


def node_states(w, k, idx):
    """coordinates [F, N, D] of the nodes of fibers idx along dim k"""
    xg = w.xgrid()
    F, N, D = idx.shape[0], w.ngrid[k], w.dx
    x = np.empty((F, N, D))
    for m in range(D):
        x[:, :, m] = xg[m][np.arange(N)][None, :] if m == k else xg[m][idx[:, m]][:, None]
    return x


def node_indices(w, k, idx):
    """multi-indices [F * N, D] of the nodes of fibers idx along dim k"""
    F, N = idx.shape[0], w.ngrid[k]
    ix = np.empty((F, N, w.dx), dtype=np.int64)
    for m in range(w.dx):
        ix[:, :, m] = np.arange(N)[None, :] if m == k else idx[:, m][:, None]
    return ix.reshape(-1, w.dx)


# ---------------------------------------------------------------------------------------------------- one node
def candidate_values(host, prm, x, V, C, h2, t, beta, q0=None, pv0=None, delta=None):
    """(values [P, nc], stationary [P], cfl [P, nc]) of every candidate C[nc, du] at P nodes x[P, D] with stencils V[P, 2D+1];
    q0, pv0 [P]: the control-independent terms inside Q and PV; delta: the horizon step (None: the infinite-horizon form, where
    NaN marks a skipped candidate)"""
    D = x.shape[1]
    xx = np.broadcast_to(x[:, None, :], (x.shape[0], len(C), D))
    uu = np.broadcast_to(C[None], (x.shape[0],) + C.shape)
    b, s, st = host(prm, xx, uu)
    Q = np.zeros(b.shape[:-1])
    PV = np.zeros(b.shape[:-1])
    if q0 is not None:
        Q = Q + q0[:, None]
    if pv0 is not None:
        PV = PV + pv0[:, None]
    for m in range(D):
        half = t[2 * m + 1] * (s[..., m] * s[..., m]) / 2.0
        tb = t[2 * m] * b[..., m]
        pm = np.where(b[..., m] < -1e-14, half - tb, half)
        pp = np.where(b[..., m] > 1e-14, half + tb, half)
        Q += pm + pp
        PV += pm * V[:, None, 2 * m] + pp * V[:, None, 2 * m + 1]
    Vs = V[:, None, 2 * D]
    if delta is not None:
        dh2 = delta / h2
        val = st * delta + np.exp(-beta * delta) * (Vs + dh2 * (PV - Q * Vs))
        return val, np.zeros(len(x), dtype=bool), Q * dh2 > 1.0
    bad = Q < 1e-14
    Qs = np.where(bad, 1.0, Q)
    dt = h2 / Qs
    val = dt * st + np.exp(-beta * dt) * (PV / Qs + (1.0 - Qs / Qs) * Vs)
    return np.where(bad, np.nan, val), bad.any(axis=1), np.zeros(val.shape, dtype=bool)


def best_impulse(c):
    """(ival [P], imark [P]) of c [P, M]: the running minimum from +inf by the first strict '<', m ascending; -1: none finite"""
    P, M = c.shape
    ival, imark = np.full(P, np.inf), np.full(P, -1)
    for m in range(M):
        take = c[:, m] < ival
        ival = np.where(take, c[:, m], ival)
        imark = np.where(take, m, imark)
    return ival, imark


def backup(vals, psi=None, c=None, forced=None, fault=None):
    """(value, index, margin) per node of the candidates' values vals [P, nc] (NaN = skipped): the first strict minimum of the
    candidates; then the stop action psi [P] of index nc, or the best of the interventions c [P, M] (best_impulse) of index
    nc + 1 + m -- either wins where strictly smaller and where no candidate was valid.  No valid action: 0.0 and -1.
    forced: the index to apply per node instead (nc: psi; above nc: an intervention, one past the last read as the last); an
    index that names nothing or a skipped candidate gives 0.0 and -1.  margin: best against second best over every action,
    relative to max(1, |best|); inf with fewer than two valid actions and on the forced path.
    fault: a planted mistake for the tests of the comparisons themselves ("index": the index nc + m, "le": '<=' for '<')"""
    if psi is not None and c is not None:
        raise ValueError("no kernel combines the stop action with interventions (form_offered)")
    P, nc = vals.shape
    ar = np.arange(P)
    if forced is not None:
        fi = np.asarray(forced).reshape(-1)
        v = vals[ar, np.clip(fi, 0, nc - 1)]
        ok = (fi >= 0) & (fi < nc) & ~np.isnan(v)
        out, ui = np.where(ok, v, 0.0), np.where(ok, fi, -1)
        if psi is not None:
            out, ui = np.where(fi == nc, psi, out), np.where(fi == nc, nc, ui)
        if c is not None:
            ci = c[ar, np.clip(fi - nc - 1, 0, c.shape[1] - 1)]
            out, ui = np.where(fi > nc, ci, out), np.where(fi > nc, fi, ui)
        return out, ui, np.full(P, np.inf)
    allv = np.where(np.isnan(vals), np.inf, vals)
    ui = np.argmin(allv, axis=1)  # the first of equal minima
    out = allv[ar, ui]
    if psi is not None:
        take = psi < out
        out, ui = np.where(take, psi, out), np.where(take, nc, ui)
        allv = np.concatenate([allv, psi[:, None]], axis=1)
    if c is not None:
        ival, imark = best_impulse(c)
        if fault == "le":
            ival, imark = c.min(axis=1), c.shape[1] - 1 - np.argmin(c[:, ::-1], axis=1)  # the last of equal minima
            imark = np.where(np.isfinite(ival), imark, -1)
        take = (imark >= 0) & ((ival <= out) if fault == "le" else (ival < out))
        out, ui = np.where(take, ival, out), np.where(take, nc + (0 if fault == "index" else 1) + imark, ui)
        allv = np.concatenate([allv, c], axis=1)
    none = ~np.isfinite(out)
    margin = np.full(P, np.inf)
    if allv.shape[1] > 1:
        srt = np.sort(allv, axis=1)
        with np.errstate(invalid="ignore"):  # inf - inf where no action is valid: replaced below
            margin = (srt[:, 1] - srt[:, 0]) / np.maximum(1.0, np.abs(np.where(none, 1.0, srt[:, 0])))
        margin = np.where(np.isfinite(srt[:, 1]), margin, np.inf)
    return np.where(none, 0.0, out), np.where(none, -1, ui), margin


def stop_margin(vals, psi):
    """the margin of the stop decision alone: |psi - continuation| relative to max(1, |continuation|), inf where no candidate
    was valid.  It is never smaller than backup's margin over every action; the stop tests choose by it which indices to compare"""
    any_ok = ~np.isnan(vals).all(axis=1)
    cont = np.where(np.isnan(vals), np.inf, vals).min(axis=1)
    return np.where(any_ok, np.abs(psi - cont) / np.maximum(1.0, np.abs(np.where(any_ok, cont, 0.0))), np.inf)


def loop_decide(vals, psi=None, c=None):
    """the decision in words, one node at a time: (value [P], index [P]) of given candidate values vals [P, nc] (NaN = skipped)"""
    P, nc = vals.shape
    out, idx = np.zeros(P), np.full(P, -1)
    for p in range(P):
        best, bi = 0.0, -1
        for a in range(nc):
            if not np.isnan(vals[p, a]) and (bi < 0 or vals[p, a] < best):
                best, bi = vals[p, a], a
        if psi is not None and (bi < 0 or psi[p] < best):
            best, bi = psi[p], nc
        if c is not None:
            ival, imark = np.inf, -1
            for m in range(c.shape[1]):
                if np.isfinite(c[p, m]) and c[p, m] < ival:
                    ival, imark = c[p, m], m
            if imark >= 0 and (bi < 0 or ival < best):
                best, bi = ival, nc + 1 + imark
        out[p], idx[p] = best, bi
    return out, idx


def loop_backup(host, prm, x, V, C, h2, t, beta, q0=None, pv0=None, psi=None, c=None, delta=None):
    """the whole rule by a Python loop over one node and one candidate at a time (the check of the vectorised restatement):
    (value [P], index [P], stationary [P], cfl [P])"""
    P, D = x.shape
    vals, stat, cfl = np.full((P, len(C)), np.nan), np.zeros(P, dtype=bool), np.zeros(P, dtype=bool)
    for p in range(P):
        for a in range(len(C)):
            b, s, st = host(prm, x[p], C[a])
            Q = 0.0 if q0 is None else q0[p]
            PV = 0.0 if pv0 is None else pv0[p]
            for m in range(D):
                half = t[2 * m + 1] * (s[m] * s[m]) / 2.0
                tb = t[2 * m] * b[m]
                pm = half - tb if b[m] < -1e-14 else half
                pp = half + tb if b[m] > 1e-14 else half
                Q += pm + pp
                PV += pm * V[p, 2 * m] + pp * V[p, 2 * m + 1]
            if delta is not None:
                vals[p, a] = st * delta + np.exp(-beta * delta) * (V[p, 2 * D] + (delta / h2) * (PV - Q * V[p, 2 * D]))
                cfl[p] |= Q * delta > h2
            elif Q < 1e-14:
                stat[p] = True
            else:
                dt = h2 / Q
                vals[p, a] = dt * st + np.exp(-beta * dt) * (PV / Q + (1.0 - Q / Q) * V[p, 2 * D])
    return loop_decide(vals, psi, c) + (stat, cfl)


# ---------------------------------------------------------------------------------------------------- the nodes of fibers
def fibers(w, host, k, idx, costs, absorbed, bcost, ocost, q0=None, pv0=None, psi=None, c=None, delta=None, forced=None, cands=None,
           decide=None):
    """the backup of every node of fibers idx along dim k from their stencils (costs [F, N, 2D+1], absorbed [F, N]: 1 boundary,
    -1 obstacle); bcost, ocost: callables of x [P, D]; q0, pv0, psi [P] and c [P, M]: the feature terms at the states
    node_states(w, k, idx) in fiber order.  cands: a candidate list in place of w.cands; decide: a decision on the values
    [P, nc] in place of backup (the game's min-max).  Returns (value, index, margin, stationary, cfl) of shape [F, N]: absorbed
    nodes pay their cost with the index -1, the flags are the live nodes' alone, and of the forced candidate on the forced path"""
    h2, t = mca_constants(w)
    x = node_states(w, k, idx).reshape(-1, w.dx)
    C = np.asarray(w.cands if cands is None else cands, dtype=np.float64)
    vals, stat, cfl = candidate_values(host, w.params, x, costs.reshape(-1, 2 * w.dx + 1), C, h2, t, w.discount, q0, pv0, delta)
    out, ui, mg = backup(vals, psi, c, forced) if decide is None else decide(vals)
    if forced is not None:
        fi = np.asarray(forced).reshape(-1)
        cfl = cfl[np.arange(len(fi)), np.clip(fi, 0, len(C) - 1)] & (fi >= 0) & (fi < len(C))
    else:
        cfl = cfl.any(axis=1)
    ab = absorbed.reshape(-1)
    out = np.where(ab == 1, bcost(x), np.where(ab == -1, ocost(x), out))
    ui = np.where(ab != 0, -1, ui)
    sh = absorbed.shape
    return out.reshape(sh), ui.reshape(sh), mg.reshape(sh), (stat & (ab == 0)).reshape(sh), (cfl & (ab == 0)).reshape(sh)


# ---------------------------------------------------------------------------------------------------- a whole 2-D grid
def grid2(w):
    """(x [P, 2], absorbed [P], sten) of the whole grid of a 2-D workload without obstacles: the states in row-major order, the
    nodes on a face of an absorbing dimension, and the gather Vn [n0, n1] -> stencils [P, 5] (the node itself beyond an end)"""
    from c3sc_amd import workloads as wl

    n0, n1 = w.ngrid
    xg = w.xgrid()
    i0, i1 = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
    x = np.stack([xg[0][i0], xg[1][i1]], axis=-1).reshape(-1, 2)
    ab = np.zeros(i0.shape, dtype=bool)
    for i, n, bc in ((i0, n0, w.bc[0]), (i1, n1, w.bc[1])):
        if bc == wl.BC_ABSORB:
            ab |= (i == 0) | (i == n - 1)
    lo0, hi0 = np.clip(i0 - 1, 0, n0 - 1), np.clip(i0 + 1, 0, n0 - 1)
    lo1, hi1 = np.clip(i1 - 1, 0, n1 - 1), np.clip(i1 + 1, 0, n1 - 1)
    sten = lambda Vn: np.stack([Vn[lo0, i1], Vn[hi0, i1], Vn[i0, lo1], Vn[i0, hi1], Vn], axis=-1).reshape(-1, 5)
    return x, ab.reshape(-1), sten


def sweeps(w, host, V0, keep, n, terms=None, psi=None, delta=None, forced=None, fault=None, cands=None, decide=None):
    """n sweeps of the operator on the whole grid of a 2-D workload (grid2) from V0 [n0, n1]: the absorbed nodes hold keep [P]
    after every sweep (V0 is taken as given).  terms(Vn) -> (q0, pv0, c, flags): the feature terms of the sweep that reads Vn
    (each may be None; flags [P]: a condition to report).  psi, delta, forced, fault, cands, decide: as in backup and fibers.
    Returns (V [n + 1, n0, n1] in sweep order, index [n, n0, n1] (-1: absorbed), margin [n, n0, n1] (of the decision at every
    node, the absorbed ones too), cfl seen, flags seen -- the last two at a live node of any sweep)"""
    n0, n1 = w.ngrid
    x, ab, sten = grid2(w)
    h2, t = mca_constants(w)
    C = np.asarray(w.cands if cands is None else cands, dtype=np.float64)
    Vn = np.asarray(V0, dtype=np.float64).reshape(n0, n1)
    out, dec, mgs, anycfl, anyflag = [Vn], [], [], False, False
    for _ in range(n):
        q0, pv0, c, flags = (None, None, None, None) if terms is None else terms(Vn)
        vals, _, cfl = candidate_values(host, w.params, x, sten(Vn), C, h2, t, w.discount, q0, pv0, delta)
        v, ui, mg = backup(vals, psi, c, forced, fault) if decide is None else decide(vals)
        anycfl |= bool((cfl.any(axis=1) & ~ab).any())
        if flags is not None:
            anyflag |= bool((flags & ~ab).any())
        Vn = np.where(ab, keep, v).reshape(n0, n1)
        out.append(Vn)
        dec.append(np.where(ab, -1, ui).reshape(n0, n1))
        mgs.append(mg.reshape(n0, n1))
    return np.array(out), np.array(dec), np.array(mgs), anycfl, anyflag
