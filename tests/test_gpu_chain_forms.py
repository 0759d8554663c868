"""The Markov chain of a run-time compiled model's own backup on the GPU, in the eight forms of the chain -- every subset of
{horizon, stop, jump} (c3sc_hip_model_compile_mc with chain = 1, c3sc_hip_chain_outcomes, c3sc_hip_chain_transitions,
c3sc_hip_simulate_chain) -- against chain_forms_ref.py on jump_lib's lqr_jd (21 x 70, ranks 4 and 12) and lqr3_jd
(5 x 128 x 5, bonds (1, 12, 9, 1)).

- Outcomes: every node of lqr_jd and 2 000 seeded nodes of lqr3_jd against the reference to TOL, flags, uidx and stop nodes
  exactly, the device call and the host call bit for bit, chain_transitions the same bits without the extra arrays; the device's own
  outputs recombine to bellman_fibers' value in the same mode (the identity).
- Walks: the lock-step check on 300 lanes x 24 steps with Philox and with supplied (v, u1), multilinear and CONSTELM;
  steps_per_launch = 5 and a split at lane 50 bit for bit; horizon rows under a stack whose stages alternate between the padded
  classes 12 and 4.
- CDF: one step from 8 nodes under a 257-point grid in v, and at a jumping node in u1.
- Refusals, each leaving the context usable.
- The reference API: c3control_simulate_chain_batch in stopping and jump mode, in a child process, against the numpy walk."""
import os
import subprocess
import sys

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import chain_forms_ref as CF
import jump_lib as JL

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 3
CASES = [("lqr", 4), ("lqr", 12), ("lqr3", 12)]
CASE_IDS = ["lqr-4", "lqr-12", "lqr3"]
FORM_IDS = [CF.form_id(f) for f in CF.FORMS]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU: the chain kernels have no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def ids():
    return {
        "lqr": E.compile_model(JL.LQR, 2, 2, ranks=(4, 12), name="lqr_mc", horizon=True, stop=True, njump=JL.LQR_NJUMP, chain=True, **JL.LQR_MASKS),
        "lqr3": E.compile_model(JL.LQR3, 3, 3, ranks=(4, 12), name="lqr3_mc", horizon=True, stop=True, njump=JL.LQR3_NJUMP, chain=True,
                                **JL.LQR3_MASKS),
    }


def _engine(w, cores, ref, constelm=False):
    """a context in the reference's form, with its stack where it has one"""
    horizon, stop, jump = ref.form
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    if constelm:
        eng.set_interp(True)
    if stop:
        eng.set_stopping(True)
    if horizon:
        eng.set_horizon_step(ref.delta)
    if jump:
        eng.set_jumps(True)
    if ref.stacked:
        eng.upload_value_stack([list(rk) for rk, _ in ref.stack], [cs for _, cs in ref.stack])
    return eng


@pytest.fixture(scope="module")
def setups(ids):
    made = {}

    def get(model, rank, form, nstack=0, constelm=False):
        key = (model, rank, form, nstack, constelm)
        if key not in made:
            w, cores, ref = CF.case(model, ids[model], rank, form, constelm=constelm, nstack=nstack)
            made[key] = (w, _engine(w, cores, ref, constelm), ref)
        return made[key]

    return get


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _nodes(w, model):
    if model == "lqr":
        return np.array([(i, j) for i in range(w.ngrid[0]) for j in range(w.ngrid[1])], dtype=np.int32)
    z = wl.splitmix64(0x0DE5, 2000 * w.dx).reshape(2000, w.dx)
    return (z % np.array(w.ngrid, dtype=np.uint64)).astype(np.int32)


def _same_bits(a, b, keys):
    for k in keys:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


@pytest.mark.parametrize("form", CF.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("model,rank", CASES, ids=CASE_IDS)
def test_outcomes_and_the_identity(setups, model, rank, form):
    torch = _torch()
    w, eng, ref = setups(model, rank, form)
    M = ref.table().M
    nodes = _nodes(w, model)
    nodes_t = torch.from_numpy(nodes).cuda()
    eng.status(clear=True)
    res = _np(eng.chain_outcomes(nodes_t, njump=M))
    assert eng.last_kernel() == f"k_chain_outcomes_form<rtc:{model}_mc,{rank}>"
    unsure = ref.check_outcomes(nodes, res)
    assert unsure <= 0.025 * len(nodes)
    assert eng.status(clear=True) == 0
    live = res["flag"] == 0
    assert (res["flag"] == 1).any() and (res["flag"] == -1).any() and live.any()
    if form[1]:
        assert (res["uidx"][live] == ref.nc).any() and (res["uidx"][live] < ref.nc).any(), "both decisions occur"
    # the host entry point and the transitions call give the same bits
    hres = eng.chain_outcomes_host(nodes, njump=M)
    _same_bits(res, hres, res.keys())
    tres = _np(eng.chain_transitions(nodes_t))
    _same_bits(res, tres, tres.keys())
    _same_bits(res, eng.chain_transitions_host(nodes), tres.keys())
    # the identity on the device's own numbers: the fiber along dimension 0 through each node, in the same mode
    fib = nodes.copy()
    fib[:, 0] = 0
    out, ui, ab = eng.bellman_fibers_host(0, fib)
    rows = np.arange(len(nodes))
    bv, bf = out[rows, nodes[:, 0]], ab[rows, nodes[:, 0]]
    assert np.array_equal(bf, res["flag"])
    assert (np.abs(bv - res["value"]) <= CF.TOL * np.maximum(1.0, np.abs(bv))).all()
    rec = ref.identity(nodes, res)
    moves = live & (res["uidx"] >= 0)
    assert not np.isnan(rec[moves]).any()
    assert (np.abs(rec[moves] - bv[moves]) <= CF.TOL * np.maximum(1.0, np.abs(bv[moves]))).all(), np.abs(rec[moves] - bv[moves]).max()


def _run(torch, eng, node0, nsteps, **kw):
    """simulate_chain with every node and decision saved, as chain_forms_ref.check wants it"""
    r = _np(eng.simulate_chain(torch.from_numpy(np.ascontiguousarray(node0)).cuda(), nsteps, save_every=1, **kw))
    r["node0"], r["nsteps"] = node0, nsteps
    return r


RUN_KEYS = ("cost", "disc", "time", "vend", "node", "exit", "traj", "uidx")
WALKS = [(m, r, f, c) for (m, r) in CASES for f in CF.FORMS for c in (False, True) if f[2] or not c]  # CONSTELM where marks land


@pytest.mark.parametrize("model,rank,form,constelm", WALKS,
                         ids=[f"{m}-{r}-{CF.form_id(f)}-{'constelm' if c else 'linear'}" for m, r, f, c in WALKS])
def test_walks_in_lock_step(setups, model, rank, form, constelm):
    torch = _torch()
    horizon, stop, jump = form
    w, eng, ref = setups(model, rank, form, CF.NSTEPS + 1 if horizon else 0, constelm)
    node0 = CF.start_nodes(ref)
    n = len(node0)
    eng.status(clear=True)
    # Philox
    run = _run(torch, eng, node0, CF.NSTEPS, seed=CF.SEED)
    assert eng.last_kernel().startswith(f"k_chain_walk_form<rtc:{model}_mc,")
    pair = CF.Ref.uniforms(CF.SEED, 0, n, CF.NSTEPS)
    run["uniform"] = pair
    out = ref.check(run)
    assert out["unsure"] <= 0.025 * max(out["steps"], 1) and out["steps"] >= n * CF.NSTEPS // 4  # half the lanes alive at mid-run (a precondition of the table)
    # supplied uniforms: (v, u1) with jumps on, v alone without
    unif = np.random.default_rng(CF.SEED + 2).random((n, CF.NSTEPS, 2))
    given = unif if jump else np.ascontiguousarray(unif[:, :, 0])
    run_u = _run(torch, eng, node0, CF.NSTEPS, uniform_t=torch.from_numpy(given).cuda())
    run_u["uniform"] = unif
    out = ref.check(run_u)
    assert out["unsure"] <= 0.025 * max(out["steps"], 1)
    assert eng.status(clear=True) == 0
    # the splits and the host entry point
    _same_bits(run, _run(torch, eng, node0, CF.NSTEPS, seed=CF.SEED, steps_per_launch=5), RUN_KEYS)
    a = _run(torch, eng, node0[:50], CF.NSTEPS, seed=CF.SEED)
    b = _run(torch, eng, node0[50:], CF.NSTEPS, seed=CF.SEED, traj_offset=50)
    _same_bits(run, {k: np.concatenate([a[k], b[k]]) for k in RUN_KEYS}, RUN_KEYS)
    _same_bits(run_u, eng.simulate_chain_host(node0, CF.NSTEPS, uniform=given, save_every=1, steps_per_launch=5), RUN_KEYS)


GRID = 257


@pytest.mark.parametrize("form", [(False, False, True), (True, True, True), (True, False, False)], ids=CF.form_id)
def test_every_pick_is_held_to_the_cdf(setups, form):
    """one step from 8 live nodes under 257 values of v each: a uniform grid with both end cells, so every outcome with a
    probability above 1/257 is drawn and the first and the last outcome are reached; with jumps, one more node whose 257 lanes all
    draw the same mark (v inside its cell) under the same grid in u1: every corner with a weight above 1/257 is reached"""
    torch = _torch()
    horizon, stop, jump = form
    w, eng, ref = setups("lqr", 4, form, 2 if horizon else 0)
    key = 1 if horizon else None
    T = ref.table(key)
    starts = [tuple(ix) for ix in CF.start_nodes(ref) if T.flag[ref.flat(ix)] == 0 and T.ui[ref.flat(ix)] < ref.nc][:8]
    assert len(starts) == 8
    grid = np.concatenate(([0.0], (np.arange(1, GRID - 1) + 0.5) / GRID, [np.nextafter(1.0, 0.0)]))
    node0 = np.repeat(np.array(starts, dtype=np.int32), GRID, axis=0)
    unif = np.stack([np.tile(grid, 8), np.full(8 * GRID, 0.5)], axis=-1).reshape(-1, 1, 2)
    if jump:  # a node whose mark 1 lands inside: v in the middle of that mark's cell, u1 on the grid
        ix = starts[0]
        o = ref.outcomes(ix, key)
        c = np.concatenate(([0.0], np.cumsum(o.weights))) / o.W
        k = 2 * w.dx + 1
        assert ref.kind(T, ref.flat(ix), k) == "mark1:inside" and c[k + 1] - c[k] > 0.0
        node0 = np.concatenate([node0, np.repeat(np.array([ix], dtype=np.int32), GRID, axis=0)])
        unif = np.concatenate([unif, np.stack([np.full(GRID, 0.5 * (c[k] + c[k + 1])), grid], axis=-1).reshape(-1, 1, 2)])
    given = unif if jump else np.ascontiguousarray(unif[:, :, 0])
    run = _run(torch, eng, node0, 1, uniform_t=torch.from_numpy(given).cuda())
    run["uniform"] = unif
    ref.check(run)
    for s, ix in enumerate(starts):  # the empirical law of the 257 picks is the CDF's to one cell per outcome
        p = ref.flat(ix)
        o = ref.outcomes(ix, key, int(run["uidx"][s * GRID, 0]))
        nxt = [tuple(v) for v in run["traj"][s * GRID:(s + 1) * GRID, 1]]
        ex = run["exit"][s * GRID:(s + 1) * GRID]
        drawn = 0.0
        for k in range(len(o.weights)):
            pk = o.weights[k] / o.W
            if pk <= 1.0 / GRID:
                continue
            drawn += pk
            nx, allowed, leaves, _ = ref.apply(ix, T, p, k, 0.5)
            if leaves:
                assert (ex == 1).sum() >= 1, (ix, k)
            elif len(allowed) == 1 and sum(ref.apply(ix, T, p, kk, 0.5)[0] == nx for kk in range(len(o.weights)) if o.weights[kk] > 0.0) == 1:
                assert abs(nxt.count(nx) / GRID - pk) <= 2.0 / GRID, (ix, k, nxt.count(nx) / GRID, pk)
        assert drawn > 0.9
        first = [k for k in range(len(o.weights)) if o.weights[k] > 0.0]
        assert nxt[0] in ref.apply(ix, T, p, first[0], 0.5)[1] and nxt[-1] in ref.apply(ix, T, p, first[-1], 0.5)[1]
    if jump:  # the corners of the cell of mark 1's target: each is reached in proportion to its multilinear weight
        ix = starts[0]
        y = JL.wrap(w, T.y[ref.flat(ix), 1][None, :])[0]
        cells = [JL.Train.cell(ref.xg[m], np.array([y[m]]), False) for m in range(w.dx)]
        nxt = [tuple(v) for v in run["traj"][8 * GRID:, 1]]
        for corner in np.ndindex(*(2,) * w.dx):
            wt = np.prod([float(cells[m][1][0]) if corner[m] else 1.0 - float(cells[m][1][0]) for m in range(w.dx)])
            node = tuple(int(cells[m][0][0]) + corner[m] for m in range(w.dx))
            if wt > 1.0 / GRID:
                assert abs(nxt.count(node) / GRID - wt) <= 2.0 / GRID, (node, nxt.count(node) / GRID, wt)


CERT_STAGES, CERT_WALKS = 12, 4096
# psi = 4 + 0.5 |x|^2 against V_12 = 2 |x|^2: continuing wins inside |x|^2 < 8/3, so of these starts (near the absorbing face, beside
# the obstacle, towards the stopping region) walks run on, stop, and leave through a face, the obstacle or a mark (chosen with
# chain_forms_ref's walk under the same stack)
CERT_C0 = 4.0
CERT_STARTS = [(18, 35), (13, 19), (6, 60)]


def test_certificate_on_the_device():
    """horizon + stop + jump on lqr_jd under an exact stack: V_12 = s |x|^2 and each V_n the device's own backup of V_{n+1} at every
    node of the grid, held as a full-rank train (the nodal matrix has 20 singular values above rounding: the two absorbing faces
    pay one function of x_1).  The chain is then the backup's own, so J + D vend over the walks still running, J over the frozen
    ones, is an unbiased estimator of V_0 at the start node; held by the rule of test_gpu_chain.py's certificate, 4 standard errors
    and 1e-9."""
    import horizon_lib as H
    import stop_lib as SL

    torch = _torch()
    mid = E.compile_model(JL.LQR, 2, 2, ranks=(20,), name="lqr_mc20", horizon=True, stop=True, njump=JL.LQR_NJUMP, chain=True, **JL.LQR_MASKS)
    w = JL.lqr_workload(mid, 20, 0.3, JL.LQR_PRM[:4] + (CERT_C0,) + JL.LQR_PRM[5:])
    xg = w.xgrid()
    X0, X1 = np.meshgrid(xg[0], xg[1], indexing="ij")
    V = SL.lqrn_terminal(w.params, np.stack([X0, X1], axis=-1))

    def train(V):
        U, S, Vt = np.linalg.svd(V)
        assert S[20:].max() <= 1e-14 * S[0], S[20:] / S[0]
        return [(U[:, :20] * S[None, :20]).reshape(-1, 20), np.ascontiguousarray(Vt[:20, :].T).reshape(-1, 20)]

    eng = E.BellmanEngine(0)
    eng.configure(w, train(V))
    eng.set_stopping(True)
    eng.set_horizon_step(CF.LQR_DELTA)
    eng.set_jumps(True)
    fib = np.zeros((w.ngrid[1], 2), dtype=np.int32)
    fib[:, 1] = np.arange(w.ngrid[1])
    stack, stopped = [train(V)], False
    for _ in range(CERT_STAGES):
        eng.upload_value(w.ranks, stack[0])
        out, ui, ab = eng.bellman_fibers_host(0, fib)
        stopped = stopped or bool((ui == w.ncand).any())
        V = np.ascontiguousarray(out.T)
        stack.insert(0, train(V))
    assert eng.status(clear=True) == 0 and stopped
    eng.upload_value(w.ranks, stack[0])
    eng.upload_value_stack([list(w.ranks)] * len(stack), stack)
    node0 = np.repeat(np.array(CERT_STARTS, dtype=np.int32), CERT_WALKS, axis=0)
    run = _np(eng.simulate_chain(torch.from_numpy(node0).cuda(), CERT_STAGES, seed=CF.SEED + 9))
    est = run["cost"] + np.where(run["exit"] == -1, run["disc"] * run["vend"], 0.0)
    kinds = set(E.decode_chain_exit(run["exit"])[1])
    assert {"running", "stopped", "exit"} <= kinds, kinds
    for s, start in enumerate(CERT_STARTS):
        e = est[s * CERT_WALKS:(s + 1) * CERT_WALKS]
        mean, se = e.mean(), e.std(ddof=1) / np.sqrt(CERT_WALKS)
        print(f"start {start}: mean {mean:.9f} se {se:.3e} V_0 {V[start]:.9f}")
        assert abs(mean - V[start]) <= 4.0 * se + 1e-9, (start, mean, V[start], se)


def _chain_rcs(torch, eng, d, n=4):
    """(return code of simulate_chain, of chain_transitions, of chain_outcomes) for n walks from node 1 of every dimension"""
    node0 = torch.ones((n, d), dtype=torch.int32).cuda()
    cost = torch.empty((n,), dtype=torch.float64).cuda()
    a = E.ChainArgs()
    a.n, a.d_node0, a.nsteps, a.d_cost = n, node0.data_ptr(), 3, cost.data_ptr()
    rc_t = eng.L.c3sc_hip_chain_transitions(eng.h, n, node0.data_ptr(), None, cost.data_ptr(), None, None, None, None, None)
    rc_o = eng.L.c3sc_hip_chain_outcomes(eng.h, n, node0.data_ptr(), None, cost.data_ptr(), None, None, None, None, cost.data_ptr(), None, None, None)
    return eng.simulate_chain_rc(a), int(rc_t), int(rc_o)


def _still_works(torch, eng, w):
    idx = torch.from_numpy(wl.synth_fibers(w, 0, 8)).cuda()
    out = eng.bellman_fibers(0, idx)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def _mode_model(mode):
    """(workload of a chain-compiled model with the mode's kernels, the call that switches the mode on, the one that ends it)"""
    import corr_lib as CL
    import impulse_lib as IL
    import stop_lib as SL

    if mode == "impulse":
        mid = E.compile_model(IL.LQR_JUMP, 2, 2, ranks=(4,), name="lqr_mc_ic", njump=JL.LQR_NJUMP, nimpulse=IL.LQR_NIMPULSE, chain=True,
                              **IL.LQR_MASKS)
        return IL.lqr_workload(mid, 4, 0.3, IL.lqr_cost_scale(4)), (lambda e: e.set_impulses(True)), (lambda e: e.set_impulses(False))
    if mode == "corr":
        mid = E.compile_model(CL.LQR, 2, 2, ranks=(4,), name="lqr_mc_cd", corr_pairs=CL.LQR_PAIRS, chain=True, **CL.LQR_MASKS)
        return CL.lqr_workload(mid, 4, 0.1, CL.LQR_PRM), (lambda e: e.set_correlation(True)), (lambda e: e.set_correlation(False))
    mid = E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_mc_game", game=True, chain=True, **SL.LQR_MASKS)
    w = wl.Workload("lqr_game", mid, tuple(SL.LQR_PRM), 2, 2, (-2.0, -2.0), (2.0, 2.0), (9, 12), wl.uniform_ranks(2, 3), 0.1,
                    (wl.BC_REFLECT, wl.BC_REFLECT), [], SL.lqr_cands())

    def game_on(e):  # the product list changes the size of the static data: the value goes up again
        e.set_game(np.array([[0.0], [1.0]]), np.array([[0.0], [0.5]]))
        e.upload_value(w.ranks, wl.synth_cores(w))

    return w, game_on, (lambda e: e.set_controls(w.cands))


def test_refusals_leave_the_context_usable(ids):
    torch = _torch()
    ok, unsup = (0, 0, 0), (ERR_UNSUPPORTED,) * 3
    # a chain-compiled model serves its modes ...
    w = JL.lqr_workload(ids["lqr"], 4, 0.3)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    assert _chain_rcs(torch, eng, 2) == ok
    eng.set_stopping(True)
    eng.set_jumps(True)
    assert _chain_rcs(torch, eng, 2) == ok
    # ... horizon mode needs the stack, for the walk
    eng.set_horizon_step(CF.LQR_DELTA)
    assert _chain_rcs(torch, eng, 2) == (ERR_ARG, 0, 0)
    eng.upload_value_stack([list(w.ranks)] * 3, [wl.synth_cores(w)] * 3)
    assert _chain_rcs(torch, eng, 2) == (ERR_ARG, 0, 0)  # nsteps = 3 needs 4 stages
    eng.upload_value_stack([list(w.ranks)] * 4, [wl.synth_cores(w)] * 4)
    assert _chain_rcs(torch, eng, 2) == ok
    eng.set_horizon_step(0.0)
    eng.set_stopping(False)
    eng.set_jumps(False)
    _still_works(torch, eng, w)
    # a mode whose flag the chain-compiled model lacks: compiled with jumps only, asked for stopping
    mj = E.compile_model(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc_j", stop=True, njump=JL.LQR_NJUMP, chain=True, **JL.LQR_MASKS)
    mjo = E.compile_model(JL.LQR, 2, 2, ranks=(4,), name="lqr_mc_jonly", njump=JL.LQR_NJUMP, chain=True, **JL.LQR_MASKS)
    wj = JL.lqr_workload(mjo, 4, 0.3)
    ej = E.BellmanEngine(0)
    ej.configure(wj, wl.synth_cores(wj))
    ej.set_jumps(True)
    assert _chain_rcs(torch, ej, 2) == ok
    ej.set_model(mj, wj.params)
    ej.set_stopping(True)
    ej.set_model(mjo, wj.params)  # the model set now lacks the stop kernels: the launch refuses
    assert _chain_rcs(torch, ej, 2) == unsup
    ej.set_stopping(False)
    assert _chain_rcs(torch, ej, 2) == ok
    _still_works(torch, ej, wj)
    # the same source without the chain flag: every mode refused (tests/test_gpu_chain.py holds the plain call)
    mn = E.compile_model(JL.LQR, 2, 2, ranks=(4,), name="lqr_nochain", stop=True, njump=JL.LQR_NJUMP, **JL.LQR_MASKS)
    wn = JL.lqr_workload(mn, 4, 0.3)
    en = E.BellmanEngine(0)
    en.configure(wn, wl.synth_cores(wn))
    assert _chain_rcs(torch, en, 2) == unsup
    en.set_jumps(True)
    assert _chain_rcs(torch, en, 2) == unsup
    en.set_jumps(False)
    _still_works(torch, en, wn)
    # game, impulse and corr modes of chain-compiled models: the features compile, the chain has no form of them
    for mode in ("game", "impulse", "corr"):
        wm, on, off = _mode_model(mode)
        em = E.BellmanEngine(0)
        em.configure(wm, wl.synth_cores(wm))
        assert _chain_rcs(torch, em, 2) == ok, mode
        on(em)
        assert _chain_rcs(torch, em, 2) == unsup, mode
        off(em)
        if mode == "game":
            em.upload_value(wm.ranks, wl.synth_cores(wm))  # the list changed the size of the static data
        assert _chain_rcs(torch, em, 2) == ok, mode
        _still_works(torch, em, wm)
    # a built-in model has no outcomes kernel
    wb = wl.c1_lqg2d(n=11, r=4)
    eb = E.BellmanEngine(0)
    eb.configure(wb, wl.synth_cores(wb))
    assert _chain_rcs(torch, eb, 2) == (0, 0, ERR_UNSUPPORTED)


def test_facade_batch_in_stop_and_jump_mode_in_a_child_process():
    _torch()
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "chain_forms_facade_child.py")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "steps held to the numpy walk" in r.stdout
