"""The approximating Markov chain on the GPU (c3sc_hip_chain_transitions, c3sc_hip_simulate_chain) against the
numpy restatement tests/chain_ref.py, on the cases of tests/chain_cases.py: every case at beta > 0 and beta = 0, on positive and
on signed cores.

- transitions: every node of the 2-D and 3-D grids, a seeded 2000 of car7d, against the reference and against bellman_fibers
  on the same context (value to 1e-12, uidx wherever the margin allows, flags exactly);
- walks: 300 lanes (a second workgroup whose tail repeats the last walk), 24 steps, with Philox and with supplied uniforms,
  both replayed in lock-step by chain_ref.check; launches of 7 steps, a batch split at lane 50 with traj_offset and the host
  entry point all give the same bits;
- one step from 8 nodes under a grid of 257 uniforms each: every pick held to the CDF;
- the certificate J_n + D_n J^pi(xi_n) of 4096 walks from 3 start nodes against the exact policy cost of the 2-D case;
- the refusals, after each of which the context still serves a plain bellman_fibers.
"""
import ctypes as C

import numpy as np
import pytest

import chain_cases as cc
import chain_ref
from c3sc_amd import engine as E
from c3sc_amd import workloads as wl

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 3
TOL = 1e-12

ALL = [(c, b, s) for c in cc.CASES for b in cc.discounts(c) for s in (False, True)]
IDS = [f"{cc.case_id(c)}-beta{b}-{'signed' if s else 'positive'}" for c, b, s in ALL]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("no GPU: the chain kernels have no CPU fallback")
    return torch


@pytest.fixture(scope="module")
def setups(oracle):
    made = {}

    def get(case, beta, signed):
        key = (cc.case_id(case), beta, signed)
        if key not in made:
            w = cc.workload(case, beta)
            cores = cc.cores(case, w, signed)
            eng = E.BellmanEngine(0)
            eng.configure(w, cores)
            eng.set_consistent_ends(True)  # for the bellman_fibers comparison; the chain calls do not read the switch
            made[key] = (w, eng, chain_ref.ChainRef(w, cores))
        return made[key]

    return get


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _run(torch, eng, node0, nsteps, **kw):
    """simulate_chain with every node and decision saved, as chain_ref.check wants it"""
    r = _np(eng.simulate_chain(torch.from_numpy(node0).cuda(), nsteps, save_every=1, **kw))
    r["node0"], r["nsteps"] = node0, nsteps
    return r


def _same_bits(a, b, keys=("cost", "disc", "time", "vend", "node", "exit", "traj", "uidx")):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k


@pytest.mark.parametrize("case,beta,signed", ALL, ids=IDS)
def test_transitions(setups, case, beta, signed):
    torch = _torch()
    w, eng, R = setups(case, beta, signed)
    nodes = cc.all_nodes(w) if w.dx <= 3 else cc.some_nodes(w)
    nodes_t = torch.from_numpy(nodes).cuda()
    res = _np(eng.chain_transitions(nodes_t))
    assert eng.last_kernel() == cc.kernel_names(case)[1]
    unsure = R.check_transitions(nodes, res)
    assert unsure <= 0.025 * len(nodes)
    assert eng.status(clear=True) == 0
    # the same context's Bellman kernels: the fiber along dimension 0 through each node
    n = len(nodes)
    out = torch.empty((n, w.ngrid[0]), dtype=torch.float64).cuda()
    ui = torch.empty((n, w.ngrid[0]), dtype=torch.int32).cuda()
    ab = torch.empty((n, w.ngrid[0]), dtype=torch.int32).cuda()
    eng.bellman_fibers(0, nodes_t, out, ui, ab)
    torch.cuda.synchronize()
    rows = np.arange(n)
    bv, bu, bf = out.cpu().numpy()[rows, nodes[:, 0]], ui.cpu().numpy()[rows, nodes[:, 0]], ab.cpu().numpy()[rows, nodes[:, 0]]
    assert np.array_equal(bf, res["flag"])
    assert (np.abs(bv - res["value"]) <= TOL * np.maximum(1.0, np.abs(bv))).all()
    differ = np.nonzero(bu != res["uidx"])[0]
    for i in differ:
        assert len(R.acceptable(R.node(nodes[i]))) > 1, f"node {nodes[i]}: uidx {res['uidx'][i]} != bellman_fibers' {bu[i]} beyond the margin"
    # the host entry point gives the same bits
    hres = eng.chain_transitions_host(nodes)
    for k in res:
        assert np.array_equal(hres[k].view(np.uint8), res[k].view(np.uint8)), k


@pytest.mark.parametrize("case,beta,signed", ALL, ids=IDS)
def test_walks_in_lock_step(setups, case, beta, signed):
    torch = _torch()
    w, eng, R = setups(case, beta, signed)
    node0 = cc.start_nodes(w)
    n = len(node0)
    # Philox
    run = _run(torch, eng, node0, cc.NSTEPS, seed=cc.SEED)
    assert eng.last_kernel() == cc.kernel_names(case)[0]
    run["uniform"] = R.uniforms(cc.SEED, 0, n, cc.NSTEPS)
    out = R.check(run)
    assert out["unsure"] <= 0.025 * max(out["steps"], 1) and out["steps"] >= n * cc.NSTEPS // 3
    # supplied uniforms
    unif = np.random.default_rng(cc.SEED + 2).random((n, cc.NSTEPS))
    run_u = _run(torch, eng, node0, cc.NSTEPS, uniform_t=torch.from_numpy(unif).cuda())
    run_u["uniform"] = unif
    out = R.check(run_u)
    assert out["unsure"] <= 0.025 * max(out["steps"], 1)
    assert eng.status(clear=True) == 0
    if signed:  # the splits and the host entry point once per (case, beta)
        return
    _same_bits(run, _run(torch, eng, node0, cc.NSTEPS, seed=cc.SEED, steps_per_launch=7))
    a = _run(torch, eng, node0[:50], cc.NSTEPS, seed=cc.SEED)
    b = _run(torch, eng, node0[50:], cc.NSTEPS, seed=cc.SEED, traj_offset=50)
    _same_bits(run, {k: np.concatenate([a[k], b[k]]) for k in a if k not in ("node0", "nsteps")})
    _same_bits(run, eng.simulate_chain_host(node0, cc.NSTEPS, seed=cc.SEED, save_every=1))
    _same_bits(run_u, eng.simulate_chain_host(node0, cc.NSTEPS, uniform=unif, save_every=1, steps_per_launch=5))
    # nothing saved, every optional output off but the cost: the same costs
    t = torch.empty((n,), dtype=torch.float64).cuda()
    a = E.ChainArgs()
    node0_t = torch.from_numpy(node0).cuda()
    a.n, a.d_node0, a.nsteps, a.seed, a.d_cost = n, node0_t.data_ptr(), cc.NSTEPS, cc.SEED, t.data_ptr()
    assert eng.simulate_chain_rc(a, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), run["cost"])


@pytest.mark.parametrize("case", [cc.CASES[1], cc.CASES[2], cc.CASES[4]], ids=cc.case_id)
def test_every_pick_is_held_to_the_cdf(setups, case):
    """one step from 8 nodes under 257 uniforms each: a uniform grid with both end cells, so every outcome with P_k > 1/257 is
    drawn and the first and the last outcome are reached"""
    torch = _torch()
    w, eng, R = setups(case, cc.discounts(case)[0], False)
    starts = [ix for ix in cc.start_nodes(w) if R.node(ix).flag == 0][:8]
    assert len(starts) == 8
    G = 257
    node0 = np.repeat(np.array(starts, dtype=np.int32), G, axis=0)
    grid = np.concatenate(([0.0], (np.arange(1, G - 1) + 0.5) / G, [np.nextafter(1.0, 0.0)]))
    unif = np.tile(grid, 8).reshape(-1, 1)
    run = _run(torch, eng, node0, 1, uniform_t=torch.from_numpy(unif).cuda())
    run["uniform"] = unif
    R.check(run)
    for s, ix in enumerate(starts):  # the empirical law of the 257 picks is the CDF's to one cell per outcome
        t = R.transitions(R.node(ix), int(run["uidx"][s * G, 0]))
        nxt = [tuple(v) for v in run["traj"][s * G:(s + 1) * G, 1]]
        for k in range(2 * w.dx):
            if t.P[k] > 0.0 and R.move(tuple(ix), k) != tuple(ix) and sum(R.move(tuple(ix), kk) == R.move(tuple(ix), k) for kk in range(2 * w.dx)) == 1:
                assert abs(nxt.count(R.move(tuple(ix), k)) / G - t.P[k]) <= 2.0 / G


def test_certificate_on_the_device(oracle):
    import test_chain_ref as T

    torch = _torch()
    case, w, cores = T.stat_problem()
    R = chain_ref.ChainRef(w, cores)
    _, Jpi = T.exact_policy_cost(R, w)
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    node0 = T.stat_start_nodes()
    run = _np(eng.simulate_chain(torch.from_numpy(node0).cuda(), cc.STAT_NSTEPS, seed=cc.STAT_SEED))
    mean, se = T.certificate(R, w, run, Jpi)
    for s, start in enumerate(cc.STAT_STARTS):
        print(f"start {start}: mean {mean[s]:.9f} se {se[s]:.3e} exact {Jpi[start]:.9f} V {R.node(start).V[2 * w.dx]:.9f}")
        assert abs(mean[s] - Jpi[start]) <= 4.0 * se[s] + 1e-9, (start, mean[s], Jpi[start], se[s])


def _plain_bellman_still_works(torch, eng, w):
    idx = torch.from_numpy(wl.synth_fibers(w, 0, 8)).cuda()
    out = eng.bellman_fibers(0, idx)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def _chain_rcs(torch, eng, d, n=4):
    """(return code of simulate_chain, of chain_transitions) for n walks from node 1 of every dimension"""
    node0 = torch.ones((n, d), dtype=torch.int32).cuda()
    cost = torch.empty((n,), dtype=torch.float64).cuda()
    a = E.ChainArgs()
    a.n, a.d_node0, a.nsteps, a.d_cost = n, node0.data_ptr(), 3, cost.data_ptr()
    rc_t = eng.L.c3sc_hip_chain_transitions(eng.h, n, node0.data_ptr(), None, cost.data_ptr(), None, None, None, None, None)
    return eng.simulate_chain_rc(a), int(rc_t)


def test_refusals_leave_the_context_usable(oracle):
    import stop_lib as SL

    torch = _torch()
    # --- C3SC_ERR_ARG on a served problem
    case = cc.CASES[0]
    w = cc.workload(case)
    eng = E.BellmanEngine(0)
    eng.configure(w, cc.cores(case, w, False))
    n, d = 4, w.dx
    node0 = torch.ones((n, d), dtype=torch.int32).cuda()
    cost = torch.empty((n,), dtype=torch.float64).cuda()
    traj = torch.empty((n, 4, d), dtype=torch.int32).cuda()

    def args(**kw):
        a = E.ChainArgs()
        a.n, a.d_node0, a.nsteps, a.d_cost = n, node0.data_ptr(), 3, cost.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert eng.simulate_chain_rc(args()) == 0
    assert eng.simulate_chain_rc(args(d_node0=None)) == ERR_ARG
    assert eng.simulate_chain_rc(args(d_traj=traj.data_ptr())) == ERR_ARG  # save_every = 0
    assert eng.simulate_chain_rc(args(d_uidx=traj.data_ptr())) == ERR_ARG
    assert eng.L.c3sc_hip_simulate_chain(eng.h, None, None) == ERR_ARG
    assert eng.L.c3sc_hip_chain_transitions(eng.h, n, None, None, cost.data_ptr(), None, None, None, None, None) == ERR_ARG
    for bad in ((-1, 1), (1, w.ngrid[1]), (w.ngrid[0], 0)):
        node0[2] = torch.tensor(bad, dtype=torch.int32)
        assert _chain_rcs(torch, eng, d) == (0, 0)  # its own, valid nodes
        assert eng.simulate_chain_rc(args()) == ERR_ARG
        assert eng.L.c3sc_hip_chain_transitions(eng.h, n, node0.data_ptr(), None, cost.data_ptr(), None, None, None, None, None) == ERR_ARG
        node0[2] = 1
    _plain_bellman_still_works(torch, eng, w)
    # no boundary types at all (set_boundary itself refuses a C3SC_EB_NONE dimension, so this is how a context has one)
    enb = E.BellmanEngine(0)
    enb.set_grid(w.ngrid, w.xgrid())
    enb.set_model(w.model, w.params)
    enb.set_controls(w.cands)
    assert _chain_rcs(torch, enb, d) == (ERR_ARG, ERR_ARG)
    # --- C3SC_ERR_UNSUPPORTED
    # a control box and no candidate list
    xg = w.xgrid()
    engb2 = E.BellmanEngine(0)
    engb2.set_grid(w.ngrid, xg)
    engb2.set_boundary(w.bc, w.obstacles)
    h2 = min(g[1] - g[0] for g in xg) ** 2
    engb2.set_mca(h2, [v for g in xg for v in (h2 / (g[1] - g[0]), h2 / (g[1] - g[0]) ** 2)], w.discount)
    engb2.set_model(w.model, w.params)
    engb2.upload_value(w.ranks, cc.cores(case, w, False))
    engb2.set_control_box([-1.0], [1.0])
    assert _chain_rcs(torch, engb2, d) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
    engb2.set_controls(w.cands)
    engb2.upload_value(w.ranks, cc.cores(case, w, False))  # the list changed the size of the static data
    assert _chain_rcs(torch, engb2, d) == (0, 0)
    # no instantiation: a model without chain kernels (chain4), and cothrust6d at the pair kernel's class 10
    import sim_kernel_cases as skc

    for wn in (skc._chain(4), wl.cothrust6d().scaled(ngrid=(5,) * 6, rank=10)):
        e = E.BellmanEngine(0)
        e.configure(wn, wl.synth_cores(wn))
        assert _chain_rcs(torch, e, wn.dx) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
        _plain_bellman_still_works(torch, e, wn)
    # the TABLE model
    et = E.BellmanEngine(0)
    et.configure(w, cc.cores(case, w, False))
    et.set_model(100, ())  # C3SC_MODEL_TABLE
    assert _chain_rcs(torch, et, d) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
    et.set_model(w.model, w.params)
    assert _chain_rcs(torch, et, d) == (0, 0)
    # a run-time compiled model, plain and with its modes on (stopping, horizon)
    mid = E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_chain_refusal", horizon=True, stop=True, **SL.LQR_MASKS)
    wr = wl.Workload("lqr_os", mid, tuple(SL.LQR_PRM), 2, 2, (-2.0, -2.0), (2.0, 2.0), (9, 12), wl.uniform_ranks(2, 3), 0.1,
                     (wl.BC_REFLECT, wl.BC_REFLECT), [], SL.lqr_cands())
    er = E.BellmanEngine(0)
    er.configure(wr, wl.synth_cores(wr))
    assert _chain_rcs(torch, er, 2) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
    _plain_bellman_still_works(torch, er, wr)
    er.set_stopping(True)
    assert _chain_rcs(torch, er, 2) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
    er.set_stopping(False)
    er.set_horizon_step(0.001)
    assert _chain_rcs(torch, er, 2) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
    er.set_horizon_step(0.0)
    _plain_bellman_still_works(torch, er, wr)


def _mode_model(mode):
    """(workload of a run-time compiled model with the mode's kernels, the call that switches the mode on, the one that ends it)"""
    import corr_lib as CL
    import impulse_lib as IL
    import jump_lib as JL
    import stop_lib as SL

    if mode in ("jump", "impulse"):
        mid = E.compile_model(IL.LQR_JUMP, 2, 2, ranks=(4,), name="lqr_chain_ic", njump=JL.LQR_NJUMP, nimpulse=IL.LQR_NIMPULSE, **IL.LQR_MASKS)
        w = IL.lqr_workload(mid, 4, 0.3, IL.lqr_cost_scale(4))
        if mode == "jump":
            return w, (lambda e: e.set_jumps(True)), (lambda e: e.set_jumps(False))
        return w, (lambda e: e.set_impulses(True)), (lambda e: e.set_impulses(False))
    if mode == "corr":
        mid = E.compile_model(CL.LQR, 2, 2, ranks=(4,), name="lqr_chain_cd", corr_pairs=CL.LQR_PAIRS, **CL.LQR_MASKS)
        return CL.lqr_workload(mid, 4, 0.1, CL.LQR_PRM), (lambda e: e.set_correlation(True)), (lambda e: e.set_correlation(False))
    mid = E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_chain_game", game=True, **SL.LQR_MASKS)
    w = wl.Workload("lqr_game", mid, tuple(SL.LQR_PRM), 2, 2, (-2.0, -2.0), (2.0, 2.0), (9, 12), wl.uniform_ranks(2, 3), 0.1,
                    (wl.BC_REFLECT, wl.BC_REFLECT), [], SL.lqr_cands())

    def game_on(e):  # the product list changes the size of the static data: the value goes up again
        e.set_game(np.array([[0.0], [1.0]]), np.array([[0.0], [0.5]]))
        e.upload_value(w.ranks, wl.synth_cores(w))

    return w, game_on, (lambda e: e.set_controls(w.cands))


@pytest.mark.parametrize("mode", ["game", "jump", "impulse", "corr"])
def test_mode_refusals_leave_the_context_usable(oracle, mode):
    """a context in game, jump, impulse or correlation mode (stopping and horizon: test_refusals_leave_the_context_usable): both
    entry points return C3SC_ERR_UNSUPPORTED, and with the mode ended the context serves a plain bellman_fibers"""
    torch = _torch()
    w, on, off = _mode_model(mode)
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    on(eng)
    assert _chain_rcs(torch, eng, w.dx) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
    idx = torch.from_numpy(wl.synth_fibers(w, 0, 8)).cuda()
    assert torch.isfinite(eng.bellman_fibers(0, idx)).all()  # the mode's own backup still runs
    assert _chain_rcs(torch, eng, w.dx) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)
    off(eng)
    if mode == "game":
        eng.upload_value(w.ranks, wl.synth_cores(w))  # the list changed the size of the static data
    _plain_bellman_still_works(torch, eng, w)
    assert _chain_rcs(torch, eng, w.dx) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED)  # a run-time compiled model has no chain kernels


def test_stuck_nodes_freeze_the_walk():
    """lqg2d without noise and with the single candidate u = 0 on 9 x 13 nodes: drift (x_1, 0), so every rate vanishes on the grid
    line x_1 = 0 (index 6) and elsewhere the chain moves along dimension 0 with probability 1.  The oracle refuses such a
    problem, so the expectations are written out here."""
    torch = _torch()
    w = wl.c1_lqg2d().scaled(ngrid=(9, 13))
    w.ranks, w.params, w.cands = (1, 3, 1), (2.0, 0.0, 0.0), np.array([[0.0]])
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    nodes = cc.all_nodes(w)
    res = _np(eng.chain_transitions(torch.from_numpy(nodes).cuda()))
    assert eng.status(clear=True) & E.STATUS_STATIONARY
    line = nodes[:, 1] == 6
    assert (res["flag"] == 0).all()
    assert (res["uidx"][line] == -1).all() and (res["dt"][line] == 0.0).all() and (res["P"][line] == 0.0).all()
    assert (res["uidx"][~line] == 0).all() and (res["dt"][~line] > 0.0).all()
    up = nodes[:, 1] > 6  # x_1 > 0: to the hi neighbour of dimension 0 with probability 1
    assert (res["P"][up, 1] == 1.0).all() and (res["P"][~line & ~up, 0] == 1.0).all() and (res["P"][:, 2:] == 0.0).all()
    xg = w.xgrid()
    x = np.stack([xg[0][nodes[:, 0]], xg[1][nodes[:, 1]]], -1)
    assert np.allclose(res["stage"], (x ** 2).sum(-1), rtol=1e-14, atol=0)
    # walks: on the line a lane is stuck at step 0 and stays; beside it the walk runs into the reflecting end and loops there
    node0 = np.array([[3, 6], [3, 7], [5, 6], [5, 2]], dtype=np.int32)
    run = _run(torch, eng, node0, 10, seed=1)
    assert eng.status(clear=True) & E.STATUS_STATIONARY
    assert run["exit"].tolist() == [-2, -1, -2, -1]  # C3SC_CHAIN_STUCK(0)
    assert E.decode_chain_exit(run["exit"])[1].tolist() == ["stuck", "running", "stuck", "running"]
    for i in (0, 2):
        assert (run["traj"][i] == node0[i]).all() and (run["uidx"][i] == -1).all()
        assert run["cost"][i] == 0.0 and run["disc"][i] == 1.0 and run["time"][i] == 0.0
    assert run["traj"][1, :, 0].tolist() == [3, 4, 5, 6, 7, 8, 8, 8, 8, 8, 8] and (run["traj"][1, :, 1] == 7).all()
    assert run["traj"][3, :, 0].tolist() == [5, 4, 3, 2, 1, 0, 0, 0, 0, 0, 0] and (run["uidx"][[1, 3]] == 0).all()
    assert run["time"][1] > 0.0 and run["disc"][1] < 1.0
