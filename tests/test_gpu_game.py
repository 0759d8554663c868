"""Zero-sum games on the GPU (c3sc_hip_set_game).

- The game per-wave kernel against the dense numpy restatement of game_lib on random fibers with boundary, obstacle and periodic
  nodes: the 2-D LQ game and the pursuit game, ranks 4 and 8, both orders, beta > 0 and beta = 0.  Values to 1e-12 relative,
  indices wherever the winning margin exceeds 1e-9 relative.
- Exact properties: lower value <= upper value node by node; with nw = 1 the outputs, indices and absorbed flags are the plain
  per-wave kernel's bits.
- A stationary candidate (Q < 1e-14) raises the status bit and takes no part in either reduction.
- Closed loops in both orders: the first saved control is the numpy saddle pair at x0 (c3sc_hip_stencil_points); forward Euler with one substep equals
  simulate without noise.  Policy evaluation applies the given pair index in both orders.
- Value iteration of the LQ game through the reference API (first-fiber check, device-resident cross) against the dense
  Markov chain sweep by sweep, and the host c3control_policy_eval against the dense saddle pairs.
- examples/pursuit_game.c builds, reaches its tolerance and reports finite capture times.
- Errors: the pair and quad variants, the control box, built-in models, the TABLE path and a model compiled without game
  kernels."""
import dataclasses
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import backup_ref as BR
import game_lib
from game_lib import (LQGAME, LQGAME_MASKS, LQGAME_PRM, PURSUIT, PURSUIT_MASKS, PURSUIT_PRM, game_backup, lqgame_host, product,
                      pursuit_host)

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = 1, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_LQ = np.linspace(-1.0, 1.0, 9).reshape(-1, 1)
W_LQ = np.linspace(-0.5, 0.5, 5).reshape(-1, 1)
U_PU = np.linspace(-1.0, 1.0, 5).reshape(-1, 1)
W_PU = np.linspace(-1.0, 1.0, 7).reshape(-1, 1)


@pytest.fixture(scope="module")
def ids():
    return {
        "lq": E.compile_model(LQGAME, 2, 2, ranks=(4, 8), name="lqgame", game=True, **LQGAME_MASKS),
        "pursuit": E.compile_model(PURSUIT, 3, 2, ranks=(4, 8), name="pursuit", game=True, **PURSUIT_MASKS),
        "lq_plain": E.compile_model(LQGAME, 2, 2, ranks=(4,), name="lqgame_nogame", **LQGAME_MASKS),
    }


def lq_workload(mid, rank, discount, ngrid=(21, 19)):
    return wl.Workload("lqgame", mid, LQGAME_PRM, 2, 2, (-2.0, -2.0), (2.0, 2.0), ngrid, wl.uniform_ranks(2, rank), discount,
                       (wl.BC_ABSORB, wl.BC_REFLECT), [((0.9, -0.9), (0.5, 0.6))], product(U_LQ, W_LQ))


def pursuit_workload(mid, rank, discount):
    return wl.Workload("pursuit", mid, PURSUIT_PRM, 3, 2, (-3.0, -3.0, -np.pi), (3.0, 3.0, np.pi), (23, 21, 17),
                       wl.uniform_ranks(3, rank), discount, (wl.BC_ABSORB, wl.BC_ABSORB, wl.BC_PERIODIC),
                       [((0.0, 0.0, 0.0), (0.5, 0.5, 2 * np.pi + 1.0))], product(U_PU, W_PU))


def _engine(w, variant=E.VARIANT_AUTO):
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    eng.set_variant(variant)
    return eng


CASES = [("lq", lq_workload, lqgame_host, U_LQ, W_LQ, 100.0), ("pursuit", pursuit_workload, pursuit_host, U_PU, W_PU, 20.0)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("rank", [4, 8])
@pytest.mark.parametrize("discount", [0.1, 0.0])
def test_per_wave_game_vs_numpy(ids, case, rank, discount):
    name, mk, host, U, W, bcost = case
    w = mk(ids[name], rank, discount)
    eng = _engine(w)
    vals = {}
    for order in ("minmax", "maxmin"):
        eng.set_game(U, W, order)
        for k in range(w.dx):
            idx = wl.synth_fibers(w, k, 257)
            out, ui, ab = eng.bellman_fibers_host(k, idx)
            assert eng.last_kernel().startswith("k_fiber_per_wave<rtc:")
            costs, sab = eng.stencil_fibers_host(k, idx)
            np.testing.assert_array_equal(ab, sab)
            assert (ab == 1).any() and (ab == 0).any(), "fibers must include boundary and live nodes"
            r_out, r_ui, mg, _ = game_backup(w, host, k, idx, costs, ab, U, W, order, bcost, 0.0)
            scale = np.maximum(1.0, np.abs(r_out))
            assert np.all(np.abs(out - r_out) <= 1e-12 * scale), (order, k, np.abs(out - r_out).max())
            sure = mg > 1e-9
            np.testing.assert_array_equal(ui[sure], r_ui[sure])
            vals[(order, k)] = (out, ui, ab)
    for k in range(w.dx):
        lo, up = vals[("maxmin", k)][0], vals[("minmax", k)][0]
        assert np.all(lo <= up), "lower value above upper value"
    if name == "pursuit":
        assert any((v[2] == -1).any() for v in vals.values()), "the capture box (obstacle) must be met"


@pytest.mark.parametrize("discount", [0.1, 0.0])
@pytest.mark.parametrize("order", ["minmax", "maxmin"])
def test_nw_1_is_the_plain_kernel_bit_for_bit(ids, discount, order):
    w = dataclasses.replace(lq_workload(ids["lq"], 4, discount), cands=product(U_LQ, [[0.25]]))
    plain = _engine(w)
    game = _engine(w)
    game.set_game(U_LQ, [[0.25]], order)
    for k in range(2):
        idx = wl.synth_fibers(w, k, 300)
        a = plain.bellman_fibers_host(k, idx)
        b = game.bellman_fibers_host(k, idx)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


def test_stationary_candidate_is_skipped_in_both_reductions(ids):
    # no diffusion: at nodes with x1 = 0 the pair u = -w has zero drift, i.e. Q = 0
    U, W = np.array([[-0.5], [0.0], [0.5]]), np.array([[-0.5], [0.0], [0.5]])
    w = dataclasses.replace(lq_workload(ids["lq"], 4, 0.1, ngrid=(21, 21)), params=(0.0, 0.0, 1.0, 4.0), cands=product(U, W))
    eng = _engine(w)
    for order in ("minmax", "maxmin"):
        eng.set_game(U, W, order)
        eng.status(clear=True)
        idx = wl.synth_fibers(w, 0, 64)
        idx[:, 1] = 10  # x1 = 0
        out, ui, ab = eng.bellman_fibers_host(0, idx)
        assert eng.status(clear=True) & 1
        costs, _ = eng.stencil_fibers_host(0, idx)
        r_out, r_ui, mg, st = game_backup(w, lqgame_host, 0, idx, costs, ab, U, W, order, 100.0, 0.0)
        assert st.any()
        np.testing.assert_allclose(out, r_out, rtol=1e-12, atol=1e-12)
        live = ab == 0
        assert np.all(ui[live] >= 0)
        sure = mg > 1e-9
        np.testing.assert_array_equal(ui[sure], r_ui[sure])


@pytest.mark.parametrize("order", ["minmax", "maxmin"])
def test_closed_loops_apply_the_saddle_pair(ids, order):
    """the rollouts look the saddle pair up at its list position (w-major in MAXMIN): the first saved control of every trajectory
    is the numpy min-max at x0 over the off-grid stencil there (c3sc_hip_stencil_points); forward Euler with one substep is
    simulate without noise"""
    import torch

    w = lq_workload(ids["lq"], 4, 0.1)
    eng = _engine(w)
    eng.set_game(U_LQ, W_LQ, order)
    rng = np.random.default_rng(5)
    n = 400
    x0 = torch.tensor(rng.uniform(-1.5, 1.5, (n, 2)), device="cuda")
    sim = eng.simulate(x0, 0.01, 20, noise_t=torch.zeros((n, 20, 2), dtype=torch.float64, device="cuda"), save_every=1)
    ode = eng.integrate(x0, 0.01, 20, method="forward-euler", save_every=1)
    np.testing.assert_array_equal(sim["traj"].cpu().numpy(), ode["traj"].cpu().numpy())
    np.testing.assert_array_equal(sim["u"].cpu().numpy(), ode["u"].cpu().numpy())
    V, ab = eng.stencil_points(x0)
    V, ab = V.cpu().numpy(), ab.cpu().numpy()
    h2, t = BR.mca_constants(w)
    vals, _ = game_lib.candidate_values(lqgame_host, w.params, x0.cpu().numpy(), V, U_LQ, W_LQ, h2, t, w.discount)
    _, ui, mg = game_lib.minmax(vals, order)
    u0 = ode["u"].cpu().numpy()[:, 0, :]
    pairs = product(U_LQ, W_LQ)
    live, sure = ab == 0, mg > 1e-9
    assert live.sum() > n // 2 and (live & sure).sum() > n // 2
    np.testing.assert_array_equal(u0[live & sure], pairs[ui[live & sure]])
    np.testing.assert_array_equal(u0[~live], 0.0)
    assert len({tuple(r) for r in u0[live]}) > 1


@pytest.mark.parametrize("order", ["minmax", "maxmin"])
def test_policy_evaluation_applies_the_given_pair(ids, order):
    """the forced path (policy_fibers) takes pair indices iu * nw + iw in either order: the value of the given pair"""
    w = lq_workload(ids["lq"], 4, 0.1)
    eng = _engine(w)
    eng.set_game(U_LQ, W_LQ, order)
    rng = np.random.default_rng(11)
    for k in range(2):
        idx = wl.synth_fibers(w, k, 100)
        pol = rng.integers(0, len(U_LQ) * len(W_LQ), (100, w.ngrid[k])).astype(np.int32)
        out, ab = eng.policy_fibers_host(k, idx, pol)
        costs, _ = eng.stencil_fibers_host(k, idx)
        h2, t = BR.mca_constants(w)
        x = BR.node_states(w, k, idx).reshape(-1, 2)
        vals, _ = game_lib.candidate_values(lqgame_host, w.params, x, costs.reshape(-1, 5), U_LQ, W_LQ, h2, t, w.discount)
        ref = vals.reshape(len(x), -1)[np.arange(len(x)), pol.reshape(-1)].reshape(out.shape)
        ref = np.where(ab == 1, 100.0, np.where(ab == -1, 0.0, ref))
        assert np.all(np.abs(out - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref)))


@pytest.mark.parametrize("order", ["minmax", "maxmin"])
def test_value_iteration_through_the_reference_api(tmp_path, order):
    """the LQ game on an 11 x 11 grid at rank 11 (padded 12; the train is exact) through libc3sc.so in a child process: a game
    c3Opt beside the host callbacks, c3control_vi_solve sweep by sweep.  The first sweep passes the first-fiber check against
    the host twin, the next ones take the device-resident cross; every sweep equals one sweep of the dense Markov chain of
    game_lib to 1e-9; c3control_policy_eval returns the dense saddle pair at every interior node"""
    out = tmp_path / "vi.npz"
    prog = f"import game_lib; game_lib.vi_child({order!r}, 6, {str(out)!r})"
    env = dict(os.environ, C3SC_CROSS_TRACE="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, "-c", prog], cwd=os.path.dirname(os.path.abspath(__file__)), env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "c3sc cross trace: speculate" in r.stderr  # the device-resident cross iterations ran
    d = np.load(out)
    hist, pol = d["V"], d["pol"]
    mid = E.compile_model(LQGAME, 2, 2, ranks=(12,), name="lqgame_vi", game=True, **LQGAME_MASKS)
    w, U, W = game_lib.lq_vi_workload(mid)
    for s in range(1, len(hist)):
        ref, _, _ = game_lib.dense_sweep(w, hist[s - 1], U, W, order)
        err = np.abs(hist[s] - ref) / np.maximum(1.0, np.abs(ref))
        assert err.max() <= 1e-9, (s, err.max())
    _, ui, mg = game_lib.dense_sweep(w, hist[-1], U, W, order)
    inner = np.zeros_like(mg, dtype=bool)
    inner[1:-1, 1:-1] = True
    sure = inner & (mg > 1e-9)
    assert sure.sum() > inner.sum() // 2
    np.testing.assert_array_equal(pol[sure], product(U, W)[ui[sure]])


def test_pursuit_example(tmp_path):
    exe = str(tmp_path / "pursuit_game")
    host, csrc = os.path.join(ROOT, "c3sc_amd", "host"), os.path.join(ROOT, "c3sc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-D_POSIX_C_SOURCE=200809L", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pursuit_game.c"), "-L", host, "-L", csrc, "-lc3sc", "-lc3sc_hip", "-lm",
                           f"-Wl,-rpath,{host}", f"-Wl,-rpath,{csrc}", "-o", exe])
    env = dict(os.environ, C3SC_CROSS_TRACE="1")
    p = subprocess.run([exe, "21"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "PURSUIT_GAME_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "c3sc cross trace: speculate" in p.stderr
    m = re.search(r"(\d+) captured \(mean capture time ([^,\s]+), longest ([^)\s]+)\)", p.stdout)
    assert int(m.group(1)) > 0 and np.isfinite(float(m.group(2))) and 0.0 < float(m.group(2)) <= float(m.group(3))


def test_errors(ids):
    w = lq_workload(ids["lq"], 4, 0.1)
    idx = wl.synth_fibers(w, 0, 8)
    for v in (E.VARIANT_FIBER_PAIR, E.VARIANT_FIBER_QUAD):
        eng = _engine(w)
        eng.set_game(U_LQ, W_LQ)
        eng.set_variant(v)
        with pytest.raises(RuntimeError):
            eng.bellman_fibers_host(0, idx)
        assert eng.L.c3sc_hip_bellman_fibers_host(eng.h, 0, 8, idx.ctypes.data, np.empty((8, 21)).ctypes.data, None, None) == ERR_UNSUPPORTED
    eng = _engine(w)
    eng.set_game(U_LQ, W_LQ)
    eng.set_control_box([-1.0, -0.5], [1.0, 0.5], grid=5, polish=0)
    with pytest.raises(RuntimeError):
        eng.bellman_fibers_box_host(0, idx)
    # sizes that do not add up, a bad order
    u = np.zeros((2, 2))
    assert eng.L.c3sc_hip_set_game(eng.h, 2, 2, u.ctypes.data_as(E.c_double_p), 2, u.ctypes.data_as(E.c_double_p), 0) == ERR_ARG
    assert eng.L.c3sc_hip_set_game(eng.h, 1, 2, u.ctypes.data_as(E.c_double_p), 2, u.ctypes.data_as(E.c_double_p), 7) == ERR_ARG
    # a model compiled without game kernels, a built-in model
    for mid in (ids["lq_plain"], wl.MODEL_LQGND):
        e2 = _engine(dataclasses.replace(w, model=mid))
        assert e2.L.c3sc_hip_set_game(e2.h, 1, 2, u.ctypes.data_as(E.c_double_p), 2, u.ctypes.data_as(E.c_double_p), 0) == ERR_UNSUPPORTED
    # the TABLE path refuses game mode
    eng = _engine(w)
    eng.set_game(U_LQ, W_LQ)
    tables = np.zeros((8, 21, len(U_LQ) * len(W_LQ), 5))
    with pytest.raises(RuntimeError):
        eng.bellman_fibers_tables_host(0, idx, tables, np.zeros((8, 21, 2)))
