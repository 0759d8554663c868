"""Policy iteration on jump diffusions on the GPU, and the several-dimension calls in every operator mode.

- c3control_pi_solve of the jump LQR through libc3sc.so in a child process (jump_lib.pi_child), once as it comes and once under
  C3SC_HOST_CROSS=1: every result equals jump_lib.dense_pi's V_K to 1e-9 at every node -- a policy taken without the jump term,
  an evaluation without it or a policy re-taken every sweep would move it by 0.32, 2.9 and 0.16 (tests/test_jump_lib.py holds
  those as preconditions); the device-resident driver did run (trace) where it should and did not where it should not; the two
  drivers agree bit for bit, and so does the host-driven driver with itself before and after the first-fiber check.
- c3sc_hip_cross_iteration_pi with both contexts in jump mode against jump_policy_model.JumpPolicyProblem, on the ragged 2-D grid
  and on a 3-D grid with three boundary types: the first greedy candidate of the policy train stays for a tag, a new tag resets
  it (cross_memo_model.run_policy_scenario; tests/test_jump_lib.py runs the same cases on the CPU, clean and with planted
  mistakes).  Contexts that differ in jump mode are refused: tests/test_gpu_jump.py::test_errors.
- c3sc_hip_bellman_fibers_all / c3sc_hip_policy_fibers_all in jump mode, jump + stop + horizon, horizon, stop and game mode equal
  the per-dimension calls bit for bit in values, indices and flags, on ragged batch sizes.
- A forced index of -1 at a live node gives 0.0 in jump mode, flags unchanged."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from c3sc_amd import engine as E
from c3sc_amd import workloads as wl
import game_lib as GL
import gpu_case_lib as GC
import horizon_lib as H
import jump_lib as JL
import jump_policy_model as JP
import stop_lib as SL
from cross_device_lib import DeviceCross

pytestmark = pytest.mark.gpu
LQR_DELTA, LQR3_DELTA = 0.01, 0.004  # inside the CFL rule on both grids (tests/test_gpu_jump.py)
TRACE = "c3sc cross trace: speculate"


@pytest.fixture(scope="module")
def ids():
    """the specs of tests/test_gpu_jump.py, test_gpu_horizon.py, test_gpu_stop.py and test_gpu_game.py word for word: a spec compiled
    earlier in the process is not compiled again, so in a run of the whole suite this file compiles nothing of its own but
    pi_child's model.  The 3-D model has rank-12 kernels only; the rank-4 trains of this file run on them padded"""
    return {
        "lqr": E.compile_model(JL.LQR, 2, 2, ranks=(4, 8, 12), name="lqr_jd", horizon=True, stop=True, njump=JL.LQR_NJUMP, **JL.LQR_MASKS),
        "lqr3": E.compile_model(JL.LQR3, 3, 3, ranks=(12,), name="lqr3_jd", horizon=True, stop=True, njump=JL.LQR3_NJUMP, **JL.LQR3_MASKS),
        "horizon": E.compile_model(H.LQR, 2, 2, ranks=(4, 8), name="lqr_fh", horizon=True, **H.LQR_MASKS),
        "stop": E.compile_model(SL.LQR, 2, 2, ranks=(4,), name="lqr_stop_only", stop=True, **SL.LQR_MASKS),
        "game": E.compile_model(GL.LQGAME, 2, 2, ranks=(4, 8), name="lqgame", game=True, **GL.LQGAME_MASKS),
    }


# ---------------------------------------------------------------------------------------------------- the reference API
def _child(out, host_cross):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, C3SC_CROSS_TRACE="1")
    env.pop("C3SC_HOST_CROSS", None)
    if host_cross:
        env["C3SC_HOST_CROSS"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    return subprocess.run([sys.executable, "-c", f"import jump_lib; jump_lib.pi_child({str(out)!r})"],
                          cwd=os.path.dirname(os.path.abspath(__file__)), env=env, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def pi_runs(tmp_path_factory):
    """jump_lib.pi_child with the default environment ("device") and under C3SC_HOST_CROSS=1 ("host"): (saved arrays, the parts of
    stderr before the first marker, between the markers and after the second); and the dense chains"""
    tmp = tmp_path_factory.mktemp("jump_pi")
    runs = {}
    for name in ("device", "host"):
        out = tmp / f"{name}.npz"
        r = _child(out, name == "host")
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert r.stderr.count(JL.PI_MARKERS[0]) == 1 and r.stderr.count(JL.PI_MARKERS[1]) == 1, r.stderr[-4000:]
        head, rest = r.stderr.split(JL.PI_MARKERS[0])
        mid, tail = rest.split(JL.PI_MARKERS[1])
        runs[name] = (dict(np.load(out)), (head, mid, tail))
    w = JL.lqr_vi_workload(0)
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    bcost = lambda x: H.lqr_terminal(JL.LQR_PRM, x)
    P = H.lqr_terminal(JL.LQR_PRM, X)
    mu, margin, V = JL.dense_pi(w, SL.lqrn_host, JL.lqr_jumps, bcost, P, max(JL.PI_AFTER))
    assert margin[mu >= 0].min() >= 1e-6, "the greedy candidate of P is pinned at every live node: every node is compared"
    vi = JL.dense_vi(w, SL.lqrn_host, JL.lqr_jumps, bcost, P, 1)
    return runs, V, vi


def _rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


@pytest.mark.parametrize("run", ["device", "host"])
def test_pi_solve_equals_the_dense_policy_iteration(pi_runs, run):
    """c3control_pi_solve(K, policy = s |x|^2) = V_K of jump_lib.dense_pi at every node to 1e-9 of max(1, |V|), before the
    first-fiber check (host-driven pi_core) and after it (device-resident cross_iteration_pi, or host-driven again under
    C3SC_HOST_CROSS=1); the vi step in between equals dense_vi's first sweep.
    Measured on the MI355X: 6.6e-15 at worst (K = 3), the vi step 4.1e-15, the same in both runs."""
    runs, V, vi = pi_runs
    z, _ = runs[run]
    assert _rel(z["V0"], V[0]) <= 1e-12, "init_value of s |x|^2 at rank 11 is exact"
    worst = 0.0
    for part, Ks in (("before", JL.PI_BEFORE), ("after", JL.PI_AFTER)):
        assert z[part].shape == (len(Ks),) + V[0].shape
        for got, K in zip(z[part], Ks):
            err = _rel(got, V[K])
            worst = max(worst, err)
            print(f"{run} run, pi_solve({K}) {part} the vi step: worst error against the dense chain {err:.3e}")
            assert err <= 1e-9, (run, part, K, err)
    err = _rel(z["vi"], vi[1])
    print(f"{run} run, the vi step: worst error against dense_vi {err:.3e}; pi_solve overall {worst:.3e}")
    assert err <= 1e-9, (run, err)


def test_pi_solve_took_the_driver_it_should_and_both_give_the_same_bits(pi_runs):
    runs, _, _ = pi_runs
    (zd, (head_d, mid_d, tail_d)), (zh, (head_h, mid_h, tail_h)) = runs["device"], runs["host"]
    print("default run: trace lines before the first marker", head_d.count(TRACE), "between the markers", mid_d.count(TRACE),
          "after the second", tail_d.count(TRACE), "; C3SC_HOST_CROSS=1 run:", (head_h + mid_h + tail_h).count(TRACE))
    assert head_d.count(TRACE) == 0, "the model was not yet checked against the host callbacks: the host-driven pi_core"
    assert tail_d.count(TRACE) >= 1, "after the first-fiber check the device-resident cross_iteration_pi runs"
    assert (head_h + mid_h + tail_h).count(TRACE) == 0, "C3SC_HOST_CROSS=1 keeps every interpolation on the host-driven path"
    for i, K in enumerate(JL.PI_AFTER):
        same = np.array_equal(zd["after"][i], zh["after"][i])
        print(f"pi_solve({K}) after the vi step: device-resident and host-driven", "bit-identical" if same else
              f"differ by {np.abs(zd['after'][i] - zh['after'][i]).max():.3e}")
        assert same, (K, np.abs(zd["after"][i] - zh["after"][i]).max())
    for i, K in enumerate(JL.PI_BEFORE):  # the host-driven driver with itself, before and after the vi step
        j = JL.PI_AFTER.index(K)
        assert np.array_equal(zh["before"][i], zh["after"][j]), (K, np.abs(zh["before"][i] - zh["after"][j]).max())
    assert np.array_equal(zd["vi"], zh["vi"]) and np.array_equal(zd["before"], zh["before"])


# ---------------------------------------------------------------------------------------------------- cross_iteration_pi at step level
class _JumpCross(DeviceCross):
    """a DeviceCross in jump mode that remembers the kernel its last launch named"""
    kernels = []

    def __init__(self, w, cores):
        super().__init__(w, cores)
        self.eng.set_jumps(True)

    def close(self):
        _JumpCross.kernels.append(self.last_kernel())
        super().close()


@pytest.mark.parametrize("case", JP.CASES, ids=[c[0] for c in JP.CASES])
def test_the_policy_memo_in_jump_mode_keeps_the_first_candidate_for_a_tag(oracle, ids, case):
    _JumpCross.kernels = []
    reps = JP.scenario(_JumpCross, oracle, case, ids[case[1]])
    for what, rep in zip(("tag 7 under P1", "tag 7 under P2", "tag 8 under P2"), reps):
        print(f"{case[0]} {what}: {rep['policies_stored']} stored, {rep['hits']} hits, {rep['policy_differing']} differing; "
              f"core 0 within {rep['raw']:.1e} of the stand-in, worst residual {max(s['residual'] or 0.0 for s in rep['steps']):.1e}")
    print(f"{case[0]}: kernels {_JumpCross.kernels}")
    assert len(_JumpCross.kernels) == 2 and all(k.startswith("k_fiber_per_wave<rtc:") for k in _JumpCross.kernels), _JumpCross.kernels


# ---------------------------------------------------------------------------------------------------- the _all forms
def _all_equals_the_per_dimension_calls(eng, w, nact, label):
    """bellman_fibers_all and policy_fibers_all against c3sc_hip_bellman_fibers / c3sc_hip_policy_fibers per dimension: values,
    indices and flags bit for bit, no status bit.  nact: the forced indices are drawn from 0 .. nact - 1"""
    import torch

    L, h, d = eng.L, eng.h, w.dx
    sizes = (5, 37, 130)[:d]
    ks = list(range(d))
    idx = [torch.from_numpy(wl.synth_fibers(w, k, F, seed=0xA11 + F)).cuda() for k, F in zip(ks, sizes)]
    shapes = [(F, w.ngrid[k]) for k, F in zip(ks, sizes)]
    gen = torch.Generator(device="cuda").manual_seed(5)
    pol = [torch.randint(0, nact, s, dtype=torch.int32, device="cuda", generator=gen) for s in shapes]
    KS, FS = (C.c_int * d)(*ks), (C.c_size_t * d)(*sizes)

    def fresh():
        return ([torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in shapes],
                [torch.full(s, -7, dtype=torch.int32, device="cuda") for s in shapes],
                [torch.full(s, -7, dtype=torch.int32, device="cuda") for s in shapes])

    eng.status(clear=True)
    out, ui, ab = fresh()
    for s, k in enumerate(ks):
        rc = L.c3sc_hip_bellman_fibers(h, k, sizes[s], idx[s].data_ptr(), out[s].data_ptr(), ui[s].data_ptr(), ab[s].data_ptr(), None)
        assert rc == 0, (label, k, eng.L.c3sc_hip_last_error(h))
        assert eng.last_kernel().startswith("k_fiber_per_wave<rtc:"), eng.last_kernel()
    torch.cuda.synchronize()
    assert eng.status(clear=True) == 0, label
    a_out, a_ui, a_ab = fresh()
    rc = L.c3sc_hip_bellman_fibers_all(h, d, KS, FS, GC.ptrs(idx), GC.ptrs(a_out), GC.ptrs(a_ui), GC.ptrs(a_ab), C.c_void_p(None))
    assert rc == 0, (label, eng.L.c3sc_hip_last_error(h))
    torch.cuda.synchronize()
    assert eng.status(clear=True) == 0, label
    assert any((t != 0).any() for t in ab), "the batches hold absorbed nodes as well"
    for s in range(d):
        assert not torch.isnan(out[s]).any() and (ab[s] == 0).any(), (label, s)
        assert torch.equal(a_out[s], out[s]) and torch.equal(a_ui[s], ui[s]) and torch.equal(a_ab[s], ab[s]), f"{label}: bellman, dimension {s}"
    p_out, _, p_ab = fresh()
    for s, k in enumerate(ks):
        rc = L.c3sc_hip_policy_fibers(h, k, sizes[s], idx[s].data_ptr(), pol[s].data_ptr(), p_out[s].data_ptr(), p_ab[s].data_ptr(), None)
        assert rc == 0, (label, k, eng.L.c3sc_hip_last_error(h))
    torch.cuda.synchronize()
    assert eng.status(clear=True) == 0, label
    q_out, _, q_ab = fresh()
    rc = L.c3sc_hip_policy_fibers_all(h, d, KS, FS, GC.ptrs(idx), GC.ptrs(pol), GC.ptrs(q_out), GC.ptrs(q_ab), C.c_void_p(None))
    assert rc == 0, (label, eng.L.c3sc_hip_last_error(h))
    torch.cuda.synchronize()
    assert eng.status(clear=True) == 0, label
    moved = 0.0
    for s in range(d):
        assert torch.equal(q_out[s], p_out[s]) and torch.equal(q_ab[s], p_ab[s]) and torch.equal(p_ab[s], ab[s]), f"{label}: policy, dimension {s}"
        live = ab[s] == 0
        moved = max(moved, float((p_out[s] - out[s])[live].abs().max()))
    assert moved > 1e-6, "the random policy is not the greedy one: the forced path ran"
    print(f"{label}: bellman_fibers_all and policy_fibers_all equal the per-dimension calls bit for bit on {sizes} fibers")


def _jump_engine(ids, model, combined):
    if model == "lqr":
        w = JL.lqr_workload(ids["lqr"], 4, 0.3)
    else:
        w = dataclasses.replace(JL.lqr3_workload(ids["lqr3"], ranks=wl.uniform_ranks(3, 4)), ngrid=(5, 16, 5))
    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    if combined:
        eng.set_horizon_step(LQR_DELTA if model == "lqr" else LQR3_DELTA)
        eng.set_stopping(True)
    eng.set_jumps(True)
    return eng, w


@pytest.mark.parametrize("combined", [False, True], ids=["jump", "jump-stop-horizon"])
@pytest.mark.parametrize("model", ["lqr", "lqr3"])
def test_all_forms_in_jump_mode(ids, model, combined):
    eng, w = _jump_engine(ids, model, combined)
    _all_equals_the_per_dimension_calls(eng, w, w.ncand + (1 if combined else 0), f"{model} {'jump + stop + horizon' if combined else 'jump'}")
    eng.close()


@pytest.mark.parametrize("mode", ["horizon", "stop", "game"])
def test_all_forms_in_the_other_modes(ids, mode):
    """the horizon, stop and game forms on their own, with the sources of horizon_lib, stop_lib and game_lib (11 x 11, rank 4)"""
    eng = E.BellmanEngine(0)
    if mode == "horizon":
        w = H.lqr_workload(ids["horizon"], rank=4)
        eng.configure(w, wl.synth_cores(w))
        eng.set_horizon_step(H.LQR_DELTA)
        nact = w.ncand
    elif mode == "stop":
        w = SL.lqr_vi_workload(ids["stop"], rank=4)
        eng.configure(w, wl.synth_cores(w))
        eng.set_stopping(True)
        nact = w.ncand + 1
    else:
        w, U, W = GL.lq_vi_workload(ids["game"], rank=4)
        eng.configure(w, wl.synth_cores(w))
        eng.set_game(U, W)
        nact = w.ncand
    _all_equals_the_per_dimension_calls(eng, w, nact, mode)
    eng.close()


# ---------------------------------------------------------------------------------------------------- no control at a live node
@pytest.mark.parametrize("combined", [False, True], ids=["jump", "jump-stop-horizon"])
def test_a_forced_index_of_minus_one_gives_zero_in_jump_mode(ids, combined):
    """what pi_core passes for a node without a cached control, and what backup_ref.backup(forced=...) gives: 0.0 at the live nodes,
    the boundary and obstacle costs and every flag unchanged; beside other indices it touches its own node only"""
    eng, w = _jump_engine(ids, "lqr", combined)
    rng = np.random.default_rng(2)
    for k in (0, 1):
        idx = wl.synth_fibers(w, k, 67)
        out, _, ab = eng.bellman_fibers_host(k, idx)
        live = ab == 0
        assert live.any() and (ab == 1).any() and (ab == -1).any()
        z_out, z_ab = eng.policy_fibers_host(k, idx, np.full(ab.shape, -1, dtype=np.int32))
        np.testing.assert_array_equal(z_ab, ab)
        assert (z_out[live] == 0.0).all() and np.array_equal(z_out[~live], out[~live])
        pol = rng.integers(0, w.ncand, size=ab.shape).astype(np.int32)
        hole = rng.random(ab.shape) < 0.3
        f_out, _ = eng.policy_fibers_host(k, idx, pol)
        h_out, h_ab = eng.policy_fibers_host(k, idx, np.where(hole, -1, pol).astype(np.int32))
        np.testing.assert_array_equal(h_ab, ab)
        np.testing.assert_array_equal(h_out, np.where(hole & live, 0.0, f_out))
        assert (hole & live).any() and (f_out[hole & live] != 0.0).all()
    assert eng.status(clear=True) == 0
    eng.close()
