"""GPU parity tests proper: the HIP path (through the C-ABI) against the CPU oracle on the same
seeded inputs.  Bar: absorbed flags / indices bit-exact; values within REL_TOL relative to the
magnitude of the value function (north_star: 1e-6 L-inf after N iterations; we hold single
backups to 1e-12).
The registered kernels one by one, by name: tests/fiber_kernel_cases.py (the case table) and tests/test_gpu_fiber_kernels.py."""
import numpy as np
import pytest

from c3sc_amd import workloads as wl

pytestmark = pytest.mark.gpu

REL_TOL = 1e-12


def _engine(w, cores, variant=0):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    if variant == 4:  # the quad kernels' padded rank (multiples of 4) follows the variant: set it before the upload
        eng.set_variant(variant)
    eng.configure(w, cores)
    if variant and variant != 4:
        eng.set_variant(variant)
    return eng


SMALL = [
    ("dubins3d", dict(ngrid=(21, 17, 16), rank=4)),
    ("dubins3d", dict(ngrid=(70, 66, 101), rank=6)),  # two nodes per lane
    ("scar4d", dict(ngrid=(12, 11, 10, 9), rank=8)),
    ("car7d", dict(ngrid=(9, 8, 10, 7, 6, 5, 11), rank=4)),
    ("car7d", dict(ngrid=(11,) * 7, rank=10)),
    ("lqg2d", dict(ngrid=(51, 51), rank=4)),
    ("lqg6d", dict(ngrid=(7, 8, 9, 6, 5, 7), rank=8)),
    ("quad10d", dict(ngrid=(5, 6, 5, 4, 5, 6, 5, 4, 5, 6), rank=4)),
    ("rossler3d", dict(ngrid=(23, 40, 31), rank=7)),  # examples/rossler: state-dependent drift in every equation
    ("tprob3d", dict(ngrid=(25, 19, 22), rank=10)),   # the reference tests' own 3-D problem (tprob_test.c f3): 3 controls, 125 candidates
    ("perch7d", dict(ngrid=(6, 5, 7, 6, 5, 6, 5), rank=4)),     # examples/perching: 7-D glider (atan2 / sin in the reference, sqrt on the device)
    ("perch7d", dict(ngrid=(20,) * 7, rank=15)),               # ... at the example's own size: N = 20, maxrank 15 (padded 16)
    ("skid5d", dict(ngrid=(9, 8, 11, 7, 10), rank=5)),          # examples/skidding5d: lateral tyre forces, state-dependent boundcost, Q13
    ("skid5d", dict(ngrid=(40,) * 5, rank=15)),                 # ... at the example's own size: N = 40, maxrank 15
    ("cothrust6d", dict(ngrid=(7, 8, 6, 9, 5, 7), rank=6)),     # examples/cothrust2: 3 controls, accelerations = per-candidate features
    ("cothrust6d", dict(ngrid=(20,) * 6, rank=10)),             # ... at the example's own size: N = 20, rank 10 (64 candidates)
]


def _check(eng, P, w, k, idx):
    ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
    out, ui, ab = eng.bellman_fibers_host(k, idx)
    assert eng.status() == 0
    np.testing.assert_array_equal(ab, ref_ab)  # integer work: bit-exact
    scale = np.abs(ref).max()
    err = np.abs(out - ref).max()
    assert err <= REL_TOL * scale, f"{w.name} k={k}: err {err:.3e} scale {scale:.3e}"
    # argmin may only differ on exact ties
    bad = ui != ref_ui
    assert not bad.any() or np.abs(out - ref)[bad].max() <= REL_TOL * scale
    return err / scale


@pytest.mark.parametrize("variant", [1, 3, 4], ids=["fiber_per_wave", "fiber_pair", "fiber_quad"])
@pytest.mark.parametrize("name,kw", [("dubins3d", dict(ngrid=(21, 17, 16), rank=4)), ("car7d", dict(ngrid=(9, 8, 10, 7, 6, 5, 11), rank=4)),
                                     ("scar4d", dict(ngrid=(12, 11, 10, 9), rank=8))], ids=["dubins3d", "car7d", "scar4d"])
def test_consistent_ends_vs_oracle(oracle, name, kw, variant):
    """c3sc_hip_set_consistent_ends (the solver loops' rule, not the reference's): end points of reflecting / periodic fibers
    keep the flags the fixed dimensions / obstacles give them.  Flags bit-exact and values to 1e-12 against the oracle with
    the same switch, on every kernel family; a fiber through an absorbing face must actually show kept flags."""
    w = wl.WORKLOADS[name]().scaled(**kw)
    if variant == 4 and name == "dubins3d":
        pytest.skip("no fiber-quad instantiation for the 3-D models")
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores, consistent_ends=True)
    Plit = oracle.Problem(w, cores)
    eng = _engine(w, cores, variant)
    eng.set_consistent_ends(True)
    seen = 0
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, 300)
        idx[0, :] = 0
        idx[1, :] = np.array(w.ngrid) - 1
        idx[2, :] = 1
        idx[:, k] = 0
        _check(eng, P, w, k, idx)
        _, _, ab = eng.bellman_fibers_host(k, idx)
        _, _, ab_lit = Plit.bellman_fibers(k, idx)
        seen += int((ab != ab_lit).sum())
    assert seen > 0
    eng.set_consistent_ends(False)  # and back: the literal rule again
    idx = wl.synth_fibers(w, w.dx - 1, 100)
    idx[0, :] = 0
    _check(eng, Plit, w, w.dx - 1, idx)


PAIR_CONFIGS = {0, 1, 2, 3, 4, 5, 6, 8}  # SMALL entries that have a fiber-pair instantiation (dubins, scar4d r8, car7d, lqg2d, lqg6d)


@pytest.mark.parametrize("variant", [0, 1, 3], ids=["auto", "fiber_per_wave", "fiber_pair"])
@pytest.mark.parametrize("name,kw", SMALL, ids=[f"{n}-r{k['rank']}-{i}" for i, (n, k) in enumerate(SMALL)])
def test_bellman_fibers_vs_oracle(oracle, name, kw, variant):
    w = wl.WORKLOADS[name]().scaled(**kw)
    if variant == 3 and SMALL.index((name, kw)) not in PAIR_CONFIGS:
        pytest.skip("no fiber-pair instantiation for this (model, rank): the per-wave kernel serves it")
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _engine(w, cores, variant)
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, 37)
        # make sure boundary faces / wrap-around are exercised
        idx[0, :] = 0
        idx[1, :] = np.array(w.ngrid) - 1
        idx[:, k] = 0
        _check(eng, P, w, k, idx)


LANE = [("dubins3d", dict(ngrid=(21, 17, 16), rank=4)), ("dubins3d", dict(ngrid=(70, 66, 101), rank=6)), ("dubins3d", dict(ngrid=(33, 40, 37), rank=8)),
        ("lqg2d", dict(ngrid=(51, 51), rank=4)), ("lqg2d", dict(ngrid=(128, 77), rank=3)), ("rossler3d", dict(ngrid=(23, 40, 31), rank=7)),
        ("rossler3d", dict(ngrid=(20, 20, 20), rank=4))]


@pytest.mark.parametrize("name,kw", LANE, ids=[f"{n}-r{k['rank']}-{i}" for i, (n, k) in enumerate(LANE)])
def test_direct_fold_pair_kernels_vs_oracle(oracle, name, kw):
    """The pair kernels of the 2-D / 3-D models fold straight from the cores in global memory (kernel_fiber_pair.hpp: fpp_direct,
    no staged copy): ragged tiles, boundary faces, the periodic wrap, every varying dimension, ranks 4 / 6 / 8 against the oracle.
    Their policy-evaluation instantiation: applying the minimiser's own argmin reproduces the (oracle-checked) minimum, and a
    random policy agrees with the per-wave kernel's evaluation (itself held to the oracle by test_policy_evaluation_vs_oracle)."""
    w = wl.WORKLOADS[name]().scaled(**kw)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _engine(w, cores, 3)
    eng1 = _engine(w, cores, 1)
    rng = np.random.default_rng(5)
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, 300)
        idx[0, :] = 0
        idx[1, :] = np.array(w.ngrid) - 1
        idx[2, :] = 1
        idx[:, k] = 0
        _check(eng, P, w, k, idx)
        assert "fiber_pair" in eng.last_kernel()
        out, ui, ab = eng.bellman_fibers_host(k, idx)
        scale = np.abs(out).max()
        back, ab2 = eng.policy_fibers_host(k, idx, ui)
        assert "fiber_pair" in eng.last_kernel()
        np.testing.assert_array_equal(ab2, ab)
        assert np.abs(back - out).max() <= REL_TOL * scale
        pol = rng.integers(0, w.ncand, size=out.shape).astype(np.int32)
        got, _ = eng.policy_fibers_host(k, idx, pol)
        want, _ = eng1.policy_fibers_host(k, idx, pol)
        assert np.abs(got - want).max() <= REL_TOL * scale


FPL = [("car7d", dict(ngrid=(9, 8, 10, 7, 6, 5, 11), rank=4)), ("car7d", dict(ngrid=(11, 12, 9, 13, 10, 11, 12), rank=10))]


@pytest.mark.parametrize("name,kw", FPL, ids=[f"{n}-r{k['rank']}" for n, k in FPL])
@pytest.mark.parametrize("variant,tag", [(3, "fiber_pair")])
def test_fiber_pair_kernel_vs_oracle(oracle, name, kw, variant, tag):
    """The fiber-pair kernels (one per varying dimension) against the oracle, incl. ragged tiles (F not a multiple
    of the tile), boundary faces and the periodic wrap."""
    w = wl.WORKLOADS[name]().scaled(**kw)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _engine(w, cores, variant)
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, 300)
        idx[0, :] = 0
        idx[1, :] = np.array(w.ngrid) - 1
        idx[2, :] = 1
        idx[:, k] = 0
        _check(eng, P, w, k, idx)
        assert tag in eng.last_kernel()


@pytest.mark.parametrize("name,kw", SMALL[:5], ids=[f"{n}-{i}" for i, (n, k) in enumerate(SMALL[:5])])
def test_stencil_vs_oracle(oracle, name, kw):
    """valuef_eval_fiber_ind_nn + process_fibers_neighbor batched (c3sc_hip_stencil_fibers)."""
    w = wl.WORKLOADS[name]().scaled(**kw)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _engine(w, cores)
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, 23)
        idx[0, :] = 0
        idx[1, :] = np.array(w.ngrid) - 1
        idx[:, k] = 0
        ref, ref_ab = P.stencil_fibers(k, idx)
        out, ab = eng.stencil_fibers_host(k, idx)
        np.testing.assert_array_equal(ab, ref_ab)
        scale = np.abs(ref).max()
        assert np.abs(out - ref).max() <= REL_TOL * scale


def test_table_model_vs_oracle(oracle):
    """c3sc_hip_bellman_fibers_tables: host-evaluated (drift, diag sigma, stage) tables, any dynamics."""
    import oracle_lib
    import ctypes as C

    w = wl.scar4d().scaled(ngrid=(9, 8, 10, 7), rank=8)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _engine(w, cores)
    L = oracle_lib.lib()
    xg = w.xgrid()
    S = 2 * w.dx + 1
    prm = np.zeros(8)
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, 17)
        idx[0, :] = 0
        idx[:, k] = 0
        N = w.ngrid[k]
        tables = np.zeros((len(idx), N, w.ncand, S))
        costs2 = np.zeros((len(idx), N, 2))
        b = np.zeros(w.dx); sg = np.zeros(w.dx); st = C.c_double(0)
        for f, row in enumerate(idx):
            for j in range(N):
                x = np.array([xg[m][j] if m == k else xg[m][row[m]] for m in range(w.dx)])
                bc = C.c_double(0); oc = C.c_double(0)
                L.orc_model_boundcost(w.model, oracle_lib.dp(prm), oracle_lib.dp(x), C.byref(bc))
                L.orc_model_obscost(w.model, oracle_lib.dp(prm), oracle_lib.dp(x), C.byref(oc))
                costs2[f, j] = (bc.value, oc.value)
                for c in range(w.ncand):
                    u = np.ascontiguousarray(w.cands[c])
                    L.orc_model_drift(w.model, oracle_lib.dp(prm), oracle_lib.dp(x), oracle_lib.dp(u), oracle_lib.dp(b))
                    L.orc_model_diff_diag(w.model, oracle_lib.dp(prm), oracle_lib.dp(x), oracle_lib.dp(u), oracle_lib.dp(sg))
                    L.orc_model_stage(w.model, oracle_lib.dp(prm), oracle_lib.dp(x), oracle_lib.dp(u), C.byref(st))
                    tables[f, j, c, :w.dx] = b
                    tables[f, j, c, w.dx:2 * w.dx] = sg
                    tables[f, j, c, 2 * w.dx] = st.value
        out, ui, ab = eng.bellman_fibers_tables_host(k, idx, tables, costs2)
        ref, ref_ui, ref_ab = P.bellman_fibers(k, idx)
        np.testing.assert_array_equal(ab, ref_ab)
        assert np.abs(out - ref).max() <= REL_TOL * np.abs(ref).max()
        assert "TableModel" in eng.last_kernel()


def test_mixed_ranks_and_smooth_value(oracle):
    """Non-uniform ranks (padded on the device) and a smooth rank-2 value function."""
    w = wl.c2_dubins().scaled(ngrid=(19, 23, 17))
    w.ranks = (1, 3, 5, 1)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _engine(w, cores)
    for k in range(3):
        _check(eng, P, w, k, wl.synth_fibers(w, k, 29))
    w2 = wl.c4_car7d().scaled(ngrid=(9,) * 7, rank=4)
    cores2 = wl.smooth_cores(w2)
    P2 = oracle.Problem(w2, cores2)
    eng2 = _engine(w2, cores2)
    for k in (0, 3, 6):
        _check(eng2, P2, w2, k, wl.synth_fibers(w2, k, 31))


def test_golden_fixture_car7d(oracle):
    """Committed golden vectors (tests/golden/car7d_small.npz, made by tests/make_golden.py from the
    pinned oracle): the HIP path reproduces them without the oracle in the loop."""
    import os

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "car7d_small.npz"))
    w = wl.c4_car7d().scaled(ngrid=tuple(int(n) for n in g["ngrid"]), rank=int(g["rank"]))
    eng = _engine(w, wl.synth_cores(w))
    for k in range(w.dx):
        out, ui, ab = eng.bellman_fibers_host(k, g[f"idx{k}"])
        np.testing.assert_array_equal(ab, g[f"ab{k}"])
        ref = g[f"out{k}"]
        assert np.abs(out - ref).max() <= REL_TOL * np.abs(ref).max()


def test_golden_fixture_policy_evaluation():
    """Committed golden vectors for bellman_pi (tests/golden/pi_dubins_small.npz, tests/make_golden.py): the policy's
    candidate indices and the evaluated right-hand side on a second value function, without the oracle in the loop."""
    import os

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "pi_dubins_small.npz"))
    w = wl.c2_dubins().scaled(ngrid=tuple(int(n) for n in g["ngrid"]), rank=int(g["rank"]))
    eng_pol = _engine(w, wl.synth_cores(w))
    eng_it = _engine(w, wl.smooth_cores(w))
    for k in range(w.dx):
        idx, pol = g[f"idx{k}"], g[f"policy{k}"]
        _, ui, ab = eng_pol.bellman_fibers_host(k, idx)
        np.testing.assert_array_equal(ab, g[f"ab{k}"])
        np.testing.assert_array_equal(ui, pol)  # three well-separated candidates: no ties on this fixture
        out, _ = eng_it.policy_fibers_host(k, idx, pol)
        ref = g[f"out{k}"]
        assert np.abs(out - ref).max() <= REL_TOL * np.abs(ref).max()


def test_full_size_properties():
    """BASELINE full size (car7d N=41 r=10): size-independent properties instead of the oracle.
    (1) absorbed nodes return exactly the boundary / obstacle cost; (2) a batch equals the
    concatenation of its halves (no cross-fiber coupling); (3) determinism; (4) with constant
    cores the value function is constant c and every live node returns dt*stage + c (beta = 0)
    minimised over controls -- bounded by c + max stage * max dt."""
    import torch

    w = wl.c4_car7d()
    cores = wl.synth_cores(w)
    eng = _engine(w, cores)
    k = 2
    # (0) the two production kernels agree at full size: 70 000 fibers = more tiles than resident workgroups for the
    # fiber-pair kernel (second trip of its tile loop, ragged last tile) against one-wave-per-fiber
    big = wl.synth_fibers(w, k, 70000)
    eng.set_variant(3)
    o_pair, u_pair, a_pair = eng.bellman_fibers_host(k, big)
    assert "fiber_pair" in eng.last_kernel()
    eng.set_variant(1)
    o_wave, u_wave, a_wave = eng.bellman_fibers_host(k, big)
    assert "fiber_per_wave" in eng.last_kernel()
    np.testing.assert_array_equal(a_pair, a_wave)
    assert np.abs(o_pair - o_wave).max() <= REL_TOL * np.abs(o_wave).max()
    assert (u_pair != u_wave).mean() < 1e-4  # argmin only differs on (near) ties
    eng.set_variant(3)
    idx = wl.synth_fibers(w, k, 4096)
    out, ui, ab = eng.bellman_fibers_host(k, idx)
    assert np.isfinite(out).all()
    assert (out[ab == 1] == 10.0).all() and (out[ab == -1] == 0.0).all()
    assert (ui[ab != 0] == -1).all() and (ui[ab == 0] >= 0).all()
    o1, _, _ = eng.bellman_fibers_host(k, idx[:1000])
    o2, _, _ = eng.bellman_fibers_host(k, idx[1000:])
    np.testing.assert_array_equal(np.concatenate([o1, o2]), out)
    out_b, _, _ = eng.bellman_fibers_host(k, idx)
    np.testing.assert_array_equal(out, out_b)
    # device-buffer API gives the same bits as the host-buffer API
    idx_t = torch.from_numpy(idx).cuda()
    out_t = eng.bellman_fibers(k, idx_t)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out_t.cpu().numpy(), out)
    # constant value function
    const = [np.zeros_like(c) for c in cores]
    for m, c in enumerate(const):
        r0, r1 = w.ranks[m], w.ranks[m + 1]
        c.reshape(w.ngrid[m], r1, r0)[:, 0, 0] = 1.0
    const[0] *= 7.5
    eng.upload_value(w.ranks, const)
    out_c, _, ab_c = eng.bellman_fibers_host(k, idx)
    live = ab_c == 0
    assert (out_c[live] > 7.5).all() and (out_c[live] < 7.5 + 40.0).all()


@pytest.mark.parametrize("name,kw", [SMALL[0], SMALL[2], SMALL[4], SMALL[6], SMALL[7]],
                         ids=lambda v: v if isinstance(v, str) else f"r{v['rank']}")
def test_policy_evaluation_vs_oracle(oracle, name, kw):
    """c3sc_hip_policy_fibers == bellman_pi (bellman.c:1702-1886): the policy is greedy for one value function
    (argmin from c3sc_hip_bellman_fibers on it), the Bellman right-hand side is evaluated on another."""
    w = wl.WORKLOADS[name]().scaled(**kw)
    cores_pol = wl.synth_cores(w)
    cores_it = [c * (1.0 + 0.05 * np.cos(np.arange(c.size)).reshape(c.shape)) for c in wl.smooth_cores(w)]
    P = oracle.Problem(w, cores_it)
    pol_vf = oracle.ValueF(w.ngrid, w.ranks, cores_pol)
    eng_pol = _engine(w, cores_pol, 0)
    eng_it = _engine(w, cores_it, 0)
    P.pi_begin()
    P.pi_step_begin()
    worst = 0.0
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, 23)
        idx[0, :] = 0
        idx[1, :] = np.array(w.ngrid) - 1
        idx[:, k] = 0
        ref, ref_ui = P.policy_fibers(pol_vf, k, idx)
        _, ui, _ = eng_pol.bellman_fibers_host(k, idx)
        out, ab = eng_it.policy_fibers_host(k, idx, ui)
        assert eng_it.status() == 0
        scale = np.abs(ref).max()
        # the oracle reports -2 where it reused the cached [prob, dt, stage] of a node seen before in this pi_iter
        fresh = ref_ui >= 0
        bad = fresh & (ui != ref_ui)
        err = np.abs(out - ref)
        assert err[~bad].max() <= REL_TOL * scale, f"{w.name} k={k}: err {err[~bad].max():.3e} scale {scale:.3e}"
        # a different argmin is only acceptable on ties of the policy objective; then compare through the oracle's choice
        if bad.any():
            out2, _ = eng_it.policy_fibers_host(k, idx, np.where(ref_ui >= 0, ref_ui, ui).astype(np.int32))
            assert np.abs(out2 - ref).max() <= REL_TOL * scale
        worst = max(worst, err[~bad].max() / scale)
    assert P.niter_node_evals() > 0 and P.npol_evals() > 0


def _with_cands(w, cands):
    return wl.Workload(w.name, w.model, w.params, w.dx, w.du, w.lb, w.ub, w.ngrid, w.ranks, w.discount, w.bc,
                       list(w.obstacles), np.asarray(cands, dtype=np.float64))


@pytest.mark.parametrize("name,kw,grid,fine", [("lqg2d", dict(ngrid=(21, 19), rank=4), 33, 20001),
                                               ("lqg6d", dict(ngrid=(7, 8, 9, 6, 5, 7), rank=8), 9, 41),
                                               ("rossler3d", dict(ngrid=(17, 21, 19), rank=6), 33, 20001),
                                               ("perch7d", dict(ngrid=(6, 5, 7, 6, 5, 6, 5), rank=4), 65, 20001),
                                               ("tprob3d", dict(ngrid=(9, 8, 7), rank=6), 21, 41),
                                               ("cothrust6d", dict(ngrid=(6, 5, 6, 7, 5, 6), rank=5), 9, 41)],
                         ids=["lqg2d-du1", "lqg6d-du3", "rossler3d-du1", "perch7d-du1", "tprob3d-du3", "cothrust6d-du3"])
def test_continuous_control_box_minimiser(oracle, name, kw, grid, fine):
    """c3sc_hip_bellman_fibers_box: the non-BRUTEFORCE branch of bellman_optimal (bellman.c:545-1118).  The optimiser
    there is C3's BFGS (third party, unpinned), so the check is the reference's own (tprob_test.c:1494-1540):
    the result must not exceed the minimum over a 100-point linspace of the control box by more than 1e-10 -- plus a
    lower bound from a much finer grid and a policy-evaluation round trip of the returned control."""
    import itertools

    w = wl.WORKLOADS[name]().scaled(**kw)
    cores = wl.synth_cores(w)
    lb, ub = -np.ones(w.du), np.ones(w.du)
    if name == "rossler3d":
        lb, ub = -4.0 * np.ones(1), 4.0 * np.ones(1)                    # rossler.c:212-213
    elif name == "perch7d":
        lb, ub = -2.0 * np.pi * np.ones(1), 2.0 * np.pi * np.ones(1)    # perch.c:329-330
    elif name == "tprob3d":
        lb, ub = -5.0 * np.ones(3), 5.0 * np.ones(3)                    # tprob_test.c:2463-2466
    elif name == "cothrust6d":
        lb, ub = np.array([-1.5, -0.4, -0.4]), np.array([1.5, 0.4, 0.4])  # copterposethrust.c:330-331 (features formed on the device)
    eng = _engine(w, cores, 0)
    eng.set_control_box(lb, ub, grid=grid, polish=2)
    n100 = 100 if w.du == 1 else 11
    axes = lambda n: list(itertools.product(*[np.linspace(lb[i], ub[i], n) for i in range(w.du)]))
    P100 = oracle.Problem(_with_cands(w, axes(n100)), cores)
    Pfine = oracle.Problem(_with_cands(w, axes(fine)), cores)
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, 9)
        idx[0, :] = 0
        idx[1, :] = np.array(w.ngrid) - 1
        out, uo, ab = eng.bellman_fibers_box_host(k, idx)
        assert eng.status() == 0 and "fiber_per_wave" in eng.last_kernel()
        r100, _, ab0 = P100.bellman_fibers(k, idx)
        rfine, _, _ = Pfine.bellman_fibers(k, idx)
        np.testing.assert_array_equal(ab, ab0)
        live = ab == 0
        scale = np.abs(rfine).max()
        assert (out[live] <= r100[live] + 1e-10).all()          # the reference's assertion on bellman_optimal
        # not below what a much finer scan finds, up to that scan's resolution (tprob3d: 41 points over [-5,5] per control, and
        # the node objective has kinks where a drift component changes sign -- the continuous minimiser legitimately gets lower)
        low_tol = 1e-2 if name == "tprob3d" else 2e-5
        assert (out[live] >= rfine[live] - low_tol * scale).all(), float((rfine[live] - out[live]).max() / scale)
        np.testing.assert_allclose(out[~live], rfine[~live], rtol=1e-12)  # absorbed nodes: boundcost / obscost
        assert (uo >= lb - 1e-15).all() and (uo <= ub + 1e-15).all()
        back, _ = eng.policy_fibers_box_host(k, idx, uo)  # bellman_pi with the continuous policy
        np.testing.assert_allclose(back, out, rtol=1e-12, atol=1e-12 * scale)


@pytest.mark.parametrize("nfib", [50, 20000], ids=["small-batch", "pair-sized-batch"])
def test_candidate_lists_longer_than_a_wavefront(oracle, nfib):
    """The kernels fill their candidate table with one lane per candidate, 64 at a time: the fiber-per-wave kernel walks longer
    lists in chunks, the fiber-pair / quad kernels decline them and the launch falls through to the per-wave kernel (found this
    round: 125 candidates used to give silently wrong minima).  97 and 200 candidates on the 2-D LQG problem, 125 on tprob3d;
    at 20 000 fibers AUTO would take the fiber-pair kernel for 64 candidates or fewer."""
    for name, kw, ncand in (("lqg2d", dict(ngrid=(31, 29), rank=4), 97), ("lqg2d", dict(ngrid=(31, 29), rank=4), 200),
                            ("tprob3d", dict(ngrid=(9, 8, 7), rank=6), 125)):
        w0 = wl.WORKLOADS[name]().scaled(**kw)
        if name == "lqg2d":
            w0 = _with_cands(w0, np.linspace(-1.0, 1.0, ncand).reshape(-1, 1) + 1e-3)
        assert w0.ncand == ncand
        cores = wl.synth_cores(w0)
        P = oracle.Problem(w0, cores)
        eng = _engine(w0, cores, 0)
        for k in range(w0.dx):
            idx = wl.synth_fibers(w0, k, nfib)
            idx[0, :] = 0
            idx[1, :] = np.array(w0.ngrid) - 1
            idx[:, k] = 0
            out, ui, ab = eng.bellman_fibers_host(k, idx)
            assert eng.status() == 0 and "fiber_per_wave" in eng.last_kernel(), eng.last_kernel()
            pick = np.arange(min(nfib, 60))
            ref, ref_ui, ref_ab = P.bellman_fibers(k, idx[pick])
            np.testing.assert_array_equal(ab[pick], ref_ab)
            scale = np.abs(ref).max()
            assert np.abs(out[pick] - ref).max() <= REL_TOL * scale
            bad = ui[pick] != ref_ui
            assert not bad.any() or np.abs(out[pick] - ref)[bad].max() <= REL_TOL * scale


def test_edge_cases_empty_batch_max_rank_max_nodes(oracle):
    """Empty batch; the largest compiled rank (scar-4D at FT rank 20) and the largest node count (128 per
    fiber: two nodes per lane, both lane-table registers in use)."""
    w = wl.WORKLOADS["scar4d"]().scaled(ngrid=(12, 11, 10, 9), rank=20)
    cores = wl.synth_cores(w)
    eng = _engine(w, cores)
    out, ui, ab = eng.bellman_fibers_host(1, np.zeros((0, w.dx), dtype=np.int32))
    assert out.shape == (0, 11) and eng.status() == 0
    P = oracle.Problem(w, cores)
    for k in range(w.dx):
        _check(eng, P, w, k, wl.synth_fibers(w, k, 9))
    w2 = wl.c2_dubins().scaled(ngrid=(128, 5, 128), rank=4)
    cores2 = wl.synth_cores(w2)
    P2 = oracle.Problem(w2, cores2)
    for variant in (1, 3):
        eng2 = _engine(w2, cores2, variant)
        for k in (0, 2):
            idx = wl.synth_fibers(w2, k, 70)
            idx[0, :] = 0
            idx[1, :] = np.array(w2.ngrid) - 1
            _check(eng2, P2, w2, k, idx)


def test_large_core_not_staged_in_lds(oracle):
    """Rank 20 on a 100-node dimension (the reference's own regression size, tprob_test.c:2284,2310): N x RP^2 doubles
    exceed the CU's LDS, the per-wave kernel then reads each node's matrix from L2 instead of staging the core.  Only a middle
    dimension holds N x RP^2 doubles (an end dimension, so both dimensions of a 2-D problem, holds N x RP and is always staged):
    the unstaged instantiation is the one the last grid reaches, 101 nodes x 257 doubles on dimension 1 of a 3-D problem."""
    w = wl.c1_lqg2d().scaled(ngrid=(100, 100), rank=20)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _engine(w, cores)
    for k in range(2):
        idx = wl.synth_fibers(w, k, 11)
        idx[0, :] = 0
        idx[1, :] = np.array(w.ngrid) - 1
        _check(eng, P, w, k, idx)
        assert "fiber_per_wave" in eng.last_kernel()
    w3 = wl.c2_dubins().scaled(ngrid=(101, 33, 101), rank=16)
    cores3 = wl.synth_cores(w3)
    P3 = oracle.Problem(w3, cores3)
    eng3 = _engine(w3, cores3)
    for k in (0, 1, 2):
        _check(eng3, P3, w3, k, wl.synth_fibers(w3, k, 9))
    w4 = wl.c2_dubins().scaled(ngrid=(33, 101, 35), rank=16)
    cores4 = wl.synth_cores(w4)
    P4 = oracle.Problem(w4, cores4)
    eng4 = _engine(w4, cores4)
    _check(eng4, P4, w4, 1, wl.synth_fibers(w4, 1, 9))
    assert eng4.last_kernel() == "k_fiber_per_wave<Dubins3D,16,2>"


@pytest.mark.gpu
def test_c_abi_error_behaviour():
    """The boundary reports, it does not crash: bad arguments and missing state give C3SC_ERR_ARG, a rank no kernel
    serves C3SC_ERR_UNSUPPORTED, each with text in c3sc_hip_last_error; F = 0 is a no-op; the context stays usable."""
    import ctypes as C

    from c3sc_amd.engine import BellmanEngine, C3scHipError, load_library

    L = load_library()
    w = wl.c2_dubins().scaled(ngrid=(11, 9, 13), rank=4)
    cores = wl.synth_cores(w)
    eng = BellmanEngine(0)
    idx = wl.synth_fibers(w, 0, 8)
    out = np.zeros((8, w.ngrid[0]))
    # nothing configured yet
    rc = L.c3sc_hip_bellman_fibers_host(eng.h, 0, C.c_size_t(8), idx.ctypes.data, out.ctypes.data, None, None)
    assert rc == 1 and len(L.c3sc_hip_last_error(eng.h)) > 0
    eng.configure(w, cores)
    for k_bad in (-1, 3):
        assert L.c3sc_hip_bellman_fibers_host(eng.h, k_bad, C.c_size_t(8), idx.ctypes.data, out.ctypes.data, None, None) == 1
    assert L.c3sc_hip_bellman_fibers_host(eng.h, 0, C.c_size_t(0), None, None, None, None) == 0  # empty batch
    assert L.c3sc_hip_bellman_fibers(eng.h, 0, C.c_size_t(8), None, None, None, None, None) == 1  # null device buffers
    assert L.c3sc_hip_get_status(None, None, 0) == 1
    assert L.c3sc_hip_max_rank(w.model, 3) >= 16 and L.c3sc_hip_max_rank(w.model, 9) == 0 and L.c3sc_hip_max_rank(12345, 3) == 0
    # a rank above every compiled kernel of this model
    big = wl.c2_dubins().scaled(ngrid=(11, 9, 13), rank=24)
    with pytest.raises(C3scHipError) as ei:
        eng.upload_value(big.ranks, wl.synth_cores(big))
    assert "code 3" in str(ei.value)
    # still usable afterwards
    eng.upload_value(w.ranks, cores)
    got, _, _ = eng.bellman_fibers_host(0, idx)
    assert np.isfinite(got).all() and eng.status() == 0


@pytest.mark.gpu
def test_host_entry_zero_copy_and_staged_paths_agree():
    """c3sc_hip_bellman_fibers_host, c3sc_hip_policy_fibers_host and the two box calls serve batches up to 1 MiB from a pinned
    device-mapped block and larger ones through device scratch: the same fibers must come back bit for bit (values, argmin or
    minimiser, absorbed flags) either way."""
    w = wl.c4_car7d().scaled(ngrid=(11,) * 7, rank=10)
    cores = wl.synth_cores(w)
    eng = _engine(w, cores, 0)
    for k in (0, 3, 6):
        big = wl.synth_fibers(w, k, 9000)  # 9000 x (28 + 88 + 88) B > 1 MiB: staged
        small = big[:100].copy()           # zero-copy
        o1, u1, a1 = eng.bellman_fibers_host(k, small)
        o2, u2, a2 = eng.bellman_fibers_host(k, big)
        assert np.array_equal(o1, o2[:100]) and np.array_equal(u1, u2[:100]) and np.array_equal(a1, a2[:100])
        pol = np.random.default_rng(k).integers(0, len(w.cands), size=u2.shape).astype(np.int32)  # same sizes as above
        p1, pa1 = eng.policy_fibers_host(k, small, pol[:100])
        p2, pa2 = eng.policy_fibers_host(k, big, pol)
        assert np.array_equal(p1, p2[:100]) and np.array_equal(pa1, pa2[:100])
    assert eng.status() == 0
    # the box pair on a model compiled with the box minimiser (car7d has none)
    wb = wl.WORKLOADS["perch7d"]().scaled(ngrid=(6, 5, 7, 6, 5, 6, 5), rank=4)
    engb = _engine(wb, wl.synth_cores(wb), 0)
    engb.set_control_box([-2.0 * np.pi], [2.0 * np.pi], grid=33, polish=2)
    for k in (0, 3, 6):
        big = wl.synth_fibers(wb, k, 12000)  # 12000 x (28 + 20 N) B > 1 MiB at N >= 5: staged
        small = big[:100].copy()
        b1, uo1, ba1 = engb.bellman_fibers_box_host(k, small)
        b2, uo2, ba2 = engb.bellman_fibers_box_host(k, big)
        assert np.array_equal(b1, b2[:100]) and np.array_equal(uo1, uo2[:100]) and np.array_equal(ba1, ba2[:100])
        q1, qa1 = engb.policy_fibers_box_host(k, small, uo2[:100])
        q2, qa2 = engb.policy_fibers_box_host(k, big, uo2)
        assert np.array_equal(q1, q2[:100]) and np.array_equal(qa1, qa2[:100])
    assert engb.status() == 0


@pytest.mark.gpu
def test_device_api_on_a_side_stream_and_repeatable():
    """c3sc_hip_upload_value_device / c3sc_hip_bellman_fibers enqueue on the stream they are given (a non-default HIP stream
    here, ordered against nothing else), and the kernels are deterministic: the same launch twice gives the same bits."""
    import torch

    w = wl.c4_car7d().scaled(ngrid=(13,) * 7, rank=10)
    cores = wl.synth_cores(w)
    eng = _engine(w, cores, 3)  # fiber-pair
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    k = 2
    idx = wl.synth_fibers(w, k, 20000)
    ref, _, _ = eng.bellman_fibers_host(k, idx)  # default stream, host buffers
    with torch.cuda.stream(side):
        core_t = [torch.from_numpy(np.ascontiguousarray(c)).to(dev, non_blocking=False) for c in cores]
        idx_t = torch.from_numpy(idx).to(dev)
        out1 = torch.empty((idx.shape[0], w.ngrid[k]), dtype=torch.float64, device=dev)
        out2 = torch.empty_like(out1)
        eng.upload_value_device(w.ranks, core_t, side.cuda_stream)
        eng.bellman_fibers(k, idx_t, out1, stream_ptr=side.cuda_stream)
        eng.bellman_fibers(k, idx_t, out2, stream_ptr=side.cuda_stream)
    side.synchronize()
    a, b = out1.cpu().numpy(), out2.cpu().numpy()
    assert np.array_equal(a, b)
    assert np.array_equal(a, ref)
    assert eng.status() == 0


@pytest.mark.gpu
def test_one_workgroup_per_tile_launch_path(oracle):
    """Above 8 tiles per resident workgroup slot the pair kernel is launched with one workgroup per tile instead of
    persistent workgroups (launch_fpp.hpp).  600 000 fibers on a small grid take that path: every row must equal the per-wave
    kernel's, and a sample of rows the oracle's."""
    w = wl.c4_car7d().scaled(ngrid=(11,) * 7, rank=4)
    cores = wl.synth_cores(w)
    eng = _engine(w, cores, 0)
    P = oracle.Problem(w, cores)
    F = 600_000  # 9375 tiles >= 8 x 1024
    for k in (0, 4):
        idx = wl.synth_fibers(w, k, F)
        eng.set_variant(3)
        a, ua, aa = eng.bellman_fibers_host(k, idx)
        assert "fiber_pair" in eng.last_kernel()
        eng.set_variant(1)
        b, ub, ab = eng.bellman_fibers_host(k, idx)
        scale = np.abs(b).max()
        assert np.abs(a - b).max() <= REL_TOL * scale and np.array_equal(aa, ab)
        pick = np.random.default_rng(k).choice(F, 300, replace=False)
        ref, _, rab = P.bellman_fibers(k, idx[pick])
        assert np.abs(a[pick] - ref).max() <= REL_TOL * scale and np.array_equal(aa[pick], rab)
    assert eng.status() == 0


# ---- the BASELINE.json configurations at the instantiations and sizes the bench / examples actually run ----------------
FULL = [
    # (workload, scale kwargs, variant, kernel tag, fibers per dim)
    ("car7d", dict(), 3, "fiber_pair<Car7D,10", 64),            # C4: N=41, r=10 -- the code object bench.py times
    ("car7d", dict(), 1, "fiber_per_wave<Car7D,10", 64),        # the kernel the solver's small batches take
    ("quad10d", dict(ngrid=(7, 6, 5, 8, 7, 6, 5, 8, 7, 25)), 0, "Chain<10>,16", 48),  # C5 at rank 15 (padded rank 16)
    ("quad10d", dict(), 4, "fiber_quad_duo<Chain<10>,16", 48),  # C5 at FULL size 25^10, rank 15: the duo kernel the bench times
    ("dubins3d", dict(), 3, "fiber_pair<Dubins3D,6", 40),       # C2: 101^3, r=6
    ("dubins3d", dict(), 1, "fiber_per_wave<Dubins3D,6", 40),
    ("lqg6d", dict(), 3, "fiber_pair<LqgNd<6>,8", 40),          # C3: 31^6, r=8
    ("lqg6d", dict(), 1, "fiber_per_wave<LqgNd<6>,8", 40),
    ("scar4d", dict(), 0, "Scar", 40),                          # the reference's own skidding car: 40^4, rank 20
]


@pytest.mark.parametrize("name,kw,variant,tag,nf", FULL, ids=[f"{f[0]}-v{f[2]}" + ("-full" if f[0] == "quad10d" and not f[1] else "") for f in FULL])
def test_baseline_configs_at_the_benched_instantiation(oracle, name, kw, variant, tag, nf):
    """Oracle comparison at the exact (model, padded rank, N) instantiations of BASELINE.json's configs: every varying
    dimension, faces and wrap-around included; a few dozen fibers per dimension cost the oracle milliseconds."""
    w = wl.WORKLOADS[name]().scaled(**kw) if kw else wl.WORKLOADS[name]()
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    eng = _engine(w, cores, variant)
    worst = 0.0
    for k in range(w.dx):
        idx = wl.synth_fibers(w, k, nf)
        idx[0, :] = 0
        idx[1, :] = np.array(w.ngrid) - 1
        idx[2, :] = 1
        idx[:, k] = 0
        worst = max(worst, _check(eng, P, w, k, idx))
        assert tag in eng.last_kernel(), eng.last_kernel()
    print(f"{name} {w.ngrid} ranks {w.ranks[1]}: {eng.last_kernel()} max rel err {worst:.2e}")


def test_stationary_node_raises_the_status_flag(oracle):
    """transition_assemble returns 1 when the total rate Q < 1e-14 (nodeutil.c:365-367) and bellman_control asserts on it
    (bellman.c:452).  2-D LQG with zero diffusion: at x1 = 0 the candidate u = 0 has zero drift in both dimensions.  The
    oracle fails the fiber with code 101; the device must raise C3SC_STATUS_STATIONARY -- and leave it clear otherwise."""
    w0 = wl.c1_lqg2d().scaled(ngrid=(51, 51), rank=4)
    w = wl.Workload(w0.name, w0.model, (2.0, 0.0, 0.0), w0.dx, w0.du, w0.lb, w0.ub, w0.ngrid, w0.ranks, w0.discount, w0.bc, [], w0.cands)
    assert w.xgrid()[1][25] == 0.0 and w.cands[16, 0] == 0.0
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    import ctypes as C

    for variant in (1, 3):
        eng = _engine(w, cores, variant)
        # fibers along dim 0 at x1 != 0: every candidate has drift x1 in dim 0 -> fine
        ok = np.array([[0, 3], [0, 40]], dtype=np.int32)
        out, _, _ = eng.bellman_fibers_host(0, ok)
        ref, _, _ = P.bellman_fibers(0, ok)
        assert eng.status() == 0 and np.abs(out - ref).max() <= REL_TOL * np.abs(ref).max()
        # a fiber through x1 = 0: stationary at u = 0
        bad = np.array([[0, 25]], dtype=np.int32)
        o = np.zeros((1, 51)); u = np.zeros((1, 51), dtype=np.int32)
        rc = P.L.orc_bellman_fibers(P.h, C.c_size_t(0), C.c_size_t(1), bad.ctypes.data_as(C.POINTER(C.c_int)), o.ctypes.data_as(C.POINTER(C.c_double)),
                                    u.ctypes.data_as(C.POINTER(C.c_int)), None)
        assert rc == 101  # 100 + transition_assemble's 1
        eng.bellman_fibers_host(0, bad)
        assert eng.status() & 1, "C3SC_STATUS_STATIONARY not raised"
        # and along dim 1 (the fiber crosses x1 = 0 at node 25)
        eng2 = _engine(w, cores, variant)
        eng2.bellman_fibers_host(1, np.array([[7, 0]], dtype=np.int32))
        assert eng2.status() & 1


def test_all_dimensions_call_matches_the_per_dimension_calls():
    """c3sc_hip_bellman_fibers_all / c3sc_hip_policy_fibers_all: the independent per-dimension launches of one batch spread over the
    caller's stream and two internal ones.  Same kernels, so the same bits as the per-dimension calls; and stream-ordered like a
    single launch -- an operation enqueued on the caller's stream right after the call sees every segment's results."""
    import torch

    w = wl.WORKLOADS["car7d"]().scaled(ngrid=(11, 12, 9, 13, 10, 11, 12), rank=10)
    cores = wl.synth_cores(w)
    eng = _engine(w, cores, 3)
    d = w.dx
    F = 20000  # a large batch: the pair kernels
    idx = [torch.from_numpy(wl.synth_fibers(w, k, F)).cuda() for k in range(d)]
    ref = [eng.bellman_fibers(k, idx[k]).clone() for k in range(d)]
    torch.cuda.synchronize()
    out = [torch.zeros_like(r) for r in ref]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for rep in range(3):
            for o in out:
                o.zero_()
            eng.bellman_fibers_all(list(range(d)), idx, out, stream_ptr=stream.cuda_stream)
            sums = torch.stack([o.sum() for o in out])  # enqueued behind the call on the same stream: must see all of it
            stream.synchronize()
            for k in range(d):
                assert torch.equal(out[k], ref[k]), f"dimension {k}, repetition {rep}"
            assert torch.equal(sums, torch.stack([r.sum() for r in ref]))
    # policy evaluation the same way
    pol = [torch.randint(0, w.ncand, r.shape, dtype=torch.int32, device="cuda") for r in ref]
    pref = []
    for k in range(d):
        o, _ = eng.policy_fibers_host(k, idx[k].cpu().numpy(), pol[k].cpu().numpy())
        pref.append(o)
    pout = [torch.zeros_like(r) for r in ref]
    eng.bellman_fibers_all(list(range(d)), idx, pout, policy_ts=pol)
    torch.cuda.synchronize()
    for k in range(d):
        assert np.array_equal(pout[k].cpu().numpy(), pref[k]), f"policy, dimension {k}"
    assert eng.status() == 0
