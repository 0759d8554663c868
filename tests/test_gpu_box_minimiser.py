"""The continuous-control minimiser on the device (node_backup_box through bellman_fibers_box_host) against tests/box_ref.py, the
numpy restatement of the same algorithm over an objective of its own (the oracle's model callbacks and backup_ref's arithmetic):
step for step, so that a skipped polish, a wrong cell, a wrong round order or a wrong UDEP_MASK shows.  tests/test_box_ref.py
holds the restatement itself (to the oracle, to the host's box_minimize) and shows every planted fault rejected.

Every row runs seven fibers along the middle k of the smallest grids (fiber_kernel_cases.GRIDS), on wl.synth_cores and on the
signed class.  What is asserted is box_ref.check_device's list: flags and absorbed values exact; on pinned live nodes the value
within REL_TOL = 1e-12 of fiber_kernel_cases.scale_of and every u_i inside the reference's interval

    [lo_i - sum_j max_e max(0, lo_i - r(j, e).lo),  hi_i + sum_j max_e max(0, r(j, e).hi - hi_i)]

([lo_i, hi_i]: the bracket the reference recorded in the last round's search of coordinate i -- or, where that search's take is
unsure or surely fails, its hull with / the interval of the point held before; r(j, e): the bracket the same search records when
coordinate j != i sits at end e of its own interval; box_ref's module docstring); for polish = 0 the grid point bit for bit; on
unpinned nodes the value not above the reference's grid scan and u inside the box; the STATIONARY bit equal to the reference's.
policy_fibers_box_host on the returned controls equals the reference objective there to REL_TOL -- the figure BOX_MARGIN rests on.

Every test prints its row's kernel, worst value error, unpinned share and objective noise (pytest -s); DESIGN.md 6.4 records them."""
import numpy as np
import pytest

import box_ref as B
import fiber_kernel_cases as T

pytestmark = pytest.mark.gpu

DATA = [False, True]
DATA_IDS = ["synth", "signed"]
KERNEL_ROWS = B.kernel_rows()
SETTING_ROWS = B.setting_rows()
_ids = lambda rows: [B.row_id(*r) for r in rows]


def _engine(case, w, cs, row):
    from c3sc_amd.engine import BellmanEngine

    eng = BellmanEngine(0)
    eng.set_variant(case.variant)
    eng.configure(w, cs)
    eng.set_control_box(np.array(row.lb), np.array(row.ub), grid=row.grid, polish=row.polish)
    return eng


def _run(oracle, case, row, signed, w=None, fib=None):
    """one launch of the row against its reference, then policy_fibers_box_host on the returned controls against the reference
    objective; returns (reference, status word)"""
    w, cs, k, ref = B.row_ref(oracle, case, row, signed, w=w, fib=fib)
    what = f"{T.case_id(case)} {row.id} {'signed' if signed else 'synth'}"
    eng = _engine(case, w, cs, row)
    eng.status()
    out, uo, ab = eng.bellman_fibers_box_host(k, ref.idx)
    status = eng.status()
    assert eng.last_kernel() == case.kernels[k], (k, eng.last_kernel())
    B.check_device(ref, out, uo, ab, status, row.lb, row.ub, row.polish, f"{what} {eng.last_kernel()}")
    # the device's objective at the returned controls against the reference's at the same controls
    got, ab2 = eng.policy_fibers_box_host(k, ref.idx, uo)
    assert eng.last_kernel() == case.kernels[k], (k, eng.last_kernel())
    eng.close()
    np.testing.assert_array_equal(ab2, ref.ab)
    want, bad = ref.obj(uo.reshape(-1, len(row.lb)))
    ok = ref.live & ~bad.reshape(ref.ab.shape)
    assert np.array_equal(got[~ref.live], ref.val[~ref.live])
    noise = float(np.abs(got - want.reshape(got.shape))[ok].max() / ref.scale) if ok.any() else 0.0
    print(f"{what}: objective at the returned controls, device against reference {noise:.2e} of the scale")
    assert noise <= T.REL_TOL, f"{what}: policy_fibers_box_host differs from the reference objective by {noise:.3e} of the scale"
    # the minimiser's own value is the objective at its own point
    assert (np.abs(got - out)[ok] <= T.REL_TOL * ref.scale).all(), f"{what}: the returned value is not the objective at the returned control"
    return ref, status


@pytest.mark.parametrize("case,row,signed", KERNEL_ROWS, ids=_ids(KERNEL_ROWS))
def test_box_kernels_vs_restatement(oracle, case, row, signed):
    """the box models at their lowest and their highest registered rank class and the NPL = 2 lqg2d row, two rounds, on the box and
    the cores of box_ref.BOXES (the rows and data classes box_ref.not_built() lists have no entry there: DESIGN.md 6.4)"""
    _run(oracle, case, row, signed)


@pytest.mark.parametrize("case,row,signed", SETTING_ROWS, ids=_ids(SETTING_ROWS))
def test_box_settings_vs_restatement(oracle, case, row, signed):
    """lqg2d (du = 1), tprob3d and cothrust6d (du = 3): polish 0 .. 3, grid = 2 (the cell is the whole box), an even grid, the
    example's grid, an asymmetric box, boxes whose face holds the minimiser of many nodes, one control with lb == ub"""
    _run(oracle, case, row, signed)


@pytest.mark.parametrize("signed", DATA, ids=DATA_IDS)
@pytest.mark.parametrize("row", B.STATIONARY, ids=[r.tag for r in B.STATIONARY])
def test_box_stationary_rows(oracle, row, signed):
    """LqgNd<2> without diffusion through the nodes with x1 = 0, where u = 0 has Q < 1e-14: on a grid point in one launch, on a
    golden-section probe alone in the other (box_ref.STATIONARY).  The status bit must be set in both; the value of a stationary
    point (1e300) is never taken where another point is valid"""
    case = B.stationary_case()
    ref, status = _run(oracle, case, row, signed, w=B.stationary_workload(case), fib=B.stationary_fibers)
    assert ref.status == B.STATUS_STATIONARY and status & B.STATUS_STATIONARY
    assert (ref.val[ref.live] < 1e299).all()


# ------------------------------------------------------------------------------------------------ closed loops
# (workload, grid and rank, box, control grid, polish, cores x mul, calls): one outer step from 40 off-grid states.  Boxes and cores
# as in box_ref.BOXES (sub-boxes of the example's range, scaled cores), for the same reason: the lanes that are pinned.  The last
# entry: the pinned lanes that the polish must have moved off their grid point.  cothrust6d: 0 -- on the oracle's off-grid stencil
# of these 40 states no box of box_ref.candidates, at 5 or 3 control points, one or two rounds and any core scale, leaves three
# pinned lanes that the polish moves; that case holds the grid scan, the clamp and the take rule of k_rollout_ode's box path, and
# the polish of that kernel stays with the 1e-5 lock-step tests against the host
CLOSED = [("lqg2d", dict(ngrid=(25, 23), rank=4), (0.2,), (0.6,), 9, 2, 16.0, ("simulate", "integrate"), 1),
          ("cothrust6d", dict(ngrid=(8,) * 6, rank=8), (0.6, 0.16, 0.16), (1.2, 0.32, 0.32), 5, 1, 16.0, ("integrate",), 0)]


@pytest.mark.parametrize("name,kw,lb,ub,G,polish,mul,calls,min_moved", CLOSED, ids=[c[0] for c in CLOSED])
def test_closed_loop_first_control(oracle, name, kw, lb, ub, G, polish, mul, calls, min_moved):
    """simulate(box=True) with zero noise and integrate(box=True, rk4): the first saved control of one outer step against
    box_ref on the DEVICE's off-grid stencil of the start states (stencil_points, held to offgrid_ref elsewhere): inside the
    reference's interval on pinned lanes, inside the box on all.  The scale is the largest grid-scan value of the lanes (synth
    cores: no cancellation).  The 1e-5 lock-step tests against the host stay as they are"""
    import torch

    from c3sc_amd import workloads as wl
    from c3sc_amd.engine import BellmanEngine

    w = wl.WORKLOADS[name]().scaled(**kw)
    cores = [c * mul for c in wl.synth_cores(w)]
    eng = BellmanEngine(0)
    eng.configure(w, cores)
    eng.set_control_box(np.array(lb), np.array(ub), grid=G, polish=polish)
    n, dt = 40, 0.01
    rng = np.random.default_rng(71)  # off-grid states in the middle 60 % of the state box
    mid, half = (np.array(w.lb) + np.array(w.ub)) / 2, (np.array(w.ub) - np.array(w.lb)) / 2 * 0.6
    x0 = np.ascontiguousarray(mid + half * rng.uniform(-1, 1, (n, w.dx)))
    x_t = torch.from_numpy(x0).cuda()
    V_t, ab_t = eng.stencil_points(x_t)
    torch.cuda.synchronize()
    V, live = V_t.cpu().numpy(), ab_t.cpu().numpy() == 0
    assert live.sum() >= 30
    obj = B.Objective(oracle, w, x0, V)
    scan = np.min([obj.at(B.grid_point(np.array(lb), np.array(ub), G, c))[0] for c in range(G ** len(lb))], axis=0)
    scale = float(np.abs(scan[live]).max())
    ref = B.minimise(obj, lb, ub, G, polish, B.BOX_MARGIN * scale)
    pin = live & ref.pinned(T.REL_TOL * scale)
    for call in calls:
        if call == "simulate":
            res = eng.simulate(x_t, dt, 1, noise_t=torch.zeros((n, 1, w.dx), dtype=torch.float64).cuda(), save_every=1, box=True)
        else:
            res = eng.integrate(x_t, dt, 1, method="rk4", save_every=1, box=True)
        torch.cuda.synchronize()
        u = res["u"].cpu().numpy()[:, 0, :]
        inside = ((u >= ref.ulo) & (u <= ref.uhi)).all(axis=1)
        moved = (ref.u != ref.grid_u).any(axis=1)
        print(f"{name} {call} {eng.last_kernel()}: {int(pin.sum())} pinned of {int(live.sum())} live lanes, {int((pin & moved).sum())} of them moved by the polish, "
              f"{int((pin & ~inside).sum())} outside their interval; largest |u - reference| {np.abs(u - ref.u)[live].max():.2e}")
        assert eng.last_kernel().startswith("k_rollout_ode<" if call == "integrate" else "k_rollout<"), eng.last_kernel()
        assert pin.sum() >= 10 and (pin & moved).sum() >= min_moved
        assert inside[pin].all(), np.flatnonzero(pin & ~inside)
        assert ((u[live] >= np.array(lb)) & (u[live] <= np.array(ub))).all()
    eng.close()
