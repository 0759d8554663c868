"""k_rollout held to the numpy restatement of one of its steps (tests/rollout_ref.py) in every form the rollouts are offered in
(DESIGN.md 4.17): plain, game, every subset of {horizon, stop, jump}, impulse, impulse + jump, at rank classes 4 and 12 (the game
at 4), once with Philox normals and once with zero normals (the jump rows draw Philox jumps in both).

Every row of rollout_ref.ROWS runs 300 lanes (a full workgroup and 44 lanes of a second one, whose tail repeats the last
trajectory) with save_every = 1, and rollout_ref.check replays the run in lock-step from its own saved states: the action of
every live lane at every step is the reference's wherever its margin exceeds MARGIN_TOL (at most 5 % may not), the saved
control is the candidate's row bit for bit and 0 for a stopped, intervening or frozen lane, next states, costs, V_end and
xfinal agree to 1e-12 max(1, |.|) and the exit codes exactly.  The occurrence counts tests/test_rollout_ref.py demands of the
reference's own closed loop hold on the device's run as well.  The 3-D rows run 125 candidates (the candidate table is filled
twice) on 5 x 128 x 5 with unequal bond ranks; one stack alternates between classes 4 and 12 from stage to stage; one jump row
and one impulse row run as a CONSTELM value function.

Launch cut and batch split: stop, stop + jump and impulse + jump give the same bits in one launch, in launches of 7 steps, and
split at lane 50 in launches of 5 steps with the second part's traj_offset moved by 50."""
import dataclasses

import numpy as np
import pytest

from c3sc_amd import engine as E
import rollout_ref as RR
from sim_kernel_cases import ODE_MAX_DROPPED as MAX_UNSURE  # the closed-loop suite's cap on unsure decisions: 5 %

pytestmark = pytest.mark.gpu
STATUS_CFL = 2
_ids = {}


def _mid(key):
    """the device model of a row: the neighbours' spec under the neighbours' name (the library compiles a spec once per process)"""
    if key not in _ids:
        name, ranks = RR.COMPILED[key]
        spec = dict(RR.specs()[key.replace("_c4", "")])
        _ids[key] = E.compile_model(spec.pop("source"), spec.pop("d"), spec.pop("du"), ranks=ranks, name=name, **spec)
    return _ids[key]


def _class(ranks):
    return 4 if max(ranks) <= 4 else 12


def _engine(row, ctx):
    form = row.form
    eng = E.BellmanEngine(0)
    eng.configure(dataclasses.replace(ctx.w, model=_mid(row.model), ranks=tuple(ctx.ranks[-1])), ctx.cores[-1])
    if "game" in form:
        eng.set_game(*ctx.game)
    if "horizon" in form:
        eng.set_horizon_step(ctx.dt)
    if "stop" in form:
        eng.set_stopping(True)
    if "jump" in form:
        eng.set_jumps(True)
    if "impulse" in form:
        eng.set_impulses(True)
    if ctx.constelm:
        eng.set_interp(True)
    if "horizon" in form:
        eng.upload_value_stack(ctx.ranks, ctx.cores)
    return eng


def _simulate(eng, ctx, x0=None, traj_offset=None, **kw):
    import torch

    x0 = ctx.x0 if x0 is None else x0
    x0_t = torch.tensor(x0, dtype=torch.float64, device="cuda")
    noise = None if ctx.noise is None else torch.tensor(ctx.noise[:len(x0)], dtype=torch.float64, device="cuda")
    r = eng.simulate(x0_t, ctx.dt, ctx.N, seed=ctx.seed, noise_t=noise, wrap_periodic=ctx.wrap, save_every=1,
                     traj_offset=ctx.traj_offset if traj_offset is None else traj_offset, **kw)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("row", RR.ROWS, ids=[r.id for r in RR.ROWS])
def test_rollout_form_vs_numpy_step(row):
    ctx = RR.make_ctx(row)
    eng = _engine(row, ctx)
    eng.status(clear=True)
    run = _simulate(eng, ctx)
    name = RR.COMPILED[row.model][0]
    assert eng.last_kernel() == f"k_rollout<rtc:{name},{_class(ctx.ranks[-1])}>", eng.last_kernel()
    if row.opts.get("mixed"):
        assert {_class(r) for r in ctx.ranks} == {4, 12} and _class(ctx.ranks[-1]) == 4
    else:
        assert _class(ctx.ranks[-1]) == row.rp
    if "horizon" in row.form:
        assert eng.status() & STATUS_CFL == 0
    counts, bad, err = RR.check(row.form, ctx, run)
    share = counts["unsure"] / max(1, counts["checked"])
    print(row.id, "max state err", err["state"], "cost err", err["cost"], "vend err", err["vend"], "unsure share", share, counts)
    assert not bad, bad
    assert share <= MAX_UNSURE, share
    RR.assert_occurrences(row, counts)
    eng.close()


@pytest.mark.parametrize("row", RR.CUT_ROWS, ids=[r.id for r in RR.CUT_ROWS])
def test_launch_cut_and_batch_split_keep_the_bits(row):
    """steps_per_launch < nsteps: x, J and ex come back from the state buffer (ex in the stop forms' -(k + 2) encoding), and the
    uniforms are keyed by traj_offset + i"""
    import torch

    ctx = RR.make_ctx(row)
    eng = _engine(row, ctx)
    whole = _simulate(eng, ctx)
    cut = _simulate(eng, ctx, steps_per_launch=7)
    a = _simulate(eng, ctx, x0=ctx.x0[:50], steps_per_launch=5)
    assert ctx.noise is None  # Philox normals: the second part's noise follows from its traj_offset
    b = _simulate(eng, ctx, x0=ctx.x0[50:], traj_offset=ctx.traj_offset + 50, steps_per_launch=5)
    for q in ("traj", "u", "cost", "exit", "vend"):
        assert torch.equal(whole[q], cut[q]), q
        assert torch.equal(whole[q], torch.cat([a[q], b[q]])), q
    ex = whole["exit"].cpu().numpy()
    step, stopped = E.decode_exit(ex) if "stop" in row.form else (ex, np.zeros(len(ex), dtype=np.int32))
    done = step >= 0
    assert (done & (step < 5)).sum() >= 3 and (done & (step > 7)).sum() >= 3, "lanes end before the first cut and after the last"
    if "stop" in row.form:
        assert (stopped[step < 5] == 1).any() and (stopped[step > 7] == 1).any() and (stopped[done] == 0).any()
    assert (ex == -1).any()
    eng.close()
