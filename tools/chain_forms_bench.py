"""The Markov-chain walker of a run-time compiled model (c3sc_hip_model_compile_mc) measured on Merton's American
put of examples/merton_put.c (tests/jump_lib.py holds the same model: 11 x 11 nodes, 20 stages of delta = 0.025, three marks).

(a) walker steps/s, device-timed, in the plain form, the jump form and the horizon + stop + jump form: the median of --repeats
    runs with the minimum and maximum, and the live share of lane-steps (a frozen lane keeps evaluating its node).  The plain
    and jump forms walk --nsteps steps under V_0; the horizon form walks the 20 stages of the solve, one launch per step.
(b) the chain's Monte-Carlo price: c3control_fh_solve (in a child process, through libc3sc.so) gives V_0 .. V_20; --price-walks
    walks of the horizon + stop + jump chain from the node S = (1, 1) under that stack, the mean of J + D vend (J alone for a walk
    that stopped or left) with its standard error, beside V_0 there.  The stack is the solver's, a cross approximation at rank
    11 of 11 x 11 nodes, so the chain is the backup's own up to the solver's tolerance.

    python tools/chain_forms_bench.py [--nwalk 65536] [--nsteps 256] [--repeats 5] [--out profiles/chain_forms_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from c3sc_amd import engine as E  # noqa: E402
import horizon_lib as H  # noqa: E402
import jump_lib as JL  # noqa: E402


def _timed(eng, torch, repeats, call):
    s = torch.cuda.current_stream().cuda_stream
    ms, last = [], None
    for _ in range(repeats):
        eng.timer_start(s)
        last = call()
        ms.append(eng.timer_stop(s))
    return float(np.median(ms)), float(min(ms)), float(max(ms)), last


def solve_stack():
    """V_0 .. V_nstages of c3control_fh_solve at every node, [nstages + 1, n0, n1] (a child process: the facade owns its context)"""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "fh.npz")
        code = f"import sys; sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); sys.path.insert(0, {ROOT!r}); import jump_lib; jump_lib.fh_child({out!r})"
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-4000:])
        return np.load(out)["V"]


def trains(V):
    """each stage as its exact train in upload_value's layout: (ranks, cores)"""
    out = []
    for Vs in V:
        rk, (c0, c1) = H.full_rank_train(Vs)
        out.append((rk, [c0.reshape(len(c0), -1), c1.reshape(len(c1), -1)]))
    return out


def engine(w, stack, form):
    horizon, stop, jump = form
    eng = E.BellmanEngine(0)
    eng.configure(w, stack[0][1])
    eng.set_stopping(stop)
    if horizon:
        eng.set_horizon_step(JL.PUT_DELTA)
        eng.upload_value_stack([rk for rk, _ in stack], [cs for _, cs in stack])
    eng.set_jumps(jump)
    return eng


def rate(torch, w, stack, name, form, nwalk, nsteps, repeats):
    eng = engine(w, stack, form)
    nsteps = len(stack) - 1 if form[0] else nsteps
    rng = np.random.default_rng(1)
    node0 = torch.from_numpy(np.ascontiguousarray(rng.integers(1, w.ngrid[0] - 1, (nwalk, 2)), dtype=np.int32)).cuda()
    eng.simulate_chain(node0, min(nsteps, 16), seed=1)  # warm-up
    torch.cuda.synchronize()
    med, lo, hi, r = _timed(eng, torch, repeats, lambda: eng.simulate_chain(node0, nsteps, seed=2))
    ex = r["exit"].cpu().numpy()
    step, kind = E.decode_chain_exit(ex)
    live = int(np.where(kind == "running", nsteps, step).sum())
    return {"form": name, "kernel": eng.last_kernel(), "nwalk": nwalk, "nsteps": nsteps, "repeats": repeats, "device_ms_median": med,
            "device_ms_min": lo, "device_ms_max": hi, "steps_per_s": nwalk * nsteps / (med * 1e-3), "live_fraction": live / (nwalk * nsteps),
            "stopped": int((kind == "stopped").sum()), "exited": int((kind == "exit").sum()), "stuck": int((kind == "stuck").sum()),
            "status": eng.status(clear=True), "counters": "none collected"}


def price(torch, w, stack, V, walks, seed):
    eng = engine(w, stack, (True, True, True))
    start = (w.ngrid[0] // 2, w.ngrid[1] // 2)
    node0 = torch.from_numpy(np.ascontiguousarray(np.repeat(np.array([start], dtype=np.int32), walks, axis=0))).cuda()
    r = {k: v.cpu().numpy() for k, v in eng.simulate_chain(node0, len(stack) - 1, seed=seed).items()}
    est = r["cost"] + np.where(r["exit"] == -1, r["disc"] * r["vend"], 0.0)
    kind = E.decode_chain_exit(r["exit"])[1]
    xg = w.xgrid()
    return {"node": list(start), "S": [float(xg[0][start[0]]), float(xg[1][start[1]])], "walks": walks, "stages": len(stack) - 1,
            "delta": JL.PUT_DELTA, "seed": seed, "V0_fh_solve": float(V[0][start]), "chain_mean": float(est.mean()),
            "chain_stderr": float(est.std(ddof=1) / np.sqrt(walks)), "stopped": int((kind == "stopped").sum()),
            "exited": int((kind == "exit").sum()), "status": eng.status(clear=True)}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--nwalk", type=int, default=1 << 16)
    ap.add_argument("--nsteps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--price-walks", type=int, default=1 << 18)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    V = solve_stack()
    stack = trains(V)
    mid = E.compile_model(JL.PUT, 2, 1, ranks=(12,), name="put_mc", horizon=True, stop=True, njump=JL.PUT_NJUMP, chain=True, **JL.PUT_MASKS)
    w = JL.put_workload(mid, rank=11)
    res = {"model": "Merton's American put (tests/jump_lib.py: PUT), 11 x 11 nodes, rank 11 padded to 12",
           "rates": [rate(torch, w, stack, name, form, a.nwalk, a.nsteps, a.repeats)
                     for name, form in (("plain", (False, False, False)), ("jump", (False, False, True)), ("horizon+stop+jump", (True, True, True)))],
           "price": price(torch, w, stack, V, a.price_walks, 11)}
    for r in res["rates"]:
        print(json.dumps(r))
    print(json.dumps(res["price"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
