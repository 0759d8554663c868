"""The Markov-chain walker (c3sc_hip_simulate_chain) measured: car7d (41^7, rank 10, 9 controls) and dubins3d
(101^3, rank 6) on the synthetic value function of tools/simulate_bench.py.

(a) walker steps/s, device-timed: the median of --repeats runs with the minimum and maximum, and the live share of lane-steps
    (a frozen lane keeps evaluating its node).  Beside it k_rollout's trajectory-steps/s on the same value function, measured
    the same way in the same process (tools/simulate_bench.py is that measurement at its own sizes).
(b) the certificate on car7d: for a seeded set of live start nodes, the mean and standard error over --cert-walks walks each of
    J_n + D_n V(xi_n), beside V(xi_0).  A record: the cores are synthetic, so the distance is not a solver's error.

    python tools/chain_bench.py [--nwalk 65536] [--nsteps 256] [--repeats 5] [--out profiles/chain_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from c3sc_amd import engine as E  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402


def _timed(eng, torch, repeats, call):
    s = torch.cuda.current_stream().cuda_stream
    ms, last = [], None
    for _ in range(repeats):
        eng.timer_start(s)
        last = call()
        ms.append(eng.timer_stop(s))
    return float(np.median(ms)), float(min(ms)), float(max(ms)), last


def live_start_nodes(eng, torch, w, n, seed):
    """n seeded nodes the chain leaves (flag 0, a valid decision), drawn uniformly from the grid"""
    rng = np.random.default_rng(seed)
    got = np.zeros((0, w.dx), dtype=np.int32)
    while len(got) < n:
        cand = np.ascontiguousarray(np.stack([rng.integers(0, N, 4 * n) for N in w.ngrid], -1), dtype=np.int32)
        ui = eng.chain_transitions(torch.from_numpy(cand).cuda())["uidx"].cpu().numpy()
        got = np.concatenate([got, cand[ui >= 0]])
    return np.ascontiguousarray(got[:n])


def rates(name, w, nwalk, nsteps, repeats, dt, wrap):
    import torch

    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    node0 = torch.from_numpy(live_start_nodes(eng, torch, w, nwalk, 1)).cuda()
    eng.simulate_chain(node0, 16, seed=1)  # warm-up
    torch.cuda.synchronize()
    med, lo, hi, r = _timed(eng, torch, repeats, lambda: eng.simulate_chain(node0, nsteps, seed=2))
    kernel = eng.last_kernel()
    ex = r["exit"].cpu().numpy()
    live = int(np.where(ex == -1, nsteps, np.where(ex >= 0, ex, -ex - 2)).sum())
    out = {"workload": name, "ngrid": list(w.ngrid), "rank": max(w.ranks), "ncand": w.ncand, "nwalk": nwalk, "nsteps": nsteps,
           "repeats": repeats, "chain_kernel": kernel, "chain_device_ms_median": med, "chain_device_ms_min": lo, "chain_device_ms_max": hi,
           "chain_steps_per_s": nwalk * nsteps / (med * 1e-3), "chain_live_fraction": live / (nwalk * nsteps),
           "chain_exited": int((ex >= 0).sum()), "chain_stuck": int((ex <= -2).sum()),
           "chain_mean_time": float(r["time"].mean().item())}
    # k_rollout on the same value function: the states of the same start nodes
    xg = w.xgrid()
    x0 = torch.from_numpy(np.ascontiguousarray(np.stack([xg[m][node0.cpu().numpy()[:, m]] for m in range(w.dx)], -1))).cuda()
    eng.simulate(x0, dt, 16, seed=1, wrap_periodic=wrap)
    torch.cuda.synchronize()
    med, lo, hi, r = _timed(eng, torch, repeats, lambda: eng.simulate(x0, dt, nsteps, seed=2, wrap_periodic=wrap))
    ex = r["exit"].cpu().numpy()
    out.update({"rollout_kernel": eng.last_kernel(), "rollout_device_ms_median": med, "rollout_device_ms_min": lo,
                "rollout_device_ms_max": hi, "rollout_traj_steps_per_s": nwalk * nsteps / (med * 1e-3),
                "rollout_live_fraction": int(np.where(ex >= 0, ex, nsteps).sum()) / (nwalk * nsteps)})
    out["chain_over_rollout"] = out["chain_steps_per_s"] / out["rollout_traj_steps_per_s"]
    out["counters"] = "none collected"
    return out


def certificate(w, nstart, walks, nsteps, seed):
    import torch

    eng = E.BellmanEngine(0)
    eng.configure(w, wl.synth_cores(w))
    starts = live_start_nodes(eng, torch, w, nstart, seed)
    node0 = torch.from_numpy(np.ascontiguousarray(np.repeat(starts, walks, axis=0))).cuda()
    v0 = eng.simulate_chain(torch.from_numpy(starts).cuda(), 0)["vend"].cpu().numpy()  # no step: V at the start nodes
    r = eng.simulate_chain(node0, nsteps, seed=seed)
    ex = r["exit"].cpu().numpy()
    est = r["cost"].cpu().numpy() + np.where(ex == -1, r["disc"].cpu().numpy() * r["vend"].cpu().numpy(), 0.0)
    est = est.reshape(nstart, walks)
    rows = [{"node": starts[i].tolist(), "V": float(v0[i]), "mean": float(est[i].mean()),
             "stderr": float(est[i].std(ddof=1) / np.sqrt(walks))} for i in range(nstart)]
    return {"workload": "car7d", "ngrid": list(w.ngrid), "rank": max(w.ranks), "value_function": "synthetic cores (workloads.synth_cores)",
            "nstart": nstart, "walks_per_start": walks, "nsteps": nsteps, "seed": seed, "exited": int((ex >= 0).sum()),
            "stuck": int((ex <= -2).sum()), "status": eng.status(clear=True), "starts": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nwalk", type=int, default=1 << 16)
    ap.add_argument("--nsteps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cert-starts", type=int, default=16)
    ap.add_argument("--cert-walks", type=int, default=1024)
    ap.add_argument("--cert-steps", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"rates": [rates("car7d", wl.c4_car7d(), a.nwalk, a.nsteps, a.repeats, 0.01, False),
                     rates("dubins3d", wl.c2_dubins(), a.nwalk, a.nsteps, a.repeats, 0.01, True)],
           "certificate": certificate(wl.c4_car7d(), a.cert_starts, a.cert_walks, a.cert_steps, 7)}
    for r in res["rates"]:
        print(json.dumps(r))
    print(json.dumps(res["certificate"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
