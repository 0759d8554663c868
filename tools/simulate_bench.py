"""Throughput of the device rollouts (c3sc_hip_simulate): car7d (41^7, rank 10, 9 controls) and dubins3d (101^3, rank 6), 2^16
trajectories x 1000 steps from seeded noise, timed with device events after a warm-up run.  Prints one JSON line per workload:
trajectory-steps/s (all lane-steps, and the live ones before each trajectory's exit), and the algorithmic flop and byte counts per trajectory-step computed from the shapes (off-grid stencil
~ (3d - 2) r^2 interpolated core entries, each read at two nodes; controller over U candidates), with the bound they imply.

    python tools/simulate_bench.py [--ntraj 65536] [--nsteps 1000] [--out profiles/simulate_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from c3sc_amd import engine as E  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402

PEAK_F64_TFLOPS = 78.6   # MI355X vector FP64
PEAK_HBM_TBS = 8.0


def shape_counts(w):
    d, r, U = w.dx, max(w.ranks), w.ncand
    mid = max(d - 2, 0)
    # stencil: suffix pass (d-2 middle cores) + prefix pass (d-2) + 2 neighbours per middle core; each entry interpolated
    # between two nodes (3 flops) and multiplied-added (2 flops); edge cores O(r)
    entries = (4 * mid) * r * r + 8 * r
    flops = entries * 5 + U * (12 * d + 20) + 20 * d
    bytes_ = entries * 2 * 8  # every interpolated entry reads two node values (L2-resident cores; no reuse assumed)
    return flops, bytes_


def run(name, w, ntraj, nsteps, dt, wrap):
    import torch

    cores = wl.synth_cores(w)
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    rng = np.random.default_rng(1)
    lo, hi = np.array(w.lb), np.array(w.ub)
    x0 = torch.from_numpy(np.ascontiguousarray((lo + hi) / 2 + (hi - lo) / 2 * 0.6 * rng.uniform(-1, 1, (ntraj, w.dx)))).cuda()
    eng.simulate(x0, dt, 64, seed=1, wrap_periodic=wrap)  # warm-up
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    eng.timer_start(s)
    t0 = time.perf_counter()
    r = eng.simulate(x0, dt, nsteps, seed=2, wrap_periodic=wrap)
    ms = eng.timer_stop(s)
    wall = time.perf_counter() - t0
    ex = r["exit"].cpu().numpy()
    live = int(np.where(ex >= 0, ex, nsteps).sum())  # lane-steps before the exit (frozen lanes keep running but park on a face)
    flops, bytes_ = shape_counts(w)
    ts = ntraj * nsteps / (ms * 1e-3)
    return {"workload": name, "ngrid": list(w.ngrid), "rank": max(w.ranks), "ncand": w.ncand, "ntraj": ntraj, "nsteps": nsteps,
            "kernel": eng.last_kernel(), "device_ms": round(ms, 3), "wall_s": round(wall, 3), "traj_steps_per_s": ts,
            "flops_per_traj_step": flops, "bytes_per_traj_step": bytes_,
            "achieved_tflops": ts * flops / 1e12, "achieved_tbs_if_from_hbm": ts * bytes_ / 1e12,
            "fraction_fp64_peak": ts * flops / 1e12 / PEAK_F64_TFLOPS, "fraction_hbm_peak": ts * bytes_ / 1e12 / PEAK_HBM_TBS,
            "exited": int((ex >= 0).sum()), "live_traj_steps": live, "live_fraction": live / (ntraj * nsteps),
            "live_traj_steps_per_s": live / (ms * 1e-3), "mean_cost": float(r["cost"].mean().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntraj", type=int, default=1 << 16)
    ap.add_argument("--nsteps", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = [run("car7d", wl.c4_car7d(), a.ntraj, a.nsteps, 0.01, False),
           run("dubins3d", wl.c2_dubins(), a.ntraj, a.nsteps, 0.01, True)]
    for r in res:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
