"""Throughput of the device closed-loop integration (c3sc_hip_integrate, RK4): dubins3d (101^3, rank 6, outer and integrator step
1e-2, 1000 outer steps, periodic heading wrapped) and perch7d (20^7, rank 15 -> padded 16, outer step 1e-2 over integrator steps of
1e-4, 120 outer steps, perch.c's keep-in box), 2^16 trajectories each from synthetic value functions, timed with device events
after a warm-up run.  Prints one JSON line per workload: controller evaluations/s (all lane-evaluations, and the live ones before
each trajectory's stop) next to c3sc_hip_simulate's numbers in profiles/simulate_bench.json.

    python tools/integrate_bench.py [--ntraj 65536] [--out profiles/integrate_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from c3sc_amd import engine as E  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402

PERCH_KEEP = ([-math.inf, -1.0] + [-math.inf] * 5, [0.1, 1.0] + [math.inf] * 5)  # perch.c:447-480: stop at x0 > 0.1 or |x1| > 1


def run(name, w, ntraj, nout, dt_out, dt_int, wrap, keep=None):
    import torch

    cores = wl.synth_cores(w)
    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    rng = np.random.default_rng(1)
    lo, hi = np.array(w.lb), np.array(w.ub)
    x0 = torch.from_numpy(np.ascontiguousarray((lo + hi) / 2 + (hi - lo) / 2 * 0.6 * rng.uniform(-1, 1, (ntraj, w.dx)))).cuda()
    kw = dict(method="rk4", dt_int=dt_int, keep_in=keep, wrap_periodic=wrap)
    eng.integrate(x0, dt_out, 2, **kw)  # warm-up
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    eng.timer_start(s)
    t0 = time.perf_counter()
    r = eng.integrate(x0, dt_out, nout, **kw)
    ms = eng.timer_stop(s)
    wall = time.perf_counter() - t0
    nsub = int(round(dt_out / dt_int))
    evals_per_outer = 4 * nsub
    stp = r["stop_step"].cpu().numpy()
    why = r["stop_reason"].cpu().numpy()
    live_outer = np.where(stp >= 0, stp, nout)
    evals = ntraj * nout * evals_per_outer
    live = int(live_outer.sum()) * evals_per_outer  # lane-evaluations before the stop (stopped lanes keep evaluating, frozen)
    return {"workload": name, "method": "rk4", "ngrid": list(w.ngrid), "rank": max(w.ranks), "ncand": w.ncand, "ntraj": ntraj,
            "nout": nout, "dt_out": dt_out, "dt_int": dt_int, "evals_per_lane": nout * evals_per_outer, "kernel": eng.last_kernel(),
            "device_ms": round(ms, 3), "wall_s": round(wall, 3), "evals_per_s": evals / (ms * 1e-3),
            "stopped": int((stp >= 0).sum()), "stop_reasons": {str(k): int((why == k).sum()) for k in range(1, 5)},
            "live_evals": live, "live_fraction": live / evals, "live_evals_per_s": live / (ms * 1e-3),
            "mean_cost": float(r["cost"].mean().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntraj", type=int, default=1 << 16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = [run("dubins3d", wl.c2_dubins(), a.ntraj, 1000, 1e-2, 1e-2, True),
           run("perch7d", wl.perch7d(), a.ntraj, 120, 1e-2, 1e-4, False, PERCH_KEEP)]
    for r in res:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
