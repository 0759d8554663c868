"""Cost of the explicit finite-horizon backup.

1. The horizon per-wave kernel against the plain (infinite-horizon) per-wave kernel of the same run-time compiled model on the
   same candidate list and the same fibers: ms per launch (median of device-timed launches, with the launch-to-launch min and
   max), node backups/s and the horizon-to-plain time ratio, for the 2-D LQR and the pendulum of tests/horizon_lib.py at ranks 4
   and 8.
2. The wall time per stage of a stage-by-stage solve of the LQR on a dense grid: upload the exact train of V_{n+1}, one launch
   over every fiber of dimension 0, read V_n back and factor it (the host SVD included).
Prints one JSON document.
    python tools/horizon_bench.py [--fibers 131072] [--reps 20] [--out profiles/horizon_bench.json]"""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from c3sc_amd import engine as E  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402
import horizon_lib as H  # noqa: E402


def timed(eng, k, idx_t, out_t, uidx_t, reps):
    import torch

    for _ in range(3):
        eng.bellman_fibers(k, idx_t, out_t, uidx_t)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        eng.timer_start()
        eng.bellman_fibers(k, idx_t, out_t, uidx_t, stream_ptr=0)
        ts.append(eng.timer_stop())
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def train(V, maxrank):
    U, S, Vt = np.linalg.svd(V)
    r = int(min(maxrank, (S > 1e-13 * S[0]).sum()))
    return [1, r, 1], [(U[:, :r] * S[None, :r]).reshape(V.shape[0], 1, r), np.ascontiguousarray(Vt[:r, :].T).reshape(V.shape[1], r, 1)]


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--fibers", type=int, default=1 << 17)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stages", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lqr = E.compile_model(H.LQR, 2, 2, ranks=(4, 8), name="lqr_fh", horizon=True, **H.LQR_MASKS)
    pen = E.compile_model(H.PENDULUM, 2, 2, ranks=(4, 8), name="pendulum_fh", horizon=True, **H.PENDULUM_MASKS)
    pen_u = np.array([(x, y) for x in np.linspace(-1.0, 1.0, 7) for y in (0.0, 0.5, 1.0)])
    cases = []
    for rank in (4, 8):
        cases.append(("lqr", 0.002, wl.Workload("lqr_fh", lqr, H.LQR_PRM, 2, 2, (-2.0, -2.0), (2.0, 2.0), (101, 101),
                                                 wl.uniform_ranks(2, rank), 0.1, (wl.BC_ABSORB, wl.BC_ABSORB), [], H.lqr_cands())))
        cases.append(("pendulum", 0.001, wl.Workload("pendulum_fh", pen, H.PENDULUM_PRM, 2, 2, (-np.pi, -3.0), (np.pi, 3.0), (101, 101),
                                                      wl.uniform_ranks(2, rank), 0.1, (wl.BC_PERIODIC, wl.BC_ABSORB), [], pen_u)))
    rows = []
    for name, delta, w in cases:
        eng = E.BellmanEngine(0)
        eng.configure(w, wl.synth_cores(w))
        k = w.dx - 1
        idx_t = torch.tensor(wl.synth_fibers(w, k, a.fibers), device="cuda")
        N = w.ngrid[k]
        out_t = torch.empty((a.fibers, N), dtype=torch.float64, device="cuda")
        ui_t = torch.empty((a.fibers, N), dtype=torch.int32, device="cuda")
        plain = timed(eng, k, idx_t, out_t, ui_t, a.reps)
        plain_kernel = eng.last_kernel()
        eng.set_horizon_step(delta)
        hz = timed(eng, k, idx_t, out_t, ui_t, a.reps)
        st = eng.status()
        nodes, nc = a.fibers * N, len(w.cands)
        rows.append({"case": name, "rank": int(w.ranks[1]), "fibers": a.fibers, "N": N, "candidates": nc, "kernel": plain_kernel,
                     "delta": delta, "cfl_flag": bool(st & 2),
                     "plain_ms": plain[0], "plain_ms_min_max": [plain[1], plain[2]], "plain_node_backups_per_s": nodes / (plain[0] * 1e-3),
                     "horizon_ms": hz[0], "horizon_ms_min_max": [hz[1], hz[2]], "horizon_node_backups_per_s": nodes / (hz[0] * 1e-3),
                     "horizon_over_plain": hz[0] / plain[0]})
        eng.close()
    # a dense stage-by-stage solve of the LQR: wall time per stage
    n = 101
    w = dataclasses.replace(H.lqr_workload(lqr, rank=8, n=n))
    term = lambda x: H.lqr_terminal(H.LQR_PRM, x)
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    Vn = term(X)
    ranks, cores = train(Vn, 8)
    eng = E.BellmanEngine(0)
    eng.configure(dataclasses.replace(w, ranks=tuple(ranks)), cores)
    eng.set_horizon_step(0.002)
    idx = np.zeros((n, 2), dtype=np.int32)
    idx[:, 1] = np.arange(n)
    per = []
    for s in range(a.stages):
        t0 = time.perf_counter()
        eng.upload_value(ranks, cores)
        out, _, _ = eng.bellman_fibers_host(0, idx)
        Vn = np.ascontiguousarray(out.T)
        ranks, cores = train(Vn, 8)
        per.append(time.perf_counter() - t0)
    solve = {"case": "lqr dense solve", "grid": [n, n], "candidates": len(w.cands), "stages": a.stages, "delta": 0.002,
             "kernel": eng.last_kernel(), "ms_per_stage_median": 1e3 * float(np.median(per[1:])),
             "ms_per_stage_min_max": [1e3 * float(np.min(per[1:])), 1e3 * float(np.max(per[1:]))], "cfl_flag": bool(eng.status() & 2)}
    eng.close()
    doc = {"device": torch.cuda.get_device_name(0), "measured": True, "rows": rows, "solve": solve}
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
