"""Cost of the stop action in the Bellman backup.

The stop form of the per-wave kernel against the plain form of the same run-time compiled model (the stopping LQR of
tests/stop_lib.py) on the same candidate list and the same fibers, in the infinite-horizon and in the horizon form, at ranks 4
and 8: ms per launch as the median of device-timed launches with the launch-to-launch min and max, node backups/s and the
stop-to-plain time ratio.  The constant c0 of psi = c0 + c1 |x|^2 is set per case to the median of the continuation values of a
sample of nodes (from the numpy restatement over the device's stencils), so that stop wins at about half of the live nodes; the
share of nodes of the timed launch whose index is ncand is recorded, which also shows that the stop form ran (the entry's name
is the same for both forms).  The plain form is timed before and after the stop form, so that a drift of the clock shows as a
difference between its two medians.  Prints one JSON document.
    python tools/stop_bench.py [--fibers 131072] [--reps 50] [--out profiles/stop_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from c3sc_amd import engine as E  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402
import backup_ref as BR  # noqa: E402
import stop_lib as SL  # noqa: E402


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


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--fibers", type=int, default=1 << 17)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mid = E.compile_model(SL.LQR, 2, 2, ranks=(4, 8), name="lqr_os", horizon=True, stop=True, **SL.LQR_MASKS)
    rows = []
    for rank in (4, 8):
        for delta in (0.0, 0.002):
            w = wl.Workload("lqr_os", mid, SL.LQR_PRM, 2, 2, (-2.0, -2.0), (2.0, 2.0), (101, 101), wl.uniform_ranks(2, rank), 0.1,
                            (wl.BC_ABSORB, wl.BC_ABSORB), [], SL.lqr_cands())
            eng = E.BellmanEngine(0)
            eng.configure(w, wl.synth_cores(w))
            eng.set_horizon_step(delta)
            k = w.dx - 1
            # psi at the median of the continuation values of a sample of live nodes
            sidx = wl.synth_fibers(w, k, 64, seed=7)
            costs, ab = eng.stencil_fibers_host(k, sidx)
            h2, t = BR.mca_constants(w)
            x = BR.node_states(w, k, sidx).reshape(-1, 2)
            vals, _, _ = BR.candidate_values(SL.lqrn_host, w.params, x, costs.reshape(-1, 5), np.asarray(w.cands), h2, t, w.discount,
                                             delta=delta if delta > 0.0 else None)
            live = ab.reshape(-1) == 0
            c0 = float(np.median(np.nanmin(vals, axis=1)[live] - SL.LQR_PRM[5] * (x[live] ** 2).sum(-1)))
            eng.set_model(mid, SL.LQR_PRM[:4] + (c0, SL.LQR_PRM[5]))
            idx_t = torch.tensor(wl.synth_fibers(w, k, a.fibers), device="cuda")
            N = w.ngrid[k]
            out_t = torch.empty((a.fibers, N), dtype=torch.float64, device="cuda")
            ui_t = torch.empty((a.fibers, N), dtype=torch.int32, device="cuda")
            plain = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            kernel = eng.last_kernel()
            eng.set_stopping(True)
            stop = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            torch.cuda.synchronize()
            share = float((ui_t == w.ncand).float().mean().item())
            eng.set_stopping(False)
            again = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            nodes = a.fibers * N
            base = 0.5 * (plain[0] + again[0])
            rows.append({"form": "horizon" if delta > 0.0 else "infinite", "rank": rank, "fibers": a.fibers, "N": N,
                         "candidates": len(w.cands), "kernel": kernel, "delta": delta, "reps": a.reps, "psi_c0": c0, "stop_share_of_nodes": share,
                         "plain_ms": plain[0], "plain_ms_min_max": [plain[1], plain[2]],
                         "plain_again_ms": again[0], "plain_again_ms_min_max": [again[1], again[2]],
                         "stop_ms": stop[0], "stop_ms_min_max": [stop[1], stop[2]],
                         "plain_node_backups_per_s": nodes / (base * 1e-3), "stop_node_backups_per_s": nodes / (stop[0] * 1e-3),
                         "stop_over_plain": stop[0] / base, "status": eng.status()})
            eng.close()
    doc = {"device": torch.cuda.get_device_name(0), "measured": True, "rows": rows}
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
