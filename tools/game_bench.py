"""Cost of the min-max scan: the game per-wave kernel against the plain per-wave kernel of the same run-time
compiled model on the same flat product list and the same fibers.  Per case: ms per launch (median of device-timed launches, with the
launch-to-launch min and max),
node backups/s and candidate evaluations/s of both, and the game-to-plain time ratio.  Prints one JSON document.
    python tools/game_bench.py [--fibers 131072] [--reps 20] [--out profiles/game_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from c3sc_amd import engine as E  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402
from game_lib import LQGAME, LQGAME_MASKS, LQGAME_PRM, PURSUIT, PURSUIT_MASKS, PURSUIT_PRM, product  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lq = E.compile_model(LQGAME, 2, 2, ranks=(4, 8), name="lqgame", game=True, **LQGAME_MASKS)
    pu = E.compile_model(PURSUIT, 3, 2, ranks=(4, 8), name="pursuit", game=True, **PURSUIT_MASKS)
    cases = []
    for rank in (4, 8):
        U, W = np.linspace(-1, 1, 9).reshape(-1, 1), np.linspace(-0.5, 0.5, 5).reshape(-1, 1)
        cases.append(("lqgame", wl.Workload("lqgame", lq, LQGAME_PRM, 2, 2, (-2.0, -2.0), (2.0, 2.0), (101, 101),
                                            wl.uniform_ranks(2, rank), 0.1, (wl.BC_ABSORB, wl.BC_REFLECT), [], product(U, W)), U, W))
        U, W = np.linspace(-1, 1, 5).reshape(-1, 1), np.linspace(-1, 1, 7).reshape(-1, 1)
        cases.append(("pursuit", wl.Workload("pursuit", pu, PURSUIT_PRM, 3, 2, (-3.0, -3.0, -np.pi), (3.0, 3.0, np.pi), (61, 61, 41),
                                             wl.uniform_ranks(3, rank), 0.0, (wl.BC_ABSORB, wl.BC_ABSORB, wl.BC_PERIODIC),
                                             [((0.0, 0.0, 0.0), (0.5, 0.5, 7.5))], product(U, W)), U, W))
    rows = []
    for name, w, U, W in cases:
        eng = E.BellmanEngine(0)
        eng.configure(w, wl.synth_cores(w))
        k = w.dx - 1
        idx_t = torch.tensor(wl.synth_fibers(w, k, a.fibers), device="cuda")
        N = w.ngrid[k]
        out_t = torch.empty((a.fibers, N), dtype=torch.float64, device="cuda")
        ui_t = torch.empty((a.fibers, N), dtype=torch.int32, device="cuda")
        plain_ms, plain_lo, plain_hi = timed(eng, k, idx_t, out_t, ui_t, a.reps)
        plain_kernel = eng.last_kernel()
        res = {}
        for order in ("minmax", "maxmin"):
            eng.set_game(U, W, order)
            res[order] = timed(eng, k, idx_t, out_t, ui_t, a.reps)
        eng.set_controls(w.cands)
        nodes, nc = a.fibers * N, len(w.cands)
        row = {"case": name, "rank": int(w.ranks[1]), "fibers": a.fibers, "N": N, "candidates": nc, "kernel": plain_kernel,
               "plain_ms": plain_ms, "plain_ms_min_max": [plain_lo, plain_hi], "plain_node_backups_per_s": nodes / (plain_ms * 1e-3),
               "plain_candidate_evals_per_s": nodes * nc / (plain_ms * 1e-3)}
        for order, (ms, lo, hi) in res.items():
            row[f"{order}_ms"] = ms
            row[f"{order}_ms_min_max"] = [lo, hi]
            row[f"{order}_node_backups_per_s"] = nodes / (ms * 1e-3)
            row[f"{order}_candidate_evals_per_s"] = nodes * nc / (ms * 1e-3)
            row[f"{order}_over_plain"] = ms / plain_ms
        rows.append(row)
        eng.close()
    doc = {"device": torch.cuda.get_device_name(0), "measured": True, "rows": rows}
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
