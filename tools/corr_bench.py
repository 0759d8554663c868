"""Cost of the cross-diffusion terms in the Bellman backup.

The corr form of the per-wave kernel against the plain form of the same run-time compiled model on the same candidate list and
the same fibers, at ranks 4 and 8: P = 1 pair on the 2-D LQR (101 x 101) and P = 3 pairs on the 3-D LQR (101 x 101 x 101, pair
(0,2) negative), fibers of 101 nodes along the last dimension: ms per launch as the median of device-timed launches with the
launch-to-launch min and max, node backups/s and the corr-to-plain time ratio.  Every pair costs two point evaluations of the
function train per node.  The share of live nodes whose value differs from the plain launch's is recorded, which also shows that
the corr form ran (the entry's name is the same for both forms).  The plain form is timed before and after the corr form, so
that a drift of the clock shows as a difference between its two medians.  Prints one JSON document.
    python tools/corr_bench.py [--fibers 131072] [--reps 50] [--out profiles/corr_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from c3sc_amd import engine as E  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402
import stop_lib as SL  # noqa: E402

# equal spacings: dominance holds iff the covariances of a dimension's pairs sum to at most sigma^2
COVAR_2D = r"""
__device__ double covar(const double *prm, const double *x, int p) { return 0.5 * prm[0] * prm[0] * cos(x[0] + x[1]); }
"""
COVAR_3D = r"""
__device__ double covar(const double *prm, const double *x, int p) { return (p == 1 ? -0.3 : 0.3) * prm[0] * prm[0]; }
"""
CASES = {1: (SL.LQR + COVAR_2D, 2, SL.LQR_MASKS, ((0, 1),), SL.lqr_cands), 3: (SL.LQR3 + COVAR_3D, 3, SL.LQR3_MASKS, ((0, 1), (0, 2), (1, 2)), SL.lqr3_cands)}


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
    rows = []
    for P, (src, d, masks, pairs, cands) in CASES.items():
        mid = E.compile_model(src, d, d, ranks=(4, 8), name=f"lqr_cd_p{P}", corr_pairs=pairs, **masks)
        for rank in (4, 8):
            w = wl.Workload("lqr_cd", mid, SL.LQR_PRM, d, d, (-2.0,) * d, (2.0,) * d, (101,) * d, wl.uniform_ranks(d, rank), 0.1,
                            (wl.BC_ABSORB,) * d, [], cands())
            eng = E.BellmanEngine(0)
            eng.configure(w, wl.synth_cores(w))
            k = w.dx - 1
            idx_t = torch.tensor(wl.synth_fibers(w, k, a.fibers), device="cuda")
            N = w.ngrid[k]
            out_t = torch.empty((a.fibers, N), dtype=torch.float64, device="cuda")
            ui_t = torch.empty((a.fibers, N), dtype=torch.int32, device="cuda")
            ab_t = torch.empty((a.fibers, N), dtype=torch.int32, device="cuda")
            eng.bellman_fibers(k, idx_t, out_t, ui_t, ab_t)
            plain_out = out_t.clone()
            plain = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            kernel = eng.last_kernel()
            eng.set_correlation(True)
            corr = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            torch.cuda.synchronize()
            live = ab_t == 0
            moved = float(((out_t != plain_out) & live).sum().item() / live.sum().item())
            eng.set_correlation(False)
            again = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            nodes = a.fibers * N
            base = 0.5 * (plain[0] + again[0])
            rows.append({"pairs": P, "d": d, "rank": rank, "fibers": a.fibers, "N": N, "candidates": len(w.cands), "kernel": kernel,
                         "reps": a.reps, "live_nodes_moved_by_the_cross_terms": moved,
                         "plain_ms": plain[0], "plain_ms_min_max": [plain[1], plain[2]],
                         "plain_again_ms": again[0], "plain_again_ms_min_max": [again[1], again[2]],
                         "corr_ms": corr[0], "corr_ms_min_max": [corr[1], corr[2]],
                         "plain_node_backups_per_s": nodes / (base * 1e-3), "corr_node_backups_per_s": nodes / (corr[0] * 1e-3),
                         "corr_over_plain": corr[0] / base, "status": eng.status()})
            eng.close()
    doc = {"device": torch.cuda.get_device_name(0), "measured": True, "rows": rows}
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
