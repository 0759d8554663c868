"""Cost of the intervention actions in the Bellman backup.

The impulse form of the per-wave kernel against the plain form of the same run-time compiled model on the same candidate list
and the same fibers, at ranks 4 and 8 and with M = 1 and M = 3 interventions: ms per launch as the median of device-timed
launches with the launch-to-launch min and max, node backups/s and the impulse-to-plain time ratio.  The model is the LQR of
tests/jump_lib.py on a 101 x 101 grid whose dimensions both absorb, with M interventions and M jump marks of compile-time
counts (displacements that are no multiples of the grid spacing, so every target is interpolated; some land beyond a face).
Four timings per case: the plain form, the impulse form, the plain form again (a drift of the clock shows as a difference
between its two medians), and the impulse form on top of the jump form.  The share of live nodes at which an intervention wins
is recorded, which also shows that the impulse form ran (the entry's name is the same for every form).
Prints one JSON document.
    python tools/impulse_bench.py [--fibers 131072] [--reps 50] [--out profiles/impulse_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from c3sc_amd import engine as E  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402
import jump_lib as JL  # noqa: E402
import stop_lib as SL  # noqa: E402

# M marks of equal weight and M interventions of the cost prm[4] (1 + 0.1 m): both move the state by 0.13 (m + 1) along
# dimension m % 2
MODEL_M = r"""
__device__ double jumprate(const double *prm, const double *x) { return prm[6] + prm[7] * x[0] * x[0]; }
__device__ double jump(const double *prm, const double *x, int m, double *y)
{
    y[0] = x[0] + ((m & 1) ? 0.0 : 0.13 * (m + 1));
    y[1] = x[1] + ((m & 1) ? 0.13 * (m + 1) : 0.0);
    return 1.0 / C3SC_NJUMP;
}
__device__ double impulse(const double *prm, const double *x, int m, double *y)
{
    y[0] = x[0] + ((m & 1) ? 0.0 : 0.13 * (m + 1));
    y[1] = x[1] + ((m & 1) ? 0.13 * (m + 1) : 0.0);
    return prm[4] * (1.0 + 0.1 * m);
}
"""
COST = {4: 0.02, 8: 0.04}  # per rank: about the spread of the seeded train's values, so that interventions win at part of the nodes


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
    for M in (1, 3):
        mid = E.compile_model(SL.LQR + MODEL_M, 2, 2, ranks=(4, 8), name=f"lqr_ic_m{M}", njump=M, nimpulse=M, **JL.LQR_MASKS)
        for rank in (4, 8):
            prm = JL.LQR_PRM[:4] + (COST[rank],) + JL.LQR_PRM[5:]
            w = wl.Workload("lqr_ic", mid, prm, 2, 2, (-2.0, -2.0), (2.0, 2.0), (101, 101), wl.uniform_ranks(2, rank), 0.1,
                            (wl.BC_ABSORB, wl.BC_ABSORB), [], SL.lqr_cands())
            eng = E.BellmanEngine(0)
            eng.configure(w, wl.synth_cores(w))
            k = w.dx - 1
            idx_t = torch.tensor(wl.synth_fibers(w, k, a.fibers), device="cuda")
            N = w.ngrid[k]
            out_t = torch.empty((a.fibers, N), dtype=torch.float64, device="cuda")
            ui_t = torch.empty((a.fibers, N), dtype=torch.int32, device="cuda")
            ab_t = torch.empty((a.fibers, N), dtype=torch.int32, device="cuda")
            eng.bellman_fibers(k, idx_t, out_t, ui_t, ab_t)
            plain = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            kernel = eng.last_kernel()
            eng.set_impulses(True)
            imp = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            torch.cuda.synchronize()
            live = ab_t == 0
            wins = float(((ui_t > len(w.cands)) & live).sum().item() / live.sum().item())
            eng.set_impulses(False)
            again = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            eng.set_jumps(True)
            eng.set_impulses(True)
            both = timed(eng, k, idx_t, out_t, ui_t, a.reps)
            torch.cuda.synchronize()
            nodes = a.fibers * N
            base = 0.5 * (plain[0] + again[0])
            rows.append({"interventions": M, "marks": M, "rank": rank, "fibers": a.fibers, "N": N, "candidates": len(w.cands),
                         "kernel": kernel, "reps": a.reps, "live_nodes_where_an_intervention_wins": wins,
                         "plain_ms": plain[0], "plain_ms_min_max": [plain[1], plain[2]],
                         "plain_again_ms": again[0], "plain_again_ms_min_max": [again[1], again[2]],
                         "impulse_ms": imp[0], "impulse_ms_min_max": [imp[1], imp[2]],
                         "impulse_jump_ms": both[0], "impulse_jump_ms_min_max": [both[1], both[2]],
                         "plain_node_backups_per_s": nodes / (base * 1e-3), "impulse_node_backups_per_s": nodes / (imp[0] * 1e-3),
                         "impulse_over_plain": imp[0] / base, "impulse_jump_over_plain": both[0] / base, "status": eng.status()})
            eng.close()
    doc = {"device": torch.cuda.get_device_name(0), "measured": True, "rows": rows}
    s = json.dumps(doc, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
