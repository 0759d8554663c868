"""Run-time compiled device models (c3sc_hip_model_compile) against the built-in functors:

- cold compile wall time per model and rank set (the first compile of each spec in this process);
- one per-wave Bellman launch over 2^14 fibers: the restated chain against the built-in Chain<4> (same masks, same bits), and
  the restated Dubins car (device sin / cos per node and candidate) against the built-in Dubins3D (host-tabulated cos / sin);
- value iteration of the damped pendulum through c3control_vi_solve (examples/pendulum_rtc.c): the TABLE path (host callbacks
  for every node and candidate) against the run-time model (device-resident cross), seconds per sweep.

    python tools/rtc_bench.py [--reps 20] [--out profiles/rtc_bench.json]
"""
import argparse
import dataclasses
import json
import os
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from c3sc_amd import engine as E  # noqa: E402
from c3sc_amd import workloads as wl  # noqa: E402
import rtc_models as R  # noqa: E402

FIBERS = 1 << 14


def compile_times():
    specs = [("chain4", R.CHAIN4, 4, 1, (4,), False, R.CHAIN4_MASKS), ("dubins3d", R.DUBINS3D, 3, 1, (4, 8), False, R.DUBINS3D_MASKS),
             ("dubins3d", R.DUBINS3D, 3, 1, (4, 8, 12, 16, 20), False, R.DUBINS3D_MASKS),
             ("pendulum", R.PENDULUM, 2, 1, (4, 8), False, R.PENDULUM_MASKS), ("lqg2d", R.LQG2D, 2, 1, (4, 8), True, R.LQG2D_MASKS)]
    out, ids = [], {}
    for name, src, d, du, ranks, box, masks in specs:
        t0 = time.perf_counter()
        mid = E.compile_model(src, d, du, ranks=ranks, box=box, name=f"{name}_r{'_'.join(map(str, ranks))}", **masks)
        dt = time.perf_counter() - t0
        co = E.code_object(src, d, du, ranks=ranks, box=box, name=f"{name}_r{'_'.join(map(str, ranks))}", **masks)
        out.append({"model": name, "ranks": list(ranks), "box": box, "compile_s": round(dt, 3), "code_object_bytes": len(co)})
        ids[(name, ranks)] = mid
    return out, ids


def launch(w, cores, k, reps):
    import torch

    eng = E.BellmanEngine(0)
    eng.configure(w, cores)
    eng.set_variant(E.VARIANT_FIBER_PER_WAVE)  # AUTO would take the fiber-pair kernel of the built-in model at 2^14 fibers
    idx = torch.from_numpy(np.ascontiguousarray(wl.synth_fibers(w, k, FIBERS), dtype=np.int32)).cuda()
    out = torch.empty((FIBERS, w.ngrid[k]), dtype=torch.float64, device="cuda")
    eng.bellman_fibers(k, idx, out)  # warm-up: module load, occupancy query
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    ms = []
    for _ in range(reps):
        eng.timer_start(s)
        eng.bellman_fibers(k, idx, out)
        ms.append(eng.timer_stop(s))
    return eng.last_kernel(), float(np.median(ms)), out.cpu().numpy()


def compare(name, w, rid, k, reps):
    cores = wl.synth_cores(w)
    kb, mb, ob = launch(w, cores, k, reps)
    kr, mr, orr = launch(dataclasses.replace(w, model=rid), cores, k, reps)
    nodes = FIBERS * w.ngrid[k]
    return {"workload": name, "ngrid": list(w.ngrid), "rank": max(w.ranks), "k": k, "fibers": FIBERS, "reps": reps,
            "builtin": {"kernel": kb, "median_ms": round(mb, 4), "nodes_per_s": nodes / (mb * 1e-3)},
            "runtime": {"kernel": kr, "median_ms": round(mr, 4), "nodes_per_s": nodes / (mr * 1e-3)},
            "runtime_over_builtin": round(mr / mb, 3), "max_rel_diff": float(np.abs(orr - ob).max() / np.abs(ob).max()),
            "bitwise_equal": bool(np.array_equal(orr, ob))}


def vi_solve(n, sweeps):
    from rtc_models import build_example

    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_example(Path(tmp))
        for mode in ("table", "rtc"):
            t0 = time.perf_counter()
            p = subprocess.run([exe, str(n), str(sweeps), mode], cwd=tmp, capture_output=True, text=True, timeout=1800)
            wall = time.perf_counter() - t0
            m = re.search(r"value iteration: (\d+) sweeps, relative change ([^,\s]+), \|V\| = ([^,\s]+), (\S+) s per sweep", p.stdout)
            if p.returncode != 0 or not m:
                raise RuntimeError(f"pendulum_rtc {mode} failed: {p.stdout[-800:]} {p.stderr[-800:]}")
            res[mode] = {"sweeps": int(m.group(1)), "rel_change": float(m.group(2)), "norm_V": float(m.group(3)),
                         "s_per_sweep": float(m.group(4)), "process_wall_s": round(wall, 3)}
    res["ngrid"] = [n, n]
    res["table_over_runtime_per_sweep"] = round(res["table"]["s_per_sweep"] / res["rtc"]["s_per_sweep"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    comp, ids = compile_times()
    for r in comp:
        print(json.dumps(r), flush=True)
    chain = wl.Workload("chain4", wl.MODEL_CHAIN, (4.0, 1.0, 0.5, 1.0), 4, 1, (-2.0,) * 4, (2.0,) * 4, (64,) * 4, wl.uniform_ranks(4, 4),
                        0.1, (wl.BC_REFLECT,) * 4, [], np.array([[-1.0], [0.0], [1.0]]))
    launches = [compare("chain4", chain, ids[("chain4", (4,))], 1, a.reps),
                compare("dubins3d", wl.c2_dubins().scaled(rank=8), ids[("dubins3d", (4, 8))], 1, a.reps)]
    for r in launches:
        print(json.dumps(r), flush=True)
    vi = [vi_solve(61, 100), vi_solve(121, 40)]  # N <= 128: the largest fiber a per-wave kernel takes
    for r in vi:
        print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"compile": comp, "per_wave_launch": launches, "pendulum_vi_solve": vi}, f, indent=1)


if __name__ == "__main__":
    main()
