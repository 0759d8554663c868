"""examples/inventory_impulse.c: a plain C program that solves the two-item stock problem under impulse control
-- host callbacks with c3control_add_impulses, the same functions as device source compiled with c3sc_hip_model_compile_ic,
c3control_vi_solve in impulse mode, the reorder region read with c3control_policy_eval_impulse."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "inventory_impulse")
    host, csrc = os.path.join(ROOT, "c3sc_amd", "host"), os.path.join(ROOT, "c3sc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-D_POSIX_C_SOURCE=200809L", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "inventory_impulse.c"), "-L", host, "-L", csrc, "-lc3sc", "-lc3sc_hip", "-lm",
                           f"-Wl,-rpath,{host}", f"-Wl,-rpath,{csrc}", "-o", exe])
    return exe


def test_example_compiles_against_the_public_headers(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_example_runs_end_to_end(tmp_path):
    import numpy as np

    import impulse_lib as IL

    exe = _build(tmp_path)
    p = subprocess.run([exe], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "INVENTORY_IMPULSE_OK" in p.stdout
    # the program's defaults are impulse_lib's inventory problem: 60 sweeps of dense_vi from the same start
    w = IL.inv_workload(0)
    xg = w.xgrid()
    X = np.stack(np.meshgrid(xg[0], xg[1], indexing="ij"), axis=-1)
    bcost = lambda x: IL.inv_bcost(w.params, x)
    dense, dec = IL.dense_vi(w, IL.inv_host, IL.inv_impulses, bcost, bcost(X), 60)
    vc = float(re.search(r"value at the centre V\(0, 0\) = ([0-9.]+)", p.stdout).group(1))
    assert abs(vc - dense[-1][5, 5]) <= 1e-5, (vc, dense[-1][5, 5])
    # the reorder boundary on the diagonal lies between the last node that orders and the first that does not
    diag = np.array([dec[-1][i, i] for i in range(IL.INV_N)])
    last = max(i for i in range(IL.INV_N) if diag[i] > w.ncand)
    b = float(re.search(r"orders are placed below s = (-?[0-9.]+)", p.stdout).group(1))
    assert xg[0][last] - 1e-9 <= b <= xg[0][last + 1] + 1e-9, (b, xg[0][last], xg[0][last + 1])
