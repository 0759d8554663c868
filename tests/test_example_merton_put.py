"""examples/merton_put.c: a plain C program that prices the American put of merton_put.c under Merton's jump diffusion
 -- host callbacks with the stopping cost and c3control_add_jumps, the same functions as device source compiled
with c3sc_hip_model_compile_jd, c3control_fh_solve in stop and jump mode, the exercise boundary read with
c3control_policy_eval_stop."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "merton_put")
    host, csrc = os.path.join(ROOT, "c3sc_amd", "host"), os.path.join(ROOT, "c3sc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-D_POSIX_C_SOURCE=200809L", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "merton_put.c"), "-L", host, "-L", csrc, "-lc3sc", "-lc3sc_hip", "-lm",
                           f"-Wl,-rpath,{host}", f"-Wl,-rpath,{csrc}", "-o", exe])
    return exe


def test_example_compiles_against_the_public_headers(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_example_runs_end_to_end(tmp_path):
    import numpy as np

    import jump_lib as JL
    import stop_lib as SL

    exe = _build(tmp_path)
    p = subprocess.run([exe], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "MERTON_PUT_OK" in p.stdout
    assert "C3SC_STATUS_CFL" not in p.stderr
    # the program's defaults are jump_lib's put: its at-the-money price is the dense chain's V_0(K, K) with the sign of a payoff
    w = JL.put_workload(0)
    dense, _, _ = JL.dense_chain(w, SL.put_host, JL.put_jumps, lambda x: SL.put_psi(JL.PUT_PRM, x), JL.PUT_DELTA, JL.PUT_STAGES)
    price = float(re.search(r"at-the-money price V_0\(K, K\) = ([0-9.]+)", p.stdout).group(1))
    assert abs(price + dense[0][5, 5]) <= 1e-5, (price, dense[0][5, 5])
    bounds = [float(b) for b in re.findall(r"exercise below s = ([0-9.]+)", p.stdout)]
    assert len(bounds) == 3 and all(0.5 < b <= 1.0 for b in bounds) and bounds == sorted(bounds), bounds  # it rises towards K
