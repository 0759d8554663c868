"""examples/heston_put.c: a plain C program that prices an American put under Heston in (log-price, variance) coordinates
 -- host callbacks with the stopping cost and c3control_add_covariance, the same functions as device source
compiled with c3sc_hip_model_compile_cd, c3control_fh_solve in stop and correlation mode, the price with and without rho."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "heston_put")
    host, csrc = os.path.join(ROOT, "c3sc_amd", "host"), os.path.join(ROOT, "c3sc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-D_POSIX_C_SOURCE=200809L", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "heston_put.c"), "-L", host, "-L", csrc, "-lc3sc", "-lc3sc_hip", "-lm",
                           f"-Wl,-rpath,{host}", f"-Wl,-rpath,{csrc}", "-o", exe])
    return exe


def test_example_compiles_against_the_public_headers(tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_example_runs_end_to_end(tmp_path):
    import dataclasses

    import corr_lib as CL

    exe = _build(tmp_path)
    p = subprocess.run([exe], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "HESTON_PUT_OK" in p.stdout
    assert "C3SC_STATUS_CFL" not in p.stderr and "C3SC_STATUS_DOMINANCE" not in p.stderr
    ratio = float(re.search(r"grid ratio h_v / h_x = ([0-9.]+)", p.stdout).group(1))
    assert abs(ratio - 0.125) <= 1e-4
    # the program's defaults are corr_lib's Heston put: its prices are the dense chains' V_0 at the middle node, with the sign
    # of a payoff
    w = CL.heston_workload(0)
    psi = lambda x: CL.heston_psi(CL.HESTON_PRM, x)
    dense, _, cfl, dom = CL.dense_chain(w, CL.heston_host, CL.heston_covar, CL.HESTON_PAIRS, psi, CL.HESTON_DELTA, CL.HESTON_STAGES)
    rho0, _, _, _ = CL.dense_chain(dataclasses.replace(w, params=CL.HESTON_RHO0_PRM), CL.heston_host, CL.heston_covar, CL.HESTON_PAIRS, psi,
                                   CL.HESTON_DELTA, CL.HESTON_STAGES)
    assert not cfl and not dom
    prices = [float(v) for v in re.findall(r"at-the-money price V_0\(log K, v = 0.12\) = ([0-9.]+)", p.stdout)]
    assert len(prices) == 2
    assert abs(prices[0] + dense[0][5, 5]) <= 1e-5, (prices[0], dense[0][5, 5])
    assert abs(prices[1] + rho0[0][5, 5]) <= 1e-5, (prices[1], rho0[0][5, 5])
