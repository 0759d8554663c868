"""Small helpers the GPU tests of the Bellman-backup features share (tests/test_gpu_horizon.py .. test_gpu_corr.py): numpy and
the standard library only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def train(V, maxrank):
    """an exact 2-D train of the nodal matrix V[n0, n1] (SVD, the singular values above 1e-13 of the largest kept; their number
    must not exceed maxrank): (ranks, [core0 (n0, 1, r), core1 (n1, r, 1)]) in upload_value's layout"""
    U, S, Vt = np.linalg.svd(V)
    r = int((S > 1e-13 * S[0]).sum())
    assert r <= maxrank, r
    c0 = (U[:, :r] * S[None, :r]).reshape(V.shape[0], 1, r)
    c1 = np.ascontiguousarray(Vt[:r, :].T).reshape(V.shape[1], r, 1)
    return [1, r, 1], [c0, c1]


def fpw_lds_bytes(w, k, rp, npl, cw):
    """dynamic LDS of a staged fiber-per-wave launch (launch_fpw.hpp: fpw_geometry): the four waves' scratch, the varying core
    with its odd stride, the candidate table of cw doubles per row"""
    ws = 4 * rp + 2 * w.dx * rp + 64 * npl
    per = (rp if k in (0, w.dx - 1) else rp * rp) | 1
    return 8 * (4 * ws + w.ngrid[k] * per + w.ncand * cw)


def child(prog):
    """the Python program `prog` in a fresh process that finds the package and tests/, with the cross trace on stderr"""
    env = dict(os.environ, C3SC_CROSS_TRACE="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    return subprocess.run([sys.executable, "-c", prog], cwd=os.path.dirname(os.path.abspath(__file__)), env=env, capture_output=True,
                          text=True, timeout=900)


def ptrs(ts):
    """a C array of the device pointers of the tensors ts"""
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def interp(G, xg, y):
    """bilinear interpolant of the nodal matrix G on the grid xg x xg at the points y[P, 2] (inside the grid)"""
    h = xg[1] - xg[0]
    i = np.clip(np.floor((y[:, 0] - xg[0]) / h).astype(int), 0, len(xg) - 2)
    j = np.clip(np.floor((y[:, 1] - xg[0]) / h).astype(int), 0, len(xg) - 2)
    a = (y[:, 0] - xg[i]) / h
    b = (y[:, 1] - xg[j]) / h
    return (1 - a) * (1 - b) * G[i, j] + a * (1 - b) * G[i + 1, j] + (1 - a) * b * G[i, j + 1] + a * b * G[i + 1, j + 1]
