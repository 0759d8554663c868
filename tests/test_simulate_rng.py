"""The counter-based noise of the device rollouts (c3sc_amd/csrc/philox.hpp, host twin c3sc_hip_normals): Philox4x32-10
against the published known answers and an independent transcription of the algorithm, the Box-Muller normals against
their moments, and the invariance of a trajectory's noise under splitting the batch.  No GPU involved."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox_py(ctr, key, rounds=10):
    """Philox4x32-R as the SC'11 paper states it: (L0, R0, L1, R1) -> (hi(M1 R1) ^ L0... ) written from the paper's
    S-box description, independently of philox.hpp"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return (c0, c1, c2, c3)


# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, expected)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_python_transcription_matches_known_answers(ctr, key, want):
    assert philox_py(ctr, key) == want


def _philox_c(tmp_path):
    """a tiny host program around philox.hpp's philox4x32_10 (the header the kernel and c3sc_hip_normals use)"""
    src = tmp_path / "kat.hip"
    src.write_text('#include "philox.hpp"\n#include <cstdio>\n#include <cstdlib>\n'
                   'int main(int argc, char **argv) {\n'
                   '  c3sc::Philox4 c = {{(uint32_t)strtoul(argv[1], 0, 16), (uint32_t)strtoul(argv[2], 0, 16),'
                   ' (uint32_t)strtoul(argv[3], 0, 16), (uint32_t)strtoul(argv[4], 0, 16)}};\n'
                   '  c3sc::Philox4 o = c3sc::philox4x32_10(c, (uint32_t)strtoul(argv[5], 0, 16), (uint32_t)strtoul(argv[6], 0, 16));\n'
                   '  printf("%08x %08x %08x %08x\\n", o.v[0], o.v[1], o.v[2], o.v[3]);\n  return 0;\n}\n')
    exe = tmp_path / "kat"
    subprocess.run([HIPCC, "-std=c++20", "-O2", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "c3sc_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, stderr=subprocess.DEVNULL)
    return exe


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_header_philox_matches_known_answers_and_transcription(tmp_path):
    exe = _philox_c(tmp_path)
    rng = np.random.default_rng(11)
    cases = [(c, k) for c, k, _ in KAT] + [(tuple(int(v) for v in rng.integers(0, 2**32, 4)),
                                           tuple(int(v) for v in rng.integers(0, 2**32, 2))) for _ in range(6)]
    for ctr, key in cases:
        out = subprocess.run([str(exe)] + ["%x" % v for v in ctr + key], check=True, capture_output=True, text=True).stdout
        got = tuple(int(v, 16) for v in out.split())
        assert got == philox_py(ctr, key), (ctr, key)
    for ctr, key, want in KAT:
        out = subprocess.run([str(exe)] + ["%x" % v for v in ctr + key], check=True, capture_output=True, text=True).stdout
        assert tuple(int(v, 16) for v in out.split()) == want


def _normals(seed, traj0, ntraj, step0, nsteps, dw):
    from c3sc_amd import engine

    return engine.normals(seed, traj0, ntraj, step0, nsteps, dw)


def _bm_reference(seed, traj, step, j):
    """philox_normal restated with numpy's libm (the header's own log / sincos agree to a few ulp)"""
    o = philox_py((traj & MASK, traj >> 32, step, j >> 1), (seed & MASK, seed >> 32))
    u1 = ((((o[0] << 32) | o[1]) >> 11) + 0.5) * 2.0**-53
    u2 = ((((o[2] << 32) | o[3]) >> 11) + 0.5) * 2.0**-53
    r = np.sqrt(-2.0 * np.log(u1))
    return r * (np.sin(2 * np.pi * u2) if j & 1 else np.cos(2 * np.pi * u2))


def test_normals_follow_the_counter_scheme():
    seed = 0x1234_5678_9ABC_DEF0
    z = _normals(seed, 5, 3, 7, 4, 7)
    for t in range(3):
        for k in range(4):
            for j in range(7):
                assert z[t, k, j] == pytest.approx(_bm_reference(seed, 5 + t, 7 + k, j), rel=1e-13, abs=1e-14)


def test_normals_moments_and_independence():
    n_traj, n_step, dw = 2000, 100, 5  # 10^6 normals
    z = _normals(2024, 0, n_traj, 0, n_step, dw)
    N = z.size
    assert N == 10**6
    flat = z.reshape(-1)
    # mean ~ N(0, 1/N), sample variance ~ N(1, 2/N): within 5 sigma
    assert abs(flat.mean()) < 5.0 / np.sqrt(N)
    assert abs(flat.var() - 1.0) < 5.0 * np.sqrt(2.0 / N)
    assert abs((flat**4).mean() - 3.0) < 5.0 * np.sqrt(96.0 / N)
    # uncorrelated across trajectories, steps and components (each sample correlation ~ N(0, 1/n))
    pairs = [(z[:-1].reshape(-1), z[1:].reshape(-1)), (z[:, :-1].reshape(-1), z[:, 1:].reshape(-1)),
             (z[:, :, 0].reshape(-1), z[:, :, 1].reshape(-1)), (z[:, :, 1].reshape(-1), z[:, :, 2].reshape(-1))]
    for a, b in pairs:
        r = float(np.corrcoef(a, b)[0, 1])
        assert abs(r) < 5.0 / np.sqrt(a.size), r
    # the two normals of one Box-Muller pair are uncorrelated in their squares too
    r2 = float(np.corrcoef(z[:, :, 0].reshape(-1) ** 2, z[:, :, 1].reshape(-1) ** 2)[0, 1])
    assert abs(r2) < 5.0 / np.sqrt(n_traj * n_step)


def test_normals_do_not_depend_on_the_batch_split():
    whole = _normals(99, 1000, 64, 0, 30, 7)
    a = _normals(99, 1000, 20, 0, 30, 7)
    b = _normals(99, 1020, 44, 0, 30, 7)
    assert np.array_equal(whole, np.concatenate([a, b]))
    # ... nor on the split of the time loop
    c = _normals(99, 1000, 64, 0, 12, 7)
    d = _normals(99, 1000, 64, 12, 18, 7)
    assert np.array_equal(whole, np.concatenate([c, d], axis=1))
    # a trajectory's noise is its own: different seeds / indices differ
    assert not np.array_equal(_normals(98, 1000, 1, 0, 30, 7), whole[:1])


def test_normals_argument_errors():
    from c3sc_amd import engine

    L = engine.load_library()
    out = np.zeros(8)
    assert L.c3sc_hip_normals(1, 0, 1, 0, 1, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert L.c3sc_hip_normals(1, 0, 1, 0, 1, 2, None) == 1
