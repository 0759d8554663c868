"""Device sources of run-time compiled models (c3sc_hip_model_compile) shared by the tests and tools/rtc_bench.py: restatements
of built-in models (models.hpp) and a problem that has no built-in functor (the damped pendulum of examples/pendulum_rtc.c)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Dubins car (models.hpp Dubins3D), with the device's cos / sin where the built-in reads host tables
DUBINS3D = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b)
{
    b[0] = cos(x[2]); b[1] = sin(x[2]); b[2] = u[0];
}
__device__ void sigma(const double *prm, const double *x, const double *u, double *s)
{
    s[0] = 1e0; s[1] = 1e0; s[2] = 1e-2;
}
__device__ double stage(const double *prm, const double *x, const double *u) { return 1.0; }
__device__ double boundcost(const double *prm, const double *x) { return 10.0; }
__device__ double obscost(const double *prm, const double *x) { return 0.0; }
"""
DUBINS3D_MASKS = dict(udep_mask=1 << 2, uconst_mask=1 << 2, stage_udep=False)

# models.hpp Chain<4> (prm = {dim, sig, sig_last, stage_mode}), statement for statement
CHAIN4 = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b)
{
    for (int i = 0; i < C3SC_D - 1; i++) b[i] = x[i + 1];
    b[C3SC_D - 1] = u[0];
}
__device__ void sigma(const double *prm, const double *x, const double *u, double *s)
{
    for (int i = 0; i < C3SC_D - 1; i++) s[i] = prm[1];
    s[C3SC_D - 1] = prm[2];
}
__device__ double stage(const double *prm, const double *x, const double *u)
{
    if (prm[3] == 0.0) return 1.0;
    double s = 0.0;
    for (int i = 0; i < C3SC_D; i++) s += x[i] * x[i];
    return s;
}
__device__ double boundcost(const double *prm, const double *x) { return 1000.0; }
__device__ double obscost(const double *prm, const double *x) { return 0.0; }
"""
CHAIN4_MASKS = dict(udep_mask=1 << 3, uconst_mask=1 << 3, stage_udep=False)

# models.hpp LqgNd<2> (prm = {dim, sig_even, sig_odd})
LQG2D = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = x[1]; b[1] = u[0]; }
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[1]; s[1] = prm[2]; }
__device__ double stage(const double *prm, const double *x, const double *u)
{
    double s = 0.0;
    for (int i = 0; i < 2; i++) s += x[i] * x[i];
    s += u[0] * u[0];
    return s;
}
__device__ double boundcost(const double *prm, const double *x) { return 100.0; }
__device__ double obscost(const double *prm, const double *x) { return 0.0; }
"""
LQG2D_MASKS = dict(udep_mask=1 << 1, uconst_mask=1 << 1, stage_udep=True)

# damped pendulum (no built-in functor): x = (angle, rate), torque u; prm = {g/l, damping, sig0, sig1}
PENDULUM = r"""
__device__ void drift(const double *prm, const double *x, const double *u, double *b)
{
    b[0] = x[1];
    b[1] = -prm[0] * sin(x[0]) - prm[1] * x[1] + u[0];
}
__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[2]; s[1] = prm[3]; }
__device__ double stage(const double *prm, const double *x, const double *u)
{
    return 1.0 - cos(x[0]) + 0.1 * x[1] * x[1] + 0.01 * u[0] * u[0];
}
__device__ double boundcost(const double *prm, const double *x) { return 50.0; }
__device__ double obscost(const double *prm, const double *x) { return 0.0; }
"""
PENDULUM_MASKS = dict(udep_mask=1 << 1, uconst_mask=0, stage_udep=True)
PENDULUM_PRM = (9.81, 0.2, 0.05, 0.5)


def pendulum_host(prm, x, u):
    """numpy twin of PENDULUM: (drift[..., 2], sigma[..., 2], stage[...]) for x[..., 2], u[..., 1]"""
    import numpy as np
    g, c, s0, s1 = prm[:4]
    b = np.stack([x[..., 1], -g * np.sin(x[..., 0]) - c * x[..., 1] + u[..., 0]], axis=-1)
    s = np.broadcast_to(np.array([s0, s1]), b.shape).copy()
    st = 1.0 - np.cos(x[..., 0]) + 0.1 * x[..., 1] * x[..., 1] + 0.01 * u[..., 0] * u[..., 0]
    return b, s, st


def build_example(tmp_path):
    """examples/pendulum_rtc.c linked against libc3sc.so and libc3sc_hip.so; returns the executable's path"""
    exe = str(tmp_path / "pendulum_rtc")
    host, csrc = os.path.join(ROOT, "c3sc_amd", "host"), os.path.join(ROOT, "c3sc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-D_POSIX_C_SOURCE=200809L", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pendulum_rtc.c"), "-L", host, "-L", csrc, "-lc3sc", "-lc3sc_hip", "-lm",
                           f"-Wl,-rpath,{host}", f"-Wl,-rpath,{csrc}", "-o", exe])
    return exe
