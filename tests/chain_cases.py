"""The cases of the Markov-chain tests (tests/test_chain_ref.py on the CPU, tests/test_gpu_chain.py on the device) -- TEST
INFRASTRUCTURE ONLY.  Cores come from sim_kernel_cases' helpers: full rank, unequal bond ranks, positive or signed.

lqg2d     9 x 12, reflecting; classes 4 and 12
dubins3d  7 x 6 x 16, absorbing x absorbing x periodic, one obstacle that reaches the face x = lb (so one grid line is face AND
          obstacle: the face wins); the lowest class (4) and a two-digit one (12)
car7d     5 nodes per dimension (absorbing, absorbing, periodic, four reflecting; the goal box is the obstacle); class 10
Every case runs at its own discount and at beta = 0 where that differs (dubins3d and car7d are undiscounted: they run at 0.1).
"""
import math

import numpy as np

import sim_kernel_cases as skc
from c3sc_amd import workloads as wl

NLANES, NSTEPS, SEED = 300, 24, 20260
STAT_NTRAJ, STAT_STARTS, STAT_NSTEPS, STAT_SEED = 4096, ((4, 6), (1, 10), (7, 2)), 24, 977

# The x and y extents are widened (dubins3d 4 times, car7d 10 times): on 7 x 6 and 5 x 5 nodes with the examples' own spacing a
# walk leaves through a face within a few steps, and half the lanes are to be alive at mid-run (test_chain_ref.py)
_WIDEN = {"dubins3d": 4.0, "car7d": 10.0}
_DUBINS_OBSTACLE = [((-12.0, 3.2, 0.0), (12.0, 4.0, 2.0 * math.pi))]
SIGNED_SCALE = 20.0  # signed cores: (synth_cores - 0.35) * 20, entries in [-1, 1] -- unscaled, a 7-D product is ~1e-9 and every
                     # decision of the car lies within the margin

CASES = [
    skc._case("rollout", "LqgNd<2>", 4, "lqg2d", (9, 12), (1, 3, 1)),
    skc._case("rollout", "LqgNd<2>", 12, "lqg2d", (9, 12), (1, 11, 1)),
    skc._case("rollout", "Dubins3D", 4, "dubins3d", (7, 6, 16), (1, 3, 2, 1)),
    skc._case("rollout", "Dubins3D", 12, "dubins3d", (7, 6, 16), (1, 11, 9, 1)),
    skc._case("rollout", "Car7D", 10, "car7d", (5,) * 7, (1, 3, 9, 7, 8, 5, 9, 1)),
]


def case_id(c):
    return f"{c.name}-{c.rp}"


def discounts(case):
    own = wl.WORKLOADS[case.name]().discount
    return (own, 0.0) if own > 0.0 else (0.1, 0.0)


def workload(case, beta=None):
    w = skc.workload(case)
    if case.name in _WIDEN:
        f = _WIDEN[case.name]
        w.lb = tuple(v * f if m < 2 else v for m, v in enumerate(w.lb))
        w.ub = tuple(v * f if m < 2 else v for m, v in enumerate(w.ub))
    if case.name == "dubins3d":
        w.obstacles = list(_DUBINS_OBSTACLE)
    if beta is not None:
        w.discount = float(beta)
    return w


def cores(case, w, signed):
    cs = skc.cores(case, w, signed)
    return [c * SIGNED_SCALE for c in cs] if signed else cs


def kernel_names(case):
    return "k_chain_walk<%s,%d>" % (case.key, case.rp), "k_chain_transitions<%s,%d>" % (case.key, case.rp)


def start_nodes(w, n=NLANES, seed=SEED):
    """n seeded start nodes: off the absorbing faces except for one lane in sixteen, which starts anywhere (faces and obstacle
    nodes included); the first lanes sit on the seam, the reflecting ends and, where there is one, the face-and-obstacle line"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, w.dx), dtype=np.int32)
    for i in range(n):
        for m in range(w.dx):
            N = w.ngrid[m]
            inner = w.bc[m] == wl.BC_ABSORB and i % 16 != 15
            out[i, m] = rng.integers(1, N - 1) if inner else rng.integers(0, N)
    for m in range(w.dx):  # ends of the non-absorbing dimensions
        if w.bc[m] != wl.BC_ABSORB:
            out[2 * m, m], out[2 * m + 1, m] = 0, w.ngrid[m] - 1
    if w.name == "dubins3d":
        out[20], out[21] = (0, 3, 5), (1, 3, 9)  # face and obstacle; obstacle alone
    return out


def all_nodes(w):
    return np.ascontiguousarray(np.stack(np.meshgrid(*[np.arange(n) for n in w.ngrid], indexing="ij"), -1).reshape(-1, w.dx), dtype=np.int32)


def some_nodes(w, n=2000, seed=SEED + 1):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([rng.integers(0, N, n) for N in w.ngrid], -1), dtype=np.int32)
