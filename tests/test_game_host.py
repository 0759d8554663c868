"""Zero-sum games on the host (libc3sc.so: c3opt_set_brute_force_game), no GPU involved.
The game c3Opt's scan returns the saddle pair of a brute-force numpy min-max (game_lib.minmax) on the candidate values of the
2-D LQ game, in both orders, with beta > 0 and beta = 0; the lower value is at most the upper value, exactly; with nw = 1 it is
the plain list scan; a skipped (NaN: stationary) candidate takes no part; policy iteration refuses a game c3Opt."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from c3sc_amd import engine as E
from game_lib import LQGAME_PRM, candidate_values, lqgame_host, minmax, product

HOST = E.LIB_PATH.replace(os.path.join("csrc", "libc3sc_hip.so"), os.path.join("host", "libc3sc.so"))
OBJ = C.CFUNCTYPE(C.c_double, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
BRUTEFORCE = 3
dpp = C.POINTER(C.c_double)


def _lib():
    L = C.CDLL(HOST)
    L.c3opt_alloc.restype = C.c_void_p
    L.c3opt_alloc.argtypes = [C.c_int, C.c_size_t]
    L.c3opt_free.argtypes = [C.c_void_p]
    L.c3opt_set_brute_force_game.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, dpp, C.c_size_t, dpp, C.c_int]
    L.c3opt_set_brute_force_vals.argtypes = [C.c_void_p, C.c_size_t, dpp]
    L.c3opt_add_objective.argtypes = [C.c_void_p, OBJ, C.c_void_p]
    L.c3opt_minimize.argtypes = [C.c_void_p, dpp, dpp]
    L.c3opt_is_bruteforce.argtypes = [C.c_void_p]
    L.c3opt_get_game.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    return L


def _scan(L, opt, table):
    """c3opt_minimize with the objective reading table[(u, w)]: returns (u vector, value)"""
    f = OBJ(lambda d, u, g, a: table[tuple(u[i] for i in range(d))])
    L.c3opt_add_objective(opt, f, None)
    x, v = np.zeros(2), C.c_double(0.0)
    assert L.c3opt_minimize(opt, x.ctypes.data_as(dpp), C.byref(v)) == 0
    return x, v.value


def _game_opt(L, U, W, order):
    opt = L.c3opt_alloc(BRUTEFORCE, 2)
    u, w = np.ascontiguousarray(U, dtype=float), np.ascontiguousarray(W, dtype=float)
    L.c3opt_set_brute_force_game(opt, 1, len(u), u.ctypes.data_as(dpp), len(w), w.ctypes.data_as(dpp), order)
    return opt


@pytest.mark.parametrize("beta", [0.1, 0.0])
def test_host_scan_is_the_numpy_minmax_on_the_lq_game(beta):
    L = _lib()
    U, W = np.linspace(-1, 1, 9).reshape(-1, 1), np.linspace(-0.5, 0.5, 5).reshape(-1, 1)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.5, 1.5, (40, 2))
    V = rng.uniform(0.2, 2.0, (40, 5))
    h2, t = 0.04, [0.2, 1.0, 0.2, 1.0]
    vals, _ = candidate_values(lqgame_host, LQGAME_PRM, x, V, U, W, h2, t, beta)
    C2 = product(U, W)
    for p in range(len(x)):
        table = {tuple(c): vals[p].reshape(-1)[i] for i, c in enumerate(C2)}
        got = {}
        for order, name in ((0, "minmax"), (1, "maxmin")):
            opt = _game_opt(L, U, W, order)
            assert L.c3opt_is_bruteforce(opt) == 1 and L.c3opt_get_game(opt, None, None, None, None, None) == order
            u, v = _scan(L, opt, table)
            r, ri, _ = minmax(vals[p:p + 1], name)
            assert v == r[0]
            np.testing.assert_array_equal(u, C2[ri[0]])
            got[name] = v
            L.c3opt_free(opt)
        assert got["maxmin"] <= got["minmax"]


def test_nw_1_is_the_plain_scan_and_nan_is_skipped():
    L = _lib()
    U, W = np.linspace(-1, 1, 7).reshape(-1, 1), np.array([[0.3]])
    vals = np.array([3.0, 1.0, np.nan, 1.0, 0.5, 0.5, 2.0])
    C2 = product(U, W)
    table = {tuple(c): vals[i] for i, c in enumerate(C2)}
    for order in (0, 1):
        u, v = _scan(L, _game_opt(L, U, W, order), table)
        assert v == 0.5 and np.array_equal(u, C2[4])  # first strict minimum
    plain = L.c3opt_alloc(BRUTEFORCE, 2)
    L.c3opt_set_brute_force_vals(plain, len(C2), np.ascontiguousarray(C2).ctypes.data_as(dpp))
    assert L.c3opt_get_game(plain, None, None, None, None, None) == -1
    u, v = _scan(L, plain, table)
    assert v == 0.5 and np.array_equal(u, C2[4])
    # every member of a group skipped: the group takes no part; nothing left: value 0, u = 0
    U2, W2 = np.array([[-1.0], [1.0]]), np.array([[0.0], [1.0]])
    C3 = product(U2, W2)
    t2 = {tuple(C3[0]): np.nan, tuple(C3[1]): np.nan, tuple(C3[2]): 5.0, tuple(C3[3]): 4.0}
    u, v = _scan(L, _game_opt(L, U2, W2, 0), t2)
    assert v == 5.0 and np.array_equal(u, C3[2])
    u, v = _scan(L, _game_opt(L, U2, W2, 0), {k: np.nan for k in t2})
    assert v == 0.0 and np.array_equal(u, [0.0, 0.0])


def test_policy_iteration_refuses_a_game_in_a_child_process():
    prog = textwrap.dedent(f"""
        import ctypes as C, numpy as np
        L = C.CDLL({HOST!r})
        L.c3opt_alloc.restype = C.c_void_p
        L.c3opt_alloc.argtypes = [C.c_int, C.c_size_t]
        dpp = C.POINTER(C.c_double)
        L.c3opt_set_brute_force_game.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, dpp, C.c_size_t, dpp, C.c_int]
        L.c3control_pi_solve.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        opt = L.c3opt_alloc({BRUTEFORCE}, 2)
        u = np.array([-1.0, 1.0]); w = np.array([0.0])
        L.c3opt_set_brute_force_game(opt, 1, 2, u.ctypes.data_as(dpp), 1, w.ctypes.data_as(dpp), 0)
        L.c3control_pi_solve(None, 3, 1e-6, None, None, opt, 0, None)
        print("NOT REFUSED")
    """)
    r = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "NOT REFUSED" not in r.stdout
    assert "policy iteration is not offered for games" in r.stderr


def test_game_lib_with_nw_1_is_the_oracle_backup(oracle):
    """anchor of the tests' reference: game_lib's dense restatement, run with nw = 1 (a dummy maximiser the physics ignore), equals
    the oracle's Bellman backup (bellman_optimal over the brute-force list) on every node of a small lqg2d grid"""
    from c3sc_amd import workloads as wl
    from backup_ref import mca_constants

    w = wl.c1_lqg2d().scaled(ngrid=(13, 11), rank=4)
    cores = wl.synth_cores(w)
    P = oracle.Problem(w, cores)
    r = w.ranks[1]
    G0 = cores[0].reshape(w.ngrid[0], r)
    G1 = cores[1].reshape(w.ngrid[1], r)
    V = G0 @ G1.T  # the train at every node (ranks (1, r, 1))

    def host(prm, x, u):
        b = np.stack([x[..., 1], u[..., 0]], axis=-1)
        s = np.broadcast_to(np.array([prm[1], prm[2]]), b.shape).copy()
        return b, s, x[..., 0] ** 2 + x[..., 1] ** 2 + u[..., 0] ** 2

    n0, n1 = V.shape
    i0, i1 = np.meshgrid(np.arange(n0), np.arange(n1), indexing="ij")
    S = np.stack([V[np.maximum(i0 - 1, 0), i1], V[np.minimum(i0 + 1, n0 - 1), i1], V[i0, np.maximum(i1 - 1, 0)],
                  V[i0, np.minimum(i1 + 1, n1 - 1)], V], axis=-1).reshape(-1, 5)  # both dimensions reflecting
    xg = w.xgrid()
    x = np.stack([xg[0][i0], xg[1][i1]], axis=-1).reshape(-1, 2)
    h2, t = mca_constants(w)
    assert np.isclose(h2, P.h2(), rtol=0, atol=0) and np.array_equal(t, P.tvec())
    vals, _ = candidate_values(host, w.params, x, S, w.cands, [[0.0]], h2, t, w.discount)
    ref, ui, mg = minmax(vals, "minmax")
    ref, ui, mg = ref.reshape(n0, n1), ui.reshape(n0, n1), mg.reshape(n0, n1)
    seen = 0
    for k in range(2):
        other = 1 - k
        idx = np.zeros((w.ngrid[other], 2), dtype=np.int32)
        idx[:, other] = np.arange(w.ngrid[other])
        out, oui, ab = P.bellman_fibers(k, idx)
        assert not ab.any()
        r_out = ref if k == 1 else ref.T  # fibers along k: [fixed index of the other dim, node along k]
        r_ui, r_mg = (ui, mg) if k == 1 else (ui.T, mg.T)
        assert np.all(np.abs(out - r_out) <= 1e-12 * np.maximum(1.0, np.abs(r_out))), np.abs(out - r_out).max()
        sure = r_mg > 1e-9
        np.testing.assert_array_equal(oui[sure], r_ui[sure])  # nw = 1: the pair index is the candidate index
        seen += out.size
    assert seen == 2 * n0 * n1
