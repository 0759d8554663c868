"""A plain extended-precision reference of the off-grid stencil (offgrid_stencil<D, RP> of kernel_rollout.hpp; on the host
mca_get_neighbor_node_costs of c3sc_bellman.c over valuef_eval of c3sc_cross.c) -- TEST INFRASTRUCTURE ONLY.

For a state x the 2D+1 points are formed (the D pairs of neighbours one grid spacing away, then x itself) and each one is
evaluated on its own as  prod_m [(1 - w_m) G_m[i_m] + w_m G_m[i_m + 1]]  in np.longdouble: no prefix or suffix is shared
between points, and neither the oracle nor the library is called.  What is a *decision* of the host code is taken as the host
takes it, on doubles: the neighbour points (x -+ h, the clamp to a face, the image across a periodic seam), the cell of a
coordinate (closed clamps, the bisection on g[mid] <= x) and the CONSTELM snap of the double weight at 0.5.  What is
*arithmetic* -- the weight that multiplies the cores and the products -- is longdouble.

Besides the values the reference returns Vabs, the same product over |G|: the scale against which a double evaluation of the
product can be judged whatever its association.  A product of D interpolated RP x RP matrices evaluated in double carries a
forward error of at most about (D RP + 3 D) 2^-53 Vabs (RP terms per inner product, D of them chained, three roundings per
interpolated entry): 1.8e-14 Vabs at D = 7, RP = 20.  TOL = 1e-12 leaves more than 50x over that bound; for positive cores
Vabs == V and it is the suite's REL_TOL."""
import numpy as np

from c3sc_amd import workloads as wl

LD = np.longdouble
TOL = 1e-12   # |device - ref| <= TOL * max(Vabs, TINY) per entry
TINY = 1e-300


def cell(g, x, constelm=False):
    """valuef_eval's cell of coordinate x on the grid g (float64): node i and the weight of node i + 1 (longdouble)"""
    N = len(g)
    if x <= g[0]:
        return 0, LD(0.0)
    if x >= g[N - 1]:
        return N - 2, LD(1.0)
    lo, hi = 0, N - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if g[mid] <= x:
            lo = mid
        else:
            hi = mid
    if constelm:  # the nearer node's value holds on its cell: the host snaps its double weight
        return lo, LD(0.0) if (x - g[lo]) / (g[lo + 1] - g[lo]) < 0.5 else LD(1.0)
    return lo, (LD(x) - LD(g[lo])) / (LD(g[lo + 1]) - LD(g[lo]))


class OffgridRef:
    def __init__(self, w, cores):
        self.w, self.d = w, w.dx
        self.g = [np.asarray(g, dtype=np.float64) for g in w.xgrid()]
        self.G = []
        for m in range(w.dx):  # cores[m][j, a + b r_m] -> G[m][j] as an r_m x r_{m+1} matrix
            r0, r1 = w.ranks[m], w.ranks[m + 1]
            self.G.append(np.asarray(cores[m], dtype=np.float64).reshape(w.ngrid[m], r1, r0).transpose(0, 2, 1).astype(LD))
        self.A = [np.abs(G) for G in self.G]
        self.obs = [(np.array(c, dtype=np.float64) - np.array(wd, dtype=np.float64) / 2.0,
                     np.array(c, dtype=np.float64) + np.array(wd, dtype=np.float64) / 2.0) for c, wd in w.obstacles]

    def cells(self, y, constelm=False):
        return [cell(self.g[m], float(y[m]), constelm) for m in range(self.d)]

    def value(self, y, constelm=False):
        """(V, Vabs) at one point, in longdouble"""
        v, a = np.ones(1, dtype=LD), np.ones(1, dtype=LD)
        for m, (i, wt) in enumerate(self.cells(y, constelm)):
            v = v @ ((LD(1.0) - wt) * self.G[m][i] + wt * self.G[m][i + 1])
            a = a @ ((LD(1.0) - wt) * self.A[m][i] + wt * self.A[m][i + 1])
        return v[0], a[0]

    def in_obstacle(self, x):
        return any(bool(np.all((x >= lo) & (x <= hi))) for lo, hi in self.obs)  # closed boxes

    def neighbours(self, x):
        """the 2D points of mca_get_neighbor_node_costs, formed in double as the host forms them"""
        pts = []
        for m in range(self.d):
            g = self.g[m]
            lb, ub, h, xm = g[0], g[-1], g[1] - g[0], x[m]
            per = self.w.bc[m] == wl.BC_PERIODIC
            yl, yr = xm - h, xm + h
            if (xm + h) < ub and (xm - h) > lb:
                pass
            elif (xm - h) <= lb:  # the left face is hit: clamp, or go across the seam
                yl = (ub - (h - (xm - lb)) if xm > lb else (ub - (lb - xm)) - h) if per else lb
            else:
                yr = (lb + (h - (ub - xm)) if xm < ub else (lb + (xm - ub)) + h) if per else ub
            for y in (yl, yr):
                p = np.array(x, dtype=np.float64)
                p[m] = y
                pts.append(p)
        return pts

    def stencil(self, x, constelm=False):
        """(V[2D+1], Vabs[2D+1], flag): entries 2m, 2m+1 the (-, +) neighbours in dimension m, entry 2D the value at x; inside
        an obstacle every entry is the value at x and the flag is -1"""
        x = np.asarray(x, dtype=np.float64)
        n = 2 * self.d + 1
        if self.in_obstacle(x):
            v, a = self.value(x, constelm)
            return np.full(n, v, dtype=LD), np.full(n, a, dtype=LD), -1
        vals = [self.value(p, constelm) for p in self.neighbours(x) + [x]]
        return np.array([v for v, _ in vals], dtype=LD), np.array([a for _, a in vals], dtype=LD), 0


def rel_err(got, V, Vabs):
    """per-entry |got - V| / max(Vabs, TINY), in longdouble"""
    return np.abs(np.asarray(got, dtype=np.float64).astype(LD) - V) / np.maximum(Vabs, LD(TINY))
