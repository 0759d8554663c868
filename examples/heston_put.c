/* heston_put.c -- an American put under Heston's stochastic volatility, in the coordinates x = (log S, v):
 *     dx = (r - v / 2) dt + sqrt(v) dW_1,     dv = kappa (theta - v) dt + xi sqrt(v) dW_2,     d<W_1, W_2> = rho dt,
 * so the covariance of the two dimensions is a(x) = rho xi v -- the cross-diffusion term a diagonal chain cannot express.
 * Exercising pays psi(x) = -max(K - exp(x), 0), discounted at beta = r; the terminal value and the absorbing faces pay psi as
 * well.  The host callbacks with the stopping cost and the covariance callback, and the same functions as device source compiled
 * at run time with the horizon, stop and corr kernels (c3sc_hip_model_compile_cd); c3control_fh_solve in stop and correlation
 * mode then returns one value function per stage.  Own code; only the API names are the reference's.
 *
 *   cc -std=c99 -I include examples/heston_put.c -L c3sc_amd/host -L c3sc_amd/csrc -lc3sc -lc3sc_hip -lm \
 *      -Wl,-rpath,$PWD/c3sc_amd/host -Wl,-rpath,$PWD/c3sc_amd/csrc -o heston_put
 *   ./heston_put [ngrid=11] [stages=20]
 *
 * Dominance.  The chain's transition probabilities stay non-negative iff, per paired dimension, the axis diffusion outweighs the
 * pair's rate.  In log-price sigma = (sqrt(v), xi sqrt(v)) and v cancels: the condition is one on the grid alone,
 *     |rho| xi <= h_v / h_x <= xi / |rho|.
 * The same number of nodes per dimension on [-0.8, 0.8] x [0.02, 0.22] gives h_v / h_x = 0.125 whatever ngrid is, inside
 * [0.12, 0.75] for xi = 0.3, rho = -0.4; the program prints the ratio, and a solve that raises C3SC_STATUS_DOMINANCE stops with a
 * message.  The step delta = T / stages must keep every self-loop probability non-negative as well (Q delta <= h^2;
 * C3SC_STATUS_CFL otherwise).  Prints the at-the-money price with and without the correlation. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "c3sc/c3sc.h"
#include "c3sc_hip.h"

static const double PRM[6] = {0.05, 1.5, 0.1, 0.3, -0.4, 1.0}; /* r, kappa, theta, xi, rho, K */
static const double T = 0.25, LB[2] = {-0.8, 0.02}, UB[2] = {0.8, 0.22};

static double psi(const double *x)
{
    const double p = PRM[5] - exp(x[0]);
    return p > 0.0 ? -p : 0.0;
}
static int drift(double t, const double *x, const double *u, double *out, double *jac, void *a)
{
    (void)t; (void)u; (void)a;
    out[0] = PRM[0] - 0.5 * x[1];
    out[1] = PRM[1] * (PRM[2] - x[1]);
    if (jac) { jac[0] = 0.0; jac[1] = 0.0; }
    return 0;
}
static int diffusion(double t, const double *x, const double *u, double *out, double *grad, void *a)
{
    (void)t; (void)u; (void)a;
    out[0] = sqrt(x[1]); out[1] = 0.0; out[2] = 0.0; out[3] = PRM[3] * sqrt(x[1]);
    if (grad) memset(grad, 0, 4 * sizeof(double));
    return 0;
}
static int stagecost(double t, const double *x, const double *u, double *out, double *grad)
{
    (void)t; (void)x; (void)u;
    *out = 0.0;
    if (grad) grad[0] = 0.0;
    return 0;
}
static int boundcost(double t, const double *x, double *out) { (void)t; *out = psi(x); return 0; }
static int obscost(const double *x, double *out) { *out = psi(x); return 0; }
static int stopcost(double t, const double *x, double *out) { (void)t; *out = psi(x); return 0; }
static double covar(const double *x, int p) { (void)p; return PRM[4] * PRM[3] * x[1]; }
static int terminal(size_t N, const double *x, double *out, void *arg)
{
    (void)arg;
    for (size_t i = 0; i < N; i++) out[i] = psi(x + 2 * i);
    return 0;
}

/* the same functions for the device (include/c3sc_hip.h states the contract); prm is PRM */
static const char *DEVICE_SOURCE =
    "__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = prm[0] - 0.5 * x[1]; b[1] = prm[1] * (prm[2] - x[1]); }\n"
    "__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = sqrt(x[1]); s[1] = prm[3] * sqrt(x[1]); }\n"
    "__device__ double stage(const double *prm, const double *x, const double *u) { return 0.0; }\n"
    "__device__ double stopcost(const double *prm, const double *x)\n"
    "{\n"
    "    const double p = prm[5] - exp(x[0]);\n"
    "    return p > 0.0 ? -p : 0.0;\n"
    "}\n"
    "__device__ double boundcost(const double *prm, const double *x) { return stopcost(prm, x); }\n"
    "__device__ double obscost(const double *prm, const double *x) { return stopcost(prm, x); }\n"
    "__device__ double covar(const double *prm, const double *x, int p) { return prm[4] * prm[3] * x[1]; }\n";

int main(int argc, char **argv)
{
    const size_t n = argc > 1 ? (size_t)atoi(argv[1]) : 11, stages = argc > 2 ? (size_t)atoi(argv[2]) : 20;
    if (n < 5 || n > 64 || n % 2 == 0 || stages < 1) { fprintf(stderr, "usage: heston_put [odd ngrid in 5..63] [stages >= 1]\n"); return 2; }
    const double delta = T / (double)stages;
    size_t dx = 2, du = 1, dw = 2, ngrid[2] = {n, n};
    double lb[2] = {LB[0], LB[1]}, ub[2] = {UB[0], UB[1]};
    const double hx = (UB[0] - LB[0]) / (double)(n - 1), hv = (UB[1] - LB[1]) / (double)(n - 1), ratio = hv / hx;
    const double rlo = fabs(PRM[4]) * PRM[3], rhi = PRM[3] / fabs(PRM[4]);
    printf("grid ratio h_v / h_x = %.4f, dominance needs [%.4f, %.4f]\n", ratio, rlo, rhi);
    if (!(rlo <= ratio && ratio <= rhi)) { fprintf(stderr, "the grid violates the dominance condition\n"); return 1; }

    double cands[1] = {0.0}; /* nothing to steer: the only decision is when to stop */
    struct c3Opt *opt = c3opt_alloc(BRUTEFORCE, du);
    c3opt_set_brute_force_vals(opt, 1, cands);
    struct ApproxArgs *aargs = approx_args_init();
    approx_args_set_cross_tol(aargs, 1e-10);
    approx_args_set_round_tol(aargs, 1e-12);
    approx_args_set_kickrank(aargs, 0);
    approx_args_set_adapt(aargs, 0);
    approx_args_set_startrank(aargs, n < 12 ? n : 12);
    approx_args_set_maxrank(aargs, n < 12 ? n : 12);

    struct C3Control *c3c = c3control_create(dx, du, dw, lb, ub, ngrid, PRM[0]);
    c3control_add_drift(c3c, drift, NULL);
    c3control_add_diff(c3c, diffusion, NULL);
    c3control_add_stagecost(c3c, stagecost);
    c3control_add_boundcost(c3c, boundcost);
    c3control_add_obscost(c3c, obscost);
    c3control_add_stopcost(c3c, stopcost);
    const size_t pair[2] = {0, 1};
    c3control_add_covariance(c3c, 1, pair, covar);
    c3control_set_external_boundary(c3c, 0, "absorb");
    c3control_set_external_boundary(c3c, 1, "absorb");

    const int ranks[3] = {4, 8, 12};
    c3sc_hip_model_spec_cd spec;
    memset(&spec, 0, sizeof(spec));
    spec.ic.jd.os.fh.ex.base.source = DEVICE_SOURCE;
    spec.ic.jd.os.fh.ex.base.name = "heston_put";
    spec.ic.jd.os.fh.ex.base.d = 2;
    spec.ic.jd.os.fh.ex.base.du = 1;
    spec.ic.jd.os.fh.ex.base.nranks = 3;
    spec.ic.jd.os.fh.ex.base.ranks = ranks;
    spec.ic.jd.os.fh.horizon = 1;
    spec.ic.jd.os.stop = 1;
    spec.ncorr = 1;
    spec.corr_dims[0] = 0;
    spec.corr_dims[1] = 1;
    int id = 0;
    if (c3sc_hip_model_compile_cd(&spec, &id) != C3SC_OK) {
        fprintf(stderr, "c3sc_hip_model_compile_cd: %s\n", c3sc_hip_model_log());
        return 1;
    }
    c3control_set_device_model(c3c, id, PRM, 6);
    c3control_set_stopping(c3c, 1);

    struct ValueF *vT = c3control_init_value(c3c, terminal, NULL, aargs, 0);
    const double atm[2] = {log(PRM[5]), 0.5 * (LB[1] + UB[1])}; /* a node: ngrid is odd */
    double price[2] = {NAN, NAN};
    int ok = 1;
    for (int corr = 1; corr >= 0; corr--) { /* with the cross term, then the same model with rho = 0 (the plain kernels) */
        c3control_set_correlation(c3c, corr);
        struct ValueF **V = c3control_fh_solve(c3c, stages, delta, vT, aargs, opt, 0);
        if (V == NULL) { printf("HESTON_PUT_FAILED\n"); return 1; }
        price[corr] = -valuef_eval(V[0], atm);
        for (size_t s = 0; s <= stages; s++) valuef_destroy(V[s]);
        free(V);
    }
    printf("american put under Heston: r = %g, kappa = %g, theta = %g, xi = %g, rho = %g, K = %g, T = %g, %zu x %zu nodes, %zu stages\n",
           PRM[0], PRM[1], PRM[2], PRM[3], PRM[4], PRM[5], T, n, n, stages);
    printf("at-the-money price V_0(log K, v = %.2f) = %.6f with rho = %g\n", atm[1], price[1], PRM[4]);
    printf("at-the-money price V_0(log K, v = %.2f) = %.6f with rho = 0\n", atm[1], price[0]);
    ok = ok && isfinite(price[0]) && isfinite(price[1]) && price[1] > 0.0 && price[1] < PRM[5] && price[0] > 0.0 && price[0] < PRM[5];
    ok = ok && fabs(price[1] - price[0]) > 1e-7; /* the correlation moves the price */
    printf("%s\n", ok ? "HESTON_PUT_OK" : "HESTON_PUT_FAILED");

    valuef_destroy(vT);
    c3control_destroy(c3c);
    c3opt_free(opt);
    approx_args_free(aargs);
    return ok ? 0 : 1;
}
