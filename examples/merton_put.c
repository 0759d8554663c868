/* merton_put.c -- the American put of american_put.c under Merton's jump diffusion: on top of
 * dS_i = r S_i dt + v S_i dW_i both assets jump together, S -> S exp(z), at the intensity lambda, with z ~ N(mu, s^2) discretised
 * into the three atoms of the Gauss-Hermite rule (z = mu, mu -+ sqrt(3) s with weights 2/3, 1/6, 1/6).  Exercising pays
 * psi(S) = -max(K - (S_1 + S_2) / 2, 0), discounted at beta = r; the terminal value and the absorbing faces pay psi as well, and so
 * does a jump out of the grid.  The host callbacks with the stopping cost and the two jump callbacks, and the same functions as
 * device source compiled at run time with the horizon, stop and jump kernels (c3sc_hip_model_compile_jd); c3control_fh_solve in
 * stop and jump mode then returns one value function per stage.  Own code; only the API names are the reference's.
 *
 *   cc -std=c99 -I include examples/merton_put.c -L c3sc_amd/host -L c3sc_amd/csrc -lc3sc -lc3sc_hip -lm \
 *      -Wl,-rpath,$PWD/c3sc_amd/host -Wl,-rpath,$PWD/c3sc_amd/csrc -o merton_put
 *   ./merton_put [ngrid=11] [stages=20]
 *
 * The step delta = T / stages must keep every self-loop probability non-negative ((Q + h^2 lambda) delta <= h^2, with Q at
 * most v^2 (S_1^2 + S_2^2) + h r (S_1 + S_2) here); the defaults do (0.64 * 0.025 / 0.0256 + 0.8 * 0.025), and a solve that raises C3SC_STATUS_CFL
 * stops with a message.  Prints the at-the-money price and the exercise boundary along the diagonal at three stages. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "c3sc/c3sc.h"
#include "c3sc_hip.h"

static const double PRM[6] = {0.1, 0.3, 1.0, 0.8, -0.1, 0.25}; /* r, v, K, lambda, mu, s */
#define NMARKS 3
static const double T = 0.5, LB = 0.2, UB = 1.8;

static double psi(const double *x)
{
    const double p = PRM[2] - 0.5 * (x[0] + x[1]);
    return p > 0.0 ? -p : 0.0;
}
static int drift(double t, const double *x, const double *u, double *out, double *jac, void *a)
{
    (void)t; (void)u; (void)a;
    out[0] = PRM[0] * x[0];
    out[1] = PRM[0] * x[1];
    if (jac) { jac[0] = 0.0; jac[1] = 0.0; }
    return 0;
}
static int diffusion(double t, const double *x, const double *u, double *out, double *grad, void *a)
{
    (void)t; (void)u; (void)a;
    out[0] = PRM[1] * x[0]; out[1] = 0.0; out[2] = 0.0; out[3] = PRM[1] * x[1];
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
static double jumprate(const double *x) { (void)x; return PRM[3]; }
static double jumpmark(const double *x, int m, double *y)
{
    const double z = PRM[4] + (m == 0 ? 0.0 : (m == 1 ? -1.7320508075688772 : 1.7320508075688772)) * PRM[5];
    const double f = exp(z);
    y[0] = x[0] * f;
    y[1] = x[1] * f;
    return m == 0 ? 2.0 / 3.0 : 1.0 / 6.0;
}
static int terminal(size_t N, const double *x, double *out, void *arg)
{
    (void)arg;
    for (size_t i = 0; i < N; i++) out[i] = psi(x + 2 * i);
    return 0;
}

/* the same functions for the device (include/c3sc_hip.h states the contract); prm is PRM */
static const char *DEVICE_SOURCE =
    "__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = prm[0] * x[0]; b[1] = prm[0] * x[1]; }\n"
    "__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[1] * x[0]; s[1] = prm[1] * x[1]; }\n"
    "__device__ double stage(const double *prm, const double *x, const double *u) { return 0.0; }\n"
    "__device__ double stopcost(const double *prm, const double *x)\n"
    "{\n"
    "    const double p = prm[2] - 0.5 * (x[0] + x[1]);\n"
    "    return p > 0.0 ? -p : 0.0;\n"
    "}\n"
    "__device__ double boundcost(const double *prm, const double *x) { return stopcost(prm, x); }\n"
    "__device__ double obscost(const double *prm, const double *x) { return stopcost(prm, x); }\n"
    "__device__ double jumprate(const double *prm, const double *x) { return prm[3]; }\n"
    "__device__ double jump(const double *prm, const double *x, int m, double *y)\n"
    "{\n"
    "    const double z = prm[4] + (m == 0 ? 0.0 : (m == 1 ? -1.7320508075688772 : 1.7320508075688772)) * prm[5];\n"
    "    const double f = exp(z);\n"
    "    y[0] = x[0] * f;\n"
    "    y[1] = x[1] * f;\n"
    "    return m == 0 ? 2.0 / 3.0 : 1.0 / 6.0;\n"
    "}\n";

int main(int argc, char **argv)
{
    const size_t n = argc > 1 ? (size_t)atoi(argv[1]) : 11, stages = argc > 2 ? (size_t)atoi(argv[2]) : 20;
    if (n < 5 || n > 64 || stages < 1) { fprintf(stderr, "usage: merton_put [ngrid in 5..64] [stages >= 1]\n"); return 2; }
    const double delta = T / (double)stages;
    size_t dx = 2, du = 1, dw = 2, ngrid[2] = {n, n};
    double lb[2] = {LB, LB}, ub[2] = {UB, UB};

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
    c3control_add_jumps(c3c, NMARKS, jumprate, jumpmark);
    c3control_set_external_boundary(c3c, 0, "absorb");
    c3control_set_external_boundary(c3c, 1, "absorb");

    const int ranks[3] = {4, 8, 12};
    c3sc_hip_model_spec_jd spec;
    memset(&spec, 0, sizeof(spec));
    spec.os.fh.ex.base.source = DEVICE_SOURCE;
    spec.os.fh.ex.base.name = "merton_put";
    spec.os.fh.ex.base.d = 2;
    spec.os.fh.ex.base.du = 1;
    spec.os.fh.ex.base.nranks = 3;
    spec.os.fh.ex.base.ranks = ranks;
    spec.os.fh.horizon = 1;
    spec.os.stop = 1;
    spec.njump = NMARKS;
    int id = 0;
    if (c3sc_hip_model_compile_jd(&spec, &id) != C3SC_OK) {
        fprintf(stderr, "c3sc_hip_model_compile_jd: %s\n", c3sc_hip_model_log());
        return 1;
    }
    c3control_set_device_model(c3c, id, PRM, 6);
    c3control_set_stopping(c3c, 1);
    c3control_set_jumps(c3c, 1);

    struct ValueF *vT = c3control_init_value(c3c, terminal, NULL, aargs, 0);
    struct ValueF **V = c3control_fh_solve(c3c, stages, delta, vT, aargs, opt, 0);
    if (V == NULL) { printf("MERTON_PUT_FAILED\n"); return 1; }

    const double atm[2] = {PRM[2], PRM[2]};
    const double price = -valuef_eval(V[0], atm);
    printf("american put on the mean of two assets with lognormal jumps: r = %g, v = %g, K = %g, lambda = %g, mu = %g, s = %g, T = %g,\n"
           "%zu x %zu nodes, %zu stages\n", PRM[0], PRM[1], PRM[2], PRM[3], PRM[4], PRM[5], T, n, n, stages);
    printf("at-the-money price V_0(K, K) = %.6f\n", price);
    int ok = isfinite(price) && price > 0.0 && price < PRM[2];
    /* the exercise boundary along the diagonal S_1 = S_2 = s: the largest s at which the policy of the stage stops */
    const size_t at[3] = {0, stages / 2, stages - 1};
    for (int q = 0; q < 3; q++) {
        c3control_add_policy_sim(c3c, V[at[q] + 1], opt, NULL); /* the decision at stage s reads V_{s+1} */
        double boundary = NAN;
        for (double s = LB + 0.05; s < PRM[2]; s += 0.005) { /* in the money only: above K both psi and the value are 0 near the deadline */
            const double x[2] = {s, s};
            double u[1];
            int stopped = 0;
            if (c3control_policy_eval_stop(c3c, (double)at[q] * delta, x, u, &stopped) != 0) ok = 0;
            if (stopped) boundary = s;
        }
        printf("stage %zu (time to go %.3f): exercise below s = %.3f\n", at[q], T - (double)at[q] * delta, boundary);
        ok = ok && isfinite(boundary); /* it rises towards K at the deadline */
    }
    printf("%s\n", ok ? "MERTON_PUT_OK" : "MERTON_PUT_FAILED");

    for (size_t s = 0; s <= stages; s++) valuef_destroy(V[s]);
    free(V);
    valuef_destroy(vT);
    c3control_destroy(c3c);
    c3opt_free(opt);
    approx_args_free(aargs);
    return ok ? 0 : 1;
}
