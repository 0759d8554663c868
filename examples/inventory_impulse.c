/* inventory_impulse.c -- a two-item stock under impulse control.  x_i is the stock of item i, negative when
 * orders are backlogged.  Demand is Brownian with the mean rate d, production runs at a rate u_i from a candidate list and costs
 * cu u_i^2:  dx_i = (u_i - d) dt + sig dW_i.  Holding costs `hold` per unit and time, a backlog `back`.  Besides steering the
 * production rates the controller may at any time place an order, which arrives at once:
 *     0: q of item 1          1: q of item 2          at the fixed cost K1 each,
 *     2: q of both            3: 2 q of both          at the joint fixed cost K12 < 2 K1,
 * plus cq per unit ordered.  The value function solves the quasi-variational inequality
 *     V(x) = min( min_u backup_u(x),  min_m [ k_m + V(y_m(x)) ] ),
 * discounted at beta; both dimensions absorb, and leaving the grid costs the running cost there for ever.  The host callbacks
 * with c3control_add_impulses, and the same functions as device source compiled at run time with the impulse kernels
 * (c3sc_hip_model_compile_ic); c3control_vi_solve in impulse mode then iterates the operator on the device.  Own code; only the
 * API names are the reference's.
 *
 *   cc -std=c99 -I include examples/inventory_impulse.c -L c3sc_amd/host -L c3sc_amd/csrc -lc3sc -lc3sc_hip -lm \
 *      -Wl,-rpath,$PWD/c3sc_amd/host -Wl,-rpath,$PWD/c3sc_amd/csrc -o inventory_impulse
 *   ./inventory_impulse [ngrid=11] [sweeps=60]
 *
 * Prints the value at the centre (an empty stock) and the boundary of the reorder region along the diagonal x_1 = x_2. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "c3sc/c3sc.h"
#include "c3sc_hip.h"

static const double PRM[8] = {0.4, 0.5, 1.0, 4.0, 0.5, 0.7, 0.5, 0.7}; /* sig, d, hold, back, cu, q, K1, K12 */
#define NORDERS 4
static const double BETA = 0.5, CQ = 0.2, LB = -2.0, UB = 2.0;

static double running(const double *x)
{
    return (x[0] > 0.0 ? PRM[2] * x[0] : -PRM[3] * x[0]) + (x[1] > 0.0 ? PRM[2] * x[1] : -PRM[3] * x[1]);
}
static int drift(double t, const double *x, const double *u, double *out, double *jac, void *a)
{
    (void)t; (void)x; (void)a;
    out[0] = u[0] - PRM[1];
    out[1] = u[1] - PRM[1];
    if (jac) { jac[0] = 1.0; jac[1] = 0.0; jac[2] = 0.0; jac[3] = 1.0; }
    return 0;
}
static int diffusion(double t, const double *x, const double *u, double *out, double *grad, void *a)
{
    (void)t; (void)x; (void)u; (void)a;
    out[0] = PRM[0]; out[1] = 0.0; out[2] = 0.0; out[3] = PRM[0];
    if (grad) memset(grad, 0, 8 * sizeof(double));
    return 0;
}
static int stagecost(double t, const double *x, const double *u, double *out, double *grad)
{
    (void)t;
    *out = running(x) + PRM[4] * (u[0] * u[0] + u[1] * u[1]);
    if (grad) { grad[0] = 2.0 * PRM[4] * u[0]; grad[1] = 2.0 * PRM[4] * u[1]; }
    return 0;
}
static int boundcost(double t, const double *x, double *out) { (void)t; *out = running(x) / BETA; return 0; }
static int obscost(const double *x, double *out) { (void)x; *out = 0.0; return 0; }
static double order(const double *x, int m, double *y)
{
    const double q = PRM[5], n0 = (m == 0 || m == 2) ? 1.0 : (m == 3 ? 2.0 : 0.0), n1 = (m == 1 || m == 2) ? 1.0 : (m == 3 ? 2.0 : 0.0);
    y[0] = x[0] + n0 * q;
    y[1] = x[1] + n1 * q;
    return (m < 2 ? PRM[6] : PRM[7]) + CQ * q * (n0 + n1);
}
static int initial(size_t N, const double *x, double *out, void *arg)
{ /* never order, never produce, pay the running cost of today's stock for ever */
    (void)arg;
    for (size_t i = 0; i < N; i++) out[i] = running(x + 2 * i) / BETA;
    return 0;
}

/* the same functions for the device (include/c3sc_hip.h states the contract); prm is PRM */
static const char *DEVICE_SOURCE =
    "__device__ void drift(const double *prm, const double *x, const double *u, double *b) { b[0] = u[0] - prm[1]; b[1] = u[1] - prm[1]; }\n"
    "__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[0]; s[1] = prm[0]; }\n"
    "__device__ double inv_run(const double *prm, const double *x)\n"
    "{\n"
    "    return (x[0] > 0.0 ? prm[2] * x[0] : -prm[3] * x[0]) + (x[1] > 0.0 ? prm[2] * x[1] : -prm[3] * x[1]);\n"
    "}\n"
    "__device__ double stage(const double *prm, const double *x, const double *u) { return inv_run(prm, x) + prm[4] * (u[0] * u[0] + u[1] * u[1]); }\n"
    "__device__ double boundcost(const double *prm, const double *x) { return inv_run(prm, x) / 0.5; }\n"
    "__device__ double obscost(const double *prm, const double *x) { return 0.0; }\n"
    "__device__ double impulse(const double *prm, const double *x, int m, double *y)\n"
    "{\n"
    "    const double q = prm[5], n0 = (m == 0 || m == 2) ? 1.0 : (m == 3 ? 2.0 : 0.0), n1 = (m == 1 || m == 2) ? 1.0 : (m == 3 ? 2.0 : 0.0);\n"
    "    y[0] = x[0] + n0 * q;\n"
    "    y[1] = x[1] + n1 * q;\n"
    "    return (m < 2 ? prm[6] : prm[7]) + 0.2 * q * (n0 + n1);\n"
    "}\n";

int main(int argc, char **argv)
{
    const size_t n = argc > 1 ? (size_t)atoi(argv[1]) : 11, sweeps = argc > 2 ? (size_t)atoi(argv[2]) : 60;
    if (n < 5 || n > 64 || sweeps < 1) { fprintf(stderr, "usage: inventory_impulse [ngrid in 5..64] [sweeps >= 1]\n"); return 2; }
    size_t dx = 2, du = 2, dw = 2, ngrid[2] = {n, n};
    double lb[2] = {LB, LB}, ub[2] = {UB, UB};

    double cands[18]; /* production rates 0, d, 2 d of either item */
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            cands[2 * (3 * a + b)] = 0.5 * a;
            cands[2 * (3 * a + b) + 1] = 0.5 * b;
        }
    struct c3Opt *opt = c3opt_alloc(BRUTEFORCE, du);
    c3opt_set_brute_force_vals(opt, 9, cands);
    struct ApproxArgs *aargs = approx_args_init();
    approx_args_set_cross_tol(aargs, 1e-12);
    approx_args_set_round_tol(aargs, 1e-15);
    approx_args_set_kickrank(aargs, 0);
    approx_args_set_adapt(aargs, 0);
    approx_args_set_startrank(aargs, n < 12 ? n : 12);
    approx_args_set_maxrank(aargs, n < 12 ? n : 12);

    struct C3Control *c3c = c3control_create(dx, du, dw, lb, ub, ngrid, BETA);
    c3control_add_drift(c3c, drift, NULL);
    c3control_add_diff(c3c, diffusion, NULL);
    c3control_add_stagecost(c3c, stagecost);
    c3control_add_boundcost(c3c, boundcost);
    c3control_add_obscost(c3c, obscost);
    c3control_add_impulses(c3c, NORDERS, order);
    c3control_set_external_boundary(c3c, 0, "absorb");
    c3control_set_external_boundary(c3c, 1, "absorb");

    const int ranks[3] = {4, 8, 12};
    c3sc_hip_model_spec_ic spec;
    memset(&spec, 0, sizeof(spec));
    spec.jd.os.fh.ex.base.source = DEVICE_SOURCE;
    spec.jd.os.fh.ex.base.name = "inventory";
    spec.jd.os.fh.ex.base.d = 2;
    spec.jd.os.fh.ex.base.du = 2;
    spec.jd.os.fh.ex.base.nranks = 3;
    spec.jd.os.fh.ex.base.ranks = ranks;
    spec.jd.os.fh.ex.base.udep_mask = 3u;   /* both drifts read u ... */
    spec.jd.os.fh.ex.base.uconst_mask = 3u; /* ... and nothing else: their rates are constants of the candidate */
    spec.jd.os.fh.ex.base.stage_udep = 1;   /* the production cost reads u */
    spec.nimpulse = NORDERS;
    int id = 0;
    if (c3sc_hip_model_compile_ic(&spec, &id) != C3SC_OK) {
        fprintf(stderr, "c3sc_hip_model_compile_ic: %s\n", c3sc_hip_model_log());
        return 1;
    }
    c3control_set_device_model(c3c, id, PRM, 8);
    c3control_set_impulses(c3c, 1);

    struct ValueF *v0 = c3control_init_value(c3c, initial, NULL, aargs, 0);
    struct ValueF *V = c3control_vi_solve(c3c, sweeps, 0.0, v0, aargs, opt, 0, NULL);
    if (V == NULL) { printf("INVENTORY_IMPULSE_FAILED\n"); return 1; }

    const double centre[2] = {0.0, 0.0};
    const double vc = valuef_eval(V, centre);
    printf("two-item stock with orders: sig = %g, d = %g, hold = %g, back = %g, cu = %g, q = %g, K1 = %g, K12 = %g, beta = %g,\n"
           "%zu x %zu nodes, %zu sweeps\n", PRM[0], PRM[1], PRM[2], PRM[3], PRM[4], PRM[5], PRM[6], PRM[7], BETA, n, n, sweeps);
    printf("value at the centre V(0, 0) = %.6f\n", vc);
    int ok = isfinite(vc) && vc > 0.0;
    /* the reorder region along the diagonal x_1 = x_2 = s: the largest s at which the policy places an order, and which */
    c3control_add_policy_sim(c3c, V, opt, NULL);
    double boundary = NAN;
    int which = -1;
    for (double s = LB + 0.05; s < UB - 0.05; s += 0.01) {
        const double x[2] = {s, s};
        int m = -1;
        if (c3control_policy_eval_impulse(c3c, x, &m) != 0) ok = 0;
        if (m >= 0) { boundary = s; which = m; }
    }
    printf("orders are placed below s = %.2f on the diagonal (the last one there: order %d)\n", boundary, which);
    ok = ok && isfinite(boundary) && boundary < 1.0; /* nobody orders into a full store */
    printf("%s\n", ok ? "INVENTORY_IMPULSE_OK" : "INVENTORY_IMPULSE_FAILED");

    valuef_destroy(V);
    valuef_destroy(v0);
    c3control_destroy(c3c);
    c3opt_free(opt);
    approx_args_free(aargs);
    return ok ? 0 : 1;
}
