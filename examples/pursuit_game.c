/* pursuit_game.c -- a zero-sum stochastic game on the device: two cars in the pursuer's frame.  The state is the evader's
 * position (x, y) relative to the pursuer and the heading difference theta (periodic); the pursuer turns at rate u (minimiser),
 * the evader at rate w (maximiser):
 *     x' = v_e cos(theta) - v_p + om_p u y,   y' = v_e sin(theta) - om_p u x,   theta' = om_e w - om_p u,   plus small diffusion.
 * Stage cost 1 (time to capture, discounted at 0.2), the capture box |x|, |y| <= 0.25 is an obstacle of cost 0, leaving the box of the grid costs
 * the escape penalty.  The dynamics are handed over twice: as the reference's host callbacks and as device source compiled at
 * run time with the game kernels (c3sc_hip_model_compile_ex, game = 1).  Value iteration of the upper value (min over u of max
 * over w) with c3control_vi_solve, then closed loops under the saddle-point policy with c3control_integrate_batch: the capture
 * times.  Own code; only the API names are the reference's.
 *
 *   cc -std=c99 -I include examples/pursuit_game.c -L c3sc_amd/host -L c3sc_amd/csrc -lc3sc -lc3sc_hip -lm \
 *      -Wl,-rpath,$PWD/c3sc_amd/host -Wl,-rpath,$PWD/c3sc_amd/csrc -o pursuit_game
 *   ./pursuit_game [ngrid=21] [sweeps=3000] [minmax|maxmin]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "c3sc/c3sc.h"
#include "c3sc_hip.h"

static const double PRM[5] = {0.4, 1.0, 1.0, 1.0, 0.05}; /* v_e, v_p, om_p, om_e, diffusion */
static const double ESCAPE = 20.0;

static int drift(double t, const double *x, const double *u, double *out, double *jac, void *a)
{
    (void)t; (void)a; (void)jac;
    out[0] = PRM[0] * cos(x[2]) - PRM[1] + PRM[2] * u[0] * x[1];
    out[1] = PRM[0] * sin(x[2]) - PRM[2] * u[0] * x[0];
    out[2] = PRM[3] * u[1] - PRM[2] * u[0];
    return 0;
}
static int diffusion(double t, const double *x, const double *u, double *out, double *grad, void *a)
{
    (void)t; (void)x; (void)u; (void)a; (void)grad;
    memset(out, 0, 9 * sizeof(double));
    out[0] = out[4] = out[8] = PRM[4];
    return 0;
}
static int stagecost(double t, const double *x, const double *u, double *out, double *grad)
{
    (void)t; (void)x; (void)u;
    *out = 1.0;
    if (grad) grad[0] = grad[1] = 0.0;
    return 0;
}
static int boundcost(double t, const double *x, double *out) { (void)t; (void)x; *out = ESCAPE; return 0; }
static int obscost(const double *x, double *out) { (void)x; *out = 0.0; return 0; }
static int startcost(size_t N, const double *x, double *out, void *arg)
{
    (void)x; (void)arg;
    for (size_t i = 0; i < N; i++) out[i] = 1.0;
    return 0;
}

static const char *DEVICE_SOURCE =
    "__device__ void drift(const double *prm, const double *x, const double *u, double *b)\n"
    "{\n"
    "    b[0] = prm[0] * cos(x[2]) - prm[1] + prm[2] * u[0] * x[1];\n"
    "    b[1] = prm[0] * sin(x[2]) - prm[2] * u[0] * x[0];\n"
    "    b[2] = prm[3] * u[1] - prm[2] * u[0];\n"
    "}\n"
    "__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[4]; s[1] = prm[4]; s[2] = prm[4]; }\n"
    "__device__ double stage(const double *prm, const double *x, const double *u) { return 1.0; }\n"
    "__device__ double boundcost(const double *prm, const double *x) { return 20.0; }\n"
    "__device__ double obscost(const double *prm, const double *x) { return 0.0; }\n";

int main(int argc, char **argv)
{
    const size_t n = argc > 1 ? (size_t)atoi(argv[1]) : 21, sweeps = argc > 2 ? (size_t)atoi(argv[2]) : 3000;
    const int order = (argc > 3 && strcmp(argv[3], "maxmin") == 0) ? C3SC_GAME_MAXMIN : C3SC_GAME_MINMAX;
    const double tol = 1e-3, pi = 3.14159265358979323846;
    size_t dx = 3, du = 2, dw = 3, ngrid[3] = {n, n, n};
    double lb[3] = {-2.0, -2.0, -pi}, ub[3] = {2.0, 2.0, pi};

    /* the players' lists: turn rates in [-1, 1] */
    double U[5], W[5];
    for (int i = 0; i < 5; i++) U[i] = W[i] = -1.0 + 0.5 * i;
    struct c3Opt *opt = c3opt_alloc(BRUTEFORCE, du);
    c3opt_set_brute_force_game(opt, 1, 5, U, 5, W, order);

    struct ApproxArgs *aargs = approx_args_init();
    approx_args_set_cross_tol(aargs, 1e-7);
    approx_args_set_round_tol(aargs, 1e-7);
    approx_args_set_kickrank(aargs, 2);
    approx_args_set_adapt(aargs, 1);
    approx_args_set_startrank(aargs, 4);
    approx_args_set_maxrank(aargs, 12);

    struct C3Control *c3c = c3control_create(dx, du, dw, lb, ub, ngrid, 0.2); /* a small discount */
    c3control_add_drift(c3c, drift, NULL);
    c3control_add_diff(c3c, diffusion, NULL);
    c3control_add_stagecost(c3c, stagecost);
    c3control_add_boundcost(c3c, boundcost);
    c3control_add_obscost(c3c, obscost);
    c3control_set_external_boundary(c3c, 0, "absorb");
    c3control_set_external_boundary(c3c, 1, "absorb");
    c3control_set_external_boundary(c3c, 2, "periodic");
    double cen[3] = {0.0, 0.0, 0.0}, wid[3] = {0.5, 0.5, 2.0 * pi + 1.0}; /* the capture box, whatever the heading */
    c3control_add_obstacle(c3c, cen, wid);

    char *src = malloc(strlen(DEVICE_SOURCE) + 1);
    strcpy(src, DEVICE_SOURCE);
    const int ranks[3] = {4, 8, 12};
    c3sc_hip_model_spec_ex spec = {{src, "pursuit", 3, 2, 0x7u, 0x4u, 0, 0, 3, ranks}, 1};
    int id = 0;
    if (c3sc_hip_model_compile_ex(&spec, &id) != C3SC_OK) {
        fprintf(stderr, "c3sc_hip_model_compile_ex: %s\n", c3sc_hip_model_log());
        return 1;
    }
    free(src);
    printf("device model: run-time id %d with game kernels, order %s\n", id, order == C3SC_GAME_MINMAX ? "minmax" : "maxmin");
    c3control_set_device_model(c3c, id, PRM, 5);

    struct ValueF *cost = c3control_init_value(c3c, startcost, NULL, aargs, 0);
    struct Diag *diag = NULL;
    double diff = 1.0;
    size_t it = 0;
    while (it < sweeps && diff > tol) {
        struct ValueF *next = c3control_vi_solve(c3c, 1, tol, cost, aargs, opt, 0, &diag);
        diff = valuef_norm2diff(next, cost) / valuef_norm(next);
        valuef_destroy(cost);
        cost = next;
        it++;
        if (it % 100 == 0) printf("  sweep %zu: relative change %.3e\n", it, diff);
    }
    printf("value iteration: %zu sweeps, relative change %.3e (tolerance %.1e), |V| = %.9e\n", it, diff, tol, valuef_norm(cost));
    int ok = isfinite(diff) && diff <= tol;

    /* closed loops under the saddle-point policy: the evader starts on a ring around the pursuer, facing away */
    enum { NT = 64, NOUT = 400 };
    const double dt_out = 0.02;
    double x0[3 * NT], jc[NT], vend[NT];
    long stop[NT];
    int why[NT];
    for (int i = 0; i < NT; i++) {
        const double a = 2.0 * pi * i / NT;
        x0[3 * i] = 1.2 * cos(a);
        x0[3 * i + 1] = 1.2 * sin(a);
        x0[3 * i + 2] = a;
    }
    c3control_add_policy_sim(c3c, cost, opt, NULL);
    ok = ok && c3control_integrate_batch(c3c, NT, x0, "rk4", 0.005, dt_out, NOUT, NULL, NULL, 1, 0, NULL, NULL, jc, stop, why, vend) == 0;
    size_t captured = 0, escaped = 0;
    double tmean = 0.0, tmax = 0.0;
    for (int i = 0; i < NT; i++) {
        ok = ok && isfinite(jc[i]);
        if (stop[i] >= 0 && why[i] == 2) {
            const double tc = (double)stop[i] * dt_out;
            captured++;
            tmean += tc;
            tmax = tc > tmax ? tc : tmax;
        } else if (stop[i] >= 0 && why[i] == 1)
            escaped++;
    }
    if (captured) tmean /= (double)captured;
    printf("closed loops: %d trajectories, %zu captured (mean capture time %.4f, longest %.4f), %zu escaped, %zu running\n", NT,
           captured, tmean, tmax, escaped, NT - captured - escaped);
    ok = ok && captured > 0 && isfinite(tmean);
    printf("%s\n", ok ? "PURSUIT_GAME_OK" : "PURSUIT_GAME_FAILED");

    valuef_destroy(cost);
    diag_destroy(&diag);
    c3control_destroy(c3c);
    c3opt_free(opt);
    approx_args_free(aargs);
    return ok ? 0 : 1;
}
