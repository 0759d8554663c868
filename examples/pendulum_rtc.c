/* pendulum_rtc.c -- a user problem that has no built-in device model, on every device path of libc3sc.so: the damped pendulum
 * x = (angle, rate), torque u, with the reference's five host callbacks AND the same physics as device source, compiled at run
 * time (c3sc_hip_model_compile) into a model id that c3control_set_device_model takes like a built-in one.  Value iteration,
 * then batches of closed loops on the GPU (c3control_integrate_batch, c3control_simulate_batch).  Own code; only the API names are the reference's.
 *
 *   cc -std=c99 -I include examples/pendulum_rtc.c -L c3sc_amd/host -L c3sc_amd/csrc -lc3sc -lc3sc_hip -lm \
 *      -Wl,-rpath,$PWD/c3sc_amd/host -Wl,-rpath,$PWD/c3sc_amd/csrc -o pendulum_rtc
 * (libc3sc_hip.so for c3sc_hip_model_compile, the one call of the device library a program makes itself)
 *   ./pendulum_rtc [ngrid=41] [sweeps=40] [rtc|table|wrong]
 *
 * rtc:   the run-time compiled model (device-resident cross sweeps, closed loops with c3control_integrate_batch)
 * table: no device model: the host evaluates the callbacks for every node and candidate (the TABLE path)
 * wrong: a device source that does not match the callbacks: bellman_vi's first-fiber check stops the program
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "c3sc/c3sc.h"
#include "c3sc_hip.h"

static const double PRM[4] = {9.81, 0.2, 0.05, 0.5}; /* g / l, damping, diffusion of the angle and of the rate */

static int drift(double t, const double *x, const double *u, double *out, double *jac, void *a)
{
    (void)t; (void)a;
    out[0] = x[1];
    out[1] = -PRM[0] * sin(x[0]) - PRM[1] * x[1] + u[0];
    if (jac) { jac[0] = 0.0; jac[1] = 1.0; }
    return 0;
}
static int diffusion(double t, const double *x, const double *u, double *out, double *grad, void *a)
{
    (void)t; (void)x; (void)u; (void)a;
    out[0] = PRM[2]; out[1] = 0.0; out[2] = 0.0; out[3] = PRM[3];
    if (grad) memset(grad, 0, 4 * sizeof(double));
    return 0;
}
static int stagecost(double t, const double *x, const double *u, double *out, double *grad)
{
    (void)t;
    *out = 1.0 - cos(x[0]) + 0.1 * x[1] * x[1] + 0.01 * u[0] * u[0];
    if (grad) grad[0] = 0.02 * u[0];
    return 0;
}
static int boundcost(double t, const double *x, double *out) { (void)t; (void)x; *out = 50.0; return 0; }
static int obscost(const double *x, double *out) { (void)x; *out = 0.0; return 0; }
static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static int startcost(size_t N, const double *x, double *out, void *arg)
{
    (void)x; (void)arg;
    for (size_t i = 0; i < N; i++) out[i] = 1.0;
    return 0;
}

/* the same physics for the device (include/c3sc_hip.h states the contract); prm is PRM, passed to c3control_set_device_model */
static const char *DEVICE_SOURCE =
    "__device__ void drift(const double *prm, const double *x, const double *u, double *b)\n"
    "{\n"
    "    b[0] = x[1];\n"
    "    b[1] = -prm[0] * sin(x[0]) - prm[1] * x[1] + u[0];\n"
    "}\n"
    "__device__ void sigma(const double *prm, const double *x, const double *u, double *s) { s[0] = prm[2]; s[1] = prm[3]; }\n"
    "__device__ double stage(const double *prm, const double *x, const double *u)\n"
    "{\n"
    "    return 1.0 - cos(x[0]) + 0.1 * x[1] * x[1] + 0.01 * u[0] * u[0];\n"
    "}\n"
    "__device__ double boundcost(const double *prm, const double *x) { return 50.0; }\n"
    "__device__ double obscost(const double *prm, const double *x) { return 0.0; }\n";

int main(int argc, char **argv)
{
    size_t n = argc > 1 ? (size_t)atoi(argv[1]) : 41, sweeps = argc > 2 ? (size_t)atoi(argv[2]) : 40;
    const char *mode = argc > 3 ? argv[3] : "rtc";
    const double tol = 1e-5;
    size_t dx = 2, du = 1, dw = 2, ngrid[2] = {n, n};
    const double pi = 3.14159265358979323846;
    double lb[2] = {-pi, -6.0}, ub[2] = {pi, 6.0};

    double cands[9];
    for (int i = 0; i < 9; i++) cands[i] = -2.0 + 0.5 * i;
    struct c3Opt *opt = c3opt_alloc(BRUTEFORCE, du);
    c3opt_set_brute_force_vals(opt, 9, cands);
    struct ApproxArgs *aargs = approx_args_init();
    approx_args_set_cross_tol(aargs, 1e-8);
    approx_args_set_round_tol(aargs, 1e-8);
    approx_args_set_kickrank(aargs, 2);
    approx_args_set_adapt(aargs, 1);
    approx_args_set_startrank(aargs, 4);
    approx_args_set_maxrank(aargs, 8);

    struct C3Control *c3c = c3control_create(dx, du, dw, lb, ub, ngrid, 0.5);
    c3control_add_drift(c3c, drift, NULL);
    c3control_add_diff(c3c, diffusion, NULL);
    c3control_add_stagecost(c3c, stagecost);
    c3control_add_boundcost(c3c, boundcost);
    c3control_add_obscost(c3c, obscost);
    c3control_set_external_boundary(c3c, 0, "periodic");
    c3control_set_external_boundary(c3c, 1, "absorb");

    const int device = strcmp(mode, "table") != 0;
    if (device) {
        char *src = malloc(strlen(DEVICE_SOURCE) + 1);
        strcpy(src, DEVICE_SOURCE);
        if (strcmp(mode, "wrong") == 0) { /* a stage cost that is not the callback's (the first-fiber check compares values) */
            char *p = strstr(src, "return 1.0 - cos");
            p[7] = '2';
        }
        const int ranks[2] = {4, 8};
        c3sc_hip_model_spec spec = {src, "pendulum", 2, 1, 1u << 1, 0u, 1, 0, 2, ranks};
        int id = 0;
        if (c3sc_hip_model_compile(&spec, &id) != C3SC_OK) {
            fprintf(stderr, "c3sc_hip_model_compile: %s\n", c3sc_hip_model_log());
            return 1;
        }
        free(src);
        printf("device model: run-time id %d\n", id);
        c3control_set_device_model(c3c, id, PRM, 4);
    }

    struct ValueF *cost = c3control_init_value(c3c, startcost, NULL, aargs, 0);
    struct Diag *diag = NULL;
    double diff = 1.0;
    size_t it = 0;
    const double t0 = now_s();
    while (it < sweeps && diff > tol) {
        struct ValueF *next = c3control_vi_solve(c3c, 1, tol, cost, aargs, opt, 0, &diag);
        diff = valuef_norm2diff(next, cost) / valuef_norm(next);
        valuef_destroy(cost);
        cost = next;
        it++;
    }
    const double secs = now_s() - t0;
    printf("value iteration: %zu sweeps, relative change %.3e, |V| = %.9e, %.6f s per sweep\n", it, diff, valuef_norm(cost), secs / (double)it);
    int ok = isfinite(diff) && isfinite(valuef_norm(cost));

    if (device) { /* closed loops on the GPU: RK4 under the implicit policy, the angle wrapped into [-pi, pi) */
        enum { NT = 256, NOUT = 200 };
        double x0[2 * NT], jc[NT], vend[NT];
        long stop[NT];
        int why[NT];
        for (int i = 0; i < NT; i++) { x0[2 * i] = -3.0 + 6.0 * i / (NT - 1); x0[2 * i + 1] = 0.0; }
        c3control_add_policy_sim(c3c, cost, opt, NULL);
        ok = ok && c3control_integrate_batch(c3c, NT, x0, "rk4", 0.005, 0.02, NOUT, NULL, NULL, 1, 0, NULL, NULL, jc, stop, why, vend) == 0;
        size_t running = 0;
        double jmean = 0.0;
        for (int i = 0; i < NT; i++) {
            ok = ok && isfinite(jc[i]) && isfinite(vend[i]);
            running += stop[i] < 0;
            jmean += jc[i] / NT;
        }
        printf("closed loops: %d trajectories x %d steps of rk4, %zu never stopped, mean cost %.6f\n", NT, NOUT, running, jmean);
        long ex[NT];
        ok = ok && c3control_simulate_batch(c3c, NT, x0, 0.02, NOUT, 7, NULL, 1, 0, NULL, NULL, jc, ex, vend) == 0;
        running = 0;
        for (int i = 0; i < NT; i++) {
            ok = ok && isfinite(jc[i]) && isfinite(vend[i]);
            running += ex[i] < 0;
        }
        printf("noisy closed loops: %zu of %d never exited\n", running, NT);
    }
    printf("%s\n", ok ? "PENDULUM_RTC_OK" : "PENDULUM_RTC_FAILED");

    valuef_destroy(cost);
    diag_destroy(&diag);
    c3control_destroy(c3c);
    c3opt_free(opt);
    approx_args_free(aargs);
    return ok ? 0 : 1;
}
