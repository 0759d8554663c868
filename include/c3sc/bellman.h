/* bellman.h -- Bellman backup API (mirrors src/bellman.h:48-194 for the value-iteration path).
 * bellman_vi keeps the callback ABI C3's cross approximation uses (valuefunc.c:615-616) and runs
 * the fiber on the MI355X through include/c3sc_hip.h. */
#ifndef C3SC_BELLMAN_H
#define C3SC_BELLMAN_H
#include <stddef.h>

#include "boundary.h"
#include "dynamics.h"
#include "nodeutil.h"
#include "util.h"
#include "valuefunc.h"

double bellmanrhs(size_t dx, size_t du, double stage_cost, const double *stage_grad, double discount,
                  const double *prob, const double *prob_grad, double dt, const double *dtgrad, const double *cost,
                  double *grad); /* bellman.c:88-112 */

struct MCAparam;
struct MCAparam *mca_param_create(size_t dx, size_t du);
void mca_add_grid_refs(struct MCAparam *, size_t *ngrid, double **xgrid, double hmin, double *hvec); /* bellman.c:171-188 */
void mca_param_destroy(struct MCAparam *);

struct DPparam;
struct DPparam *dp_param_create(size_t dx, size_t du, size_t dw, double discount);
void dp_param_destroy(struct DPparam *);
void dp_param_add_drift(struct DPparam *, c3sc_dyn_fn, void *);
void dp_param_add_diff(struct DPparam *, c3sc_dyn_fn, void *);
void dp_param_add_boundary(struct DPparam *, struct Boundary *);
void dp_param_add_stagecost(struct DPparam *, int (*)(double, const double *, const double *, double *, double *));
void dp_param_add_boundcost(struct DPparam *, int (*)(double, const double *, double *));
void dp_param_add_obscost(struct DPparam *, int (*)(const double *, double *));
/* new (opt-in): the device functor (include/c3sc_hip.h C3SC_MODEL_*) that restates the callbacks above for the
 * kernels.  bellman_vi cross-checks it against the host callbacks on the first fiber it runs. */
void dp_param_set_device_model(struct DPparam *, int model, const double *params, size_t nparams);

struct ControlParams;
struct ControlParams *control_params_create(size_t dx, size_t dw, struct DPparam *, struct MCAparam *, struct Workspace *,
                                            struct c3Opt *);
void control_params_add_time_and_states(struct ControlParams *, double time, size_t N, const double *x);
int control_params_get_last_res(const struct ControlParams *);
void control_params_destroy(struct ControlParams *);

double bellman_control(size_t du, const double *u, double *grad_u, void *args); /* bellman.c:367-480 */
int bellman_optimal(size_t du, double *u, double *val, void *arg);             /* bellman.c:504-543 (BRUTEFORCE) */

struct VIparam;
struct VIparam *vi_param_create(double convergence);
void vi_param_destroy(struct VIparam *);
void vi_param_add_cp(struct VIparam *, struct ControlParams *);
void vi_param_add_value(struct VIparam *, struct ValueF *);
size_t vi_param_get_nnode_evals(const struct VIparam *);
int bellman_vi(size_t N, const double *x, double *out, void *arg); /* bellman.c:1295-1423 */

/* new: many fibers in one launch (what an own cross driver would call per core step); x is F blocks of
 * N x dx; memo semantics identical to F successive bellman_vi calls */
int bellman_vi_batch(size_t F, size_t N, const double *x, double *out, void *arg);
/* new: fibers by grid indices idx[F][dx] along dim k (entry k ignored); integer-keyed twin of the memo */
#include <stdint.h>
int bellman_vi_batch_idx(size_t F, size_t k, const int32_t *idx, double *out, void *arg);

/* policy evaluation (bellman.c:1430-1491, 1702-1886): vf_policy fixes the control at every node, the Bellman
 * right-hand side is evaluated on vf_iteration */
struct PIparam;
struct PIparam *pi_param_create(double convergence, struct ValueF *policy);
void pi_param_destroy(struct PIparam *);
void pi_param_add_cp(struct PIparam *, struct ControlParams *);
void pi_param_add_value(struct PIparam *, struct ValueF *);
size_t pi_param_get_npol_evals(const struct PIparam *);       /* new: read-only views of the reference's counters */
size_t pi_param_get_niter_node_evals(const struct PIparam *);
int bellman_pi(size_t N, const double *x, double *out, void *arg); /* bellman.c:1702-1886 */
int bellman_pi_batch(size_t F, size_t N, const double *x, double *out, void *arg); /* new: many fibers per launch */
int bellman_pi_batch_idx(size_t F, size_t k, const int32_t *idx, double *out, void *arg); /* new: by grid indices */

struct C3Control;
struct C3Control *c3control_create(size_t dx, size_t du, size_t dw, double *lb, double *ub, size_t *ngrid,
                                   double discount); /* bellman.c:1962-1999 */
void c3control_destroy(struct C3Control *);
size_t *c3control_get_ngrid(struct C3Control *);
double **c3control_get_xgrid(struct C3Control *);
struct Boundary *c3control_get_boundary(struct C3Control *); /* new: read access for callers of the nodeutil functions */
void c3control_set_external_boundary(struct C3Control *, size_t dim, char *type);
void c3control_add_obstacle(struct C3Control *, double *center, double *widths);
void c3control_add_drift(struct C3Control *, c3sc_dyn_fn, void *);
void c3control_add_diff(struct C3Control *, c3sc_dyn_fn, void *);
void c3control_add_stagecost(struct C3Control *, int (*)(double, const double *, const double *, double *, double *));
void c3control_add_boundcost(struct C3Control *, int (*)(double, const double *, double *));
void c3control_add_obscost(struct C3Control *, int (*)(const double *, double *));
void c3control_set_device_model(struct C3Control *, int model, const double *params, size_t nparams); /* new */
/* new: ON by default for a C3Control.  The end points of a reflecting / periodic fiber keep the absorbed flag the fixed
 * dimensions and obstacles give them, so a node's value does not depend on the direction of the fiber that computes it
 * (process_fibers_neighbor resets them, nodeutil.c:570-612: the reference's memo then keeps whichever direction came first).
 * 0, or C3SC_LITERAL_ENDS=1 in the environment, restores the literal rule. */
void c3control_set_consistent_ends(struct C3Control *, int on);
/* new: multi-GPU (one process per GPU, every rank runs the same solver): the fibers of every core step of step_vi /
 * step_pi are split over `world` ranks and all-gathered by `exchange` (valuefunc.h: valuef_interp_idx_sharded) */
void c3control_set_fiber_sharding(struct C3Control *, size_t world, size_t rank, c3sc_exchange_fn exchange, void *xarg);
/* new: the same with the library's own RCCL communicator (c3sc_hip_comm_*): a C main() shards over the GPUs of a node without
 * writing an exchange function.  id128 = the bytes of c3sc_hip_comm_unique_id from rank 0.  Collective.  0 on success. */
int c3control_shard_over_gpus(struct C3Control *, size_t world, size_t rank, const void *id128);
int c3control_comm_unique_id(void *id128); /* rank 0: the 128 bytes every rank passes to c3control_shard_over_gpus */
/* one value-iteration sweep's callback state, as c3control_step_vi builds it (bellman.c:2177-2199); the
 * cross approximation that consumes it (valuef_interp -> C3) is out of scope, so the caller drives the fibers */
struct VIparam *c3control_begin_vi(struct C3Control *, struct ValueF *vf, struct c3Opt *opt);
void c3control_end_vi(struct C3Control *, struct VIparam *, size_t *nevals);
/* the same for policy iteration: c3control_pi_solve's head (bellman.c:2351-2354) and c3control_step_pi's
 * callback state (bellman.c:2236-2249) */
struct PIparam *c3control_begin_pi(struct C3Control *, struct ValueF *policy);
void c3control_begin_pi_step(struct C3Control *, struct PIparam *, struct ValueF *vf, struct c3Opt *opt);
void c3control_end_pi_step(struct C3Control *, struct PIparam *, size_t *niter_evals);

/* ---- implicit policy for closed-loop simulation (bellman.c:2034-2042, 2105-2175) ---- */
void c3control_add_policy_sim(struct C3Control *, struct ValueF *pol, struct c3Opt *opt_sim,
                              void (*transform)(size_t, const double *, double *));
int c3control_policy_eval(struct C3Control *, double t, const double *x, double *u);
int c3control_controller(double t, const double *x, double *u, void *args /* struct C3Control * */);
/* new: Euler(-Maruyama) closed loop in place of the cdyn integrators the examples use; traj (nsteps+1) x dx */
int c3control_simulate(struct C3Control *, const double *x0, double dt, size_t nsteps, const double *noise, double *traj,
                       double *utraj);
/* new: ntraj closed loops at once on the GPU (libc3sc_hip.so: c3sc_hip_simulate, one lane per trajectory).  Host arrays:
 *   x0 ntraj x dx; noise NULL (Philox normals keyed by (seed, trajectory, step, component)) or ntraj x nsteps x dx standard normals;
 *   traj ntraj x (nsteps/save_every + 1) x dx, utraj ntraj x ceil(nsteps/save_every) x du (NULL, or save_every > 0);
 *   cost[ntraj] = sum_{n < exit} e^{-beta n dt} stage(x_n, u_n) dt + e^{-beta exit dt} (boundcost | obscost)(x_exit), beta the
 *   control's discount; exit_step[ntraj] = first n with x_n outside an absorbing face or inside an obstacle (-1: never; the state
 *   is frozen from then on); vend[ntraj] = value of policy_sim at the final state.  Any output may be NULL.
 * The controller is the implicit policy of c3control_add_policy_sim: policy_sim's value function, opt_sim's minimiser (BRUTEFORCE
 * list or the box minimiser) and the DEVICE model (c3control_set_device_model; the host callbacks are not used).  prevpol is neither
 * read nor written: both minimisers ignore the starting point.
 * wrap_periodic = 1 maps the PERIODIC coordinates into [lb, ub) before the controller sees the state -- what the examples'
 * state_transform does on their domains: dubinscar.c:168 (heading in [-pi, pi]) and both skidding cars (scar.c orientation,
 * skidding5d/scar.c orientation, both on [-pi, pi]; the transform keeps x = pi where the wrap gives -pi, the same point of the
 * periodic grid).  A transform_sim set with wrap_periodic = 0 is rejected: it is a host
 * callback the device cannot call.
 * Returns 0, or non-zero with a message on stderr: C3SC_ERR_ARG (no device model, no policy_sim, transform without wrap, dw != dx,
 * null x0, dt <= 0, save_every = 0 with traj / utraj, sizes), C3SC_ERR_UNSUPPORTED (no rollout kernel for this model at this
 * rank), C3SC_ERR_HIP. */
int c3control_simulate_batch(struct C3Control *, size_t ntraj, const double *x0, double dt, size_t nsteps, uint64_t seed,
                             const double *noise, int wrap_periodic, size_t save_every, double *traj, double *utraj, double *cost,
                             long *exit_step, double *vend);
/* new: the approximating Markov chain itself (c3sc_hip.h has the operator, the outcome order and the sampling
 * rule).  c3control_simulate_chain walks ONE trajectory of the chain on the host: from the multi-index node0[dx], at each step
 * the stencil of policy_sim at the node and its 2 dx index-rule neighbours, bellman_optimal over opt_sim's candidate list for the
 * decision, the user's callbacks and transition_assemble for the winner's probabilities P_k and dt; J += D stage dt, T += dt,
 * D *= exp(-beta dt), then uniforms[s] in [0, 1) picks the first outcome k with v < P_0 + .. + P_k (k = 2m lo, 2m + 1 hi of
 * dimension m), else the last with P_k > 0.  An absorbing-face node pays D boundcost, an obstacle node D obscost (exit_step = s;
 * the face wins); a node whose winner has no rate to leave with freezes the walk with exit_step = -(s + 2); -1: still running.
 * traj (nsteps+1) x dx nodes and uidx[nsteps] list positions of the decisions (-1 once frozen) may be NULL, as may cost (J), disc
 * (D), time (T), vend (policy_sim at the final node) and exit_step.  This is the twin c3sc_hip_simulate_chain is tested against.
 * c3control_simulate_chain_batch runs ntraj walks on the GPU (c3sc_hip_simulate_chain_host): policy_sim's value function,
 * opt_sim's candidate list and the DEVICE model, with c3control_simulate_batch's rejections.  Host arrays: node0 ntraj x dx;
 * uniforms NULL (Philox, keyed by (seed, walk, step)) or ntraj x nsteps; traj ntraj x (nsteps/save_every + 1) x dx and uidx
 * ntraj x ceil(nsteps/save_every) (NULL, or save_every > 0); cost, disc, time, vend, exit_step [ntraj], node ntraj x dx (final).
 * Both return C3SC_ERR_ARG with a message on stderr for: no policy_sim, a control box, a node index out of range, and every mode
 * other than the plain backup (stopping, jumps, impulses, correlation, the horizon step, a game); the batch form also for no
 * device model, and C3SC_ERR_UNSUPPORTED where the model has no chain kernel at this rank.
 * Where the device model carries chain kernels (c3sc_hip_model_compile_mc with chain = 1), c3control_simulate_chain_batch honours
 * the control's stopping, jump and horizon switches: it walks the chain of that form (c3sc_hip.h; exit_step then also holds
 * C3SC_CHAIN_STOPPED(s) and the word s + 1 of a jump out, and with jumps on uniforms is ntraj x nsteps x 2 = (v, u1)).  Horizon
 * mode needs the device's value stack, which this API does not upload: the device's refusal (C3SC_ERR_ARG) is passed on.  The
 * one-trajectory host twin c3control_simulate_chain keeps the plain form and rejects every mode as before. */
int c3control_simulate_chain(struct C3Control *, const int32_t *node0, size_t nsteps, const double *uniforms, int32_t *traj,
                             int32_t *uidx, double *cost, double *disc, double *time, double *vend, long *exit_step);
int c3control_simulate_chain_batch(struct C3Control *, size_t ntraj, const int32_t *node0, size_t nsteps, uint64_t seed,
                                   const double *uniforms, size_t save_every, int32_t *traj, int32_t *uidx, double *cost,
                                   double *disc, double *time, double *vend, long *exit_step, int32_t *node);
/* new: the examples' closed-loop tail without cdyn (integrator_create_controlled + trajectory_step + their goal test, e.g.
 * dubinscar.c:379-412, perch.c:447-480) for ONE trajectory on the host, over the user's callbacks and c3control_controller
 * (transform_sim as given): nout outer steps of dt_out, each dt_out / dt_int substeps (an integer to 1e-9 relative; dt_int = 0:
 * one substep) of method "forward-euler" or "rk4" (cdyn's names; RK4 calls the controller at each of its four stages).  The
 * discounted cost c' = e^{-beta t} stage(y, u(y)) is integrated as one more ODE component.  Stops are tested at x_0 .. x_nout,
 * the first that holds wins: 1 outside an absorbing face / 2 inside an obstacle (both pay e^{-beta t} boundcost | obscost),
 * 3 strictly inside goal = (lo[dx], hi[dx]), 4 outside keep = (lo[dx], hi[dx]) (either may be NULL; +-inf allowed).
 * traj (nout+1) x dx and utraj nout x du (the control of the first stage of each outer step) may be NULL; after a stop the
 * state is frozen and the controls are 0.  stop_step = -1 / stop_reason = 0: never stopped.  Returns 0, C3SC_ERR_ARG (with a
 * message on stderr: method name, dt_out, a non-integer dt_out / dt_int, lo > hi in a box, no policy_sim or host callbacks),
 * or a callback's non-zero return.  This is the reference c3sc_hip_integrate is tested against. */
int c3control_integrate(struct C3Control *, const char *method, double dt_int, double dt_out, size_t nout, const double *x0,
                        const double *goal, const double *keep, double *traj, double *utraj, double *cost, long *stop_step,
                        int *stop_reason);
/* new: ntraj such closed loops at once on the GPU (c3sc_hip_integrate_host): policy_sim's value function, opt_sim's minimiser
 * (BRUTEFORCE list or the box minimiser) and the DEVICE model, as c3control_simulate_batch, with its rejections (no device
 * model, no policy_sim, a transform_sim without wrap_periodic, sizes) and the checks of c3control_integrate.  Host arrays:
 * x0 ntraj x dx; traj ntraj x (nout/save_every + 1) x dx and utraj ntraj x ceil(nout/save_every) x du (NULL, or save_every
 * > 0); cost, stop_step, stop_reason, vend (value of policy_sim at the final state) [ntraj].  Any output may be NULL. */
int c3control_integrate_batch(struct C3Control *, size_t ntraj, const double *x0, const char *method, double dt_int, double dt_out,
                              size_t nout, const double *goal, const double *keep, int wrap_periodic, size_t save_every, double *traj,
                              double *utraj, double *cost, long *stop_step, int *stop_reason, double *vend);

/* ---- solver loops over the own cross driver (valuefunc.h: valuef_interp) ---- */
#include <stdio.h>
struct ApproxArgs;
struct Diag; /* bellman.c:2409-2514: per-iteration log */
void diag_destroy(struct Diag **head);
struct Diag *diag_create(size_t iter, int type, double norm, double abs_diff, size_t dim, size_t *ranks, double frac);
void diag_append(struct Diag **diag, size_t iter, int type, double norm, double abs_diff, size_t dim, size_t *ranks,
                 double frac);
void diag_print(struct Diag *head, FILE *fp);
int diag_save(struct Diag *head, char *filename);
size_t diag_count(const struct Diag *head);     /* new: read-only helpers for callers without the struct layout */
double diag_last_diff(const struct Diag *head);
struct ValueF *c3control_init_value(struct C3Control *, int (*f)(size_t, const double *, double *, void *), void *args,
                                    struct ApproxArgs *aargs, int verbose);                 /* bellman.c:2264-2280 */
struct ValueF *c3control_step_vi(struct C3Control *, struct ValueF *vf, struct ApproxArgs *, struct c3Opt *, int verbose,
                                 size_t *nevals);                                           /* bellman.c:2177-2212 */
struct ValueF *c3control_step_pi(struct C3Control *, struct ValueF *vf, struct PIparam *, struct ApproxArgs *,
                                 struct c3Opt *, int verbose, size_t *niter_evals);         /* bellman.c:2214-2262 */
/* new: finite-horizon problems.  c3control_set_horizon_step(c, delta) switches the Bellman operator to Kushner's
 * explicit scheme with the fixed step delta (0 switches back): V_n(x) = min_u [ g delta + e^{-beta delta} (V_self + (delta / h^2)
 * (PV - Q V_self)) ] over the stencil of V_{n+1}.  It holds for the host scan (bellman_optimal, c3control_policy_eval /
 * c3control_controller), the first-fiber check and the device context (which needs a model compiled with
 * c3sc_hip_model_compile_fh, horizon = 1, and a candidate list).  Policy iteration stops with a message in horizon mode.
 * c3control_fh_solve returns V_0 .. V_nstages (nstages + 1 value functions, the caller frees each and the array): V_nstages is a
 * copy of terminal, V_n = c3control_step_vi(V_{n+1}) in horizon mode.  It leaves horizon mode on with delta.  A stage that raises
 * C3SC_STATUS_CFL (Q delta > h^2: a negative self-loop) stops the solve: a message, and NULL. */
void c3control_set_horizon_step(struct C3Control *, double delta);
double c3control_get_horizon_step(const struct C3Control *);
struct ValueF **c3control_fh_solve(struct C3Control *, size_t nstages, double delta, struct ValueF *terminal, struct ApproxArgs *,
                                   struct c3Opt *, int verbose);
/* new: optimal stopping.  c3control_add_stopcost gives the stopping cost psi(t, x); c3control_set_stopping(c, 1)
 * adds the stop action to the Bellman operator, V = min(psi, min_u backup): scanned last, it wins where psi is strictly smaller
 * than the minimiser's value.  It holds for the host scan (bellman_optimal), the first-fiber check and the device context (which
 * needs a model compiled with c3sc_hip_model_compile_os, stop = 1, whose stopcost is the device form of psi, and a candidate
 * list).  c3control_step_vi, c3control_vi_solve and, with the horizon step, c3control_fh_solve (American options) work in stop
 * mode; policy iteration stops with a message.  c3control_policy_eval_stop is c3control_policy_eval with the decision: *stopped
 * = 1 where the policy stops, and u is 0 there (as it is from c3control_policy_eval and c3control_controller).
 * c3control_simulate_batch returns the exit step encoded as c3sc_hip_simulate does: k >= 0 an exit at step k, -1 never, -(k + 2)
 * a voluntary stop at step k.  c3control_simulate and c3control_integrate(_batch) return an error in stop mode.
 * One difference from the device: at a node whose candidates are all stationary (Q < 1e-14) the device returns psi with the stop
 * index, while the host scan stops at the first stationary candidate as it does without stopping (bellman_control asserts, as
 * bellman.c:452 does): a first-fiber check over such a node ends the program instead of agreeing. */
void c3control_add_stopcost(struct C3Control *, int (*)(double t, const double *x, double *out));
void c3control_set_stopping(struct C3Control *, int on);
int c3control_get_stopping(const struct C3Control *);
int c3control_policy_eval_stop(struct C3Control *, double t, const double *x, double *u, int *stopped);
/* new: jump diffusions.  c3control_add_jumps registers the host forms of the device model's jumprate and jump
 * for M marks (1 <= M <= C3SC_JUMP_MAX): rate(x) = lambda(x) >= 0; mark(x, m, y) writes the post-jump state y = x + q_m(x) and
 * returns the weight pi_m(x) >= 0, the weights summing to 1 (the host twin stops with a message when |sum - 1| > 1e-12).
 * c3control_set_jumps(c, 1) adds the jump term to the Bellman operator, Q += h^2 lambda, PV += h^2 lambda sum_m pi_m Vjump(y_m):
 * in the host scan (bellman_optimal, which reads the jump targets with valuef_eval, the exit costs beyond absorbing faces and
 * in obstacles), the first-fiber check and the device context (which needs a model compiled with c3sc_hip_model_compile_jd,
 * njump = M, and a candidate list).  c3control_step_vi, c3control_vi_solve, with the horizon step c3control_fh_solve, and
 * c3control_simulate_batch work in jump mode, and it combines with c3control_set_stopping; policy iteration launches through the
 * same context (the forced path shares the jump term).  c3control_simulate
 * and c3control_integrate(_batch) return an error in jump mode. */
void c3control_add_jumps(struct C3Control *, int M, double (*rate)(const double *x), double (*mark)(const double *x, int m, double *y));
void c3control_set_jumps(struct C3Control *, int on);
int c3control_get_jumps(const struct C3Control *);
/* c3control_policy_eval_stop with the backup's value at x as well (the host twin's number: what the first-fiber check compares
 * with the device); stopped and value may be NULL */
int c3control_policy_eval_value(struct C3Control *, double t, const double *x, double *u, int *stopped, double *value);
/* new: impulse control.  c3control_add_impulses registers the host form of the device model's impulse for M
 * interventions (1 <= M <= C3SC_IMPULSE_MAX): fn(x, m, y) writes the post-intervention state y = y_m(x) and returns the cost
 * k_m(x); a return value that is not finite means "not admissible at x".  c3control_set_impulses(c, 1) makes the Bellman operator
 * the quasi-variational inequality V = min(min_u backup_u, min_m [k_m + Vt(y_m)]): in the host scan (bellman_optimal, after the
 * minimiser and the stop comparison's place; the targets are read as the jump targets are, with valuef_eval and the exit costs
 * beyond absorbing faces and in obstacles; m ascending, the first strict '<'), the first-fiber check and the device context
 * (which needs a model compiled with c3sc_hip_model_compile_ic, nimpulse = M, and a candidate list).  c3control_step_vi,
 * c3control_vi_solve and c3control_simulate_batch work in impulse mode (a simulated intervention occupies one step slot:
 * c3sc_hip.h), and it combines with c3control_set_jumps.  c3control_pi_solve and c3control_fh_solve stop with a message;
 * c3control_simulate and c3control_integrate(_batch) return an error; the horizon step and the stopping switch are refused
 * when the device context is set up.  c3control_policy_eval_value returns the value; c3control_policy_eval_impulse reports the
 * decision at x: *m = the intervention taken, -1 where the policy steers with a control (the control is 0 where it intervenes). */
void c3control_add_impulses(struct C3Control *, int M, double (*fn)(const double *x, int m, double *y));
void c3control_set_impulses(struct C3Control *, int on);
int c3control_get_impulses(const struct C3Control *);
int c3control_policy_eval_impulse(struct C3Control *, const double *x, int *m);
/* new: correlated noise.  c3control_add_covariance registers P pairs of dimensions, dims = {i_0, j_0, i_1, j_1,
 * ...} with i_p < j_p < dx, no pair twice, 1 <= P <= C3SC_CORR_MAX, and the host form of the device model's covar:
 * covar(x, p) = (sigma sigma^T)_{i_p j_p}(x), which reads no control; the diffusion of a paired dimension must not read the
 * control either.  c3control_set_correlation(c, 1) adds the cross-diffusion terms of Kushner and Dupuis 5.3 to the Bellman
 * operator: per pair the rate r_p = (h^2 / (h_i h_j)) |a_p| / 2 to two diagonal neighbours and off each of the four axis rates,
 * i.e. Q += sum (-2 r_p) and PV += sum r_p [(V_d1 + V_d2) - (axis values of i and j)] -- in the host scan (bellman_optimal, which
 * reads the diagonal targets x +- h_i e_i +- h_j e_j with valuef_eval, each coordinate clamped to an absorbing or reflecting
 * face and wrapped across a periodic one as mca_get_neighbor_node_costs does, so c3control_policy_eval_value works off the
 * grid, where it also writes a message to stderr if the state violates the dominance condition below; at a grid node off the
 * absorbing faces these targets are the nodes the device reads, ON an absorbing face the device reads the node itself on both
 * sides), the first-fiber check and the device context (which needs a model compiled with c3sc_hip_model_compile_cd and the same
 * pairs, and a candidate list).  c3control_step_vi, c3control_vi_solve, with the horizon step c3control_fh_solve, and
 * c3control_pi_solve work in correlation mode, and it combines with c3control_set_stopping and c3control_set_jumps, not with
 * c3control_set_impulses or a game.  A node whose pairs take more off an axis rate than its diffusion supplies raises
 * C3SC_STATUS_DOMINANCE on the device; the solver loops then stop with a message and return NULL, as c3control_fh_solve does on
 * C3SC_STATUS_CFL.  c3control_simulate, c3control_simulate_batch and c3control_integrate(_batch) return an error in correlation
 * mode: a correlated rollout needs correlated increments. */
void c3control_add_covariance(struct C3Control *, size_t P, const size_t *dims, double (*covar)(const double *x, int p));
void c3control_set_correlation(struct C3Control *, int on);
int c3control_get_correlation(const struct C3Control *);
struct ValueF *c3control_vi_solve(struct C3Control *, size_t maxiter, double abs_conv_tol, struct ValueF *vo,
                                  struct ApproxArgs *, struct c3Opt *, int verbose, struct Diag **diag); /* :2282-2340 */
struct ValueF *c3control_pi_solve(struct C3Control *, size_t maxiter, double abs_conv_tol, struct ValueF *policy,
                                  struct ApproxArgs *, struct c3Opt *, int verbose, struct Diag **diag); /* :2343-2407 */
#endif
