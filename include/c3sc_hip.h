/* c3sc_hip.h -- C-ABI of libc3sc_hip.so: the MI355X (gfx950) Bellman-backup engine.
 *
 * Plain C: opaque handle, plain pointers and sizes, int error codes.  No C++/torch types.
 * This is the boundary a c3sc maintainer binds from the C host code (INTEGRATION.md shows the
 * stub).  Every entry point names the reference interface it replaces; citations are
 * relative to the reference tree (goroda/c3sc).
 *
 * Data model
 *   grid      d per-dimension node arrays xgrid[m][0..N_m)     (c3control_create, bellman.c:1962-1999)
 *   boundary  EBTYPE per dim + <=10 box obstacles              (boundary.c:374-397, 470-481)
 *   mca       h2 = hmin^2, t[2m] = h2/h_m, t[2m+1] = h2/h_m^2  (mca_add_grid_refs, bellman.c:171-188)
 *   value     nodal FT cores, cores[m][j*r_m*r_{m+1} + a + b*r_m] (valuef_precompute_cores, valuefunc.c:165-189)
 *   controls  brute-force candidate list, U x du row-major      (c3opt_set_brute_force_vals, e.g. dubinscar.c:290-293)
 *   model     device functor id + params replacing the host drift/diff/stagecost/boundcost/obscost
 *             callbacks (dynamics.c:127-139,224-239; bellman.c:215-217), which a kernel cannot call.
 *   fibers    F grid fibers along dim k: int32 idx[F*d] fixed indices (entry k ignored)  -- the
 *             index form of the x[N x d] block C3's cross approximation hands to bellman_vi
 *             (bellman.c:1295; convert_fiber_to_ind nodeutil.c:437-470 does that mapping on the host).
 *
 * Pointers named d_* are DEVICE pointers (hipMalloc / torch CUDA tensors); h_* / unprefixed
 * configuration pointers are HOST pointers that are copied during the call.
 * `stream` is a hipStream_t passed as void* (NULL = default stream).
 */
#ifndef C3SC_HIP_H
#define C3SC_HIP_H

#ifndef __HIPCC_RTC__ /* run-time compiled device code (hipRTC) has no C headers: csrc/rtc_prelude.hpp */
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define C3SC_MAX_DIM 12
#define C3SC_MAX_OBSTACLES 10 /* boundary.c:393 */
#define C3SC_MAX_PARAMS 8
#define C3SC_MAX_DU 4 /* control dimensions of the continuous (box) minimiser */

/* error codes (0 = ok, like the reference's int returns) */
enum {
    C3SC_OK = 0,
    C3SC_ERR_ARG = 1,         /* bad argument / state not set */
    C3SC_ERR_HIP = 2,         /* a HIP runtime call failed (c3sc_hip_last_error has the text) */
    C3SC_ERR_UNSUPPORTED = 3, /* no kernel instantiation for this (model, dim, rank, N) */
    C3SC_ERR_NODEVICE = 4
};

/* enum EBTYPE (boundary.h:42-47) */
enum { C3SC_EB_NONE = 0, C3SC_ABSORB = 1, C3SC_PERIODIC = 2, C3SC_REFLECT = 3 };

/* device problem models (restating the examples' callbacks; see c3sc_amd/csrc/models.hpp) */
enum {
    C3SC_MODEL_DUBINS3D = 1, /* examples/dubinscar_new/dubinscar.c:40-121 */
    C3SC_MODEL_SCAR4D = 2,   /* examples/skidding_car/scar.c:40-169 */
    C3SC_MODEL_CAR7D = 3,    /* synthetic 7-D car */
    C3SC_MODEL_LQGND = 4,    /* examples/lqgnd/lqgnd.c:80-198; params {dim, sig_even, sig_odd} */
    C3SC_MODEL_CHAIN = 5,    /* examples/double_int/double_int.c:80-157; params {dim, sig, sig_last, stage_mode} */
    C3SC_MODEL_ROSSLER3D = 6, /* examples/rossler/rossler.c:80-157; params {3, sig, sig_last} */
    C3SC_MODEL_PERCH7D = 8,  /* examples/perching/perch.c:36-273: glider perching, 7 states, elevator rate u in [-2 pi, 2 pi] */
    C3SC_MODEL_TPROB3D = 7,  /* the reference tests' 3-D problem: test/transition_prob/tprob_test.c f3 :223-251, s2, stagecost3d */
    C3SC_MODEL_SKID5D = 9,   /* examples/skidding5d/scar.c:39-176: 5-D skidding car (x, y, orientation, yaw rate, lateral speed), steering u */
    C3SC_MODEL_COTHRUST6D = 10, /* examples/cothrust2/copterposethrust.c:40-222: quadcopter position + velocity, controls (thrust, roll, pitch) */
    C3SC_MODEL_TABLE = 100,  /* host-evaluated callbacks (c3sc_hip_bellman_fibers_tables); not set with set_model */
    C3SC_MODEL_USER = 1000   /* first id of the run-time compiled models (c3sc_hip_model_compile) */
};

/* status bits accumulated by the kernels (c3sc_hip_get_status) */
enum {
    C3SC_STATUS_STATIONARY = 1u, /* transition_assemble would have returned 1 (Q < 1e-14, nodeutil.c:365);
                                   the reference asserts (bellman.c:452); the candidate is skipped here */
    C3SC_STATUS_CFL = 2u,        /* horizon mode (c3sc_hip_set_horizon_step): a candidate with Q delta > h^2, i.e. a negative
                                   self-loop probability 1 - Q delta / h^2; it still took part in the scan */
    C3SC_STATUS_DOMINANCE = 4u   /* correlation mode (c3sc_hip_set_correlation): a live node where the pairs take more off an axis
                                   rate than its diffusion supplies (a negative transition probability); the backup still returned
                                   the algebra's value */
};

/* kernel variants (c3sc_hip_set_variant); 0 lets the library choose.  Set the variant BEFORE uploading the value: the padded
 * rank of the device copy follows it (the quad kernel wants multiples of 4).  2 (one wavefront per 64 fibers) was retired (twice: DESIGN.md 4.5).
 * FIBER_QUAD covers both forms of that kernel (one or two wavefronts per 16 fibers).  Within a variant -- and across variants
 * under AUTO -- an instantiation whose LDS layout does not hold the grid declines and the next one of the same padded rank
 * runs; C3SC_ERR_UNSUPPORTED comes back only when none fits. */
enum { C3SC_VARIANT_AUTO = 0, C3SC_VARIANT_FIBER_PER_WAVE = 1, C3SC_VARIANT_FIBER_PER_LANE = 2, C3SC_VARIANT_FIBER_PAIR = 3,
       C3SC_VARIANT_FIBER_QUAD = 4 };

typedef struct c3sc_hip_ctx c3sc_hip_ctx;

/* lifetime: replaces c3control_create/destroy for the device side (bellman.c:1962-2019) */
int c3sc_hip_ctx_create(int device, c3sc_hip_ctx **out);
void c3sc_hip_ctx_destroy(c3sc_hip_ctx *ctx);
const char *c3sc_hip_last_error(const c3sc_hip_ctx *ctx);
int c3sc_hip_device_count(void);
/* largest FT rank the compiled kernels serve for (model id, state dimension d); 0 if none.  The reference has no such
 * limit (valuefunc.c:625-631 only clamps maxrank to min N); a caller clamps ApproxArgs.maxrank with it. */
int c3sc_hip_max_rank(int model, int d);

/* c3control_create's grid (bellman.c:1972-1986): ngrid[d], xgrid[m] host arrays of ngrid[m] doubles */
int c3sc_hip_set_grid(c3sc_hip_ctx *ctx, int d, const size_t *ngrid, const double *const *xgrid);
/* c3control_set_external_boundary / c3control_add_obstacle (bellman.c:2047-2062): bctype[d];
 * obstacles as inclusive boxes lb/ub (nobs x d row-major), lb = center - width/2 (boundary.c:264-267) */
int c3sc_hip_set_boundary(c3sc_hip_ctx *ctx, const int *bctype, int nobs, const double *obs_lb, const double *obs_ub);
/* NOT in the reference (default 0 = the reference's literal behaviour).  process_fibers_neighbor resets the absorbed flag of
 * a fiber's two end points from the varying dimension's own boundary type (nodeutil.c:570-612): a node on an absorbing face
 * of a fixed dimension, or inside an obstacle, is an ordinary node when it is the end point of a reflecting / periodic fiber
 * and a boundary / obstacle node along every other direction, so its value depends on the direction of the fiber it is
 * computed in (and, through the reference's memo, on which direction reached it first, bellman.c:1349-1353).  on = 1: end
 * points keep the flag the fixed dimensions and obstacles give them -- the batched Bellman operator becomes a function of
 * the node.  The solver loops of libc3sc.so switch it on (c3control_set_consistent_ends); the per-fiber entry points used
 * through the reference's callback ABI keep the literal behaviour. */
int c3sc_hip_set_consistent_ends(c3sc_hip_ctx *ctx, int on);
int c3sc_hip_get_consistent_ends(const c3sc_hip_ctx *ctx); /* 1 / 0; -1 for a null context */
/* mca_add_grid_refs (bellman.c:171-188) + dp_param_create's discount (bellman.c:220-235) */
int c3sc_hip_set_mca(c3sc_hip_ctx *ctx, double h2, const double *t, double discount);
/* replaces c3control_add_drift/diff/stagecost/boundcost/obscost (bellman.c:2064-2103) */
int c3sc_hip_set_model(c3sc_hip_ctx *ctx, int model, const double *params, int nparams);
/* replaces c3opt_alloc(BRUTEFORCE)+c3opt_set_brute_force_vals: cands[ncand*du], scanned in order, strict '<' */
int c3sc_hip_set_controls(c3sc_hip_ctx *ctx, int ncand, int du, const double *cands);
/* replaces vi_param_add_value + valuef_precompute_cores (bellman.c:1173, valuefunc.c:165-189):
 * ranks[d+1], cores[m] host arrays in the reference layout */
int c3sc_hip_upload_value(c3sc_hip_ctx *ctx, const size_t *ranks, const double *const *cores);
/* same, cores already resident on the device (e.g. after the RCCL all-gather of updated cores).  Asynchronous on `stream`: the
 * padded cores and the kernels' derived images are built by launches on that stream -- launch the fibers on the same stream or
 * synchronise first.  (c3sc_hip_upload_value above is complete on return.) */
int c3sc_hip_upload_value_device(c3sc_hip_ctx *ctx, const size_t *ranks, const double *const *d_cores, void *stream);
int c3sc_hip_set_variant(c3sc_hip_ctx *ctx, int variant);

/* THE HOT PATH.  Batched bellman_vi (bellman.c:1295-1423) without the memo: for each of the F
 * fibers along dim k and each of its N_k nodes: boundary stencil (process_fibers_neighbor,
 * nodeutil.c:489-627), FT neighbour costs (valuef_eval_fiber_ind_nn, valuefunc.c:369-585),
 * then bellman_optimal / bellman_control / transition_assemble / bellmanrhs per node
 * (bellman.c:504-543, 367-480; nodeutil.c:267-406; bellman.c:88-112).
 *   d_idx      int32 [F*d]        device
 *   d_out      double [F*N_k]     device, out[f*N_k + j] like the callback's out[]
 *   d_uidx     int32 [F*N_k] or NULL: winning candidate index, -1 for absorbed nodes
 *   d_absorbed int32 [F*N_k] or NULL: absorbed[] of process_fibers_neighbor (0 / 1 / -1)
 * Asynchronous on `stream`.  Large fiber-pair batches with an absorbing fixed dimension are partitioned on the device first
 * (live fibers first, grouped by the indices of the two fold levels next to k so that a tile's 64 fibers share those levels'
 * matrices; C3SC_FIBER_PARTITION=0 in the environment switches the pass off, n > 0 sets the smallest such batch,
 * C3SC_FIBER_GROUP=0 keeps the pass but leaves the live fibers in batch order, n > 0 sets the fewest fibers per key a level is
 * grouped by -- meant for tests: 1 groups every batch, which costs a production batch more than it gains; the results do not
 * depend on any of them; C3SC_PAIR_TABLE3=0 keeps a partitioned launch on the two-core product tables where a kernel with
 * three-core tables exists -- the same values bit for bit) into
 * scratch the context owns: the Bellman launches of ONE context must be ordered with respect to each other (one stream, or
 * events between streams); c3sc_hip_bellman_fibers_all orders its own. */
int c3sc_hip_bellman_fibers(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *d_idx, double *d_out,
                            int32_t *d_uidx, int32_t *d_absorbed, void *stream);
/* The same for SEVERAL varying dimensions of one batch -- a sweep over independent fiber batches (SURVEY.md 8d's roofline batch, a
 * rank's share of it) -- as one call: segment s is dimension ks[s] with F[s] fibers, indices d_idx[s] (F[s] x d) and values
 * d_out[s] (F[s] x N_ks[s], distinct arrays); d_uidx / d_absorbed may be NULL or hold NULL entries.  The per-dimension launches
 * are independent, so the library spreads them over `stream` and two internal streams, forked from and joined to `stream` by
 * events: the next dimension's workgroups take the slots the previous dimension's last tiles leave, which d launches on one
 * stream cannot (car7d: 3 % off a sweep at 2^20 fibers per dimension, 8 % at 2^17; tools/multistream_probe.py).  Stream-ordered
 * like a single launch; results are those of the per-dimension calls, bit for bit (the same kernels).  C3SC_NO_OVERLAP=1 keeps
 * everything on `stream`. */
int c3sc_hip_bellman_fibers_all(c3sc_hip_ctx *ctx, int nk, const int *ks, const size_t *F, const int32_t *const *d_idx, double *const *d_out,
                                int32_t *const *d_uidx, int32_t *const *d_absorbed, void *stream);

/* Policy evaluation: batched bellman_pi (bellman.c:1702-1886) without its memo tables.  Same stencil and
 * neighbour costs from the uploaded value function (the reference's vf_iteration), but every node applies the
 * GIVEN control candidate instead of minimising: out = bellmanrhs(stage(u), discount, prob(u), dt(u), costs)
 * (:1807-1815, :1857-1865); absorbed / obstacle nodes get boundcost / obscost (:1787-1801).
 *   d_policy   int32 [F*N_k]  device: candidate index per node, as returned in d_uidx by
 *              c3sc_hip_bellman_fibers run on the policy's value function (-1 = no control: value 0)
 * The reference caches [prob, dt, stage] of the policy per node; here the candidate index is the cache and the
 * rates are recomputed (a few dozen flops). */
int c3sc_hip_policy_fibers(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *d_idx, const int32_t *d_policy,
                           double *d_out, int32_t *d_absorbed, void *stream);
/* ... and policy evaluation for several varying dimensions in one call (see c3sc_hip_bellman_fibers_all) */
int c3sc_hip_policy_fibers_all(c3sc_hip_ctx *ctx, int nk, const int *ks, const size_t *F, const int32_t *const *d_idx,
                               const int32_t *const *d_policy, double *const *d_out, int32_t *const *d_absorbed, void *stream);
int c3sc_hip_policy_fibers_host(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *h_idx, const int32_t *h_policy,
                                double *h_out, int32_t *h_absorbed);

/* Continuous controls (bellman_optimal's non-BRUTEFORCE branch, bellman.c:545-1118; the reference hands the node
 * objective to C3's BFGS with multistarts -- third party, unseeded for du >= 2, unpinned): the device minimises over
 * the box [lb, ub]^du with a tensor grid of `grid` points per control dimension followed by `polish` rounds of
 * coordinate golden-section search in the cell around the best grid point.  Models with per-candidate features
 * (C3SC_MODEL_SCAR4D: tan(u0)) are not served.  set_controls is not needed in this mode.
 *   d_uopt double [F*N_k*du] or NULL: the minimiser per node (zeros at absorbed nodes)
 * c3sc_hip_policy_fibers_box evaluates a given control per node (bellman_pi with continuous controls). */
int c3sc_hip_set_control_box(c3sc_hip_ctx *ctx, int du, const double *lb, const double *ub, int grid, int polish);
int c3sc_hip_bellman_fibers_box(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *d_idx, double *d_out, double *d_uopt,
                                int32_t *d_absorbed, void *stream);
int c3sc_hip_bellman_fibers_box_host(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *h_idx, double *h_out, double *h_uopt,
                                     int32_t *h_absorbed);
int c3sc_hip_policy_fibers_box(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *d_idx, const double *d_policy_u,
                               double *d_out, int32_t *d_absorbed, void *stream);
int c3sc_hip_policy_fibers_box_host(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *h_idx, const double *h_policy_u,
                                    double *h_out, int32_t *h_absorbed);

/* The same hot path for ARBITRARY host callbacks (the reference's examples unchanged): the host evaluates
 * drift_eval / diff_eval / stagecost (dynamics.c:127-139,224-239; bellman.c:414-444) for every (node, candidate)
 * and boundcost / obscost (bellman.c:458,467) for every node of the fibers it submits:
 *   d_tables double [F][N_k][U][2d+1] = (drift[d], diag(diffusion)[d], stage cost)
 *   d_costs2 double [F][N_k][2]       = (boundcost, obscost)
 * set_grid / set_boundary / set_mca / set_controls / upload_value must have been called; set_model is not needed. */
int c3sc_hip_bellman_fibers_tables(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *d_idx, const double *d_tables,
                                   const double *d_costs2, double *d_out, int32_t *d_uidx, int32_t *d_absorbed,
                                   void *stream);
int c3sc_hip_bellman_fibers_tables_host(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *h_idx,
                                        const double *h_tables, const double *h_costs2, double *h_out,
                                        int32_t *h_uidx, int32_t *h_absorbed);
/* policy evaluation (bellman_pi) with host-evaluated callbacks: as c3sc_hip_policy_fibers, rates from the tables */
int c3sc_hip_policy_fibers_tables(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *d_idx, const double *d_tables,
                                  const double *d_costs2, const int32_t *d_policy, double *d_out, int32_t *d_absorbed,
                                  void *stream);
int c3sc_hip_policy_fibers_tables_host(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *h_idx,
                                       const double *h_tables, const double *h_costs2, const int32_t *h_policy,
                                       double *h_out, int32_t *h_absorbed);

/* Batched mca_get_neighbor_costs (nodeutil.c:647-713) only: d_costs double [F*N_k*(2d+1)],
 * layout out[j*(2d+1) + 2m + {0,1}] = (-,+) neighbour in dim m, [.. + 2d] = self. */
int c3sc_hip_stencil_fibers(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *d_idx, double *d_costs,
                            int32_t *d_absorbed, void *stream);

/* The literal valuef_eval_fiber_ind_nn interface (valuefunc.c:369-371) batched: the caller supplies the
 * neighbour indices instead of having them derived from the boundary types.
 *   d_nb_fixed int32 [F][2(d-1)]  (-,+) neighbour index of every fixed dim, dims != k in order
 *   d_nb_vary  int32 [F][N_k][2]  (-,+) neighbour node of every fiber node
 * either may be NULL (then derived as in c3sc_hip_stencil_fibers). */
int c3sc_hip_stencil_fibers_nb(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *d_idx, const int32_t *d_nb_fixed,
                               const int32_t *d_nb_vary, double *d_costs, int32_t *d_absorbed, void *stream);
int c3sc_hip_stencil_fibers_nb_host(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *h_idx,
                                    const int32_t *h_nb_fixed, const int32_t *h_nb_vary, double *h_costs,
                                    int32_t *h_absorbed);

/* Convenience for host callers (the C facade's bellman_vi): host buffers, synchronous.  c3sc_hip_bellman_fibers_host,
 * c3sc_hip_policy_fibers_host, c3sc_hip_bellman_fibers_box_host and c3sc_hip_policy_fibers_box_host serve batches whose
 * buffers total <= 1 MiB (a cross-approximation core step) from a pinned, device-mapped block of the context -- the kernel
 * reads the indices and writes its rows in place, no hipMemcpy; larger ones are staged through device scratch, and so is
 * every batch of the tables and stencil calls.  C3SC_NO_ZEROCOPY=1 in the environment forces the staged path. */
int c3sc_hip_bellman_fibers_host(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *h_idx, double *h_out,
                                 int32_t *h_uidx, int32_t *h_absorbed);
int c3sc_hip_stencil_fibers_host(c3sc_hip_ctx *ctx, int k, size_t F, const int32_t *h_idx, double *h_costs,
                                 int32_t *h_absorbed);

/* Closed-loop policy rollouts on the device (new; the reference runs them one state at a time on the host:
 * c3control_add_policy_sim + c3control_controller + an Euler integration, e.g. dubinscar.c:376-382, lqg2d.c:346-353).
 *
 * c3sc_hip_set_interp: constelm = 1 evaluates the value function off the grid as a CONSTELM ValueF does (valuef_eval: the
 * nearer node of each cell), 0 (default) piecewise multilinearly.
 *
 * c3sc_hip_stencil_points: mca_get_neighbor_node_costs (nodeutil.c:718-816) for n states at once: the 2d+1 values of the
 * interpolant of the uploaded value function around each state x (d_x double [n*d], device).  d_out double [n*(2d+1)]:
 * out[i*(2d+1) + 2m + {0,1}] = value at the (-,+) neighbour one grid spacing away in dim m (boundary branches of the host
 * code: absorbing / reflecting faces clamp to the bound, periodic ones wrap), [.. + 2d] = value at x.  d_absorbed int32 [n]
 * or NULL: -1 inside an obstacle (then all 2d+1 entries are the value at x), 0 otherwise.  set_grid / set_boundary (no
 * C3SC_EB_NONE dimension) / upload_value must have been called.  Asynchronous on `stream`. */
int c3sc_hip_set_interp(c3sc_hip_ctx *ctx, int constelm);
int c3sc_hip_stencil_points(c3sc_hip_ctx *ctx, size_t n, const double *d_x, double *d_out, int32_t *d_absorbed, void *stream);

/* c3sc_hip_simulate: n trajectories of the implicit policy of the uploaded value function, one GPU lane each.  Step k of a
 * trajectory (x_k its state, t_k = k dt):
 *   exit test    x_k outside [lb, ub] on an ABSORB dimension or inside an obstacle: the trajectory stops at k (exit_step = k),
 *                pays e^{-beta t_k} (obscost if inside an obstacle, else boundcost)(x_k) and keeps its state from then on;
 *                REFLECT and PERIODIC dimensions never stop a trajectory.  x_nsteps is tested as well.
 *   controller   y = x_k (wrap_periodic: its PERIODIC coordinates mapped into [lb, ub)); the off-grid stencil at y, then the
 *                minimiser the Bellman kernels use: the candidate list (box = 0; first minimum, strict '<') or the control box
 *                (box = 1, c3sc_hip_set_control_box).  Inside an obstacle u = 0 (bellman_optimal's absorbed branch).
 *   cost         + e^{-beta t_k} stage(x_k, u_k) dt, beta = the discount of set_mca
 *   dynamics     x_{k+1} = x_k + b(x_k, u_k) dt + s(x_k, u_k) * sqrt(dt) xi_k (diagonal diffusion, dw = d), c3control_simulate's step
 * The noise xi is d_noise when given, else Philox4x32-10 + Box-Muller keyed by (seed, traj_offset + i, k, component): the bits
 * of a trajectory depend on its global index only, not on n or on how a batch is split (c3sc_hip_normals is the host twin).
 * The call is cut into launches of steps_per_launch steps (0 = 64); the state is kept in a buffer of the context between them.
 * Errors: C3SC_ERR_ARG (state not set, null x0, dt <= 0, a C3SC_EB_NONE dimension, save_every = 0 with d_traj / d_u ...),
 * C3SC_ERR_UNSUPPORTED (the TABLE model, no rollout instantiation for this model at this padded rank, a box without one).
 * n is at most 2^31 per call (split larger batches with traj_offset).  The state between launches lives in ONE buffer of the
 * context: calls on the same context must not overlap (same stream, or synchronise between them); use one context per stream.
 * last_kernel names the rollout kernel.  Asynchronous on `stream`. */
typedef struct c3sc_hip_sim_args {
    size_t n;                /* trajectories */
    const double *d_x0;      /* [n*d] initial states */
    double dt;
    size_t nsteps;
    uint64_t traj_offset;    /* global index of trajectory 0 (noise counter) */
    uint64_t seed;
    const double *d_noise;   /* [n*nsteps*d] standard normals or NULL (seeded Philox); wins when non-NULL */
    int wrap_periodic;
    int box;                 /* 0: candidate list (set_controls), 1: control box (set_control_box) */
    int steps_per_launch;    /* 0 = 64 */
    size_t save_every;       /* 0 = none; else states k = 0, s, 2s, ... <= nsteps and controls k = 0, s, ... < nsteps */
    double *d_traj;          /* [n][nsteps/save_every + 1][d] or NULL */
    double *d_u;             /* [n][ceil(nsteps/save_every)][du] or NULL (0 after exit) */
    double *d_cost;          /* [n] discounted cost J or NULL */
    int64_t *d_exit;         /* [n] exit step, -1 = never, or NULL */
    double *d_vend;          /* [n] interpolant at the final state (wrapped like the controller's input) or NULL */
    double *d_xfinal;        /* [n*d] final state or NULL */
} c3sc_hip_sim_args;
int c3sc_hip_simulate(c3sc_hip_ctx *ctx, const c3sc_hip_sim_args *args, void *stream);
/* the same with HOST arrays in every pointer of args (d_* names notwithstanding): staged through device memory, synchronous.
 * This is what libc3sc.so's c3control_simulate_batch calls. */
int c3sc_hip_simulate_host(c3sc_hip_ctx *ctx, const c3sc_hip_sim_args *args);

/* c3sc_hip_integrate: deterministic closed loops x' = b(x, pi(x)) of the implicit policy of the uploaded value function, n
 * trajectories, one GPU lane each -- the examples' cdyn tail (c3control_add_policy_sim + a controlled integrator + a goal test
 * after every trajectory_step) on the device.  No diffusion (c3sc_hip_simulate is the stochastic path).
 *   steps        nout outer steps of dt_out, each nsub = dt_out / dt_int integrator substeps of h = dt_int (dt_int = 0: nsub = 1,
 *                h = dt_out); nsub must be an integer to 1e-9 relative.
 *   method       C3SC_ODE_FORWARD_EULER: y + h b(y, pi(y)); C3SC_ODE_RK4: classical RK4, the controller evaluated at each of
 *                the four stage states.
 *   controller   pi(y) is c3sc_hip_simulate's: y (wrap_periodic: its PERIODIC coordinates mapped into [lb, ub)), the off-grid
 *                stencil, the candidate list (box = 0) or the control box (box = 1, where the model's kernels serve one);
 *                u = 0 inside an obstacle.  The drift is evaluated at the unwrapped y.
 *   cost         one more ODE component c' = e^{-beta t} stage(y, pi(y)), same method and stage controls.  Forward Euler uses
 *                c3sc_hip_simulate's arithmetic (c + e^{-beta t} stage h, x + b h): with nsub = 1 and no stop boxes its results
 *                equal c3sc_hip_simulate's with an all-zero d_noise.  An exit pays e^{-beta t_j} (boundcost | obscost)(x_j)
 *                as c3sc_hip_simulate does; goal and keep-in stops pay nothing.
 *   stops        tested at every outer step j = 0 .. nout (t_j = j dt_out), the first that holds wins: 1 outside an ABSORB face,
 *                2 inside an obstacle, 3 inside the goal box (lo < x < hi on every dimension; +-inf allowed), 4 outside the
 *                keep-in box (x < lo or x > hi on some dimension).  A stopped lane is frozen: state and cost stay, saved
 *                controls are 0.  d_goal / d_keep: HOST arrays [2*d] = (lo[d], hi[d]) or NULL; lo > hi is an error.
 *   outputs      any may be NULL: d_cost[n], d_stop_step[n] (-1 = never), d_stop_reason[n] (0 = never), d_xfinal[n*d],
 *                d_vend[n] (interpolant at the final state, wrapped like the controller's input); with save_every > 0
 *                d_traj[n][nout/save_every + 1][d] (states at j = 0, s, 2s, ...) and d_u[n][ceil(nout/save_every)][du] (the
 *                control of the first stage of outer steps j = 0, s, ...).
 *   launches     a call is cut into launches of at most evals_per_launch controller evaluations per lane (0 = 256), rounded
 *                to whole substeps (at least one); state, cost and stop fields stay in the context's buffer between them.
 *                Results do not depend on evals_per_launch or on how a batch is split.
 * Errors: C3SC_ERR_ARG (state not set, null x0, dt_out <= 0, dt_int < 0 or a non-integer nsub, a bad method, save_every misuse,
 * inverted stop boxes), C3SC_ERR_UNSUPPORTED (the TABLE model, no integrate instantiation for this model at this padded rank, a
 * box without one).  Calls on one context must not overlap with each other or with c3sc_hip_simulate (one state buffer).
 * last_kernel names the k_rollout_ode kernel.  Asynchronous on `stream`. */
enum { C3SC_ODE_FORWARD_EULER = 0, C3SC_ODE_RK4 = 1 };
typedef struct c3sc_hip_ode_args {
    size_t n;                /* trajectories */
    const double *d_x0;      /* [n*d] initial states */
    double dt_out;           /* outer step */
    double dt_int;           /* integrator step (0: dt_out) */
    size_t nout;             /* outer steps */
    int method;              /* C3SC_ODE_* */
    int wrap_periodic;
    int box;                 /* 0: candidate list (set_controls), 1: control box (set_control_box) */
    int evals_per_launch;    /* controller evaluations per lane per launch, 0 = 256 */
    const double *goal;      /* host [2*d] (lo, hi) or NULL */
    const double *keep;      /* host [2*d] (lo, hi) or NULL */
    size_t save_every;       /* 0 = none */
    double *d_traj;          /* [n][nout/save_every + 1][d] or NULL */
    double *d_u;             /* [n][ceil(nout/save_every)][du] or NULL */
    double *d_cost;          /* [n] or NULL */
    int64_t *d_stop_step;    /* [n] or NULL */
    int32_t *d_stop_reason;  /* [n] or NULL */
    double *d_vend;          /* [n] or NULL */
    double *d_xfinal;        /* [n*d] or NULL */
} c3sc_hip_ode_args;
int c3sc_hip_integrate(c3sc_hip_ctx *ctx, const c3sc_hip_ode_args *args, void *stream);
/* the same with HOST arrays in every pointer of args: staged through device memory, synchronous (c3control_integrate_batch) */
int c3sc_hip_integrate_host(c3sc_hip_ctx *ctx, const c3sc_hip_ode_args *args);
/* host twin of the rollouts' noise: out[(t*nsteps + k)*dw + j] = the normal of component j at step step0 + k of trajectory
 * traj0 + t under `seed` -- the same bits the device draws (philox.hpp) */
int c3sc_hip_normals(uint64_t seed, uint64_t traj0, size_t ntraj, uint64_t step0, size_t nsteps, int dw, double *out);

/* The approximating Markov chain itself.  At a live node xi the chain of the greedy policy of the uploaded
 * value function moves to the 2d index-rule neighbours with probabilities p_k / C after the interval dt = h^2 / C, C = sum p_k.
 * Outcome order = stencil order: k = 2m is the lo and k = 2m + 1 the hi neighbour of dimension m, by the fixed-dimension index
 * rule in EVERY dimension (a reflecting end names the node itself -- a self-loop that still costs its dt; the periodic seam is
 * n - 2 / 1).  Node flags: 1 on an absorbing face (index 0 or N - 1 of any ABSORB dimension), else -1 inside an obstacle, else 0;
 * this is the consistent end-point rule and does not depend on c3sc_hip_set_consistent_ends (a walk has no fiber direction).
 *
 * c3sc_hip_chain_transitions: the deterministic half for n nodes, d_nodes int32 [n*d] multi-indices.  Per node (each output may
 * be NULL): d_uidx int32 the greedy candidate (plain backup over the candidate list, first minimum), d_value the backup's value,
 * d_stage g(x, u), d_dt, d_P [n*2d] the probabilities in outcome order, d_flag int32.  A flagged node has uidx = -1, dt = 0,
 * P = 0 and value = stage = the bound / obstacle cost.  A stuck node -- live, with no valid candidate or a winner with
 * C < 1e-14 -- raises C3SC_STATUS_STATIONARY and has uidx = -1, dt = 0, P = 0.
 *
 * c3sc_hip_simulate_chain: n walks of that chain, one GPU lane each.  Step s of a walk at the node xi_s:
 *   flag test    an absorbed node pays D boundcost(x), an obstacle node D obscost(x); exit = s and the walk is frozen
 *   stuck        a stuck node freezes the walk: exit = -(s + 2)   (C3SC_CHAIN_STUCK(s); -1 stays "still running")
 *   accumulate   J += D stage dt, T += dt, D *= exp(-beta dt)   (D starts at 1)
 *   sample       v = d_uniform[i*nsteps + s] when given, else the first uniform of c3sc_hip_jump_uniforms(seed, traj_offset + i, s);
 *                with c_k = p_0 + .. + p_k the outcome is the first k with v C < c_k, else the last k with p_k > 0
 * xi_nsteps gets the flag test as well and d_vend = V(xi_nsteps).  With J^pi, the exact cost of the greedy policy pi in the discrete
 * problem, J_n + D_n J^pi(xi_n) is an unbiased estimator of J^pi(xi_0); with d_vend in its place the mean equals V(xi_0) only where V
 * is the fixed point of its own greedy operator.  The call is cut into launches of steps_per_launch steps (0 = 64); results do not
 * depend on that, on n, or on how a batch is split (traj_offset).  The state between launches shares c3sc_hip_simulate's buffer
 * of the context: calls on one context must not overlap.
 * Errors: C3SC_ERR_ARG (state not set, null inputs, a node index out of range, a C3SC_EB_NONE dimension, save_every = 0 with
 * d_traj / d_uidx, a save_every above nsteps and above 1 with either, as c3sc_hip_simulate); C3SC_ERR_UNSUPPORTED, the context staying usable: the TABLE model, a run-time compiled model without chain
 * kernels (c3sc_hip_model_compile_mc, below, adds them and the chain of the horizon, stopping and jump modes), no instantiation at
 * the padded rank, a context in game, impulse or correlation mode, a built-in model in any mode, a mode the model's chain kernels
 * were not compiled with.  The control box is
 * not served: the calls take the candidate list.  Both calls read the node indices back to check them, so they synchronise
 * `stream` once before they launch.  last_kernel names the kernel. */
#define C3SC_CHAIN_STUCK(s) (-((int64_t)(s) + 2))
int c3sc_hip_chain_transitions(c3sc_hip_ctx *ctx, size_t n, const int32_t *d_nodes, int32_t *d_uidx, double *d_value, double *d_stage,
                               double *d_dt, double *d_P, int32_t *d_flag, void *stream);
int c3sc_hip_chain_transitions_host(c3sc_hip_ctx *ctx, size_t n, const int32_t *nodes, int32_t *uidx, double *value, double *stage,
                                    double *dt, double *P, int32_t *flag);
typedef struct c3sc_hip_chain_args {
    size_t n;                /* walks */
    const int32_t *d_node0;  /* [n*d] start nodes */
    size_t nsteps;
    uint64_t traj_offset;    /* global index of walk 0 (Philox counter) */
    uint64_t seed;
    const double *d_uniform; /* [n*nsteps] uniforms in [0, 1) or NULL (seeded Philox); wins when non-NULL; with jumps on
                              * [n*nsteps*2] = (v, u1) */
    int steps_per_launch;    /* 0 = 64 */
    size_t save_every;       /* 0 = none; else nodes s = 0, e, 2e, ... <= nsteps and decisions s = 0, e, ... < nsteps */
    double *d_cost;          /* [n] J or NULL */
    double *d_disc;          /* [n] D or NULL */
    double *d_time;          /* [n] T or NULL */
    double *d_vend;          /* [n] V(xi_nsteps) or NULL */
    int32_t *d_node;         /* [n*d] final node or NULL */
    int64_t *d_exit;         /* [n] -1 running, s >= 0 absorbed / obstacle at step s, C3SC_CHAIN_STUCK(s) stuck at step s,
                              * C3SC_CHAIN_STOPPED(s) stopped at step s, s + 1 a jump out at step s; or NULL */
    int32_t *d_traj;         /* [n][nsteps/save_every + 1][d] or NULL */
    int32_t *d_uidx;         /* [n][ceil(nsteps/save_every)] (-1 once frozen) or NULL */
} c3sc_hip_chain_args;
int c3sc_hip_simulate_chain(c3sc_hip_ctx *ctx, const c3sc_hip_chain_args *args, void *stream);
/* the same with HOST arrays in every pointer of args: staged through device memory, synchronous */
int c3sc_hip_simulate_chain_host(c3sc_hip_ctx *ctx, const c3sc_hip_chain_args *args);

/* Device-resident core steps of the cross approximation that calls the path (valuefunc.c:603-767 hands bellman_vi to C3's
 * ftapprox_cross; c3sc_amd/host/c3sc_cross.c is this library's driver).  A cross iteration is 2 d sequential core steps of
 * r_k r_{k+1} fibers each; with fibers on the GPU and factorisation + node memo on the host a sweep is host-bound.  These
 * entry points keep a whole iteration on one stream: fiber index lists from the device-resident index sets, the batched
 * Bellman kernel, the node memo (first value stays: bellman.c:1333-1353, 1412-1417; keyed by node id and sweep epoch) and a
 * one-workgroup pivoted factorisation + maxvol that writes the interpolatory core and the next index set.
 *   ranks[d+1]; I[k]: ranks[k] tuples over dims 0..k-1 (int32, row-major); J[k]: ranks[k+1] tuples over dims k+1..d-1
 *   new_sweep != 0 starts a new memo epoch (workspace_increment_vi_iter, bellman.c:2199)
 *   Every set-up -- and ONLY a set-up -- starts a new generation of cached step values: a core step that finds the fiber list it
 *   already holds, with values of the current generation, keeps them and launches nothing.  c3sc_hip_upload_value[_device] does
 *   NOT start one.  So whenever the value function changes between two iterations (ctx's own, or policy_ctx's for
 *   c3sc_hip_cross_iteration_pi, or the policy tag), call c3sc_hip_cross_setup in between -- new_sweep = 0 keeps the memo epoch and
 *   its entries -- or a step whose list did not change returns the values (the policy) of the OLD function.
 *   box: 0 = candidate list (set_controls), 1 = control box (set_control_box)
 *   fetch waits for the stream and returns the cores of the last half sweep in the layout G_k[a + r_k (j + N_k b)], both
 *   families of index sets, and info[4] = {nodes stored in the memo since the last fetch (the reference's nnode_evals),
 *   1 if a fiber matrix was numerically rank deficient, maxvol row swaps, 1 if the memo overflowed / 2 if a rank of a sharded
 *   sweep failed (its rows arrived as NaN)}
 *   ranks up to 48 (above 32 a core step runs on global scratch).  Streams: setup works on the NULL stream and is COMPLETE when it
 *   returns, so iteration / confirm / speculate / fetch may be given any stream (all calls of one context on the same one) */
int c3sc_hip_cross_setup(c3sc_hip_ctx *ctx, const size_t *ranks, const int32_t *const *I, const int32_t *const *J, int new_sweep);
int c3sc_hip_cross_iteration(c3sc_hip_ctx *ctx, int box, void *stream);
/* The same iteration with its cores STREAMED to the host: the right-to-left half sweep produces the cores in the order k = d-1 .. 0,
 * the order in which a right-to-left orthogonalisation (the first half of the TT rounding, what C3's ftapprox_cross_rankadapt does
 * behind valuefunc.c:728-733) consumes them.  Each core is copied to the pinned block on a stream of its own as soon as its step
 * has run; c3sc_hip_cross_wait_core(k, h_core) waits for THAT copy only and hands the core over (working layout), while the later
 * steps are still running.  c3sc_hip_cross_fetch afterwards brings the index sets and counters (pass h_cores = NULL).  Same kernels,
 * same results as c3sc_hip_cross_iteration. */
int c3sc_hip_cross_iteration_streamed(c3sc_hip_ctx *ctx, int box, void *stream);
int c3sc_hip_cross_wait_core(c3sc_hip_ctx *ctx, int k, double *h_core);
/* after an iteration that changed index sets: the confirming iteration as ONE launch (all core steps side by side on the values
 * they already hold, comparing instead of writing their index sets).  *confirmed = 1: the iteration that would follow changes
 * nothing and its cores are in place -- fetch them; 0: run c3sc_hip_cross_iteration[_pi] as usual.  Synchronises the stream. */
int c3sc_hip_cross_confirm(c3sc_hip_ctx *ctx, int *confirmed, void *stream);
/* at the start of a sweep whose index sets come from the previous sweep: the whole iteration in d + 1 launches -- the fiber lists
 * of all d cores from the current sets, evaluated back to back (no core step in between), then the confirming launch above.
 * *confirmed = 1: every step reproduced its index set, so the sequential iteration would have returned exactly these cores (fetch
 * them); 0: run c3sc_hip_cross_iteration[_pi] -- what was evaluated here stays cached.  policy_ctx == NULL: bellman_vi's fibers, else
 * bellman_pi's as in c3sc_hip_cross_iteration_pi.  Unsharded contexts; otherwise nothing is launched and *confirmed = 0.  Because the
 * lists are evaluated before any set is known to survive, a failed attempt may have put nodes into the memo that the sequential
 * iteration would not have asked for: use it only where a node's value does not depend on the fiber that computes it
 * (c3sc_hip_set_consistent_ends).  Synchronises the stream. */
int c3sc_hip_cross_speculate(c3sc_hip_ctx *ctx, c3sc_hip_ctx *policy_ctx, long long policy_tag, int box, int *confirmed, void *stream);
/* the same for bellman_pi (bellman.c:1702-1886): per core step the greedy policy of the value function uploaded to policy_ctx
 * (cached per node for the whole policy iteration policy_tag: the reference's prob table, bellman.c:1806, 1877), then its
 * evaluation on ctx's value function.  info[0] of the fetch then counts the nodes whose policy was computed (npol_evals). */
int c3sc_hip_cross_iteration_pi(c3sc_hip_ctx *ctx, c3sc_hip_ctx *policy_ctx, long long policy_tag, void *stream);
/* pivot search of the core steps: warm_pivots != 0 starts it from the rows of the index set the step produced last time,
 * swap_tol is maxvol's dominance tolerance (row swaps while max |B| > 1 + swap_tol); defaults 1 and 0.05 */
int c3sc_hip_cross_options(c3sc_hip_ctx *ctx, int warm_pivots, double swap_tol);
/* after info[3] == 1 (memo full): double the memo tables keeping the current epoch's entries (no reference counterpart: the
 * reference's hash table never fills, util.c:760-766 -- it chains) */
int c3sc_hip_cross_grow_memo(c3sc_hip_ctx *ctx);
int c3sc_hip_cross_fetch(c3sc_hip_ctx *ctx, double *const *h_cores, int32_t *const *h_I, int32_t *const *h_J, unsigned long long *info,
                         void *stream);
void c3sc_hip_cross_free(c3sc_hip_ctx *ctx);

/* Multi-GPU (one process per GPU, RCCL over xGMI, opened at run time -- no link dependency).  The path shards
 * by independent fibers: every rank evaluates a contiguous block of each core step's fibers on its own device and ONE all-gather
 * per core step puts the F x N values on every rank (tens of KB, latency-bound).  bellman.c:2201 passes the value function
 * read-only during a sweep, which is what makes the fibers independent.
 *   unique_id: rank 0 creates the 128-byte id and hands it to the other ranks (file, environment, socket ...)
 *   create:    collective over all ranks of the node
 *   allgather: count doubles per rank, device buffers, in place when d_send == d_recv + rank * count; asynchronous on stream
 *   cross_set_comm: the device-resident cross iterations of ctx shard their core steps over the communicator
 *   exchange:  a c3sc_exchange_fn (include/c3sc/valuefunc.h) for the host-driven sharded driver: pass it with xarg = the
 *              communicator to c3control_set_fiber_sharding / valuef_interp_idx_sharded */
typedef struct c3sc_hip_comm c3sc_hip_comm;
int c3sc_hip_comm_unique_id(void *id128);
int c3sc_hip_comm_create(c3sc_hip_ctx *ctx, int world, int rank, const void *id128, c3sc_hip_comm **out);
void c3sc_hip_comm_destroy(c3sc_hip_comm *comm);
int c3sc_hip_comm_world(const c3sc_hip_comm *comm);
int c3sc_hip_comm_rank(const c3sc_hip_comm *comm);
int c3sc_hip_comm_allgather(c3sc_hip_comm *comm, const double *d_send, double *d_recv, size_t count, void *stream);
int c3sc_hip_cross_set_comm(c3sc_hip_ctx *ctx, c3sc_hip_comm *comm);
int c3sc_hip_comm_exchange(double *out, size_t F, size_t N, size_t lo, size_t hi, void *comm);

/* ---- run-time compiled device models: a user's own dynamics on every device path
 *
 * c3sc_hip_model_compile compiles the device source of a model with hipRTC (loaded at first use) and returns a model id
 * (>= C3SC_MODEL_USER) that c3sc_hip_set_model, the Bellman / box / simulate / integrate calls and the reference API's
 * c3control_set_device_model accept like a built-in id.  No GPU is needed to compile: the code object is loaded on each
 * device at its first launch there.  The source defines, for x[C3SC_D], u[C3SC_DU] and prm = the C3SC_MAX_PARAMS values of
 * c3sc_hip_set_model (C3SC_D and C3SC_DU are defined for it; the library wraps it in a namespace of its own):
 *
 *   __device__ void   drift    (const double *prm, const double *x, const double *u, double *b);  b[C3SC_D]
 *   __device__ void   sigma    (const double *prm, const double *x, const double *u, double *s);  diagonal diffusion, s[C3SC_D]
 *   __device__ double stage    (const double *prm, const double *x, const double *u);
 *   __device__ double boundcost(const double *prm, const double *x);
 *   __device__ double obscost  (const double *prm, const double *x);
 *
 * The device libm (sin, cos, exp, ...) may be used.  Unlike the built-in models, whose transcendentals are host tables, these
 * run on the device and differ from glibc's by about an ulp.  No #include is available to the source.
 *   udep_mask    dims whose drift / diffusion read u (0 = all); uconst_mask: those of them that read nothing else (0 = none):
 *                their rates are constants of the candidate.  stage_udep: the stage cost reads u.  Wrong masks give wrong values.
 *   box          also compile the box-minimiser (continuous controls) kernels
 *   ranks        padded FT ranks to compile, each in {4, 8, 12, 16, 20} (NULL / 0 = {4, 8}); a value function of higher
 *                rank, and the fiber-pair / fiber-quad variants, give C3SC_ERR_UNSUPPORTED at use
 * Compiled per rank: the fiber-per-wave Bellman kernels (1 and 2 nodes per lane: N <= 128), k_rollout, k_rollout_ode, and
 * the model-independent stencil kernels of a (d, rank) the library lacks.  A compile takes seconds; the same spec compiled
 * again returns the same id.  Compiles are serialised process-wide; models are never unloaded.
 * Errors: C3SC_ERR_ARG (bad d / du / masks / ranks, a compile error: c3sc_hip_model_log has the compiler's message with the
 * source's line), C3SC_ERR_UNSUPPORTED (hipRTC missing).  c3sc_hip_model_code_object copies the gfx950 code object (buf NULL:
 * *size receives its size; otherwise *size is the capacity of buf on entry and the size on return): for a spec already
 * compiled, the one its model loads; otherwise it compiles (nothing is registered or kept) what c3sc_hip_model_compile would
 * build now -- the id and default name it would assign appear in the kernel names, so a compile of another model in between
 * changes them.  Each call without a compiled model compiles again. */
typedef struct c3sc_hip_model_spec {
    const char *source;
    const char *name;        /* [A-Za-z0-9_.-]{1,48}: appears in c3sc_hip_last_kernel; NULL = "model<id>" */
    int d, du;               /* 2..10, 1..C3SC_MAX_DU */
    unsigned udep_mask, uconst_mask;
    int stage_udep;
    int box;
    int nranks;
    const int *ranks;
} c3sc_hip_model_spec;
int c3sc_hip_model_compile(const c3sc_hip_model_spec *spec, int *model_id);
int c3sc_hip_model_code_object(const c3sc_hip_model_spec *spec, void *buf, size_t *size);
/* the compiler's log / the reason of the last failed model compile on this thread ("" if none) */
const char *c3sc_hip_model_log(void);

/* ---- zero-sum stochastic games
 * Two players share the control vector (u, w) of a run-time compiled model: the first du_min components belong to the
 * minimiser, the remaining du_max to the maximiser, du_min + du_max = the model's du.  c3sc_hip_set_game builds the candidate
 * list as the product of the minimiser's list U (nu x du_min, row-major) and the maximiser's W (nw x du_max) and makes the
 * Bellman operator a min-max over it:
 *   C3SC_GAME_MINMAX (default, the upper value)  min over u of max over w
 *   C3SC_GAME_MAXMIN (the lower value)           max over w of min over u
 * Per candidate everything is the plain scan's (rates, dead zone, Q, dt, discount, the stationary skip and its status bit).  The
 * kernel reduces a grouped list (the library orders it u-major for MINMAX, w-major for MAXMIN): the inner reduction inside a
 * group, the outer one over the groups.  Both keep the scan order: a min takes the first strict '<', a max the first strict
 * '>'.  A stationary candidate (Q < 1e-14) is skipped and raises C3SC_STATUS_STATIONARY; a group whose members were all skipped
 * takes no part in the outer reduction; with nothing left the node's value is 0 and its index -1.  With beta = 0 the scan
 * compares fractions and divides once for the winner, as the plain scan does.
 * The reported index (uidx) is the saddle pair iu * nw + iw in either order, -1 on absorbed nodes.  Policy evaluation
 * (policy_fibers*) applies a given pair index (the forced path, unchanged).  Game mode is honoured by bellman_fibers(_all),
 * the device-resident cross iterations, simulate and integrate (the controller applies the saddle pair; d_u holds the full
 * du vector); cross_iteration_pi refuses it.  Only the fiber-per-wave kernel has a game form: a forced pair or quad variant,
 * the control box and the box calls return C3SC_ERR_UNSUPPORTED; AUTO picks the per-wave kernel.
 * nu = 0 clears game mode; so does c3sc_hip_set_controls.  Errors: C3SC_ERR_ARG (sizes that do not add up to the model's du,
 * a bad order, null lists), C3SC_ERR_UNSUPPORTED (a built-in or the TABLE model, a model compiled without game kernels).
 * Set the model first. */
enum { C3SC_GAME_MINMAX = 0, C3SC_GAME_MAXMIN = 1 };
int c3sc_hip_set_game(c3sc_hip_ctx *ctx, int du_min, int nu, const double *U, int nw, const double *W, int order);
/* a run-time compiled model with game kernels: c3sc_hip_model_compile's spec plus a flag.  game = 1 adds the game forms of the
 * per-wave, rollout and integrate kernels at every requested rank (box must be 0 then: C3SC_ERR_UNSUPPORTED); game = 0 is
 * exactly c3sc_hip_model_compile.  c3sc_hip_model_code_object_ex is c3sc_hip_model_code_object for such a spec. */
typedef struct c3sc_hip_model_spec_ex {
    c3sc_hip_model_spec base;
    int game;
} c3sc_hip_model_spec_ex;
int c3sc_hip_model_compile_ex(const c3sc_hip_model_spec_ex *spec, int *model_id);
int c3sc_hip_model_code_object_ex(const c3sc_hip_model_spec_ex *spec, void *buf, size_t *size);

/* Finite-horizon problems: a deadline T = N delta, a terminal cost V_N and a value V_n per stage.  In horizon
 * mode the Bellman operator is Kushner's explicit scheme with the fixed step delta (one stage back, V_{n+1} -> V_n):
 *     V_n(x) = min_u [ g(x,u) delta + e^{-beta delta} ( V_self + (delta / h^2) (PV - Q V_self) ) ]
 * with the upwind rates p_i of the infinite-horizon operator, Q = sum p_i, PV = sum p_i V_i and V_self the node's own value, all
 * of V_{n+1} (the uploaded value).  The transition probabilities are delta p_i / h^2 and the self-loop 1 - Q delta / h^2.  There
 * is no division: a candidate with Q = 0 ("stay") is not skipped.  A candidate with Q delta > h^2 (negative self-loop) still takes
 * part and raises C3SC_STATUS_CFL.  Scan order and ties, absorbed and obstacle nodes and the forced path (policy evaluation) are
 * the infinite-horizon operator's.
 * The horizon kernels exist only in run-time compiled models built with c3sc_hip_model_compile_fh and horizon = 1 (the forms of
 * the per-wave and rollout kernels at every requested rank).  horizon = 1 with ex.game = 1 or ex.base.box = 1 returns
 * C3SC_ERR_UNSUPPORTED; horizon = 0 is exactly c3sc_hip_model_compile_ex. */
typedef struct c3sc_hip_model_spec_fh {
    c3sc_hip_model_spec_ex ex;
    int horizon;
} c3sc_hip_model_spec_fh;
int c3sc_hip_model_compile_fh(const c3sc_hip_model_spec_fh *spec, int *model_id);
int c3sc_hip_model_code_object_fh(const c3sc_hip_model_spec_fh *spec, void *buf, size_t *size);
/* horizon mode on with the step dt > 0, off with dt = 0.  C3SC_ERR_UNSUPPORTED for built-in and TABLE models, a model compiled
 * without horizon kernels and a context in game mode.  Honoured by bellman_fibers(_all|_host), policy_fibers(_all|_host) (on the
 * fiber-per-wave kernel: AUTO picks it, a forced pair or quad variant is refused) and the cross calls that launch through them.
 * Refused (C3SC_ERR_UNSUPPORTED): the box calls, cross_iteration_pi and integrate.  set_mca after it keeps delta and recomputes
 * the wave-uniform constants. */
int c3sc_hip_set_horizon_step(c3sc_hip_ctx *ctx, double dt);
/* V_0 .. V_{nstack-1} on the device for c3sc_hip_simulate in horizon mode: ranks is [nstack][d + 1] (each row as
 * c3sc_hip_upload_value's), cores is [nstack][d] host pointers in c3sc_hip_upload_value's layout.  Stages may differ in rank;
 * each is padded to its own instantiation.  nstack = 0 frees the stack.  The uploaded value (upload_value) is untouched.
 * c3sc_hip_simulate in horizon mode with a stack needs dt == delta (to 1e-12 relative) and nsteps <= nstack - 1; the controller
 * of step k uses V_{k+1}; a trajectory still alive after nsteps adds e^{-beta nsteps delta} V_nsteps(x_nsteps) to d_cost (so the
 * mean of J estimates V_0(x_0)), and d_vend is V_nsteps(x_nsteps).  The noise keying is the infinite-horizon rollouts'. */
int c3sc_hip_upload_value_stack(c3sc_hip_ctx *ctx, int nstack, const size_t *ranks, const double *const *cores);

/* Optimal stopping: the controller may end the process at any node and pay a stopping cost psi(x) instead of
 * continuing.  A stopping model's source defines one more function,
 *   __device__ double stopcost(const double *prm, const double *x);
 * and the operator gains one action with the index ncand:
 *     V(x)   = min( psi(x), min_u [plain backup] )                                      (infinite horizon)
 *     V_n(x) = min( psi(x), min_u [ g delta + e^{-beta delta} ( V_self + (delta / h^2) (PV - Q V_self) ) ] )   (horizon mode)
 * The stop action is scanned last and wins by the rule of every other candidate, the first strict '<': the candidate scan runs as
 * it does without it (at beta = 0 with its fraction comparison and single division) and psi is compared once per node with the
 * scan's result.  psi also wins where the scan left no valid candidate: the value is then psi and no longer 0.  uidx is 0..ncand,
 * -1 on absorbed nodes.  Stop raises neither C3SC_STATUS_STATIONARY nor C3SC_STATUS_CFL; the bits the scanned candidates raise
 * are unchanged.  Policy evaluation (policy_fibers*): a forced index ncand yields psi and applies no candidate, any other index
 * applies that candidate and does not compare with psi.  Absorbed and obstacle nodes, the end-point rule and the node memo are
 * unchanged.
 * The stop kernels exist only in run-time compiled models built with c3sc_hip_model_compile_os and stop = 1: the stop forms of
 * the per-wave kernels and of k_rollout at every requested rank, and with fh.horizon = 1 their combined (American) forms as
 * well; k_rollout_ode has none.  stop = 1 with a game or the box returns C3SC_ERR_UNSUPPORTED, a flag other than 0 or 1
 * C3SC_ERR_ARG; stop = 0 is exactly c3sc_hip_model_compile_fh, and the source need not define stopcost then. */
typedef struct c3sc_hip_model_spec_os {
    c3sc_hip_model_spec_fh fh;
    int stop;
} c3sc_hip_model_spec_os;
int c3sc_hip_model_compile_os(const c3sc_hip_model_spec_os *spec, int *model_id);
int c3sc_hip_model_code_object_os(const c3sc_hip_model_spec_os *spec, void *buf, size_t *size);
/* stopping on (on != 0) or off.  C3SC_ERR_UNSUPPORTED for built-in and TABLE models, a model compiled without stop kernels (also
 * one set after this call: the launch then refuses) and a context in game mode; c3sc_hip_set_game is refused while stopping is
 * on.  Honoured by bellman_fibers(_all|_host), policy_fibers(_all|_host) (on the fiber-per-wave kernel: AUTO picks it, a forced
 * pair or quad variant is refused), the cross calls that launch through them, and simulate.  With the horizon step set as well
 * the launches take the combined form, which needs a model compiled with both flags.  Refused (C3SC_ERR_UNSUPPORTED): the box
 * and TABLE calls, cross_iteration_pi and integrate.
 * c3sc_hip_simulate with stopping on: a trajectory whose controller returns the stop action at step k stops there, pays
 * e^{-beta k dt} psi(x_k) and is frozen like an exited one; its saved controls from k on are 0.  With wrap_periodic psi is taken
 * at the wrapped state, the one the controller compared it at (stage and exit costs are charged at the state itself).  d_exit tells the two apart:
 * an exit keeps its step k >= 0, "never" stays -1, a voluntary stop at step k is stored as -(k + 2).  In horizon mode under a
 * value stack the decision at step k uses V_{k+1}, as the controls do, and a trajectory alive after nsteps still adds the
 * discounted V_nsteps. */
int c3sc_hip_set_stopping(c3sc_hip_ctx *ctx, int on);

/* Jump diffusions: dx = b dt + sigma dw + a compound-Poisson term with intensity lambda(x) whose mark
 * distribution is discretised into M atoms, 1 <= M <= C3SC_JUMP_MAX.  A jump model's source defines two more functions,
 *   __device__ double jumprate(const double *prm, const double (&x)[C3SC_D]);                          lambda(x) >= 0
 *   __device__ double jump(const double *prm, const double (&x)[C3SC_D], int m, double (&y)[C3SC_D]);  y = x + q_m(x), returns pi_m(x)
 * with weights pi_m >= 0 that sum to 1 over m = 0 .. M-1; neither may depend on the control.  The chain is the rate form of
 * Kushner and Dupuis, section 5.6: a jump is one more transition with the un-normalised rate h^2 lambda(x),
 *     Q0 += h^2 lambda,   PV0 = fma(h^2 lambda, J, PV0),   J(x) = sum_m pi_m(x) Vjump(y_m)   (m ascending, one fma chain from 0.0)
 * and everything downstream is the backup of the other switches: dt = h^2 / Q with the jump rate inside Q; in horizon mode the
 * term delta lambda (J - V_self), with the rate in the CFL test; a node with b = sigma = 0 and lambda > 0 is not STATIONARY;
 * the forced (policy) path uses the same Q0 and PV0.  lambda = 0 leaves every bit of the backup without jumps.
 * Vjump(y): periodic dimensions of y are wrapped into [lb, ub); a target inside an obstacle, or outside [lb, ub] on an absorbing
 * dimension, pays obscost(y) resp. boundcost(y) (the choice c3sc_hip_simulate's exit test makes); any other target pays the
 * interpolant of c3sc_hip_stencil_points at y -- multilinear, or the nearer node under c3sc_hip_set_interp(ctx, 1) -- clamped to
 * the grid hull, so reflecting dimensions clamp.
 * The jump kernels exist only in run-time compiled models built with c3sc_hip_model_compile_jd and njump = M > 0: the jump forms
 * of the per-wave kernels and of k_rollout that the other flags select (plain, horizon, stop, horizon with stop) at every
 * requested rank; k_rollout_ode has none.  njump = 0
 * is exactly c3sc_hip_model_compile_os, and the source need not define the two functions then; njump outside 0..C3SC_JUMP_MAX
 * returns C3SC_ERR_ARG, njump > 0 with a game or the box C3SC_ERR_UNSUPPORTED. */
#define C3SC_JUMP_MAX 8
typedef struct c3sc_hip_model_spec_jd {
    c3sc_hip_model_spec_os os;
    int njump;
} c3sc_hip_model_spec_jd;
int c3sc_hip_model_compile_jd(const c3sc_hip_model_spec_jd *spec, int *model_id);
int c3sc_hip_model_code_object_jd(const c3sc_hip_model_spec_jd *spec, void *buf, size_t *size);
/* jumps on (on != 0) or off.  C3SC_ERR_UNSUPPORTED for built-in and TABLE models, a model compiled without jump kernels (also
 * one set after this call: the launch then refuses) and a context in game mode; c3sc_hip_set_game is refused while jumps are on.
 * Honoured by bellman_fibers(_all|_host), policy_fibers(_all|_host) (on the fiber-per-wave kernel: AUTO picks it, a forced pair
 * or quad variant is refused), the cross calls that launch through them, cross_iteration_pi included, and simulate.  Combines
 * with the horizon step and the stopping switch; the model must then be compiled with those flags as well.  Refused
 * (C3SC_ERR_UNSUPPORTED): the box and TABLE calls and integrate.
 * c3sc_hip_simulate with jumps on: the controller's backup gets the jump term at the state it sees, and the step adds a
 * compound-Poisson increment evaluated at x_k like the Euler-Maruyama increment.  Two uniforms per (seed, trajectory, step)
 * come from a Philox counter component no normal uses (c3sc_hip_jump_uniforms is the host twin), with caller-supplied normals
 * too; the diffusion noise of a run keeps its bits.  A jump happens when u0 < min(lambda(x_k) dt, 1); its mark is the first m
 * with u1 < pi_0 + .. + pi_m (the last mark catches rounding); x_{k+1} = x_k + b dt + sigma sqrt(dt) xi + (y_m(x_k) - x_k).  A
 * trajectory that jumps out of the domain is an exit at step k + 1 like any other. */
int c3sc_hip_set_jumps(c3sc_hip_ctx *ctx, int on);
/* out[0], out[1] = the uniforms (u0, u1) in (0, 1) of step `step` of global trajectory `traj` under `seed` */
int c3sc_hip_jump_uniforms(uint64_t seed, uint64_t traj, uint64_t step, double *out);

/* Impulse control: besides steering through drift and diffusion the controller may at any state pay k_m(x) and
 * move the state at once to y_m(x), m = 0 .. M-1, 1 <= M <= C3SC_IMPULSE_MAX.  An impulse model's source defines one more function,
 *   __device__ double impulse(const double *prm, const double (&x)[C3SC_D], int m, double (&y)[C3SC_D]);  y = y_m(x), returns k_m(x)
 * which may not depend on the control.  A return value that is not finite means "intervention m is not admissible at x": it
 * never wins (y is not used then).  The operator is the quasi-variational inequality
 *     V(x) = min( min_u backup_u(x),  min_m [ k_m(x) + Vt(y_m(x)) ] )
 * with Vt exactly the Vjump of the jump kernels above: periodic wrap, obscost / boundcost at a target inside an obstacle or
 * beyond an absorbing face, otherwise the interpolant of c3sc_hip_set_interp clamped to the grid hull.  The interventions are
 * scanned after the candidates, m ascending, and compared by the rule of every candidate, the first strict '<'; they also win
 * where the scan left no valid candidate.  Intervention m has the index ncand + 1 + m -- ncand stays the stop action's -- so
 * uidx is 0 .. ncand-1 or ncand+1 .. ncand+M, and -1 on absorbed nodes.  A forced index ncand + 1 + m applies intervention m and
 * no candidate; a forced index above ncand + M names nothing and gives 0.0 and -1, as an out-of-range candidate index does.
 * No status bit is raised.
 * The impulse kernels exist only in run-time compiled models built with c3sc_hip_model_compile_ic and nimpulse = M > 0: the
 * impulse forms of the per-wave kernels and of k_rollout for the plain model and, with njump > 0, for the jump model too;
 * k_rollout_ode has none.  nimpulse = 0 is exactly c3sc_hip_model_compile_jd, and the source need not define impulse then;
 * nimpulse outside 0..C3SC_IMPULSE_MAX returns C3SC_ERR_ARG, nimpulse > 0 with a game, the box, horizon or stop
 * C3SC_ERR_UNSUPPORTED.  The source may read C3SC_NIMPULSE. */
#define C3SC_IMPULSE_MAX 8
typedef struct c3sc_hip_model_spec_ic {
    c3sc_hip_model_spec_jd jd;
    int nimpulse;
} c3sc_hip_model_spec_ic;
int c3sc_hip_model_compile_ic(const c3sc_hip_model_spec_ic *spec, int *model_id);
int c3sc_hip_model_code_object_ic(const c3sc_hip_model_spec_ic *spec, void *buf, size_t *size);
/* interventions on (on != 0) or off.  C3SC_ERR_UNSUPPORTED for built-in and TABLE models, a model compiled without impulse
 * kernels (also one set after this call: the launch then refuses), a context in game mode, and while the horizon step or the
 * stopping switch is set; c3sc_hip_set_game, c3sc_hip_set_horizon_step and c3sc_hip_set_stopping are refused while it is on.
 * Honoured by bellman_fibers(_all|_host), policy_fibers(_all|_host) (on the fiber-per-wave kernel: AUTO picks it, a forced pair
 * or quad variant is refused), the value-iteration cross calls that launch through them, and simulate.  Combines with
 * c3sc_hip_set_jumps; the model must then be compiled with njump > 0 as well.  Refused (C3SC_ERR_UNSUPPORTED): the box and TABLE
 * calls, cross_iteration_pi and integrate.
 * c3sc_hip_simulate with interventions on: the time of step s is s dt throughout, so an intervention occupies one step slot.
 * A live trajectory whose controller returns ncand + 1 + m at step s pays exp(-beta s dt) k_m(xin), xin the state the controller
 * saw (wrapped under wrap), pays no stage cost and takes no drift, diffusion or Poisson increment in that step, and continues
 * from x_{s+1} = y_m(xin); its saved control of that step is 0.  The exit test of x_{s+1} is the ordinary one at the top of step
 * s + 1, and exit_step is as without interventions: they are visible in the saved trajectory.  The continuous-time problem
 * intervenes in no time, so each intervention delays the clock of its trajectory by dt: an O(dt) error per intervention in the
 * discounting and in the time left, which vanishes with the step. */
int c3sc_hip_set_impulses(c3sc_hip_ctx *ctx, int on);

/* Correlated noise: diffusions whose covariance sigma sigma^T has off-diagonal entries, after Kushner and Dupuis,
 * section 5.3.  A model declares P unordered pairs (i_p, j_p), i_p < j_p < d, no pair twice, 1 <= P <= C3SC_CORR_MAX, in
 * corr_dims = {i_0, j_0, i_1, j_1, ...}, and its source defines one more function,
 *   __device__ double covar(const double *prm, const double (&x)[C3SC_D], int p);     a_p(x) = (sigma sigma^T)_{i_p j_p}(x)
 * which does not read the control.  Contract: the diffusion of a paired dimension must not read the control either (sigma's
 * entries of i_p and j_p are taken at the first candidate for the dominance test below).  The source may read C3SC_NCORR, and
 * C3SC_CORR_I / C3SC_CORR_J, the comma-separated dimension lists.
 * With t_m = h^2 / h_m, for each pair in ascending p:
 *     r_p = (t_i t_j / h^2) |a_p| / 2
 * is the un-normalised rate to each of two diagonal neighbours -- (+,+) and (-,-) where a_p > 0, (+,-) and (-,+) where
 * a_p < 0 -- and the same r_p is taken off each of the four axis rates of i and j.  All of it is linear in the rates:
 *     Q0 += sum_p (-2 r_p),   PV0 += sum_p r_p [(V_d1 + V_d2) - ((V[2i] + V[2i+1]) + (V[2j] + V[2j+1]))]   (one fma chain from 0.0)
 * and everything downstream is the backup of the other switches: dt = h^2 / Q with the corrected Q, the explicit scheme and its
 * CFL test in horizon mode, the forced (policy) path; the stationary test is unchanged.  a_p = 0 leaves every bit of the backup
 * without the term.
 * A diagonal neighbour is a grid node and pays the function train's value there.  In each of the two dimensions its index is
 * the axis stencil's for a fixed dimension -- of the fiber's varying dimension too: i - 1 / i + 1; at a reflecting end the node
 * itself; across the periodic seam n - 2 / 1; on an absorbing face the node itself.  No exit test, no obstacle cost and no
 * interpolation: the bits do not depend on c3sc_hip_set_interp.
 * Dominance: the transition probabilities along dimension m are non-negative iff t2_m sigma_m^2 / 2 >= sum_{p with m} r_p
 * (t2_m = h^2 / h_m^2).  A live node that violates it raises C3SC_STATUS_DOMINANCE; the backup still returns the algebra's value,
 * as with C3SC_STATUS_CFL.
 * The corr kernels exist only in run-time compiled models built with c3sc_hip_model_compile_cd and ncorr = P > 0: the corr forms
 * of the per-wave kernels that the other flags select (plain, horizon, stop, njump and their combinations) at every requested
 * rank; k_rollout and k_rollout_ode have none.  ncorr = 0 is exactly c3sc_hip_model_compile_ic, and the source need not define
 * covar then.  C3SC_ERR_ARG: ncorr outside 0..C3SC_CORR_MAX, a dimension out of range, i >= j, a repeated pair;
 * C3SC_ERR_UNSUPPORTED: ncorr > 0 with a game, the box or nimpulse > 0. */
#define C3SC_CORR_MAX 8
typedef struct c3sc_hip_model_spec_cd {
    c3sc_hip_model_spec_ic ic;
    int ncorr;
    int corr_dims[2 * C3SC_CORR_MAX];
} c3sc_hip_model_spec_cd;
int c3sc_hip_model_compile_cd(const c3sc_hip_model_spec_cd *spec, int *model_id);
int c3sc_hip_model_code_object_cd(const c3sc_hip_model_spec_cd *spec, void *buf, size_t *size);
/* correlation on (on != 0) or off.  C3SC_ERR_UNSUPPORTED for built-in and TABLE models, a model compiled without corr kernels
 * (also one set after this call: the launch then refuses) and a context in game or impulse mode; c3sc_hip_set_game and
 * c3sc_hip_set_impulses are refused while it is on.  Honoured by bellman_fibers(_all|_host), policy_fibers(_all|_host) (on the
 * fiber-per-wave kernel: AUTO picks it, a forced pair or quad variant is refused) and the cross calls that launch through them.
 * Combines with the horizon step, the stopping switch and c3sc_hip_set_jumps; the model must then be compiled with those flags
 * as well.  Refused (C3SC_ERR_UNSUPPORTED): the box and TABLE calls, simulate and integrate -- a correlated rollout needs
 * correlated increments and off-grid diagonal targets, which are not offered. */
int c3sc_hip_set_correlation(c3sc_hip_ctx *ctx, int on);

/* The Markov chain of a run-time compiled model's own backup.  chain = 1 adds, per requested rank, the walk and
 * the outcomes kernel of c3sc_hip_simulate_chain, c3sc_hip_chain_transitions and c3sc_hip_chain_outcomes, in the plain form and in
 * every subset of {horizon, stop, jump} among the spec's features; game, impulse and corr features are allowed and add no chain
 * kernel (the chain calls stay refused in those modes).  chain = 0 is exactly c3sc_hip_model_compile_cd: the same model id and
 * code object, and a model the chain calls refuse.  C3SC_ERR_ARG: chain outside {0, 1}.
 *
 * The chain of a form, at a live node: the decision is the backup's (with jumps: jump_term under c3sc_hip_set_interp's class).
 * With p_k the winner's 2d upwind rates, rJ = h^2 lambda(x) (0 without jumps), pi_m the mark weights and C = sum p_k + rJ, the
 * outcomes are, in this order: the 2d axis neighbours (weights p_k), the marks m ascending (weights rJ pi_m) and, in horizon mode
 * only, the self-loop (weight W - C).  The total is W = C and the interval dt = h^2 / C without the horizon; W = h^2 / delta and
 * dt = delta with it.  J += D g dt, T += dt, D *= exp(-beta dt) as in the plain chain; then the outcome is the first k with
 * v W < c_k (cumulative weights in outcome order), else the last k with a positive weight, so a negative self-loop weight (the
 * backup raises C3SC_STATUS_CFL) is never drawn.  Stuck nodes: without the horizon a live node with no valid candidate or
 * C < 1e-14, rJ inside C; in horizon mode none.
 * A mark outcome m at step s has the target y = jump(x, m) with periodic coordinates wrapped.  If y lies inside an obstacle, or
 * outside [lb, ub] on an absorbing dimension, the walk pays D_{s+1} (obscost | boundcost)(y) -- D after the interval -- its exit
 * word is s + 1 and it stays at its node.  Otherwise it lands on a node of y's grid cell (clamped to the hull): with whi the
 * interpolation weight of the upper node of dimension m and t = u1 at the start, for m ascending the upper node is taken iff
 * t < whi, and then t = t / whi if it was taken, else t = (t - whi) / (1 - whi).  Under c3sc_hip_set_interp(ctx, 1) whi is 0 or 1
 * and the walk lands on the nearer node.  The expectation of V over the corners is the interpolant the backup used.
 * Stop: where the decision is the stop action (uidx = ncand) the walk pays D psi(x) and is frozen with the exit word
 * C3SC_CHAIN_STOPPED(s); a saved decision row holds ncand there.  The transitions report uidx = ncand, dt = 0, P = 0,
 * value = stage = psi.
 * Horizon mode needs the value stack (c3sc_hip_upload_value_stack) with nsteps + 1 <= nstack, as c3sc_hip_simulate does: one
 * launch per step, step s decides with V_{s+1}, d_vend = V_nsteps(xi_nsteps); J is not topped up with the terminal value.
 * c3sc_hip_chain_transitions and c3sc_hip_chain_outcomes use the uploaded value: one stage of the operator.
 * Uniforms: with jumps on, d_uniform is [n][nsteps][2] = (v, u1); Philox supplies both values of c3sc_hip_jump_uniforms.
 *
 * c3sc_hip_chain_outcomes: c3sc_hip_chain_transitions' outputs and d_pself [n], d_pmark [n*M] (the probabilities w / W) and
 * d_markval [n*M] = Vjump(y_m) (what a jump to y_m pays in the backup), each NULL or given; M = njump, and without jumps
 * d_pmark and d_markval must be NULL.  Over axis neighbours, marks and self-loop the probabilities of a moving node sum to one.
 * Run-time compiled models with chain kernels only (C3SC_ERR_UNSUPPORTED otherwise). */
#define C3SC_CHAIN_STOPPED(s) (-((int64_t)(s) + 2) - ((int64_t)1 << 32))
typedef struct c3sc_hip_model_spec_mc {
    c3sc_hip_model_spec_cd cd;
    int chain;
} c3sc_hip_model_spec_mc;
int c3sc_hip_model_compile_mc(const c3sc_hip_model_spec_mc *spec, int *model_id);
int c3sc_hip_model_code_object_mc(const c3sc_hip_model_spec_mc *spec, void *buf, size_t *size);
/* 1 if model_id names a model compiled with chain = 1, else 0 */
int c3sc_hip_model_has_chain(int model_id);
int c3sc_hip_chain_outcomes(c3sc_hip_ctx *ctx, size_t n, const int32_t *d_nodes, int32_t *d_uidx, double *d_value, double *d_stage,
                            double *d_dt, double *d_P, int32_t *d_flag, double *d_pself, double *d_pmark, double *d_markval,
                            void *stream);
int c3sc_hip_chain_outcomes_host(c3sc_hip_ctx *ctx, size_t n, const int32_t *nodes, int32_t *uidx, double *value, double *stage,
                                 double *dt, double *P, int32_t *flag, double *pself, double *pmark, double *markval);

int c3sc_hip_sync(c3sc_hip_ctx *ctx, void *stream);
int c3sc_hip_get_status(c3sc_hip_ctx *ctx, unsigned *flags, int clear);
/* name of the kernel the last launch used (for profiles) */
const char *c3sc_hip_last_kernel(const c3sc_hip_ctx *ctx);

/* diagnostic builds only (C3SC_DBG & 128): per-wave segment cycle sums written by the kernels */
int c3sc_hip_debug_read(c3sc_hip_ctx *ctx, unsigned long long *out, size_t n);
/* diagnostics: Bellman / policy / stencil kernel launches made by this process so far (the reference calls its fiber
 * callback once per fiber, bellman.c:1295; here one launch serves a batch -- this counts them) */
unsigned long long c3sc_hip_launch_count(void);
/* ... and how many of them ran a fiber-pair kernel with the three-core product tables (tests: C3SC_PAIR_TABLE3=0 switches them off) */
unsigned long long c3sc_hip_table3_launch_count(void);
/* tests: the last partition a fiber-pair launch ran in scratch block `slot` (0: the caller's stream and the single-launch entry
 * points; 1, 2: the side streams of c3sc_hip_bellman_fibers_all).  Synchronises that launch's stream, then copies perm[F] (fiber
 * of every tile position: live fibers first, grouped by the fold's key levels, dead ones last) into `perm` (cap entries; NULL: not
 * wanted) and reports F and the number of live fibers.  An error if no partition has run on the slot. */
int c3sc_hip_last_partition(c3sc_hip_ctx *ctx, int slot, int32_t *perm, size_t cap, size_t *F, int *nlive);

/* device-side timing on `stream` with HIP events (used by bench.py's roofline leg) */
int c3sc_hip_timer_start(c3sc_hip_ctx *ctx, void *stream);
int c3sc_hip_timer_stop(c3sc_hip_ctx *ctx, void *stream, float *ms);

/* FP64 micro-benchmarks used to confirm the peaks quoted in DESIGN.md (results in TFLOP/s) */
int c3sc_hip_peak_fma_f64(c3sc_hip_ctx *ctx, double *tflops);
int c3sc_hip_peak_mfma_f64(c3sc_hip_ctx *ctx, double *tflops);

#ifdef __cplusplus
}
#endif
#endif
