/* c3sc_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain C99, scalar, single thread) of the Bellman-backup hot path of
 * goroda/c3sc: src/bellman.c + src/valuefunc.c + src/nodeutil.c + src/hashgrid.c +
 * src/boundary.c (only the functions SURVEY.md section 8a lists).  Each function cites the
 * reference file:line it follows.  No reference source text is included or copied: the
 * algorithms are restated from reading the reference.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this
 * library, and only as the checker.  The product (c3sc_amd/) never links, loads or calls it.
 *
 * Pinning status: the reference itself is unbuildable in this image (it needs the absent
 * third-party C3 headers/library, cdyn and CBLAS), so this restatement is pinned by
 *   (1) the known-answer tests the reference's own test-suite holds for this path
 *       (test/transition_prob/tprob_test.c; restated in tests/test_oracle_pins.py), and
 *   (2) the outputs of the real reference recorded in SURVEY.md section 10.6
 *       (tests/golden/survey_known_answers.json).
 * Behaviour that lives in C3 (c3opt BRUTEFORCE scan order / tie-break, ftapprox_cross)
 * is "parity unpinned": see DESIGN.md.
 */
#ifndef C3SC_ORACLE_H
#define C3SC_ORACLE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enum EBTYPE, boundary.h:42-47 */
enum orc_ebtype { ORC_EB_NONE = 0, ORC_ABSORB = 1, ORC_PERIODIC = 2, ORC_REFLECT = 3 };

/* ------------------------------------------------------------------ nodeutil.c ---- */
int orc_transition_assemble(size_t dx, size_t du, size_t dw, double h, const double *hvec,
                            const double *drift, const double *grad_drift,
                            const double *ddiff, const double *grad_ddiff,
                            double *prob, double *grad_prob, double *dt, double *grad_dt,
                            double *space);
int orc_transition_assemble_old(size_t dx, size_t du, size_t dw, double h, const double *hvec,
                                const double *drift, const double *grad_drift,
                                const double *ddiff, const double *grad_ddiff,
                                double *prob, double *grad_prob, double *dt, double *grad_dt,
                                double *space);
size_t orc_convert_x_to_ind(double x, size_t N, const double *grid);
int orc_convert_fiber_to_ind(size_t d, size_t N, const double *x, const size_t *Ngrid,
                             const double *const *xgrid, size_t *fixed_ind, size_t *dim_vary);

/* ------------------------------------------------------------------ boundary.c ---- */
struct orc_boundary; /* external BC type per dim + axis-aligned box obstacles */
struct orc_boundary *orc_boundary_alloc(size_t d, const double *lb, const double *ub);
void orc_boundary_free(struct orc_boundary *b);
int orc_boundary_external_set_type(struct orc_boundary *b, size_t dim, const char *type);
int orc_boundary_add_obstacle(struct orc_boundary *b, const double *center, const double *lengths);
enum orc_ebtype orc_boundary_type_dim(const struct orc_boundary *b, size_t dim, int right);
int orc_boundary_in_obstacle(const struct orc_boundary *b, const double *x);
void orc_boundary_set_consistent_ends(struct orc_boundary *b, int on); /* not the reference's behaviour: see the .c file */
size_t orc_boundary_get_nobs(const struct orc_boundary *b);
const double *orc_boundary_obstacle_lb(const struct orc_boundary *b, size_t i);
const double *orc_boundary_obstacle_ub(const struct orc_boundary *b, size_t i);

int orc_process_fibers_neighbor(size_t d, const size_t *fixed_ind, size_t dim_vary,
                                const double *x, int *absorbed, size_t *neighbors_vary,
                                size_t *neighbors_fixed, const size_t *ngrid,
                                const struct orc_boundary *bound);

/* ----------------------------------------------------------------- valuefunc.c ---- */
/* Nodal function-train value function: cores[m][j*r_m*r_{m+1} + a + b*r_m]. */
struct orc_valuef;
struct orc_valuef *orc_valuef_create(size_t d, const size_t *N, const size_t *ranks /* d+1 */,
                                     const double *const *cores);
void orc_valuef_destroy(struct orc_valuef *vf);
double orc_valuef_eval_ind(const struct orc_valuef *vf, const size_t *ind); /* brute-force chain */
int orc_valuef_eval_fiber_ind_nn(struct orc_valuef *vf, const size_t *fixed_ind, size_t dim_vary,
                                 const size_t *neighbors, const size_t *neighbors_vary, double *out);
int orc_mca_get_neighbor_costs(size_t d, size_t N, const double *x, const struct orc_boundary *bound,
                               struct orc_valuef *vf, const size_t *ngrid, const double *const *xgrid,
                               size_t *fixed_ind, size_t *dim_vary, int *absorbed, double *out);

/* ------------------------------------------------------------------- bellman.c ---- */
double orc_bellmanrhs(size_t dx, size_t du, double stage_cost, const double *stage_grad,
                      double discount, const double *prob, const double *prob_grad, double dt,
                      const double *dtgrad, const double *cost, double *grad);
void orc_mca_grid_refs(size_t dx, double hmin, const double *hvec, double *h2, double *t /* 2dx */);
double *orc_linspace(double lb, double ub, size_t N); /* C3 array helper as used by bellman.c:1977 */

/* ------------------------------------------------------------------ hashgrid.c ---- */
char *orc_size_t_a_to_char(const size_t *arr, size_t n, char *buffer /* >=256 */);
size_t orc_hashchar(size_t size, const char *str);
struct orc_htable;
struct orc_htable *orc_htable_create(size_t size);
void orc_htable_destroy(struct orc_htable *ht);
int orc_htable_add_element(struct orc_htable *ht, const char *key, const double *data, size_t N);
double *orc_htable_get_element(struct orc_htable *ht, const char *key, size_t *N);
size_t orc_htable_count(const struct orc_htable *ht);

/* ------------------------------------------------- problem callbacks (dynamics.h) -- */
typedef int (*orc_drift_fn)(double t, const double *x, const double *u, double *out, double *jac, void *args);
typedef int (*orc_diff_fn)(double t, const double *x, const double *u, double *out, double *grad, void *args);
typedef int (*orc_stage_fn)(double t, const double *x, const double *u, double *out, double *grad);
typedef int (*orc_bound_fn)(double t, const double *x, double *out);
typedef int (*orc_obs_fn)(const double *x, double *out);

/* Built-in problem models: C restatement of the examples' callbacks (model ids shared with
 * include/c3sc_hip.h).  params meaning is documented in oracle/c3sc_oracle.c. */
enum orc_model {
    ORC_MODEL_DUBINS3D = 1, /* examples/dubinscar_new/dubinscar.c:40-121 */
    ORC_MODEL_SCAR4D = 2,   /* examples/skidding_car/scar.c:40-169       */
    ORC_MODEL_CAR7D = 3,    /* synthetic 7-D car, SURVEY.md 8d config C4  */
    ORC_MODEL_LQGND = 4,    /* examples/lqgnd/lqgnd.c:80-198 (dim=2: lqg2d_new/lqg2d.c:72-153) */
    ORC_MODEL_CHAIN = 5,    /* examples/double_int/double_int.c:80-157; params[2]=1 -> stage sum x^2 */
    ORC_MODEL_ROSSLER3D = 6, /* examples/rossler/rossler.c:80-157 */
    ORC_MODEL_PERCH7D = 8,   /* examples/perching/perch.c:36-273 */
    ORC_MODEL_SKID5D = 9,    /* examples/skidding5d/scar.c:39-176 (Q13: the diffusion callback writes out[28] of a 25-element matrix) */
    ORC_MODEL_COTHRUST6D = 10, /* examples/cothrust2/copterposethrust.c:40-222 */
    ORC_MODEL_TPROB3D = 7    /* test/transition_prob/tprob_test.c: f3 :223-251, s2 :197-220, stagecost3d :273-300, boundcost, ocost */
};
int orc_model_dims(int model, const double *params, size_t *dx, size_t *du);
int orc_model_drift(int model, const double *params, const double *x, const double *u, double *out);
int orc_model_diff_diag(int model, const double *params, const double *x, const double *u, double *out);
int orc_model_stage(int model, const double *params, const double *x, const double *u, double *out);
int orc_model_boundcost(int model, const double *params, const double *x, double *out);
int orc_model_obscost(int model, const double *params, const double *x, double *out);

/* ------------------------------------------- one fiber of the Bellman operator ---- */
/* Problem bundle = C3Control + brute-force c3Opt restated (bellman.c:1942-1999, 293-349). */
struct orc_problem;
struct orc_problem *orc_problem_create(size_t dx, size_t du, size_t dw, const double *lb, const double *ub,
                                       const size_t *ngrid, double discount);
void orc_problem_destroy(struct orc_problem *p);
struct orc_boundary *orc_problem_boundary(struct orc_problem *p);
const double *orc_problem_xgrid(const struct orc_problem *p, size_t dim);
double orc_problem_h2(const struct orc_problem *p);
const double *orc_problem_t(const struct orc_problem *p);
void orc_problem_set_model(struct orc_problem *p, int model, const double *params, size_t nparams);
void orc_problem_set_callbacks(struct orc_problem *p, orc_drift_fn b, void *bargs, orc_diff_fn s, void *sargs,
                               orc_stage_fn stage, orc_bound_fn bound, orc_obs_fn obs);
void orc_problem_set_bruteforce(struct orc_problem *p, size_t ncand, const double *cands /* ncand*du */);
void orc_problem_set_value(struct orc_problem *p, struct orc_valuef *vf); /* borrowed */
void orc_problem_increment_vi_iter(struct orc_problem *p);
void orc_problem_reset_vi_htable(struct orc_problem *p);
size_t orc_problem_nnode_evals(const struct orc_problem *p);

/* bellman_vi (bellman.c:1295-1423): x is N x dx row-major, one grid fiber. uidx (may be NULL)
 * receives the winning candidate index per node (-1 for absorbed nodes, -2 for memo hits). */
int orc_bellman_vi(struct orc_problem *p, size_t N, const double *x, double *out, int *uidx, int use_memo);

/* Batch driver used by tests/bench: F fibers along dim k with fixed indices idx[F*dx]
 * (entry k ignored); builds x and calls orc_bellman_vi per fiber, memo disabled.
 * absorbed_out (may be NULL) F*N ints. */
int orc_bellman_fibers(struct orc_problem *p, size_t k, size_t F, const int *idx, double *out, int *uidx,
                       int *absorbed_out);
/* Policy iteration (bellman.c:1702-1886, 2214-2262, 2343-2407).  p's value is vf_iteration; vf_policy is the value
 * function the policy is greedy for.  uidx (may be NULL): candidate applied per node (-1 absorbed, -2 taken from the
 * cached [prob, dt, stage] of this pi_iter). */
void orc_problem_pi_begin(struct orc_problem *p);      /* c3control_pi_solve head: ++pi_iter, reset both tables */
void orc_problem_pi_step_begin(struct orc_problem *p); /* c3control_step_pi head: ++pi_subiter, zero the counters */
size_t orc_problem_npol_evals(const struct orc_problem *p);
size_t orc_problem_niter_node_evals(const struct orc_problem *p);
int orc_bellman_pi(struct orc_problem *p, struct orc_valuef *vf_policy, size_t N, const double *x, double *out, int *uidx);
int orc_policy_fibers(struct orc_problem *p, struct orc_valuef *vf_policy, size_t k, size_t F, const int *idx, double *out,
                      int *uidx);
/* ---- policy simulation tail ---- */
double orc_valuef_eval(const struct orc_valuef *vf, const double *const *xgrid, const double *x); /* valuefunc.c:337-343 */
int orc_mca_get_neighbor_node_costs(size_t d, const double *x, const struct orc_boundary *bound, const struct orc_valuef *vf,
                                    const size_t *ngrid, const double *const *xgrid, int *absorbed, double *out); /* nodeutil.c:718-816 */
int orc_policy_eval(struct orc_problem *p, const double *x, int *uidx, double *val); /* bellman.c:2105-2158 */
/* Same for the FT stencil only: out F*N*(2dx+1). */
int orc_stencil_fibers(struct orc_problem *p, size_t k, size_t F, const int *idx, double *out, int *absorbed_out);
/* The value of every candidate at every node: q F*N*ncand (an absorbed node: its cost in every column), so that a test can
 * tell how far the runner-up of orc_bellman_fibers' minimum lies from it.  Fails (101) where orc_bellman_fibers does. */
int orc_q_fibers(struct orc_problem *p, size_t k, size_t F, const int *idx, double *q, int *absorbed_out);

/* The fiber callbacks in the cross approximation's ABI (valuefunc.c:615-616); args points to a struct orc_cb_args. */
struct orc_cb_args { struct orc_problem *p; struct orc_valuef *policy; int use_memo; size_t ncalls; };
int orc_cb_bellman_vi(size_t N, const double *x, double *out, void *args); /* bellman_vi, bellman.h:96  */
int orc_cb_bellman_pi(size_t N, const double *x, double *out, void *args); /* bellman_pi, bellman.h:105 */

#ifdef __cplusplus
}
#endif
#endif
