// ctx.hpp -- the device context behind the C-ABI handle (shared by c3sc_hip.hip and cross_device.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/c3sc_hip.h"
#include "kernel_common.hpp"

struct c3sc_cross_dev; // cross_device.hip: device-resident state of the cross-approximation core steps
struct c3sc_hip_comm;  // comm_rccl.hip: RCCL communicator (one process per GPU)

struct c3sc_hip_ctx {
    int device = 0;
    std::string err;
    // host copy of the static problem description
    int d = 0;
    int ngrid[c3sc::MAXD] = {0};
    std::vector<double> xgrid_flat;
    int xg_off_rel[c3sc::MAXD] = {0};
    int bctype[c3sc::MAXD] = {0};
    int cends = 0; // c3sc_hip_set_consistent_ends
    bool have_boundary = false;
    int nobs = 0;
    std::vector<double> obs; // [nobs][2][d]
    bool have_mca = false;
    double h2 = 0, discount = 0, t[2 * c3sc::MAXD] = {0};
    int model = 0;
    double prm[C3SC_MAX_PARAMS] = {0};
    int ncand = 0, du = 0;
    bool cands_placeholder = false; // the single zero row set_control_box puts where no list was set (nothing reads it in box mode)
    std::vector<double> cands;
    // zero-sum game (c3sc_hip_set_game): cands is the product list, game_ngrp groups of game_gsz; game_gsz = 0: no game
    int game_gsz = 0, game_ngrp = 0, game_order = 0;
    // finite horizon (c3sc_hip_set_horizon_step): the step delta (0: off); {delta, exp(-beta delta), delta / h^2} sit at hz_off of
    // the static section.  The value stack (c3sc_hip_upload_value_stack): one buffer [static copy | stage 0 cores | stage 1 ...]
    // laid out for a static section of hz_stack_static doubles; stage s padded to hz_rp[s], its cores at hz_core_off[s * MAXD + m]
    double hz_dt = 0.0;
    int hz_off = 0;
    // the switches that carry no data (c3sc_hip_set_stopping / _jumps / _impulses / _correlation): FORM_STOP | FORM_JUMP |
    // FORM_IMPULSE | FORM_CORR.  The launches take that form of the run-time compiled model's kernels; ctx_form() below is the
    // whole mask
    unsigned switches = 0;
    double *hz_stack = nullptr;
    size_t hz_stack_static = 0;
    int hz_nstack = 0;
    std::vector<int> hz_rp;
    std::vector<long> hz_core_off;
    // continuous controls (c3sc_hip_set_control_box)
    int box_du = 0, box_grid = 0, box_polish = 0;
    double box_lb[C3SC_MAX_DU] = {0}, box_ub[C3SC_MAX_DU] = {0};
    // value function
    bool have_value = false;
    size_t ranks[c3sc::MAXD + 1] = {0};
    int rp = 0;
    // device arena: [xgrid | obs | cands | pad | cores]
    double *arena = nullptr;
    size_t arena_cap = 0;     // doubles
    size_t static_doubles = 0; // size of the static section the arena was laid out with
    bool static_dirty = true;
    long core_off[c3sc::MAXD] = {0};
    long coreT_off[c3sc::MAXD] = {0}, aop_off[c3sc::MAXD] = {0}; // fiber-quad copies of the middle cores (0 = none)
    long img_off[c3sc::MAXD] = {0};                        // fiber-pair LDS images of all cores (padded node stride)
    long qimgL_off[c3sc::MAXD] = {0}, qimgR_off[c3sc::MAXD] = {0}; // fiber-quad-duo LDS images (node stride elems + 2)
    long tabL_off = 0, tabR_off = 0;                       // fiber-pair product tables of the two outer cores of each side (0 = none)
    // ... and of the three outer cores (kernel_common.hpp: pair_tab3L_off; 0 = not reserved).  Built lazily: an upload marks them
    // stale, the first launch that runs a three-core kernel enqueues the build on its stream (ensure_tab3) and records tab3_ev; a
    // later launch on another stream waits for that event
    long tab3L_off = 0, tab3R_off = 0;
    bool tab3_stale = true;
    hipStream_t tab3_stream = nullptr;
    hipEvent_t tab3_ev = nullptr;
    int obs_off = 0, cands_off = 0, tab_off[4] = {0, 0, 0, 0}, cfeat_off = 0;
    unsigned *d_status = nullptr;
    // the status word as of the last c3sc_hip_cross_fetch, valid until the next launch through this context: the solver reads the
    // status once per sweep, right after the fetch that already waited for the stream -- no second device round trip
    unsigned status_cache = 0;
    bool status_cache_valid = false;
    unsigned long long *d_dbg = nullptr; // diagnostic stamps (C3SC_DBG & 128)
    int variant = C3SC_VARIANT_AUTO;
    const char *last_kernel = "";
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // c3sc_hip_bellman_fibers_all: side streams the independent per-dimension launches of one batch are spread over, with the
    // events that fork them from and join them to the caller's stream (created on first use)
    static constexpr int NSIDE = 2;
    hipStream_t side[NSIDE] = {nullptr, nullptr};
    hipEvent_t fork_ev = nullptr, join_ev[NSIDE] = {nullptr, nullptr};
    // fiber-pair launches: scratch of the live-first partition of a batch (fiber_partition.hpp), grow-only, one block per stream
    // of c3sc_hip_bellman_fibers_all (0: the caller's stream, which also serves the single-launch entry points).  A block is read
    // by the pair kernel it was filled for, so the launches of one context that partition are ordered by the caller: one stream
    // at a time (c3sc_hip.h, c3sc_hip_bellman_fibers).  Growing a block frees the old one, which synchronises the device.
    void *part[NSIDE + 1] = {nullptr, nullptr, nullptr};
    size_t part_bytes[NSIDE + 1] = {0, 0, 0};
    // the last partition of each block, for c3sc_hip_last_partition (tests): valid until the block grows or the context goes
    struct {
        int32_t *perm = nullptr, *nlive = nullptr;
        long F = 0;
        hipStream_t stream = nullptr;
    } part_last[NSIDE + 1];
    // scratch for the *_host convenience calls
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    // c3sc_hip_simulate: trajectory state between the launches of one call ([n][d] x, [n] cost, [n] exit step)
    void *sim_state = nullptr;
    size_t sim_state_bytes = 0;
    int constelm = 0; // c3sc_hip_set_interp: off-grid evaluation as the reference's CONSTELM (nearest node per dimension)
    // pinned, device-mapped host block for small *_host batches (read and written by the kernel in place)
    void *pinned = nullptr, *pinned_dev = nullptr;
    size_t pinned_bytes = 0;
    // node memo requested for the next Bellman launch (set by c3sc_hip_cross_iteration around its launches)
    struct {
        unsigned long long *keys = nullptr;
        double *vals = nullptr;
        unsigned long long capmask = 0, epoch_bits = 0;
        int shift = 0;
        long long stride[c3sc::MAXD] = {0};
        unsigned long long *counters = nullptr;
        int mode = 0;         // KArgs::memo_mode
        bool applied = false; // the launched kernel carried the memo in its epilogue
    } memo;
    const int *skip_flag = nullptr; // device flag the next fiber-per-wave launch returns on at once when set (cross_device.hip)
    c3sc_hip_comm *shard_comm = nullptr; // borrowed: the cross iterations shard their core steps over it (c3sc_hip_cross_set_comm)
    c3sc_cross_dev *cross = nullptr; // owned; freed by c3sc_hip_cross_free (called from c3sc_hip_ctx_destroy)
};

// the form of the Bellman backup this context asks for (kernel_common.hpp: FORM_*): the game and the horizon step from the data
// they carry, the rest from the switch word
static inline unsigned ctx_form(const c3sc_hip_ctx *c)
{
    return (c->game_gsz > 0 ? c3sc::FORM_GAME : 0u) | (c->hz_dt > 0.0 ? c3sc::FORM_HORIZON : 0u) | c->switches;
}

#define HIPCHK(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                 \
            return C3SC_ERR_HIP;                                                             \
        }                                                                                    \
    } while (0)

static inline int fail(c3sc_hip_ctx *ctx, int code, const char *msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

