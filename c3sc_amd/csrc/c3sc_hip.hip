// c3sc_hip.hip -- host side of libc3sc_hip.so: the C-ABI declared in include/c3sc_hip.h.
// Owns the device-resident problem description (one read-only arena: grids, obstacles, control
// candidates, rank-padded FT cores), selects a kernel instantiation and launches it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/c3sc_hip.h"
#include "fiber_partition.hpp"
#include "fiber_partition_sort.hpp"
#include "kernel_chain_walk.hpp"
#include "kernel_common.hpp"
#include "kernel_rollout.hpp"
#include "kernel_rollout_ode.hpp"
#include "model_tables.hpp"
#include "pad_cores.hpp"
#include "registry.hpp"

namespace c3sc {

std::vector<KernelEntry> &kernel_registry()
{
    static std::vector<KernelEntry> reg;
    return reg;
}

// Re-pack one FT core from the reference layout cores[m][j*r0*r1 + a + b*r0] (valuefunc.c:165-189)
// into the rank-padded device layout: first core [N][RP] (index b), last core [N][RP] (index a),
// middle cores [N][RP*RP] (a + b*RP); padding entries are zero, which leaves every contraction exact.
// One core per launch; c3sc_hip_upload_value_device pads all cores in one launch of k_pad_cores (pad_cores.hpp, prepass.hip) and
// launches this kernel no more.  It stays because tests/test_chain_build.py holds every kernel of the build before the chain
// kernels, by name, to that build's resource remarks.
__global__ void k_pad_core(const double *__restrict__ src, double *__restrict__ dst, int N, int r0, int r1, int RP,
                           int kind /*0 first, 1 middle, 2 last*/)
{
    const int per = (kind == 1) ? RP * RP : RP;
    const long total = (long)N * per;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int j = (int)(e / per), w = (int)(e - (long)j * per);
        int a, b;
        if (kind == 0) { a = 0; b = w; }
        else if (kind == 2) { a = w; b = 0; }
        else { a = w % RP; b = w / RP; }
        double v = 0.0;
        if (a < r0 && b < r1) v = src[(size_t)j * r0 * r1 + a + (size_t)b * r0];
        dst[e] = v;
    }
}

// LDS images of the cores (the arena layout once more with the node stride a kernel uses in LDS), all in ONE launch: the
// fiber-pair kernel copies its fixed cores into LDS by LDS-DMA (global_load_lds, 16 bytes per lane), which writes
// lane-linearly and cannot pad, so the padding (elems | 1 doubles per node there, elems + 2 for the fiber-quad kernels) is
// laid down here.  blockIdx.y = job.
// Two more jobs of the same launch build the fiber-pair kernel's product tables (kernel_fiber_pair.hpp: fpp_edge_tables), one row
// of RP doubles per index pair (a, b) of a side's two outer cores:
//   tab 1: row[beta]  = sum_alpha G_0[a][alpha] G_1[b][alpha + beta RP]          (src = G_0, src2 = G_1,     nodes2 = N_1)
//   tab 2: row[alpha] = sum_beta  G_{d-2}[a][alpha + beta RP] G_{d-1}[b][beta]   (src = G_{d-2}, src2 = G_{d-1}, nodes2 = N_{d-1})
// Each entry is ONE fma chain from 0.0 with the summed index ascending -- the order of vecmat_lds / matvec_lds (fold_lds.hpp), so a
// row is bit for bit the vector the kernel used to fold from the two cores.  Built from the padded cores: padding stays exact zero.
struct ImgJobs {
    int n;
    long src[3 * MAXD + 2], dst[3 * MAXD + 2];
    int nodes[3 * MAXD + 2], per[3 * MAXD + 2], stride[3 * MAXD + 2];
    int tab[3 * MAXD + 2], nodes2[3 * MAXD + 2]; // tab: 0 image, 1 / 2 product table (per = RP)
    long src2[3 * MAXD + 2];
};
__global__ void k_core_images(double *__restrict__ arena, const ImgJobs J)
{
    const int jb = blockIdx.y;
    const double *core = arena + J.src[jb];
    double *img = arena + J.dst[jb];
    const int per = J.per[jb], stride = J.stride[jb];
    if (J.tab[jb] != 0) {
        const double *core2 = arena + J.src2[jb];
        const int RP = per, n2 = J.nodes2[jb];
        const bool left = J.tab[jb] == 1;
        const long total = (long)J.nodes[jb] * n2 * RP;
        for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
            const long row = e / RP;
            const int c = (int)(e - row * RP), a = (int)(row / n2), b = (int)(row - (long)a * n2);
            // left: the edge core is the row vector G_0[a] and c the column of G_1[b]; right: the edge core is the column vector
            // G_{d-1}[b] and c the row of G_{d-2}[a]
            const double *vec = left ? core + (size_t)a * RP : core2 + (size_t)b * RP;
            const double *mat = left ? core2 + (size_t)b * RP * RP + (size_t)c * RP : core + (size_t)a * RP * RP + c;
            const int ms = left ? 1 : RP;
            double t = 0.0;
            for (int s = 0; s < RP; s++) t = fma(vec[s], mat[(size_t)s * ms], t);
            img[e] = t;
        }
        return;
    }
    const long total = (long)J.nodes[jb] * stride;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int j = (int)(e / stride), w = (int)(e - (long)j * stride);
        img[e] = (w < per) ? core[(size_t)j * per + w] : 0.0;
    }
}

// The fiber-pair kernel's three-core product tables (kernel_common.hpp: pair_tab3L_off), one thread per entry:
//   left:  row (c, a, b)[beta]  = sum_alpha tabL(a, b)[alpha] G_2[c][alpha + beta RP]
//   right: row (a, b, c)[alpha] = sum_beta  G_{d-3}[a][alpha + beta RP] tabR(b, c)[beta]
// Each entry is ONE fma chain from 0.0 with the summed index ascending, as in k_core_images: a row is bit for bit the two-core row
// pushed through the third core by vecmat_lds / matvec_lds or the uniform products.  Inputs are the padded core and the two-core
// table, so padding stays exact zero.
// Only the sides that some instantiation reads are built (kernel_common.hpp: fpp_table3_sides): blockIdx.y = job.
struct Tab3Jobs {
    long tab2[2], core[2], dst[2]; // the side's two-core table, its third core, the three-core table
    int n3[2], npairs[2];          // nodes of the third core; index pairs of the two-core table
    int left[2];                   // the job's side
};
__global__ void k_pair_tab3(double *__restrict__ arena, const Tab3Jobs J, int RP)
{
    const int sd = blockIdx.y;
    const bool left = J.left[sd] != 0;
    const double *tab2 = arena + J.tab2[sd], *core = arena + J.core[sd];
    double *dst = arena + J.dst[sd];
    const long np = J.npairs[sd], total = (long)J.n3[sd] * np * RP;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long row = e / RP;
        const int c = (int)(e - row * RP);
        // left: the third index is the slowest of the row; right: it is the slowest too (a = i_{d-3}), the pair (b, c) behind it
        const long i3 = row / np, pair = row - i3 * np;
        const double *vec = tab2 + pair * RP;
        const double *mat = left ? core + i3 * RP * RP + (long)c * RP : core + i3 * RP * RP + c;
        const int ms = left ? 1 : RP;
        double t = 0.0;
        for (int s = 0; s < RP; s++) t = fma(vec[s], mat[(long)s * ms], t);
        dst[e] = t;
    }
}

// Derived copies of a rank-padded middle core for the fiber-quad kernel (kernel_fiber_quad.hpp), made on the device from
// the padded core itself: (1) the row-major transpose, (2) the two MFMA A operands of the varying-core products
// c = G R (x = a, y = b) and a = L G (x = b, y = a): element [prod][mb][s][l] = M[x][y] with x = (i%4) C + 4 mb + i/4
// (i = l % 16; a zero row when 4 mb + i/4 >= C) and y = (l/16) C + s, so that D register r of lane (q, t) is component
// q C + 4 mb + r of the product for fiber t.
__global__ void k_quad_aux(const double *__restrict__ core, double *__restrict__ coreT, double *__restrict__ aop, int N, int RP)
{
    const int C = RP / 4, MB = (C + 3) / 4;
    const int per_t = RP * RP, per_a = 2 * MB * C * 64;
    const long total = (long)N * (per_t + per_a);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int j = (int)(e / (per_t + per_a)), w = (int)(e - (long)j * (per_t + per_a));
        const double *G = core + (size_t)j * per_t; // a + b*RP
        if (w < per_t) {
            const int a = w / RP, b = w % RP;
            coreT[(size_t)j * per_t + w] = G[a + b * RP];
        } else {
            const int u = w - per_t;
            const int l = u % 64, s = (u / 64) % C, mb = (u / (64 * C)) % MB, prod = u / (64 * C * MB);
            const int i = l % 16, g = 4 * mb + i / 4; // D register r of lane (q, t) is row 4 r + q of the 16 x 16 block (probed:
            const int xc = (i % 4) * C + g, yc = (l / 16) * C + s; // tools/probe_mfma_layout.hip), so A row i serves (q, r) = (i % 4, i / 4)
            double v = 0.0;
            if (g < C) v = (prod == 0) ? G[xc + yc * RP] : G[yc + xc * RP];
            aop[(size_t)j * per_a + u] = v;
        }
    }
}

// FP64 peak probes (DESIGN.md "Roofline peaks"): dependent-free FMA streams per lane
__global__ void k_peak_fma(double *out, int iters)
{
    double a0 = threadIdx.x * 1e-9, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
    const double m = 1.0000001, c = 1e-9;
    for (int i = 0; i < iters; i++) {
        a0 = fma(a0, m, c); a1 = fma(a1, m, c); a2 = fma(a2, m, c); a3 = fma(a3, m, c);
        a4 = fma(a4, m, c); a5 = fma(a5, m, c); a6 = fma(a6, m, c); a7 = fma(a7, m, c);
    }
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
}

typedef double v4d __attribute__((ext_vector_type(4)));
__global__ void k_peak_mfma(double *out, int iters)
{
    v4d c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
    const double a = 1.0 + threadIdx.x * 1e-9, b = 1e-9;
    for (int i = 0; i < iters; i++) {
        c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c2, 0, 0, 0);
        c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c3, 0, 0, 0);
    }
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = c0[0] + c1[1] + c2[2] + c3[3];
}

} // namespace c3sc

using namespace c3sc;

#include "ctx.hpp"

// Host companions of the device models (models.hpp): the univariate functions of a grid coordinate and of
// a control candidate are evaluated HERE with libm, exactly as the reference's callbacks would
// (dubinscar.c:48-49, scar.c:65-67), and handed to the kernels as tables.
// Besides the trigonometric tables, any other expensive univariate function of a grid coordinate is tabulated
// here with the host's IEEE arithmetic (correctly rounded division, the same result the device's division sequence
// gives): the car models' speed factor v / (0.2 (1 + v/8)) costs a ~15-instruction dependent chain per node otherwise.
// model_ntab / model_tab_dim / model_table_value: model_tables.hpp (the rollouts evaluate them on the device as well)
static int model_ncf(int model) { return model == C3SC_MODEL_SCAR4D ? 1 : (model == C3SC_MODEL_COTHRUST6D ? 3 : 0); }
static double model_cand_feature(int model, int q, const double *u)
{
    if (model == C3SC_MODEL_COTHRUST6D) { /* copterposethrust.c:104-117, the callback's own expressions */
        const double m = 1.227, g = 9.81, mg = m * g;
        const double cphi = cos(u[1]), sphi = sin(u[1]), cth = cos(u[2]), sth = sin(u[2]);
        return q == 0 ? cphi * sth * (u[0] - mg) / m : (q == 1 ? -sphi * (u[0] - mg) / m : g + cth * cphi * (u[0] - mg) / m);
    }
    (void)q;
    return tan(u[0]); /* scar.c:67 */
}

static size_t static_layout(c3sc_hip_ctx *c)
{ // offsets of the static section; returns its size in doubles (rounded to 16)
    size_t off = c->xgrid_flat.size();
    c->obs_off = (int)off;
    off += c->obs.size();
    c->cands_off = (int)off;
    off += c->cands.size();
    for (int t = 0; t < 4; t++) c->tab_off[t] = 0;
    const int nt = model_ntab(c->model);
    for (int t = 0; t < nt; t++) {
        const int dim = model_tab_dim(c->model, t);
        c->tab_off[t] = (int)off;
        off += (dim < c->d) ? (size_t)c->ngrid[dim] : 0;
    }
    c->cfeat_off = (int)off;
    off += (size_t)model_ncf(c->model) * c->ncand;
    c->hz_off = (int)off; // the horizon constants (c3sc_hip_set_horizon_step): zeros when horizon mode is off
    off += 4;
    return (off + 15) & ~(size_t)15;
}

static int upload_static(c3sc_hip_ctx *c)
{
    std::vector<double> st(c->static_doubles, 0.0);
    std::copy(c->xgrid_flat.begin(), c->xgrid_flat.end(), st.begin());
    std::copy(c->obs.begin(), c->obs.end(), st.begin() + c->obs_off);
    std::copy(c->cands.begin(), c->cands.end(), st.begin() + c->cands_off);
    const int nt = model_ntab(c->model);
    for (int t = 0; t < nt; t++) {
        const int dim = model_tab_dim(c->model, t);
        if (dim >= c->d) continue;
        const double *g = c->xgrid_flat.data() + c->xg_off_rel[dim];
        for (int i = 0; i < c->ngrid[dim]; i++) st[c->tab_off[t] + i] = model_table_value(c->model, t, g[i]);
    }
    const int ncf = model_ncf(c->model);
    for (int q = 0; q < c->ncand * ncf; q++)
        st[c->cfeat_off + q] = model_cand_feature(c->model, q % ncf, c->cands.data() + (size_t)(q / ncf) * c->du);
    if (c->hz_dt > 0.0) { // wave-uniform constants of the explicit scheme (kernel_common.hpp, node_backup HORIZON)
        st[c->hz_off] = c->hz_dt;
        st[c->hz_off + 1] = std::exp(-c->discount * c->hz_dt);
        st[c->hz_off + 2] = c->hz_dt / c->h2;
    }
    st[c->hz_off + 3] = c->constelm ? 1.0 : 0.0; // the interpolation class of the jump targets (kernel_common.hpp: jump_constelm)
    HIPCHK(c, hipMemcpy(c->arena, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice));
    c->static_dirty = false;
    return C3SC_OK;
}

// AUTO picks by batch size: the fiber-pair kernel needs 64 fibers x 1024 resident workgroups to fill the chip and a
// single tile takes ~0.12 ms whatever F is, while one-wave-per-fiber scales down to ~20 us (measured on car7d:
// 0.020 / 0.065 / 0.23 ms at F = 2k / 8k / 32k against 0.12 / 0.12 / 0.15 ms) -- cross-approximation core steps
// (F = r_k r_{k+1}, a few hundred fibers) are latency-bound and take the per-wave kernel.
static const size_t SMALL_BATCH_FIBERS = 16384;

// every kernel entry a lookup for `model` may use: the compiled-in instantiations and, for a run-time compiled model (id >=
// C3SC_MODEL_USER) or the model-independent kernels (model 0, which a run-time compile adds where the library lacks them),
// the entries of rtc.hip
template <class Fn>
static void each_entry(int model, Fn &&f)
{
    for (const auto &e : kernel_registry()) f(e);
    if (model == 0 || model >= C3SC_MODEL_USER) {
        const RtcEntries r = rtc_entries();
        for (int i = 0; i < r.n; i++) f(*r.e[i]);
    }
}

static const KernelEntry *find_kernel(int model, int d, int rank_needed, int N, int variant, int k, size_t F = (size_t)-1,
                                      const std::vector<const KernelEntry *> *skip = nullptr)
{
    const KernelEntry *best = nullptr;
    const bool small = (variant == C3SC_VARIANT_AUTO) && F < SMALL_BATCH_FIBERS;
    each_entry(model, [&](const KernelEntry &e) {
        if (!is_fiber_variant(e.variant)) return;
        if (e.model != model || e.d != d || e.rp < rank_needed || e.max_n < N) return;
        if (skip && std::find(skip->begin(), skip->end(), &e) != skip->end()) return;
        if (e.k >= 0 && e.k != k) return;
        if (variant != C3SC_VARIANT_AUTO && e.variant != variant) return;
        auto pref = [small](int v) {
            if (small) return v == C3SC_VARIANT_FIBER_PER_WAVE ? 0 : (v == C3SC_VARIANT_FIBER_PAIR ? 1 : (v == C3SC_VARIANT_FIBER_QUAD ? 2 : 3));
            return v == C3SC_VARIANT_FIBER_PAIR ? 0 : (v == C3SC_VARIANT_FIBER_QUAD ? 1 : (v == C3SC_VARIANT_FIBER_PER_WAVE ? 2 : 3));
        };
        if (!best || e.rp < best->rp || (e.rp == best->rp && pref(e.variant) < pref(best->variant)) ||
            (e.rp == best->rp && e.variant == best->variant && e.npl < best->npl))
            best = &e;
    });
    return best;
}

static int pick_rp(int d, int maxrank, int model, int variant)
{ // smallest padded rank an instantiation of this dimension offers -- of the selected variant and model when a variant
  // is forced (its padded ranks may differ from the other kernels': the quad kernel wants multiples of 4)
    int rp = 0;
    if (variant != C3SC_VARIANT_AUTO)
        each_entry(model, [&](const KernelEntry &e) {
            if (is_fiber_variant(e.variant) && e.d == d && e.variant == variant && (model == 0 || e.model == model) && e.rp >= maxrank && (rp == 0 || e.rp < rp)) rp = e.rp;
        });
    if (rp) return rp;
    if (model != 0) // the padded classes compiled for THIS model (another model of the same dimension may offer others)
        each_entry(model, [&](const KernelEntry &e) {
            if (is_fiber_variant(e.variant) && e.d == d && e.model == model && e.rp >= maxrank && (rp == 0 || e.rp < rp)) rp = e.rp;
        });
    if (rp) return rp;
    each_entry(model, [&](const KernelEntry &e) {
        if (is_fiber_variant(e.variant) && e.d == d && e.rp >= maxrank && (rp == 0 || e.rp < rp)) rp = e.rp;
    });
    return rp;
}

static unsigned long long g_tab3_launches = 0; // ... of which fiber-pair launches with the three-core tables (c3sc_hip_table3_launch_count)
static unsigned long long g_launches = 0; // Bellman / stencil kernel launches of this process (c3sc_hip_launch_count)
static int fill_args(c3sc_hip_ctx *c, int k, size_t F, KArgs &A, bool need_model);

// One row per feature of the Bellman backup (kernel_common.hpp: FORM_*), in the order refusals are reported: what differs between
// the features in the messages below.  Which features combine is form_offered's to say
struct FormRow {
    unsigned bit;
    const char *kind;     // its kernels and forms: "stop kernels", "no stop form"
    const char *subject;  // the feature as the subject of a sentence ...
    bool plural;          // ... which takes "need" or "needs"
    const char *problems; // deterministic closed loops are not offered ...
    const char *compile;  // the entry point that compiles its kernels ...
    const char *field;    // ... and what its spec asks for them with
    const char *off;      // the call that switches the feature off
};
static const FormRow FORM_ROWS[] = {
    {FORM_GAME, "game", "game mode", false, "for games", "c3sc_hip_model_compile_ex", "game = 1", "c3sc_hip_set_game with nu = 0"},
    {FORM_HORIZON, "horizon", "horizon mode", false, "in horizon mode", "c3sc_hip_model_compile_fh", "horizon = 1", "c3sc_hip_set_horizon_step(ctx, 0)"},
    {FORM_STOP, "stop", "stopping", false, "for stopping problems", "c3sc_hip_model_compile_os", "stop = 1", "c3sc_hip_set_stopping(ctx, 0)"},
    {FORM_JUMP, "jump", "jumps", true, "for jump diffusions", "c3sc_hip_model_compile_jd", "njump > 0", "c3sc_hip_set_jumps(ctx, 0)"},
    {FORM_IMPULSE, "impulse", "interventions", true, "for impulse control", "c3sc_hip_model_compile_ic", "nimpulse > 0", "c3sc_hip_set_impulses(ctx, 0)"},
    {FORM_CORR, "corr", "correlated noise", false, "with correlated noise", "c3sc_hip_model_compile_cd", "ncorr > 0", "c3sc_hip_set_correlation(ctx, 0)"},
};

static const FormRow &form_row(unsigned bit) { return FORM_ROWS[__builtin_ctz(bit)]; } // the rows are in the order of the bits

static int fails(c3sc_hip_ctx *c, int code, const std::string &msg) { return fail(c, code, msg.c_str()); }
static std::string verb(const FormRow &r, const char *singular, const char *plural) { return std::string(r.subject) + " " + (r.plural ? plural : singular); }
static int no_box_form(c3sc_hip_ctx *c, const char *who, const FormRow &r)
{
    return fails(c, C3SC_ERR_UNSUPPORTED, std::string(who) + ": " + verb(r, "has", "have") + " no control-box form");
}

// The features among `bits` that are on are served by the model set now (set_model may have replaced the one their setters
// checked): a run-time compiled model with their kernels, for a game of the game's du.  The first that is not is reported
static int check_form_model(c3sc_hip_ctx *c, const char *who, unsigned bits = FORM_ALL)
{
    const unsigned want = ctx_form(c) & bits, have = c->model >= C3SC_MODEL_USER ? rtc_model_forms(c->model) : 0u;
    if (want && !form_offered(ctx_form(c))) return fails(c, C3SC_ERR_UNSUPPORTED, std::string(who) + ": this combination of modes is not offered");
    for (const FormRow &r : FORM_ROWS) {
        if (!(want & r.bit)) continue;
        int du = 0;
        const bool game_du = r.bit != FORM_GAME || (rtc_model_info(c->model, du) && du == c->du);
        if (!(have & r.bit) || !game_du)
            return fails(c, C3SC_ERR_UNSUPPORTED, std::string(who) + ": " + verb(r, "needs", "need") + " a model compiled with " + r.kind + " kernels" +
                                                      (r.bit == FORM_GAME ? " of the game's du" : "") + " (" + r.compile + ", " + r.field + ")");
    }
    return C3SC_OK;
}

// Switching the feature of row r on (c3sc_hip_set_game, _set_horizon_step and the four switches): the model must have its
// kernels, and no feature that is on may exclude it
static int check_switch_model(c3sc_hip_ctx *c, const FormRow &r, const char *who)
{
    if (c->model == 0) return fails(c, C3SC_ERR_ARG, std::string(who) + ": set_model first");
    if (c->model < C3SC_MODEL_USER || !rtc_model_known(c->model))
        return fails(c, C3SC_ERR_UNSUPPORTED, std::string(who) + ": " + verb(r, "needs", "need") + " a run-time compiled model (" + r.compile + " with " + r.field + ")");
    if (!(rtc_model_forms(c->model) & r.bit))
        return fails(c, C3SC_ERR_UNSUPPORTED, std::string(who) + ": this model was compiled without " + r.kind + " kernels (" + r.compile + ", " + r.field + ")");
    return C3SC_OK;
}

static int check_switch_conflicts(c3sc_hip_ctx *c, const FormRow &r, const char *who)
{
    for (const FormRow &o : FORM_ROWS)
        if ((ctx_form(c) & o.bit) && !form_offered(r.bit | o.bit))
            return fails(c, C3SC_ERR_UNSUPPORTED, std::string(who) + ": " + r.subject + " and " + o.subject + " are not offered together (" + o.off + " first)");
    return C3SC_OK;
}

static int ensure_scratch(c3sc_hip_ctx *c, size_t bytes)
{
    if (bytes <= c->scratch_bytes) return C3SC_OK;
    if (c->scratch) HIPCHK(c, hipFree(c->scratch));
    c->scratch = nullptr;
    c->scratch_bytes = 0;
    HIPCHK(c, hipMalloc(&c->scratch, bytes));
    c->scratch_bytes = bytes;
    return C3SC_OK;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Small batches of the *_host entry points (a cross-approximation core step: ~100 fibers, 3 KB in, 33 KB out) skip
// the staging copies: indices are placed in a pinned host block the device maps, the kernel reads them and writes its
// rows there, and the call is launch + stream synchronise.  The two hipMemcpy calls they replace cost 25 us of a
// 53 us call (tools/call_latency.py).  Large batches keep the copies: PCIe would bound the kernel.
static constexpr size_t ZERO_COPY_MAX_BYTES = (size_t)1 << 20;
static bool zero_copy_batch(size_t bytes)
{
    static const bool off = getenv("C3SC_NO_ZEROCOPY") != nullptr;
    return !off && bytes <= ZERO_COPY_MAX_BYTES;
}
static int ensure_pinned(c3sc_hip_ctx *c, size_t bytes)
{
    if (bytes <= c->pinned_bytes) return C3SC_OK;
    if (c->pinned) HIPCHK(c, hipHostFree(c->pinned));
    c->pinned = c->pinned_dev = nullptr;
    c->pinned_bytes = 0;
    const size_t cap = bytes < ((size_t)256 << 10) ? ((size_t)256 << 10) : bytes;
    HIPCHK(c, hipHostMalloc(&c->pinned, cap, hipHostMallocMapped | hipHostMallocPortable));
    HIPCHK(c, hipHostGetDevicePointer(&c->pinned_dev, c->pinned, 0));
    c->pinned_bytes = cap;
    return C3SC_OK;
}

// The staging of every host-buffer (*_host) entry point.  A call lists its buffers as segments; stage_host lays them out one
// after the other at 256-byte alignment in one block of the storage `kind` names, copies the IN segments there, runs `call`
// with one device pointer per segment and copies the OUT segments back.  The device pointer is null where the host pointer is,
// but the segment's space is laid out all the same: which outputs a caller wants does not change the block's size (a segment
// that needs no space has 0 bytes).
enum SegDir { SEG_IN, SEG_OUT };
struct HostSeg { const void *host; size_t bytes; SegDir dir; }; // SEG_OUT: `host` is the caller's writable buffer
enum Staging {
    STAGE_MAPPED_OR_SCRATCH, // the pinned, device-mapped block for a batch zero_copy_batch admits, else c->scratch
    STAGE_SCRATCH,           // c->scratch
    STAGE_PER_CALL,          // a device block of this call alone, freed on every return (trajectory buffers can be large)
};
struct DevPtr { // a segment's device pointer, handed to the device call as whatever pointer type its parameter has
    void *p;
    template <class T> operator T *() const { return static_cast<T *>(p); }
};

template <size_t NS, class Call>
static int stage_host(c3sc_hip_ctx *c, Staging kind, const char *what, const HostSeg (&segs)[NS], Call &&call)
{
    size_t off[NS + 1] = {0};
    for (size_t i = 0; i < NS; i++) off[i + 1] = off[i] + align256(segs[i].bytes);
    // the segments of one direction: plain memcpy on the mapped block (hb: its host address; the call reads and writes it in
    // place), else blocking hipMemcpy to or from device memory, whose copies back wait for the call
    auto copy = [&](SegDir dir, char *hb, const DevPtr *dev) -> int {
        for (size_t i = 0; i < NS; i++) {
            if (!dev[i].p || segs[i].dir != dir || segs[i].bytes == 0) continue;
            void *h = const_cast<void *>(segs[i].host), *b = hb ? hb + off[i] : dev[i].p;
            void *dst = dir == SEG_IN ? b : h, *src = dir == SEG_IN ? h : b;
            if (hb) memcpy(dst, src, segs[i].bytes);
            else if (hipError_t e = hipMemcpy(dst, src, segs[i].bytes, dir == SEG_IN ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost); e != hipSuccess) {
                c->err = std::string(what) + ": hipMemcpy of buffer " + std::to_string(i) + (dir == SEG_IN ? " in: " : " out: ") + hipGetErrorString(e);
                return C3SC_ERR_HIP;
            }
        }
        return C3SC_OK;
    };
    auto run = [&](char *hb, char *db) -> int {
        DevPtr dev[NS];
        for (size_t i = 0; i < NS; i++) dev[i].p = segs[i].host ? db + off[i] : nullptr;
        int rc = copy(SEG_IN, hb, dev);
        if (rc == C3SC_OK) rc = call(dev);
        if (rc != C3SC_OK) return rc;
        if (hb) HIPCHK(c, hipStreamSynchronize(nullptr));
        return copy(SEG_OUT, hb, dev);
    };
    HIPCHK(c, hipSetDevice(c->device));
    const size_t total = off[NS];
    int rc;
    if (kind == STAGE_MAPPED_OR_SCRATCH && zero_copy_batch(total))
        return (rc = ensure_pinned(c, total)) != C3SC_OK ? rc : run((char *)c->pinned, (char *)c->pinned_dev);
    if (kind != STAGE_PER_CALL) return (rc = ensure_scratch(c, total)) != C3SC_OK ? rc : run(nullptr, (char *)c->scratch);
    void *buf = nullptr; // STAGE_PER_CALL
    HIPCHK(c, hipMalloc(&buf, total));
    rc = run(nullptr, (char *)buf);
    (void)hipFree(buf);
    return rc;
}

extern "C" {

int c3sc_hip_max_rank(int model, int d)
{ // largest FT rank any compiled kernel of this (model, state dimension) serves; 0 = none
    int rp = 0;
    each_entry(model, [&](const KernelEntry &e) {
        if (e.model == model && e.d == d && e.rp > rp) rp = e.rp;
    });
    return rp;
}

int c3sc_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int c3sc_hip_ctx_create(int device, c3sc_hip_ctx **out)
{
    if (!out) return C3SC_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return C3SC_ERR_NODEVICE;
    c3sc_hip_ctx *c = new c3sc_hip_ctx();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipMalloc((void **)&c->d_status, sizeof(unsigned)) != hipSuccess ||
        hipMemset(c->d_status, 0, sizeof(unsigned)) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess) {
        delete c;
        return C3SC_ERR_HIP;
    }
    *out = c;
    return C3SC_OK;
}

void c3sc_hip_ctx_destroy(c3sc_hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->arena) (void)hipFree(c->arena);
    if (c->hz_stack) (void)hipFree(c->hz_stack);
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->d_dbg) (void)hipFree(c->d_dbg);
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->sim_state) (void)hipFree(c->sim_state);
    for (void *p : c->part)
        if (p) (void)hipFree(p);
    if (c->pinned) (void)hipHostFree(c->pinned);
    c3sc_hip_cross_free(c);
    for (int i = 0; i < c3sc_hip_ctx::NSIDE; i++) {
        if (c->side[i]) { (void)hipStreamSynchronize(c->side[i]); (void)hipStreamDestroy(c->side[i]); }
        if (c->join_ev[i]) (void)hipEventDestroy(c->join_ev[i]);
    }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->tab3_ev) (void)hipEventDestroy(c->tab3_ev);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    delete c;
}

const char *c3sc_hip_last_error(const c3sc_hip_ctx *c) { return c ? c->err.c_str() : "null context"; }
const char *c3sc_hip_last_kernel(const c3sc_hip_ctx *c) { return c ? c->last_kernel : ""; }

int c3sc_hip_set_grid(c3sc_hip_ctx *c, int d, const size_t *ngrid, const double *const *xgrid)
{
    if (!c || !ngrid || !xgrid || d < 2 || d > MAXD) return fail(c, C3SC_ERR_ARG, "set_grid: need 2 <= d <= 12");
    c->d = d;
    c->xgrid_flat.clear();
    for (int m = 0; m < d; m++) {
        if (ngrid[m] < 2 || ngrid[m] > 4096) return fail(c, C3SC_ERR_ARG, "set_grid: need 2 <= N_m <= 4096");
        c->ngrid[m] = (int)ngrid[m];
        c->xg_off_rel[m] = (int)c->xgrid_flat.size();
        c->xgrid_flat.insert(c->xgrid_flat.end(), xgrid[m], xgrid[m] + ngrid[m]);
    }
    c->static_dirty = true;
    c->have_value = false; // grid change invalidates the uploaded value function
    return C3SC_OK;
}

int c3sc_hip_set_boundary(c3sc_hip_ctx *c, const int *bctype, int nobs, const double *obs_lb, const double *obs_ub)
{
    if (!c || c->d == 0 || !bctype) return fail(c, C3SC_ERR_ARG, "set_boundary: set_grid first");
    if (nobs < 0 || nobs > C3SC_MAX_OBSTACLES) return fail(c, C3SC_ERR_ARG, "set_boundary: at most 10 obstacles (boundary.c:393)");
    for (int m = 0; m < c->d; m++) {
        if (bctype[m] != C3SC_ABSORB && bctype[m] != C3SC_PERIODIC && bctype[m] != C3SC_REFLECT)
            return fail(c, C3SC_ERR_ARG, "set_boundary: boundary type must be absorb/periodic/reflect (nodeutil.c:532-535)");
        c->bctype[m] = bctype[m];
    }
    c->nobs = nobs;
    c->obs.assign((size_t)nobs * 2 * c->d, 0.0);
    for (int o = 0; o < nobs; o++)
        for (int m = 0; m < c->d; m++) {
            c->obs[((size_t)o * 2 + 0) * c->d + m] = obs_lb[(size_t)o * c->d + m];
            c->obs[((size_t)o * 2 + 1) * c->d + m] = obs_ub[(size_t)o * c->d + m];
        }
    c->have_boundary = true;
    c->static_dirty = true;
    return C3SC_OK;
}

int c3sc_hip_set_consistent_ends(c3sc_hip_ctx *c, int on)
{
    if (!c) return C3SC_ERR_ARG;
    c->cends = on ? 1 : 0;
    return C3SC_OK;
}

int c3sc_hip_get_consistent_ends(const c3sc_hip_ctx *c) { return c ? c->cends : -1; }

int c3sc_hip_set_mca(c3sc_hip_ctx *c, double h2, const double *t, double discount)
{
    if (!c || c->d == 0 || !t) return fail(c, C3SC_ERR_ARG, "set_mca: set_grid first");
    c->h2 = h2;
    c->discount = discount;
    for (int i = 0; i < 2 * c->d; i++) c->t[i] = t[i];
    c->have_mca = true;
    if (c->hz_dt > 0.0) c->static_dirty = true; // the horizon constants depend on beta and h^2
    return C3SC_OK;
}

int c3sc_hip_set_horizon_step(c3sc_hip_ctx *c, double dt)
{
    if (!c) return C3SC_ERR_ARG;
    if (dt == 0.0) {
        if (c->hz_dt > 0.0) c->static_dirty = true;
        c->hz_dt = 0.0;
        return C3SC_OK;
    }
    if (!(dt > 0.0) || !std::isfinite(dt)) return fail(c, C3SC_ERR_ARG, "set_horizon_step: dt must be positive and finite (0 clears)");
    if (!c->have_mca) return fail(c, C3SC_ERR_ARG, "set_horizon_step: set_mca first");
    int rc = check_switch_model(c, form_row(FORM_HORIZON), "set_horizon_step");
    if (rc == C3SC_OK) rc = check_switch_conflicts(c, form_row(FORM_HORIZON), "set_horizon_step");
    if (rc != C3SC_OK) return rc;
    c->hz_dt = dt;
    c->static_dirty = true;
    return C3SC_OK;
}

// the four switches that carry no data: one bit of c->switches each
static int set_switch(c3sc_hip_ctx *c, unsigned bit, const char *who, int on)
{
    if (!c) return C3SC_ERR_ARG;
    if (!on) {
        c->switches &= ~bit;
        return C3SC_OK;
    }
    int rc = check_switch_model(c, form_row(bit), who);
    if (rc == C3SC_OK) rc = check_switch_conflicts(c, form_row(bit), who);
    if (rc != C3SC_OK) return rc;
    c->switches |= bit;
    return C3SC_OK;
}

int c3sc_hip_set_stopping(c3sc_hip_ctx *c, int on) { return set_switch(c, FORM_STOP, "set_stopping", on); }
int c3sc_hip_set_jumps(c3sc_hip_ctx *c, int on) { return set_switch(c, FORM_JUMP, "set_jumps", on); }
int c3sc_hip_set_impulses(c3sc_hip_ctx *c, int on) { return set_switch(c, FORM_IMPULSE, "set_impulses", on); }
int c3sc_hip_set_correlation(c3sc_hip_ctx *c, int on) { return set_switch(c, FORM_CORR, "set_correlation", on); }

int c3sc_hip_set_model(c3sc_hip_ctx *c, int model, const double *params, int nparams)
{
    if (!c || model <= 0 || nparams < 0 || nparams > C3SC_MAX_PARAMS) return fail(c, C3SC_ERR_ARG, "set_model: bad arguments");
    if (model >= C3SC_MODEL_USER && !rtc_model_known(model)) return fail(c, C3SC_ERR_ARG, "set_model: no run-time model has this id");
    c->model = model;
    std::memset(c->prm, 0, sizeof(c->prm));
    for (int i = 0; i < nparams; i++) c->prm[i] = params[i];
    c->static_dirty = true; // model tables live in the static section
    return C3SC_OK;
}

int c3sc_hip_set_controls(c3sc_hip_ctx *c, int ncand, int du, const double *cands)
{
    if (!c || ncand < 1 || du < 1 || !cands) return fail(c, C3SC_ERR_ARG, "set_controls: bad arguments");
    c->ncand = ncand;
    c->cands_placeholder = false;
    c->du = du;
    c->cands.assign(cands, cands + (size_t)ncand * du);
    c->static_dirty = true;
    c->game_gsz = c->game_ngrp = c->game_order = 0;
    return C3SC_OK;
}

int c3sc_hip_set_game(c3sc_hip_ctx *c, int du_min, int nu, const double *U, int nw, const double *W, int order)
{
    if (!c) return C3SC_ERR_ARG;
    if (nu == 0) { // clear: the product list stays as a plain candidate list
        c->game_gsz = c->game_ngrp = c->game_order = 0;
        return C3SC_OK;
    }
    if (order != C3SC_GAME_MINMAX && order != C3SC_GAME_MAXMIN) return fail(c, C3SC_ERR_ARG, "set_game: order must be C3SC_GAME_MINMAX or C3SC_GAME_MAXMIN");
    if (c->model == 0) return fail(c, C3SC_ERR_ARG, "set_game: set_model first");
    if (c->model == C3SC_MODEL_TABLE) return fail(c, C3SC_ERR_UNSUPPORTED, "set_game: the TABLE model has no game kernels");
    int rc = check_switch_conflicts(c, form_row(FORM_GAME), "set_game");
    if (rc == C3SC_OK) rc = check_switch_model(c, form_row(FORM_GAME), "set_game");
    if (rc != C3SC_OK) return rc;
    int mdu = 0;
    rtc_model_info(c->model, mdu);
    if (nu < 0 || nw < 1 || du_min < 1 || du_min >= mdu || !U || !W)
        return fail(c, C3SC_ERR_ARG, "set_game: du_min + du_max must equal the model's du, each at least 1, with nu, nw >= 1 and both lists given");
    if ((long long)nu * nw > (1ll << 24)) return fail(c, C3SC_ERR_ARG, "set_game: nu * nw too large");
    const int dmax = mdu - du_min, ncand = nu * nw;
    std::vector<double> cands((size_t)ncand * mdu);
    for (int iu = 0; iu < nu; iu++)
        for (int iw = 0; iw < nw; iw++) { // u-major (MINMAX: groups are u) or w-major (MAXMIN: groups are w)
            const size_t p = order == C3SC_GAME_MINMAX ? (size_t)iu * nw + iw : (size_t)iw * nu + iu;
            double *row = cands.data() + p * mdu;
            for (int i = 0; i < du_min; i++) row[i] = U[(size_t)iu * du_min + i];
            for (int i = 0; i < dmax; i++) row[du_min + i] = W[(size_t)iw * dmax + i];
        }
    c->ncand = ncand;
    c->cands_placeholder = false;
    c->du = mdu;
    c->cands.swap(cands);
    c->static_dirty = true;
    c->game_order = order;
    c->game_gsz = order == C3SC_GAME_MINMAX ? nw : nu;
    c->game_ngrp = order == C3SC_GAME_MINMAX ? nu : nw;
    return C3SC_OK;
}

int c3sc_hip_set_control_box(c3sc_hip_ctx *c, int du, const double *lb, const double *ub, int grid, int polish)
{
    if (!c || du < 1 || du > C3SC_MAX_DU || !lb || !ub || grid < 2 || polish < 0) return fail(c, C3SC_ERR_ARG, "set_control_box: bad arguments");
    double tot = 1.0;
    for (int i = 0; i < du; i++) {
        if (!(lb[i] <= ub[i])) return fail(c, C3SC_ERR_ARG, "set_control_box: lb > ub");
        c->box_lb[i] = lb[i];
        c->box_ub[i] = ub[i];
        tot *= grid;
    }
    if (tot > 1e6) return fail(c, C3SC_ERR_ARG, "set_control_box: grid^du too large");
    c->box_du = du; c->box_grid = grid; c->box_polish = polish;
    if (c->ncand == 0) { // the arena layout wants at least one candidate row; it is not read in box mode
        c->ncand = 1; c->du = du;
        c->cands_placeholder = true; // ... so a call that takes the list only (simulate_chain) knows there is none
        c->cands.assign(du, 0.0);
        c->static_dirty = true;
    }
    return C3SC_OK;
}

int c3sc_hip_set_variant(c3sc_hip_ctx *c, int variant)
{
    if (!c) return C3SC_ERR_ARG;
    c->variant = variant;
    return C3SC_OK;
}

static int prepare_value(c3sc_hip_ctx *c, const size_t *ranks, size_t *cores_doubles)
{
    if (!c || c->d == 0 || !ranks) return fail(c, C3SC_ERR_ARG, "upload_value: set_grid first");
    const int d = c->d;
    if (ranks[0] != 1 || ranks[d] != 1) return fail(c, C3SC_ERR_ARG, "upload_value: ranks[0] and ranks[d] must be 1");
    size_t maxrank = 1;
    for (int m = 0; m <= d; m++) {
        if (ranks[m] < 1) return fail(c, C3SC_ERR_ARG, "upload_value: rank < 1");
        maxrank = std::max(maxrank, ranks[m]);
    }
    const int rp = pick_rp(d, (int)maxrank, c->model, c->variant);
    if (rp == 0) return fail(c, C3SC_ERR_UNSUPPORTED, "upload_value: no kernel instantiation for this (dim, rank)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t stat = static_layout(c);
    size_t off = stat;
    long core_off[MAXD];
    for (int m = 0; m < d; m++) {
        core_off[m] = (long)off;
        const size_t per = (m == 0 || m == d - 1) ? rp : (size_t)rp * rp;
        off += ((size_t)c->ngrid[m] * per + 15) & ~(size_t)15;
    }
    const size_t primary_end = off;
    long coreT_off[MAXD] = {0}, aop_off[MAXD] = {0};
    bool have_quad = false; // the derived copies are made only when a fiber-quad kernel of this (model, dimension, padded rank) exists
    for (const auto &e : kernel_registry())
        if (e.variant == C3SC_VARIANT_FIBER_QUAD && e.d == d && e.rp == rp && (c->model == 0 || e.model == c->model)) have_quad = true;
    if (rp % 4 == 0 && have_quad) { // derived copies for the fiber-quad kernel (k_quad_aux)
        const int C = rp / 4, MB = (C + 3) / 4;
        for (int m = 1; m < d - 1; m++) {
            coreT_off[m] = (long)off;
            off += ((size_t)c->ngrid[m] * rp * rp + 15) & ~(size_t)15;
            aop_off[m] = (long)off;
            off += ((size_t)c->ngrid[m] * 2 * MB * C * 64 + 15) & ~(size_t)15;
        }
    }
    long img_off[MAXD] = {0};
    for (int m = 0; m < d; m++) { // LDS images for the fiber-pair kernel's LDS-DMA staging (+2: its last 16-byte piece may overhang)
        const size_t per = (m == 0 || m == d - 1) ? rp : (size_t)rp * rp;
        img_off[m] = (long)off;
        off += (size_t)pair_img_doubles(c->ngrid[m], (int)per);
    }
    // product tables of each side's two outer cores for the staged fiber-pair kernels (kernel_common.hpp: pair_tabL_off), right
    // behind the last image: made only when such a kernel of this (dimension, padded rank) exists -- of ANY model: the model may
    // be set after the upload, and a pair kernel must never run without its tables
    long tabL_off = 0, tabR_off = 0;
    bool have_pair = false;
    for (const auto &e : kernel_registry())
        if (e.variant == C3SC_VARIANT_FIBER_PAIR && e.d == d && e.rp == rp) have_pair = true;
    if (d >= 4 && have_pair) {
        tabL_off = (long)off;
        off += (size_t)pair_tab_doubles(c->ngrid[0], c->ngrid[1], rp);
        tabR_off = (long)off;
        off += (size_t)pair_tab_doubles(c->ngrid[d - 2], c->ngrid[d - 1], rp);
    }
    // the three-core tables behind them, where a three-core instantiation exists and the tables stay within their memory bound
    long tab3L_off = 0, tab3R_off = 0;
    if (tabL_off && pair_tab3_reserved(d, c->ngrid, rp)) {
        tab3L_off = (long)off;
        off += (size_t)pair_tab3_doubles(c->ngrid[0], c->ngrid[1], c->ngrid[2], rp);
        tab3R_off = (long)off;
        off += (size_t)pair_tab3_doubles(c->ngrid[d - 3], c->ngrid[d - 2], c->ngrid[d - 1], rp);
    }
    long qimgL_off[MAXD] = {0}, qimgR_off[MAXD] = {0};
    if (rp % 4 == 0 && have_quad) { // LDS images for the duo kernel's double-buffered LDS-DMA staging
        for (int m = 0; m < d; m++) {
            const size_t per = (m == 0 || m == d - 1) ? rp : (size_t)rp * rp;
            const size_t sz = ((size_t)c->ngrid[m] * (per + 2) + 15) & ~(size_t)15;
            if (m < d - 1) { qimgL_off[m] = (long)off; off += sz; }
            if (m > 0) { qimgR_off[m] = (long)off; off += sz; }
        }
    }
    if (off > c->arena_cap) {
        if (c->arena) HIPCHK(c, hipFree(c->arena));
        c->arena = nullptr;
        c->arena_cap = 0;
        HIPCHK(c, hipMalloc((void **)&c->arena, off * sizeof(double)));
        c->arena_cap = off;
        c->static_dirty = true;
    }
    if (stat != c->static_doubles) c->static_dirty = true;
    c->static_doubles = stat;
    for (int m = 0; m < d; m++) { c->core_off[m] = core_off[m]; c->coreT_off[m] = coreT_off[m]; c->aop_off[m] = aop_off[m]; c->img_off[m] = img_off[m]; c->qimgL_off[m] = qimgL_off[m]; c->qimgR_off[m] = qimgR_off[m]; }
    c->tabL_off = tabL_off;
    c->tabR_off = tabR_off;
    c->tab3L_off = tab3L_off;
    c->tab3R_off = tab3R_off;
    c->tab3_stale = true; // both upload paths come through here: the next three-core launch rebuilds the tables (ensure_tab3)
    for (int m = 0; m <= d; m++) c->ranks[m] = ranks[m];
    c->rp = rp;
    *cores_doubles = primary_end - stat;
    if (c->static_dirty) return upload_static(c);
    return C3SC_OK;
}

static int make_quad_aux(c3sc_hip_ctx *c, void *stream)
{ // after the padded cores are in the arena (ordered on `stream`)
    for (int m = 1; m < c->d - 1; m++) {
        if (c->aop_off[m] == 0) continue;
        const long total = (long)c->ngrid[m] * (c->rp * c->rp + 2 * ((c->rp / 4 + 3) / 4) * (c->rp / 4) * 64);
        const int grid = (int)std::min<long>((total + 255) / 256, 1024);
        hipLaunchKernelGGL(k_quad_aux, dim3(grid), dim3(256), 0, (hipStream_t)stream, c->arena + c->core_off[m],
                           c->arena + c->coreT_off[m], c->arena + c->aop_off[m], c->ngrid[m], c->rp);
    }
    ImgJobs J; // after k_quad_aux: the suffix-side images copy the transposed cores
    J.n = 0;
    long maxtotal = 1;
    auto add = [&](long src, long dst, int nodes, int per, int stride) {
        J.src[J.n] = src; J.dst[J.n] = dst; J.nodes[J.n] = nodes; J.per[J.n] = per; J.stride[J.n] = stride;
        J.tab[J.n] = 0; J.nodes2[J.n] = 0; J.src2[J.n] = 0;
        J.n++;
        maxtotal = std::max(maxtotal, (long)nodes * stride);
    };
    for (int m = 0; m < c->d; m++) {
        const int per = (m == 0 || m == c->d - 1) ? c->rp : c->rp * c->rp;
        add(c->core_off[m], c->img_off[m], c->ngrid[m], per, per | 1);
        if (c->qimgL_off[m]) add(c->core_off[m], c->qimgL_off[m], c->ngrid[m], per, per + 2);
        if (c->qimgR_off[m]) add((m == c->d - 1) ? c->core_off[m] : c->coreT_off[m], c->qimgR_off[m], c->ngrid[m], per, per + 2);
    }
    auto add_tab = [&](int tab, long dst, int ma, int mb) { // one thread per table entry, grid-stride like the images
        add(c->core_off[ma], dst, c->ngrid[ma], c->rp, c->rp);
        J.tab[J.n - 1] = tab; J.nodes2[J.n - 1] = c->ngrid[mb]; J.src2[J.n - 1] = c->core_off[mb];
        maxtotal = std::max(maxtotal, (long)c->ngrid[ma] * c->ngrid[mb] * c->rp);
    };
    if (c->tabL_off) add_tab(1, c->tabL_off, 0, 1);
    if (c->tabR_off) add_tab(2, c->tabR_off, c->d - 2, c->d - 1);
    hipLaunchKernelGGL(k_core_images, dim3((unsigned)std::min<long>((maxtotal + 255) / 256, 64), (unsigned)J.n), dim3(256), 0, (hipStream_t)stream,
                       c->arena, J);
    HIPCHK(c, hipGetLastError());
    return C3SC_OK;
}

// cores in c3sc_hip_upload_value's host layout ([N_m][r_m][r_{m+1}], column-major per node) into the padded layout of k_pad_core
// at padded rank rp; dst[m] is where core m goes
static void pad_cores_host(int d, const int *ngrid, int rp, const size_t *ranks, const double *const *cores, double *const *dst)
{
    for (int m = 0; m < d; m++) {
        const size_t r0 = ranks[m], r1 = ranks[m + 1];
        const double *src = cores[m];
        const size_t per = (m == 0 || m == d - 1) ? rp : (size_t)rp * rp;
        for (int j = 0; j < ngrid[m]; j++)
            for (size_t b = 0; b < r1; b++)
                for (size_t a = 0; a < r0; a++) {
                    const size_t w = (m == 0) ? b : ((m == d - 1) ? a : a + b * rp);
                    dst[m][(size_t)j * per + w] = src[(size_t)j * r0 * r1 + a + b * r0];
                }
    }
}

int c3sc_hip_upload_value(c3sc_hip_ctx *c, const size_t *ranks, const double *const *cores)
{
    size_t cd = 0;
    int rc = prepare_value(c, ranks, &cd);
    if (rc != C3SC_OK) return rc;
    const int d = c->d, rp = c->rp;
    std::vector<double> buf(cd, 0.0);
    double *dst[MAXD];
    for (int m = 0; m < d; m++) dst[m] = buf.data() + (c->core_off[m] - (long)c->static_doubles);
    pad_cores_host(d, c->ngrid, rp, ranks, cores, dst);
    HIPCHK(c, hipMemcpy(c->arena + c->static_doubles, buf.data(), cd * sizeof(double), hipMemcpyHostToDevice));
    rc = make_quad_aux(c, nullptr);
    if (rc != C3SC_OK) return rc;
    // the synchronous entry point is complete on return: the derived images are built by kernels on the NULL stream, and a caller
    // may launch on a non-blocking stream next
    HIPCHK(c, hipStreamSynchronize(nullptr));
    c->have_value = true;
    return C3SC_OK;
}

int c3sc_hip_upload_value_stack(c3sc_hip_ctx *c, int nstack, const size_t *ranks, const double *const *cores)
{
    if (!c) return C3SC_ERR_ARG;
    if (nstack == 0) {
        if (c->hz_stack) HIPCHK(c, hipFree(c->hz_stack));
        c->hz_stack = nullptr;
        c->hz_nstack = 0;
        return C3SC_OK;
    }
    if (nstack < 0 || !ranks || !cores) return fail(c, C3SC_ERR_ARG, "upload_value_stack: bad arguments");
    if (c->d == 0 || !c->have_value) return fail(c, C3SC_ERR_ARG, "upload_value_stack: upload_value first (the stack shares its static section)");
    if (static_layout(c) != c->static_doubles)
        return fail(c, C3SC_ERR_ARG, "upload_value_stack: static data changed size after upload_value; upload the value again");
    const int d = c->d;
    std::vector<int> rps(nstack);
    std::vector<long> offs((size_t)nstack * MAXD, 0);
    size_t off = c->static_doubles;
    for (int s = 0; s < nstack; s++) {
        const size_t *r = ranks + (size_t)s * (d + 1);
        if (r[0] != 1 || r[d] != 1) return fail(c, C3SC_ERR_ARG, "upload_value_stack: ranks[s][0] and ranks[s][d] must be 1");
        size_t maxrank = 1;
        for (int m = 0; m <= d; m++) {
            if (r[m] < 1) return fail(c, C3SC_ERR_ARG, "upload_value_stack: rank < 1");
            maxrank = std::max(maxrank, r[m]);
        }
        for (int m = 0; m < d; m++)
            if (!cores[(size_t)s * d + m]) return fail(c, C3SC_ERR_ARG, "upload_value_stack: null core");
        rps[s] = pick_rp(d, (int)maxrank, c->model, C3SC_VARIANT_AUTO);
        if (rps[s] == 0) return fail(c, C3SC_ERR_UNSUPPORTED, "upload_value_stack: no kernel instantiation for a stage's (dim, rank)");
        for (int m = 0; m < d; m++) {
            offs[(size_t)s * MAXD + m] = (long)off;
            const size_t per = (m == 0 || m == d - 1) ? rps[s] : (size_t)rps[s] * rps[s];
            off += ((size_t)c->ngrid[m] * per + 15) & ~(size_t)15;
        }
    }
    std::vector<double> buf(off - c->static_doubles, 0.0);
    for (int s = 0; s < nstack; s++) {
        double *dst[MAXD];
        for (int m = 0; m < d; m++) dst[m] = buf.data() + (offs[(size_t)s * MAXD + m] - (long)c->static_doubles);
        pad_cores_host(d, c->ngrid, rps[s], ranks + (size_t)s * (d + 1), cores + (size_t)s * d, dst);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (c->hz_stack) HIPCHK(c, hipFree(c->hz_stack));
    c->hz_stack = nullptr;
    c->hz_nstack = 0;
    HIPCHK(c, hipMalloc((void **)&c->hz_stack, off * sizeof(double)));
    // the static section is copied from the arena at each simulate call (it may be rewritten in between)
    HIPCHK(c, hipMemcpy(c->hz_stack + c->static_doubles, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice));
    c->hz_stack_static = c->static_doubles;
    c->hz_rp.swap(rps);
    c->hz_core_off.swap(offs);
    c->hz_nstack = nstack;
    return C3SC_OK;
}

int c3sc_hip_upload_value_device(c3sc_hip_ctx *c, const size_t *ranks, const double *const *d_cores, void *stream)
{
    size_t cd = 0;
    int rc = prepare_value(c, ranks, &cd);
    if (rc != C3SC_OK) return rc;
    const int d = c->d, rp = c->rp;
    PadJobs J{};
    J.d = d;
    long maxtotal = 1;
    for (int m = 0; m < d; m++) {
        J.src[m] = d_cores[m];
        J.dst[m] = c->core_off[m];
        J.N[m] = c->ngrid[m];
        J.r0[m] = (int)ranks[m];
        J.r1[m] = (int)ranks[m + 1];
        maxtotal = std::max(maxtotal, (long)c->ngrid[m] * ((m == 0 || m == d - 1) ? rp : rp * rp));
    }
    HIPCHK(c, pad_cores_launch(c->arena, J, rp, (unsigned)std::min<long>((maxtotal + 255) / 256, 1024), (hipStream_t)stream));
    HIPCHK(c, hipGetLastError());
    rc = make_quad_aux(c, stream);
    if (rc != C3SC_OK) return rc;
    c->have_value = true;
    return C3SC_OK;
}

static int fill_args(c3sc_hip_ctx *c, int k, size_t F, KArgs &A, bool need_model)
{
    if (!c) return C3SC_ERR_ARG;
    if (c->d == 0 || !c->have_boundary || !c->have_value) return fail(c, C3SC_ERR_ARG, "launch: grid, boundary and value must be set");
    if (need_model && (!c->have_mca || c->model == 0 || c->ncand == 0))
        return fail(c, C3SC_ERR_ARG, "launch: mca, model and controls must be set");
    if (k < 0 || k >= c->d) return fail(c, C3SC_ERR_ARG, "launch: dim_vary out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->static_dirty) {
        if (static_layout(c) != c->static_doubles)
            return fail(c, C3SC_ERR_ARG, "launch: static data changed size after upload_value; upload the value again");
        int rc = upload_static(c);
        if (rc != C3SC_OK) return rc;
    }
    std::memset(&A, 0, sizeof(A));
    A.d = c->d;
    A.k = k;
    A.N = c->ngrid[k];
    A.ncand = c->ncand;
    A.F = (long)F;
    for (int m = 0; m < c->d; m++) {
        A.ngrid[m] = c->ngrid[m];
        A.bctype[m] = c->bctype[m];
        A.xg_off[m] = c->xg_off_rel[m];
        A.core_off[m] = c->core_off[m];
        A.quad_coreT_off[m] = c->coreT_off[m];
        A.quad_aop_off[m] = c->aop_off[m];
        A.pair_img_off[m] = c->img_off[m];
        A.quad_imgL_off[m] = c->qimgL_off[m];
        A.quad_imgR_off[m] = c->qimgR_off[m];
    }
    A.img_base = c->arena;
    if (c->tabL_off && (c->tabL_off != pair_tabL_off(A, c->rp) || c->tabR_off != pair_tabR_off(A, c->rp)))
        return fail(c, C3SC_ERR_ARG, "launch: the pair kernel's product tables are not where the kernel looks for them");
    if (c->tab3L_off && (c->tab3L_off != pair_tab3L_off(A, c->rp) || c->tab3R_off != pair_tab3R_off(A, c->rp)))
        return fail(c, C3SC_ERR_ARG, "launch: the pair kernel's three-core tables are not where the kernel looks for them");
    A.cends = c->cends;
    A.memo_keys = nullptr; // only the launch paths that found a fiber-per-wave kernel switch the memo epilogue on
    A.skip = c->skip_flag;
    A.nobs = c->nobs;
    A.obs_off = c->obs_off;
    A.cands_off = c->cands_off;
    for (int t = 0; t < 4; t++) A.tab_off[t] = c->tab_off[t];
    A.cfeat_off = c->cfeat_off;
    A.h2 = c->h2;
    A.discount = c->discount;
    for (int i = 0; i < 2 * c->d; i++) A.t[i] = c->t[i];
    for (int i = 0; i < C3SC_MAX_PARAMS; i++) A.prm[i] = c->prm[i];
    A.status = c->d_status;
    A.game_gsz = c->game_gsz; // 0 unless c3sc_hip_set_game: read by the game instantiations only
    A.game_ngrp = c->game_ngrp;
    A.game_order = c->game_order;
    A.hz_off = c->hz_dt > 0.0 ? c->hz_off : 0; // > 0 selects the horizon instantiations of a run-time compiled model
    { // ablation switches of the diagnostic build (make STAMPS=1); read once
        static const int dbg_env = [] { const char *e = getenv("C3SC_DBG"); return e ? atoi(e) : 0; }();
        A.dbg = dbg_env;
        if (dbg_env && !c->d_dbg) { HIPCHK(c, hipMalloc((void **)&c->d_dbg, 65536 * 8 * sizeof(unsigned long long))); } // stamp buffer
        A.dbgbuf = c->d_dbg;
        if (A.dbg & 8) A.ncand = 1;
        if (A.dbg & 16) A.ncand = 3;
    }
    return C3SC_OK;
}

// switch the memo epilogue of the fiber-per-wave kernel on for this launch if one was requested (c3sc_hip_cross_iteration)
static void arm_memo(c3sc_hip_ctx *c, const KernelEntry *e, KArgs &A)
{
    A.memo_keys = nullptr;
    if (c->memo.keys == nullptr || e->variant != C3SC_VARIANT_FIBER_PER_WAVE) return;
    A.memo_keys = c->memo.keys; A.memo_vals = c->memo.vals; A.memo_capmask = c->memo.capmask; A.memo_epoch_bits = c->memo.epoch_bits;
    A.memo_shift = c->memo.shift; A.memo_counters = c->memo.counters; A.memo_mode = c->memo.mode;
    for (int m = 0; m < c->d; m++) A.memo_stride[m] = c->memo.stride[m];
    c->memo.applied = true;
}

// the one launch of a call served by a single kernel entry: counted (c3sc_hip_launch_count), the cached status word dropped; with
// `unsupported`, a launcher that does not serve the call (hipErrorNotSupported) is reported as C3SC_ERR_UNSUPPORTED with that text
// every launch through a context carries its switches: a run-time compiled model's kernels of that form run (rtc_launch; the
// compiled-in kernels and the model-independent stencil kernels have no forms)
static hipError_t ctx_launch(const c3sc_hip_ctx *c, const KernelEntry &e, const KArgs &A, LaunchIO io)
{
    io.form = c->switches;
    // Parked node split of the pair kernels (kernel_fiber_pair.hpp: fpp_parked).  C3SC_PAIR_PARKED, read at every launch like
    // C3SC_PAIR_TABLE3: 0 runs the rank-split kernels it replaces, in the same build
    const char *pk = getenv("C3SC_PAIR_PARKED");
    io.parked = !(pk && *pk && atol(pk) == 0);
    return launch_entry(e, A, io);
}

static int launch_one(c3sc_hip_ctx *c, const KernelEntry *e, const KArgs &A, const LaunchIO &io, const char *unsupported = nullptr)
{
    c->last_kernel = e->name;
    g_launches++;
    c->status_cache_valid = false;
    const hipError_t he = ctx_launch(c, *e, A, io);
    if (he == hipErrorNotSupported && unsupported) return fail(c, C3SC_ERR_UNSUPPORTED, unsupported);
    HIPCHK(c, he);
    return C3SC_OK;
}

// Smallest batch the fiber-pair launches partition (fiber_partition.hpp).  C3SC_FIBER_PARTITION, read at every launch, replaces
// it: 0 switches the pass off, n > 0 runs it from n fibers on.  The three partition launches stand in front of every pair launch
// whatever the batch, what the absorbed and the grouped tiles save grows with it.  Traced at 2^20 fibers and 1682 bins the pass
// takes 40 us per launch (count 20.5, scan 9.2, scatter 10.9; 53 us while the scatter sorted, 42 us before the grouping, and never
// the 10 us first inferred here).  car7d, ms per step (profiles/r10_car7d_prepass.txt), pass off -> on:
//   2^17 fibers  1.469 -> 1.543 (an earlier build; not measured again)
//   2^18 fibers  2.660-2.711 -> 2.577-2.605, three alternating runs each way: the slowest run with the pass is 2.0 % under the
//                fastest without it, so the threshold came down from 2^19 to here
//   2^19 fibers  4.969-4.980 -> 4.789-4.827 and 2^20 fibers 9.320-9.365 -> 8.870-8.895 (profiles/r07_car7d_grouped_fold.txt)
// The grouping by the fold's key levels rides in the same three launches (FPART_MIN_PER_BIN in fiber_partition.hpp: two keys from
// 128 fibers per key on; 2^18 fibers are 156 per key).
constexpr long FIBER_PARTITION_MIN = 262144;
static long fiber_partition_min()
{
    const char *e = getenv("C3SC_FIBER_PARTITION");
    if (!e || !*e) return FIBER_PARTITION_MIN;
    const long v = atol(e);
    return v > 0 ? v : -1;
}

// Live fibers first (fiber_partition.hpp) for a fiber-pair launch of a batch that can hold absorbed fibers: some fixed dimension
// is absorbing.  Enqueued on the launch's stream into the scratch block `slot`; io.perm stays null where the pass does not run.
// `launched` reports the pass's kernel launches; the pair launcher's own early refusal (launch_fpp_impl: more than 64 candidates) is
// anticipated here, so that nothing is enqueued in front of a launcher that declines.
// C3SC_FIBER_GROUP, read at every launch like C3SC_FIBER_PARTITION: 0 leaves the partition at live fibers first (no grouping by
// the fold's key levels), n > 0 replaces FPART_MIN_PER_BIN, the fewest fibers per bin a key level is grouped by (1: every batch
// the bin cap allows -- a setting for the tests, which group batches of a few hundred fibers)
static long fiber_group_floor()
{
    const char *e = getenv("C3SC_FIBER_GROUP");
    if (!e || !*e) return FPART_MIN_PER_BIN;
    const long v = atol(e);
    return v > 0 ? v : -1;
}

// C3SC_FIBER_RANK, read at every launch like C3SC_FIBER_PARTITION: 0 runs the pre-pass with the sorting kernels of
// fiber_partition.hpp in the same build (the same permutation; for comparing the two)
static bool fiber_rank()
{
    const char *e = getenv("C3SC_FIBER_RANK");
    return !(e && *e && atol(e) == 0);
}

// whether partition_fibers runs its pass for this launch
static bool partitions(const KernelEntry *e, const KArgs &A)
{
    if (e->variant != C3SC_VARIANT_FIBER_PAIR || e->rtc || A.ncand > 64) return false;
    bool faces = false;
    for (int m = 0; m < A.d; m++) faces = faces || (m != A.k && A.bctype[m] == C3SC_ABSORB);
    const long fmin = fiber_partition_min();
    return faces && fmin >= 0 && A.F >= fmin && A.F <= 0x40000000L; // perm and nlive are int32
}

// Three-core product tables (kernel_common.hpp: pair_tab3L_off).  C3SC_PAIR_TABLE3, read at every launch like
// C3SC_FIBER_PARTITION: 0 runs the two-core kernels in the same build.  A launch runs a three-core kernel when it partitions, the
// tables are reserved and not switched off, and its K is not on the opt-out list (launch_fpp picks the kernel by LaunchIO::tab3).
static bool runs_tab3(const c3sc_hip_ctx *c, const KernelEntry *e, const KArgs &A)
{
    if (!c->tab3L_off || fpp_table3_optout(A.d, e->rp, A.k) || !partitions(e, A)) return false;
    const char *env = getenv("C3SC_PAIR_TABLE3");
    return !(env && *env && atol(env) == 0);
}

// The tables are built lazily, so that the solver's small batches and every launch without a partition never pay for them: after an
// upload the first launch that runs a three-core kernel enqueues the build on its stream, ahead of its pre-pass
// (c3sc_hip_bellman_fibers_all: before it forks its streams).  A later launch on another stream waits for the build's event.  The
// build is not counted by c3sc_hip_launch_count: it belongs to the upload, like k_core_images.
static int ensure_tab3(c3sc_hip_ctx *c, hipStream_t st)
{
    if (!c->tab3_stale) {
        if (st != c->tab3_stream) HIPCHK(c, hipStreamWaitEvent(st, c->tab3_ev, 0));
        return C3SC_OK;
    }
    const int d = c->d, rp = c->rp;
    if (!c->tab3_ev) HIPCHK(c, hipEventCreateWithFlags(&c->tab3_ev, hipEventDisableTiming));
    Tab3Jobs J{};
    const Tab3Sides sides = fpp_table3_sides(d, rp); // a table no kernel of this (dimension count, rank) reads stays unbuilt
    int n = 0;
    long total = 0;
    if (sides.left) {
        J.left[n] = 1;
        J.tab2[n] = c->tabL_off; J.core[n] = c->core_off[2]; J.dst[n] = c->tab3L_off;
        J.n3[n] = c->ngrid[2]; J.npairs[n] = c->ngrid[0] * c->ngrid[1];
        total = std::max(total, (long)J.n3[n] * J.npairs[n] * rp);
        n++;
    }
    if (sides.right) {
        J.left[n] = 0;
        J.tab2[n] = c->tabR_off; J.core[n] = c->core_off[d - 3]; J.dst[n] = c->tab3R_off;
        J.n3[n] = c->ngrid[d - 3]; J.npairs[n] = c->ngrid[d - 2] * c->ngrid[d - 1];
        total = std::max(total, (long)J.n3[n] * J.npairs[n] * rp);
        n++;
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_pair_tab3, dim3((unsigned)std::min<long>((total + 255) / 256, 4096), (unsigned)n), dim3(256), 0, st, c->arena, J, rp);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->tab3_ev, st));
    c->tab3_stream = st;
    c->tab3_stale = false;
    return C3SC_OK;
}

static int partition_fibers(c3sc_hip_ctx *c, const KernelEntry *e, const KArgs &A, LaunchIO &io, int slot, int &launched)
{
    io.perm = nullptr;
    io.nlive = nullptr;
    launched = 0;
    if (!partitions(e, A)) return C3SC_OK;
    PartArgs P;
    P.d = A.d;
    P.k = A.k;
    P.F = A.F;
    for (int m = 0; m < MAXD; m++) { P.ngrid[m] = A.ngrid[m]; P.bctype[m] = A.bctype[m]; }
    fpart_plan(P, fpp_group_levels(A.d, e->rp, A.k), fiber_group_floor()); // the keys of the grouped fold, where the kernel has one
    const size_t need = fpart_bytes(A.F, P.nbins);
    if (need > c->part_bytes[slot]) {
        if (c->part[slot]) HIPCHK(c, hipFree(c->part[slot])); // synchronises the device: the launches that read the block are done
        c->part[slot] = nullptr;
        c->part_bytes[slot] = 0;
        c->part_last[slot] = {}; // c3sc_hip_last_partition must not read the freed block
        HIPCHK(c, hipMalloc(&c->part[slot], need));
        c->part_bytes[slot] = need;
    }
    const PartScratch ps = fpart_carve(c->part[slot], A.F, P.nbins);
    c->part_last[slot] = {ps.perm, ps.nlive, A.F, io.stream};
    HIPCHK(c, fiber_rank() ? fpart_launch(P, io.idx, ps, io.stream) : fpart_launch_sorting(P, io.idx, ps, io.stream));
    launched = 3;
    io.perm = ps.perm;
    io.nlive = ps.nlive;
    return C3SC_OK;
}

static int launch_bellman(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, const int32_t *d_policy, double *d_out,
                          int32_t *d_uidx, int32_t *d_absorbed, void *stream, int part_slot = 0)
{
    KArgs A;
    int rc = fill_args(c, k, F, A, true);
    if (rc != C3SC_OK) return rc;
    int variant = c->variant;
    for (const FormRow &r : FORM_ROWS) { // a feature that is on: only the per-wave kernel has its form (AUTO picks it)
        if (!(ctx_form(c) & r.bit)) continue;
        rc = check_form_model(c, "bellman_fibers", r.bit);
        if (rc != C3SC_OK) return rc;
        if (variant != C3SC_VARIANT_AUTO && variant != C3SC_VARIANT_FIBER_PER_WAVE)
            return fails(c, C3SC_ERR_UNSUPPORTED, "bellman_fibers: " + verb(r, "runs", "run") + " on the fiber-per-wave kernel only (the pair and quad variants have no " +
                                                      r.kind + " form)");
        variant = C3SC_VARIANT_FIBER_PER_WAVE;
    }
    if (F == 0) return C3SC_OK;
    if (!d_idx || !d_out) return fail(c, C3SC_ERR_ARG, "bellman_fibers: null buffer");
    A.forced = d_policy;
    LaunchIO io{c->arena, d_idx, d_out, d_uidx, d_absorbed, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream};
    // A launcher declines (nothing launched) when its LDS layout does not fit this grid or it does not serve this call; the
    // next-best instantiation of the same padded rank is tried then (e.g. the duo kernel's two staging buffers hold N <= 25 at
    // rank 16, the one-buffer quad kernel behind it N <= 75, the per-wave kernel behind that only stages the varying core).
    std::vector<const KernelEntry *> declined;
    hipError_t he = hipSuccess;
    int part_launches = 0; // of the entry that served the call
    for (;;) {
        const KernelEntry *e = find_kernel(c->model, c->d, c->rp, A.N, variant, k, F, &declined);
        if (!e || e->rp != c->rp) {
            if (declined.empty()) return fail(c, C3SC_ERR_UNSUPPORTED, "bellman_fibers: no kernel instantiation for (model, dim, rank, N)");
            return fail(c, C3SC_ERR_UNSUPPORTED, he == hipErrorOutOfMemory
                            ? "bellman_fibers: N x rank^2 of the varying core exceeds the 160 KB of LDS the per-wave kernel stages it in"
                            : "bellman_fibers: no kernel instantiation serves this call (model, dim, rank, N, control mode)");
        }
        c->last_kernel = e->name;
        arm_memo(c, e, A);
        io.tab3 = runs_tab3(c, e, A);
        if (io.tab3) {
            rc = ensure_tab3(c, io.stream);
            if (rc != C3SC_OK) return rc;
        }
        rc = partition_fibers(c, e, A, io, part_slot, part_launches);
        if (rc != C3SC_OK) return rc;
        he = ctx_launch(c, *e, A, io);
        if (he != hipErrorOutOfMemory && he != hipErrorNotSupported) break;
        c->memo.applied = false;
        if (getenv("C3SC_VERBOSE")) fprintf(stderr, "c3sc: %s declined (%s), trying the next instantiation\n", e->name, hipGetErrorName(he));
        declined.push_back(e);
    }
    g_launches += 1 + part_launches;
    if (io.tab3 && io.perm) g_tab3_launches++;
    c->status_cache_valid = false;
    HIPCHK(c, he);
    return C3SC_OK;
}

int c3sc_hip_bellman_fibers(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, double *d_out, int32_t *d_uidx,
                            int32_t *d_absorbed, void *stream)
{
    return launch_bellman(c, k, F, d_idx, nullptr, d_out, d_uidx, d_absorbed, stream);
}

// All varying dimensions of one batch.  The launches are independent, so they are spread over the caller's stream and two side
// streams (forked from and joined to the caller's stream by events): the next dimension's workgroups fill the slots the previous
// dimension's last tiles leave.  Stream-ordered like a single launch: work enqueued on `stream` before / after the call runs
// before / after all of it.  With a memo or skip flag armed (the cross iterations' sequential steps), small AUTO batches or
// C3SC_NO_OVERLAP=1 the launches simply run in order on `stream`.
static int launch_bellman_all(c3sc_hip_ctx *c, int nk, const int *ks, const size_t *F, const int32_t *const *d_idx,
                              const int32_t *const *d_policy, double *const *d_out, int32_t *const *d_uidx, int32_t *const *d_absorbed,
                              void *stream)
{
    if (!c) return C3SC_ERR_ARG;
    if (nk < 1 || nk > MAXD || !ks || !F || !d_idx || !d_out) return fail(c, C3SC_ERR_ARG, "bellman_fibers_all: bad arguments");
    static const bool no_overlap = getenv("C3SC_NO_OVERLAP") != nullptr;
    bool overlap = nk > 1 && !no_overlap && c->memo.keys == nullptr && c->skip_flag == nullptr;
    for (int s = 0; s < nk; s++) {
        if (ks[s] < 0 || ks[s] >= c->d) return fail(c, C3SC_ERR_ARG, "bellman_fibers_all: dim_vary out of range");
        if (F[s] > 0 && (!d_idx[s] || !d_out[s])) return fail(c, C3SC_ERR_ARG, "bellman_fibers_all: null buffer");
        if (d_policy && !d_policy[s]) return fail(c, C3SC_ERR_ARG, "bellman_fibers_all: null policy");
        for (int q = 0; q < s; q++)
            if (d_out[q] == d_out[s] && F[s] > 0) return fail(c, C3SC_ERR_ARG, "bellman_fibers_all: two segments share an output array");
    }
    hipStream_t st = (hipStream_t)stream;
    if (overlap && c->tab3L_off && c->tab3_stale && ctx_form(c) == 0) {
        // stale three-core tables: built here, ahead of the fork, if a segment is going to run a three-core kernel -- every
        // side stream is then ordered behind the build by the fork itself
        const long fmin = fiber_partition_min();
        for (int s = 0; s < nk && c->tab3_stale; s++) {
            if (F[s] == 0 || fmin < 0 || (long)F[s] < fmin) continue; // no partition, no three-core kernel: nothing to look up
            KArgs A;
            int rc = fill_args(c, ks[s], F[s], A, true);
            if (rc != C3SC_OK) return rc;
            const KernelEntry *e = find_kernel(c->model, c->d, c->rp, A.N, c->variant, ks[s], F[s]);
            if (e && e->rp == c->rp && runs_tab3(c, e, A)) {
                rc = ensure_tab3(c, st);
                if (rc != C3SC_OK) return rc;
            }
        }
    }
    if (overlap) {
        HIPCHK(c, hipSetDevice(c->device));
        if (!c->fork_ev) {
            HIPCHK(c, hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
            for (int i = 0; i < c3sc_hip_ctx::NSIDE; i++) {
                HIPCHK(c, hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking));
                HIPCHK(c, hipEventCreateWithFlags(&c->join_ev[i], hipEventDisableTiming));
            }
        }
        HIPCHK(c, hipEventRecord(c->fork_ev, st));
        for (int i = 0; i < c3sc_hip_ctx::NSIDE; i++) HIPCHK(c, hipStreamWaitEvent(c->side[i], c->fork_ev, 0));
    }
    int rc = C3SC_OK;
    for (int s = 0; s < nk && rc == C3SC_OK; s++) {
        const int lane = overlap ? s % (c3sc_hip_ctx::NSIDE + 1) : 0; // 0: the caller's stream
        rc = launch_bellman(c, ks[s], F[s], d_idx[s], d_policy ? d_policy[s] : nullptr, d_out[s], d_uidx ? d_uidx[s] : nullptr,
                            d_absorbed ? d_absorbed[s] : nullptr, lane == 0 ? stream : (void *)c->side[lane - 1], lane);
    }
    if (overlap) // join even after a failed launch: what was enqueued on the side streams must not outlive the call's ordering
        for (int i = 0; i < c3sc_hip_ctx::NSIDE; i++) {
            HIPCHK(c, hipEventRecord(c->join_ev[i], c->side[i]));
            HIPCHK(c, hipStreamWaitEvent(st, c->join_ev[i], 0));
        }
    return rc;
}

int c3sc_hip_bellman_fibers_all(c3sc_hip_ctx *c, int nk, const int *ks, const size_t *F, const int32_t *const *d_idx, double *const *d_out,
                                int32_t *const *d_uidx, int32_t *const *d_absorbed, void *stream)
{
    return launch_bellman_all(c, nk, ks, F, d_idx, nullptr, d_out, d_uidx, d_absorbed, stream);
}

int c3sc_hip_policy_fibers_all(c3sc_hip_ctx *c, int nk, const int *ks, const size_t *F, const int32_t *const *d_idx,
                               const int32_t *const *d_policy, double *const *d_out, int32_t *const *d_absorbed, void *stream)
{
    if (!d_policy) return fail(c, C3SC_ERR_ARG, "policy_fibers_all: null policy");
    return launch_bellman_all(c, nk, ks, F, d_idx, d_policy, d_out, nullptr, d_absorbed, stream);
}

static int launch_box(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, const double *d_policy_u, double *d_out,
                      double *d_uopt, int32_t *d_absorbed, void *stream)
{
    if (!c) return C3SC_ERR_ARG;
    if (c->box_du == 0) return fail(c, C3SC_ERR_ARG, "bellman_fibers_box: c3sc_hip_set_control_box first");
    for (const FormRow &r : FORM_ROWS)
        if ((ctx_form(c) & r.bit) && !form_offered(r.bit, FORM_BOX)) return no_box_form(c, "bellman_fibers_box", r);
    if (model_ncf(c->model) != 0 && c->model != C3SC_MODEL_COTHRUST6D) // cothrust forms its features from u on the device (models.hpp: CF_FROM_U)
        return fail(c, C3SC_ERR_UNSUPPORTED, "bellman_fibers_box: this model needs transcendental functions of the control");
    KArgs A;
    int rc = fill_args(c, k, F, A, true);
    if (rc != C3SC_OK) return rc;
    if (F == 0) return C3SC_OK;
    if (!d_idx || !d_out) return fail(c, C3SC_ERR_ARG, "bellman_fibers_box: null buffer");
    A.cmode = 1;
    A.ugrid = c->box_grid;
    A.upolish = c->box_polish;
    for (int i = 0; i < c->box_du; i++) { A.ulb[i] = c->box_lb[i]; A.uub[i] = c->box_ub[i]; }
    A.uopt = d_uopt;
    A.forced_u = d_policy_u;
    const KernelEntry *e = find_kernel(c->model, c->d, c->rp, A.N, C3SC_VARIANT_FIBER_PER_WAVE, k);
    if (!e || e->rp != c->rp) return fail(c, C3SC_ERR_UNSUPPORTED, "bellman_fibers_box: no fiber-per-wave instantiation for (model, dim, rank, N)");
    arm_memo(c, e, A);
    LaunchIO io{c->arena, d_idx, d_out, nullptr, d_absorbed, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream};
    return launch_one(c, e, A, io, "bellman_fibers_box: no box-minimiser instantiation for this model");
}

int c3sc_hip_bellman_fibers_box(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, double *d_out, double *d_uopt,
                                int32_t *d_absorbed, void *stream)
{
    return launch_box(c, k, F, d_idx, nullptr, d_out, d_uopt, d_absorbed, stream);
}

int c3sc_hip_policy_fibers_box(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, const double *d_policy_u, double *d_out,
                               int32_t *d_absorbed, void *stream)
{
    if (F != 0 && !d_policy_u) return fail(c, C3SC_ERR_ARG, "policy_fibers_box: null policy");
    return launch_box(c, k, F, d_idx, d_policy_u, d_out, nullptr, d_absorbed, stream);
}

int c3sc_hip_bellman_fibers_box_host(c3sc_hip_ctx *c, int k, size_t F, const int32_t *h_idx, double *h_out, double *h_uopt,
                                     int32_t *h_absorbed)
{
    if (!c || c->d == 0 || k < 0 || k >= c->d || c->box_du == 0) return fail(c, C3SC_ERR_ARG, "bellman_fibers_box_host: bad arguments");
    if (F == 0) return C3SC_OK;
    const size_t FN = F * c->ngrid[k];
    return stage_host(c, STAGE_MAPPED_OR_SCRATCH, "bellman_fibers_box_host",
                      {{h_idx, F * c->d * sizeof(int32_t), SEG_IN}, {h_out, FN * sizeof(double), SEG_OUT},
                       {h_uopt, FN * c->box_du * sizeof(double), SEG_OUT}, {h_absorbed, FN * sizeof(int32_t), SEG_OUT}},
                      [&](const DevPtr *d) { return c3sc_hip_bellman_fibers_box(c, k, F, d[0], d[1], d[2], d[3], nullptr); });
}

int c3sc_hip_policy_fibers_box_host(c3sc_hip_ctx *c, int k, size_t F, const int32_t *h_idx, const double *h_policy_u, double *h_out,
                                    int32_t *h_absorbed)
{
    if (F != 0 && !h_policy_u) return fail(c, C3SC_ERR_ARG, "policy_fibers_box_host: null policy");
    if (!c || c->d == 0 || k < 0 || k >= c->d || c->box_du == 0) return fail(c, C3SC_ERR_ARG, "policy_fibers_box_host: bad arguments");
    if (F == 0) return C3SC_OK;
    const size_t FN = F * c->ngrid[k];
    return stage_host(c, STAGE_MAPPED_OR_SCRATCH, "policy_fibers_box_host",
                      {{h_idx, F * c->d * sizeof(int32_t), SEG_IN}, {h_out, FN * sizeof(double), SEG_OUT},
                       {h_policy_u, FN * c->box_du * sizeof(double), SEG_IN}, {h_absorbed, FN * sizeof(int32_t), SEG_OUT}},
                      [&](const DevPtr *d) { return c3sc_hip_policy_fibers_box(c, k, F, d[0], d[2], d[1], d[3], nullptr); });
}

int c3sc_hip_policy_fibers(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, const int32_t *d_policy, double *d_out,
                           int32_t *d_absorbed, void *stream)
{
    if (F != 0 && !d_policy) return fail(c, C3SC_ERR_ARG, "policy_fibers: null policy");
    return launch_bellman(c, k, F, d_idx, d_policy, d_out, nullptr, d_absorbed, stream);
}

static int launch_tables(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, const double *d_tables, const double *d_costs2,
                         const int32_t *d_policy, double *d_out, int32_t *d_uidx, int32_t *d_absorbed, void *stream)
{
    if (!c) return C3SC_ERR_ARG;
    const int saved_model = c->model;
    for (const FormRow &r : FORM_ROWS)
        if (ctx_form(c) & r.bit) return fails(c, C3SC_ERR_UNSUPPORTED, std::string("bellman_fibers_tables: the TABLE model has no ") + r.kind + " kernels");
    c->model = C3SC_MODEL_TABLE; // fill_args only checks that a model is set
    KArgs A;
    int rc = fill_args(c, k, F, A, true);
    c->model = saved_model;
    if (rc != C3SC_OK) return rc;
    if (F == 0) return C3SC_OK;
    if (!d_idx || !d_out || !d_tables || !d_costs2) return fail(c, C3SC_ERR_ARG, "bellman_fibers_tables: null buffer");
    A.forced = d_policy;
    const KernelEntry *e = find_kernel(C3SC_MODEL_TABLE, c->d, c->rp, A.N, C3SC_VARIANT_AUTO, k);
    if (!e || e->rp != c->rp) return fail(c, C3SC_ERR_UNSUPPORTED, "bellman_fibers_tables: no kernel instantiation for (dim, rank, N)");
    LaunchIO io{c->arena, d_idx, d_out, d_uidx, d_absorbed, nullptr, nullptr, d_tables, d_costs2, (hipStream_t)stream};
    return launch_one(c, e, A, io);
}

int c3sc_hip_bellman_fibers_tables(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, const double *d_tables,
                                   const double *d_costs2, double *d_out, int32_t *d_uidx, int32_t *d_absorbed, void *stream)
{
    return launch_tables(c, k, F, d_idx, d_tables, d_costs2, nullptr, d_out, d_uidx, d_absorbed, stream);
}

int c3sc_hip_policy_fibers_tables(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, const double *d_tables,
                                  const double *d_costs2, const int32_t *d_policy, double *d_out, int32_t *d_absorbed, void *stream)
{
    if (F != 0 && !d_policy) return fail(c, C3SC_ERR_ARG, "policy_fibers_tables: null policy");
    return launch_tables(c, k, F, d_idx, d_tables, d_costs2, d_policy, d_out, nullptr, d_absorbed, stream);
}

int c3sc_hip_bellman_fibers_tables_host(c3sc_hip_ctx *c, int k, size_t F, const int32_t *h_idx, const double *h_tables,
                                        const double *h_costs2, double *h_out, int32_t *h_uidx, int32_t *h_absorbed)
{
    if (!c || c->d == 0 || k < 0 || k >= c->d || c->ncand == 0) return fail(c, C3SC_ERR_ARG, "bellman_fibers_tables_host: bad arguments");
    if (F == 0) return C3SC_OK;
    const size_t FN = F * c->ngrid[k], S = 2 * c->d + 1;
    return stage_host(c, STAGE_SCRATCH, "bellman_fibers_tables_host",
                      {{h_idx, F * c->d * sizeof(int32_t), SEG_IN}, {h_out, FN * sizeof(double), SEG_OUT}, {h_uidx, FN * sizeof(int32_t), SEG_OUT},
                       {h_absorbed, FN * sizeof(int32_t), SEG_OUT}, {h_tables, FN * c->ncand * S * sizeof(double), SEG_IN},
                       {h_costs2, FN * 2 * sizeof(double), SEG_IN}},
                      [&](const DevPtr *d) { return c3sc_hip_bellman_fibers_tables(c, k, F, d[0], d[4], d[5], d[1], d[2], d[3], nullptr); });
}

int c3sc_hip_policy_fibers_tables_host(c3sc_hip_ctx *c, int k, size_t F, const int32_t *h_idx, const double *h_tables,
                                       const double *h_costs2, const int32_t *h_policy, double *h_out, int32_t *h_absorbed)
{
    if (F != 0 && !h_policy) return fail(c, C3SC_ERR_ARG, "policy_fibers_tables_host: null policy");
    if (!c || c->d == 0 || k < 0 || k >= c->d || c->ncand == 0) return fail(c, C3SC_ERR_ARG, "policy_fibers_tables_host: bad arguments");
    if (F == 0) return C3SC_OK;
    const size_t FN = F * c->ngrid[k], S = 2 * c->d + 1;
    return stage_host(c, STAGE_SCRATCH, "policy_fibers_tables_host",
                      {{h_idx, F * c->d * sizeof(int32_t), SEG_IN}, {h_out, FN * sizeof(double), SEG_OUT}, {h_policy, FN * sizeof(int32_t), SEG_IN},
                       {h_absorbed, FN * sizeof(int32_t), SEG_OUT}, {h_tables, FN * c->ncand * S * sizeof(double), SEG_IN},
                       {h_costs2, FN * 2 * sizeof(double), SEG_IN}},
                      [&](const DevPtr *d) { return c3sc_hip_policy_fibers_tables(c, k, F, d[0], d[4], d[5], d[2], d[1], d[3], nullptr); });
}

int c3sc_hip_stencil_fibers(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, double *d_costs, int32_t *d_absorbed,
                            void *stream)
{
    return c3sc_hip_stencil_fibers_nb(c, k, F, d_idx, nullptr, nullptr, d_costs, d_absorbed, stream);
}

int c3sc_hip_stencil_fibers_nb(c3sc_hip_ctx *c, int k, size_t F, const int32_t *d_idx, const int32_t *d_nb_fixed,
                               const int32_t *d_nb_vary, double *d_costs, int32_t *d_absorbed, void *stream)
{
    KArgs A;
    int rc = fill_args(c, k, F, A, false);
    if (rc != C3SC_OK) return rc;
    if (F == 0) return C3SC_OK;
    if (!d_idx || !d_costs) return fail(c, C3SC_ERR_ARG, "stencil_fibers: null buffer");
    const KernelEntry *e = find_kernel(0, c->d, c->rp, A.N, C3SC_VARIANT_AUTO, k);
    if (!e || e->rp != c->rp) return fail(c, C3SC_ERR_UNSUPPORTED, "stencil_fibers: no kernel instantiation for (dim, rank, N)");
    LaunchIO io{c->arena, d_idx, d_costs, nullptr, d_absorbed, d_nb_fixed, d_nb_vary, nullptr, nullptr, (hipStream_t)stream};
    return launch_one(c, e, A, io);
}

int c3sc_hip_bellman_fibers_host(c3sc_hip_ctx *c, int k, size_t F, const int32_t *h_idx, double *h_out, int32_t *h_uidx,
                                 int32_t *h_absorbed)
{
    if (!c || c->d == 0 || k < 0 || k >= c->d) return fail(c, C3SC_ERR_ARG, "bellman_fibers_host: bad arguments");
    if (F == 0) return C3SC_OK;
    const size_t FN = F * c->ngrid[k];
    return stage_host(c, STAGE_MAPPED_OR_SCRATCH, "bellman_fibers_host",
                      {{h_idx, F * c->d * sizeof(int32_t), SEG_IN}, {h_out, FN * sizeof(double), SEG_OUT},
                       {h_uidx, FN * sizeof(int32_t), SEG_OUT}, {h_absorbed, FN * sizeof(int32_t), SEG_OUT}},
                      [&](const DevPtr *d) { return c3sc_hip_bellman_fibers(c, k, F, d[0], d[1], d[2], d[3], nullptr); });
}

int c3sc_hip_policy_fibers_host(c3sc_hip_ctx *c, int k, size_t F, const int32_t *h_idx, const int32_t *h_policy, double *h_out,
                                int32_t *h_absorbed)
{
    if (!c || c->d == 0 || k < 0 || k >= c->d || (F != 0 && !h_policy)) return fail(c, C3SC_ERR_ARG, "policy_fibers_host: bad arguments");
    if (F == 0) return C3SC_OK;
    const size_t FN = F * c->ngrid[k];
    return stage_host(c, STAGE_MAPPED_OR_SCRATCH, "policy_fibers_host",
                      {{h_idx, F * c->d * sizeof(int32_t), SEG_IN}, {h_out, FN * sizeof(double), SEG_OUT},
                       {h_policy, FN * sizeof(int32_t), SEG_IN}, {h_absorbed, FN * sizeof(int32_t), SEG_OUT}},
                      [&](const DevPtr *d) { return c3sc_hip_policy_fibers(c, k, F, d[0], d[2], d[1], d[3], nullptr); });
}

int c3sc_hip_stencil_fibers_host(c3sc_hip_ctx *c, int k, size_t F, const int32_t *h_idx, double *h_costs, int32_t *h_absorbed)
{
    return c3sc_hip_stencil_fibers_nb_host(c, k, F, h_idx, nullptr, nullptr, h_costs, h_absorbed);
}

int c3sc_hip_stencil_fibers_nb_host(c3sc_hip_ctx *c, int k, size_t F, const int32_t *h_idx, const int32_t *h_nb_fixed,
                                    const int32_t *h_nb_vary, double *h_costs, int32_t *h_absorbed)
{
    if (!c || c->d == 0 || k < 0 || k >= c->d) return fail(c, C3SC_ERR_ARG, "stencil_fibers_host: bad arguments");
    if (F == 0) return C3SC_OK;
    const size_t FN = F * c->ngrid[k], S = 2 * c->d + 1;
    return stage_host(c, STAGE_SCRATCH, "stencil_fibers_host",
                      {{h_idx, F * c->d * sizeof(int32_t), SEG_IN}, {h_costs, FN * S * sizeof(double), SEG_OUT},
                       {h_absorbed, FN * sizeof(int32_t), SEG_OUT}, {h_nb_fixed, F * 2 * (c->d - 1) * sizeof(int32_t), SEG_IN},
                       {h_nb_vary, FN * 2 * sizeof(int32_t), SEG_IN}},
                      [&](const DevPtr *d) { return c3sc_hip_stencil_fibers_nb(c, k, F, d[0], d[3], d[4], d[1], d[2], nullptr); });
}

int c3sc_hip_sync(c3sc_hip_ctx *c, void *stream)
{
    if (!c) return C3SC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
    return C3SC_OK;
}

int c3sc_hip_get_status(c3sc_hip_ctx *c, unsigned *flags, int clear)
{
    if (!c || !flags) return C3SC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->status_cache_valid) *flags = c->status_cache; /* read with the last cross fetch; nothing was launched since */
    else HIPCHK(c, hipMemcpy(flags, c->d_status, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (clear && *flags) { /* nothing to clear otherwise */
        HIPCHK(c, hipMemset(c->d_status, 0, sizeof(unsigned)));
        c->status_cache = 0;
    }
    return C3SC_OK;
}

// ------------------------------------------------------------------ closed-loop rollouts (kernel_rollout.hpp)
int c3sc_hip_set_interp(c3sc_hip_ctx *c, int constelm)
{
    if (!c) return C3SC_ERR_ARG;
    if (c->constelm != (constelm ? 1 : 0)) c->static_dirty = true; // the jump kernels read the class from the static section
    c->constelm = constelm ? 1 : 0;
    return C3SC_OK;
}

// one 1-D launch covers a call: 2^31 lanes stay below the launch limit of 2^32 work-items
static const size_t SIM_MAX_TRAJ = (size_t)1 << 31;

static const KernelEntry *find_sim_kernel(int variant, int model, int d, int rp)
{
    const KernelEntry *hit = nullptr;
    each_entry(model, [&](const KernelEntry &e) {
        if (!hit && e.variant == variant && e.model == model && e.d == d && e.rp == rp) hit = &e;
    });
    return hit;
}

static int check_bounds_set(c3sc_hip_ctx *c, const char *what)
{
    for (int m = 0; m < c->d; m++)
        if (c->bctype[m] != C3SC_ABSORB && c->bctype[m] != C3SC_PERIODIC && c->bctype[m] != C3SC_REFLECT)
            return fail(c, C3SC_ERR_ARG, what); // the host code asserts ("No boundary specified!")
    return C3SC_OK;
}

int c3sc_hip_stencil_points(c3sc_hip_ctx *c, size_t n, const double *d_x, double *d_out, int32_t *d_absorbed, void *stream)
{
    KArgs A;
    int rc = fill_args(c, 0, 0, A, false);
    if (rc != C3SC_OK) return rc;
    rc = check_bounds_set(c, "stencil_points: every dimension needs a boundary type");
    if (rc != C3SC_OK) return rc;
    if (n == 0) return C3SC_OK;
    if (!d_x || !d_out) return fail(c, C3SC_ERR_ARG, "stencil_points: null buffer");
    if (n > SIM_MAX_TRAJ) return fail(c, C3SC_ERR_ARG, "stencil_points: more than 2^31 points in one call");
    const KernelEntry *e = find_sim_kernel(VARIANT_STENCIL_POINTS, 0, c->d, c->rp);
    if (!e) return fail(c, C3SC_ERR_UNSUPPORTED, "stencil_points: no instantiation for this (dim, padded rank)");
    SimK S;
    std::memset(&S, 0, sizeof(S));
    S.n = (long)n;
    S.constelm = c->constelm;
    S.x0 = d_x;
    S.out = d_out;
    S.absorbed = d_absorbed;
    LaunchIO io{c->arena, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream, &S};
    return launch_one(c, e, A, io);
}

// ---- the front end c3sc_hip_simulate and c3sc_hip_integrate share.  who = "simulate" / "integrate" opens every message; Args is
// c3sc_hip_sim_args / c3sc_hip_ode_args (the fields read here have the same names in both).  The callers keep the order of their
// checks: it decides which error a bad call gets.
extern "C++" { // templates
static int failw(c3sc_hip_ctx *c, int code, const char *who, const char *msg) { return fail(c, code, (std::string(who) + msg).c_str()); }

// what the context must hold before a closed loop of either kind
template <class Args>
static int closed_loop_setup(c3sc_hip_ctx *c, const char *who, const Args *a)
{
    if (!c) return C3SC_ERR_ARG;
    if (!a) return failw(c, C3SC_ERR_ARG, who, ": null argument struct");
    if (c->model == C3SC_MODEL_TABLE) return failw(c, C3SC_ERR_UNSUPPORTED, who, ": the TABLE model has no device dynamics");
    if (!c->have_mca || c->model == 0) return failw(c, C3SC_ERR_ARG, who, ": mca and model must be set");
    if (a->box ? c->box_du == 0 : c->ncand == 0) return failw(c, C3SC_ERR_ARG, who, a->box ? ": set_control_box first" : ": set_controls first");
    if (a->box && model_ncf(c->model) != 0 && c->model != C3SC_MODEL_COTHRUST6D)
        return failw(c, C3SC_ERR_UNSUPPORTED, who, ": this model needs transcendental functions of the control in a box");
    if (a->box && c->game_gsz > 0) return no_box_form(c, who, form_row(FORM_GAME));
    if (check_form_model(c, who, FORM_GAME) != C3SC_OK) return C3SC_ERR_UNSUPPORTED;
    return C3SC_OK;
}

// the batch size and the rows saved of nouter steps; many / late: the caller's texts for too many trajectories and for a
// save_every beyond its step count
template <class Args>
static int closed_loop_sizes(c3sc_hip_ctx *c, const char *who, const Args *a, size_t nouter, const char *many, const char *late)
{
    if (a->n > SIM_MAX_TRAJ) return fail(c, C3SC_ERR_ARG, many);
    if (a->save_every == 0 && (a->d_traj || a->d_u)) return failw(c, C3SC_ERR_ARG, who, ": d_traj / d_u need save_every > 0");
    if (a->save_every > nouter && a->save_every > 1 && (a->d_traj || a->d_u)) return fail(c, C3SC_ERR_ARG, late);
    return C3SC_OK;
}

// the state between launches (x | cost | what the kernel adds), grow-only
static int closed_loop_state(c3sc_hip_ctx *c, size_t bytes)
{
    if (bytes <= c->sim_state_bytes) return C3SC_OK;
    if (c->sim_state) HIPCHK(c, hipFree(c->sim_state));
    c->sim_state = nullptr;
    c->sim_state_bytes = 0;
    HIPCHK(c, hipMalloc(&c->sim_state, bytes));
    c->sim_state_bytes = bytes;
    return C3SC_OK;
}

static void closed_loop_box(const c3sc_hip_ctx *c, int box, KArgs &A)
{
    A.cmode = box ? 1 : 0;
    A.ugrid = c->box_grid;
    A.upolish = c->box_polish;
    for (int i = 0; i < c->box_du; i++) { A.ulb[i] = c->box_lb[i]; A.uub[i] = c->box_ub[i]; }
}

static int copy_back(c3sc_hip_ctx *c, void *dst, const void *src, size_t bytes, void *stream)
{
    if (dst) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return C3SC_OK;
}

// final states, costs and the step each trajectory ended at (-1: none), from the state block to the caller's buffers
template <class Args>
static int closed_loop_results(c3sc_hip_ctx *c, const Args *a, int64_t *d_step, void *stream)
{
    const size_t n = a->n, d = (size_t)c->d;
    const double *st_x = (const double *)c->sim_state, *st_cost = st_x + n * d;
    int rc = copy_back(c, a->d_xfinal, st_x, n * d * sizeof(double), stream);
    if (rc == C3SC_OK) rc = copy_back(c, a->d_cost, st_cost, n * sizeof(double), stream);
    if (rc == C3SC_OK) rc = copy_back(c, d_step, st_cost + n, n * sizeof(int64_t), stream);
    return rc;
}

// the host-buffer variants: the checks before staging, and the buffer shapes (rows of d_traj and d_u per trajectory)
struct HostShape {
    size_t n, d, du, nrow, nurow;
};

template <class Args>
static int closed_loop_host_shape(c3sc_hip_ctx *c, const char *who, const Args *h, size_t nouter, HostShape &sh)
{
    if (!h->d_x0) return failw(c, C3SC_ERR_ARG, who, "_host: null x0");
    if (h->n > SIM_MAX_TRAJ || nouter > ((size_t)1 << 30)) return failw(c, C3SC_ERR_ARG, who, "_host: sizes too large");
    if (h->save_every == 0 && (h->d_traj || h->d_u)) return failw(c, C3SC_ERR_ARG, who, ": d_traj / d_u need save_every > 0");
    if (c->d == 0) return failw(c, C3SC_ERR_ARG, who, "_host: set_grid first");
    const size_t se = h->save_every;
    sh = {h->n, (size_t)c->d, (size_t)(h->box ? c->box_du : c->du), se ? nouter / se + 1 : 0, se ? (nouter + se - 1) / se : 0};
    return C3SC_OK;
}
} // extern "C++"

int c3sc_hip_simulate(c3sc_hip_ctx *c, const c3sc_hip_sim_args *a, void *stream)
{
    const char *who = "simulate";
    int rc = closed_loop_setup(c, who, a);
    if (rc != C3SC_OK) return rc;
    const bool hz = c->hz_dt > 0.0; // horizon mode: one launch per step, step k's controller on the cores of V_{k+1}
    // the features that are on, in this call's own order of refusals (it decides which error a call with several of them gets)
    for (unsigned bit : {FORM_HORIZON, FORM_JUMP, FORM_CORR, FORM_IMPULSE, FORM_STOP}) {
        const FormRow &r = form_row(bit);
        if (!(ctx_form(c) & bit)) continue;
        if (!form_offered(bit, FORM_ROLLOUT)) // correlated increments and off-grid diagonal targets are not offered
            return fails(c, C3SC_ERR_UNSUPPORTED, std::string("simulate: rollouts are not offered ") + r.problems + " (" + r.off + " first)");
        if (check_form_model(c, who, bit) != C3SC_OK) return C3SC_ERR_UNSUPPORTED;
        if (a->box) return no_box_form(c, who, r);
        if (bit != FORM_HORIZON) continue;
        if (c->hz_nstack == 0) return fail(c, C3SC_ERR_ARG, "simulate: horizon mode needs the value stack (c3sc_hip_upload_value_stack)");
        if (!(std::fabs(a->dt - c->hz_dt) <= 1e-12 * c->hz_dt))
            return fail(c, C3SC_ERR_ARG, "simulate: in horizon mode dt must equal the horizon step (c3sc_hip_set_horizon_step)");
        if (a->nsteps + 1 > (size_t)c->hz_nstack) return fail(c, C3SC_ERR_ARG, "simulate: nsteps exceeds the value stack (nstack - 1 stages)");
    }
    KArgs A;
    rc = fill_args(c, 0, 0, A, false);
    if (rc != C3SC_OK) return rc;
    if (hz) {
        if (c->hz_stack_static != c->static_doubles)
            return fail(c, C3SC_ERR_ARG, "simulate: static data changed size after upload_value_stack; upload the stack again");
        for (size_t s = 0; s <= a->nsteps; s++)
            if (!find_sim_kernel(VARIANT_ROLLOUT, c->model, c->d, c->hz_rp[s]))
                return fail(c, C3SC_ERR_UNSUPPORTED, "simulate: no rollout instantiation for a stage's padded rank");
    }
    rc = check_bounds_set(c, "simulate: every dimension needs a boundary type");
    if (rc != C3SC_OK) return rc;
    if (!(a->dt > 0.0) || !std::isfinite(a->dt)) return fail(c, C3SC_ERR_ARG, "simulate: dt must be positive and finite");
    if (a->nsteps > (size_t)1 << 30) return fail(c, C3SC_ERR_ARG, "simulate: nsteps too large");
    rc = closed_loop_sizes(c, who, a, a->nsteps, "simulate: more than 2^31 trajectories in one call (split the batch, traj_offset)",
                           "simulate: save_every larger than nsteps");
    if (rc != C3SC_OK) return rc;
    if (a->steps_per_launch < 0) return fail(c, C3SC_ERR_ARG, "simulate: steps_per_launch < 0");
    const KernelEntry *e = find_sim_kernel(VARIANT_ROLLOUT, c->model, c->d, hz ? c->hz_rp[a->nsteps] : c->rp);
    if (!e) return fail(c, C3SC_ERR_UNSUPPORTED, "simulate: no rollout instantiation for this model at this padded rank");
    if (a->n == 0) return C3SC_OK;
    if (!a->d_x0) return fail(c, C3SC_ERR_ARG, "simulate: null d_x0");
    const int d = c->d;
    const size_t n = a->n;
    rc = closed_loop_state(c, n * (size_t)(d + 2) * sizeof(double)); // x | cost | exit_step
    if (rc != C3SC_OK) return rc;
    closed_loop_box(c, a->box, A);
    SimK S;
    std::memset(&S, 0, sizeof(S));
    S.n = (long)n;
    S.traj_offset = (long long)a->traj_offset;
    S.nsteps = (int)a->nsteps;
    S.save_every = (int)a->save_every;
    S.wrap = a->wrap_periodic ? 1 : 0;
    S.constelm = c->constelm;
    S.seed = a->seed;
    S.dt = a->dt;
    S.sqdt = std::sqrt(a->dt);
    S.x0 = a->d_x0;
    S.noise = a->d_noise;
    S.x = (double *)c->sim_state;
    S.cost = S.x + n * d;
    S.exit_step = (long long *)(S.cost + n);
    S.traj = a->d_traj;
    S.u = a->d_u;
    S.vend = a->d_vend;
    const int chunk = hz ? 1 : (a->steps_per_launch > 0 ? a->steps_per_launch : 64);
    if (hz) HIPCHK(c, hipMemcpyAsync(c->hz_stack, c->arena, c->static_doubles * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    int s0 = 0;
    do { // at least one launch: nsteps = 0 still tests x_0 and evaluates V_end
        S.s0 = s0;
        S.s1 = (int)std::min<long long>((long long)s0 + chunk, (long long)a->nsteps);
        const KernelEntry *ek = e;
        double *ro = c->arena;
        if (hz) { // the launch of step s0 (or the terminal-only launch of nsteps = 0) reads stage s1: V_{s0+1}, and V_nsteps at the end
            for (int m = 0; m < c->d; m++) A.core_off[m] = c->hz_core_off[(size_t)S.s1 * MAXD + m];
            ek = find_sim_kernel(VARIANT_ROLLOUT, c->model, c->d, c->hz_rp[S.s1]);
            ro = c->hz_stack;
        }
        LaunchIO io{ro, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream, &S};
        rc = launch_one(c, ek, A, io, "simulate: this rollout kernel has no box minimiser");
        if (rc != C3SC_OK) return rc;
        s0 = S.s1;
    } while (s0 < (int)a->nsteps);
    return closed_loop_results(c, a, a->d_exit, stream);
}

int c3sc_hip_simulate_host(c3sc_hip_ctx *c, const c3sc_hip_sim_args *h)
{
    if (!c) return C3SC_ERR_ARG;
    if (!h) return fail(c, C3SC_ERR_ARG, "simulate_host: null argument struct");
    if (h->n == 0) return c3sc_hip_simulate(c, h, nullptr);
    HostShape sh;
    const int rc = closed_loop_host_shape(c, "simulate", h, h->nsteps, sh);
    if (rc != C3SC_OK) return rc;
    const size_t n = sh.n, d = sh.d, D = sizeof(double);
    return stage_host(c, STAGE_PER_CALL, "simulate_host",
                      {{h->d_x0, n * d * D, SEG_IN}, {h->d_noise, h->d_noise ? n * h->nsteps * d * D : 0, SEG_IN},
                       {h->d_traj, h->d_traj ? n * sh.nrow * d * D : 0, SEG_OUT}, {h->d_u, h->d_u ? n * sh.nurow * sh.du * D : 0, SEG_OUT},
                       {h->d_cost, n * D, SEG_OUT}, {h->d_exit, n * sizeof(int64_t), SEG_OUT}, {h->d_vend, n * D, SEG_OUT},
                       {h->d_xfinal, n * d * D, SEG_OUT}},
                      [&](const DevPtr *b) {
                          c3sc_hip_sim_args a = *h;
                          a.d_x0 = b[0]; a.d_noise = b[1]; a.d_traj = b[2]; a.d_u = b[3];
                          a.d_cost = b[4]; a.d_exit = b[5]; a.d_vend = b[6]; a.d_xfinal = b[7];
                          return c3sc_hip_simulate(c, &a, nullptr);
                      });
}

// ------------------------------------------------------------------ the approximating Markov chain (kernel_chain_walk.hpp)
// What both chain calls need of the context, in the order that decides which error a bad call gets; on success A is filled
// and e is the kernel of `variant`
static int chain_setup(c3sc_hip_ctx *c, const char *who, int variant, KArgs &A, const KernelEntry *&e)
{
    if (c->model == C3SC_MODEL_TABLE) return failw(c, C3SC_ERR_UNSUPPORTED, who, ": the TABLE model has no device dynamics");
    if (!c->have_mca || c->model == 0) return failw(c, C3SC_ERR_ARG, who, ": mca and model must be set");
    // a run-time compiled model with chain kernels (c3sc_hip_model_compile_mc) serves the modes the chain has a form of, where it
    // was compiled with them; every other model serves the plain chain only
    int njump = 0;
    const bool mc = c->model >= C3SC_MODEL_USER && rtc_model_chain(c->model, njump);
    for (const FormRow &r : FORM_ROWS)
        if ((ctx_form(c) & r.bit) && !(mc && form_offered(r.bit, FORM_CHAIN)))
            return fails(c, C3SC_ERR_UNSUPPORTED, std::string(who) + ": the chain is not offered " + r.problems + " (" + r.off + " first)");
    if (c->model >= C3SC_MODEL_USER && !mc)
        return failw(c, C3SC_ERR_UNSUPPORTED, who, ": this model was compiled without chain kernels (c3sc_hip_model_compile_mc, chain = 1)");
    if (check_form_model(c, who) != C3SC_OK) return C3SC_ERR_UNSUPPORTED;
    if (c->ncand == 0 || c->cands_placeholder)
        return c->box_du > 0 ? failw(c, C3SC_ERR_UNSUPPORTED, who, ": the control box is not served (set_controls: the chain takes a candidate list)")
                             : failw(c, C3SC_ERR_ARG, who, ": set_controls first");
    int rc = fill_args(c, 0, 0, A, false);
    if (rc != C3SC_OK) return rc;
    rc = check_bounds_set(c, (std::string(who) + ": every dimension needs a boundary type").c_str());
    if (rc != C3SC_OK) return rc;
    e = find_sim_kernel(variant, c->model, c->d, c->rp);
    if (!e) return failw(c, C3SC_ERR_UNSUPPORTED, who, ": no chain instantiation for this model at this padded rank");
    A.cmode = 0;
    return C3SC_OK;
}

// every index of the n nodes lies in the grid (the kernels clamp what they load, so this decides the error, not the addresses)
static bool chain_nodes_in_range(const c3sc_hip_ctx *c, const int32_t *nodes, size_t n)
{
    for (size_t i = 0; i < n; i++)
        for (int m = 0; m < c->d; m++)
            if (nodes[i * c->d + m] < 0 || nodes[i * c->d + m] >= c->ngrid[m]) return false;
    return true;
}

// the device entry points read the nodes back to check them: one copy and one synchronisation of the stream per call
static int chain_check_device_nodes(c3sc_hip_ctx *c, const char *who, const int32_t *d_nodes, size_t n, void *stream)
{
    std::vector<int32_t> h(n * (size_t)c->d);
    HIPCHK(c, hipMemcpyAsync(h.data(), d_nodes, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
    if (!chain_nodes_in_range(c, h.data(), n)) return failw(c, C3SC_ERR_ARG, who, ": a node index is out of range");
    return C3SC_OK;
}

static int chain_outcomes(c3sc_hip_ctx *c, const char *who, bool extra, size_t n, const int32_t *d_nodes, int32_t *d_uidx, double *d_value,
                          double *d_stage, double *d_dt, double *d_P, int32_t *d_flag, double *d_pself, double *d_pmark, double *d_markval,
                          void *stream)
{
    if (!c) return C3SC_ERR_ARG;
    KArgs A;
    const KernelEntry *e = nullptr;
    int rc = chain_setup(c, who, VARIANT_CHAIN_TRANSITIONS, A, e);
    if (rc != C3SC_OK) return rc;
    if (n == 0) return C3SC_OK;
    if (!d_nodes) return failw(c, C3SC_ERR_ARG, who, ": null d_nodes");
    if (n > SIM_MAX_TRAJ) return failw(c, C3SC_ERR_ARG, who, ": more than 2^31 nodes in one call");
    if (extra) { // the outcomes call: the kernels of a chain-compiled model only (chain_setup let a built-in model through)
        int njump = 0;
        if (!(c->model >= C3SC_MODEL_USER && rtc_model_chain(c->model, njump)))
            return failw(c, C3SC_ERR_UNSUPPORTED, who, ": needs a model compiled with chain kernels (c3sc_hip_model_compile_mc, chain = 1)");
        if ((d_pmark || d_markval) && !(ctx_form(c) & FORM_JUMP))
            return failw(c, C3SC_ERR_ARG, who, ": d_pmark / d_markval need jumps on (c3sc_hip_set_jumps)");
    }
    rc = chain_check_device_nodes(c, who, d_nodes, n, stream);
    if (rc != C3SC_OK) return rc;
    ChainK S;
    std::memset(&S, 0, sizeof(S));
    S.n = (long)n;
    S.pself = d_pself;
    S.pmark = d_pmark;
    S.markval = d_markval;
    S.node0 = d_nodes;
    S.uidx = d_uidx;
    S.value = d_value;
    S.stage = d_stage;
    S.dt = d_dt;
    S.P = d_P;
    S.flag = d_flag;
    LaunchIO io{c->arena, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream, &S};
    return launch_one(c, e, A, io, "chain_transitions: the chain kernels take a candidate list");
}

int c3sc_hip_chain_transitions(c3sc_hip_ctx *c, size_t n, const int32_t *d_nodes, int32_t *d_uidx, double *d_value, double *d_stage,
                               double *d_dt, double *d_P, int32_t *d_flag, void *stream)
{
    return chain_outcomes(c, "chain_transitions", false, n, d_nodes, d_uidx, d_value, d_stage, d_dt, d_P, d_flag, nullptr, nullptr, nullptr, stream);
}

int c3sc_hip_chain_outcomes(c3sc_hip_ctx *c, size_t n, const int32_t *d_nodes, int32_t *d_uidx, double *d_value, double *d_stage,
                            double *d_dt, double *d_P, int32_t *d_flag, double *d_pself, double *d_pmark, double *d_markval, void *stream)
{
    return chain_outcomes(c, "chain_outcomes", true, n, d_nodes, d_uidx, d_value, d_stage, d_dt, d_P, d_flag, d_pself, d_pmark, d_markval, stream);
}

int c3sc_hip_chain_outcomes_host(c3sc_hip_ctx *c, size_t n, const int32_t *nodes, int32_t *uidx, double *value, double *stage, double *dt,
                                 double *P, int32_t *flag, double *pself, double *pmark, double *markval)
{
    if (!c) return C3SC_ERR_ARG;
    if (n == 0) return c3sc_hip_chain_outcomes(c, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!nodes) return fail(c, C3SC_ERR_ARG, "chain_outcomes_host: null nodes");
    if (n > SIM_MAX_TRAJ) return fail(c, C3SC_ERR_ARG, "chain_outcomes_host: sizes too large");
    if (c->d == 0) return fail(c, C3SC_ERR_ARG, "chain_outcomes_host: set_grid first");
    int njump = 0;
    (void)rtc_model_chain(c->model, njump);
    if ((pmark || markval) && (njump == 0 || !(ctx_form(c) & FORM_JUMP)))
        return fail(c, C3SC_ERR_ARG, "chain_outcomes_host: pmark / markval need a jump model with jumps on (c3sc_hip_set_jumps)");
    const size_t d = (size_t)c->d, D = sizeof(double), I = sizeof(int32_t), M = (size_t)njump;
    return stage_host(c, STAGE_PER_CALL, "chain_outcomes_host",
                      {{nodes, n * d * I, SEG_IN}, {uidx, n * I, SEG_OUT}, {value, n * D, SEG_OUT}, {stage, n * D, SEG_OUT},
                       {dt, n * D, SEG_OUT}, {P, n * 2 * d * D, SEG_OUT}, {flag, n * I, SEG_OUT}, {pself, n * D, SEG_OUT},
                       {pmark, n * M * D, SEG_OUT}, {markval, n * M * D, SEG_OUT}},
                      [&](const DevPtr *b) {
                          return c3sc_hip_chain_outcomes(c, n, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], b[9], nullptr);
                      });
}

int c3sc_hip_chain_transitions_host(c3sc_hip_ctx *c, size_t n, const int32_t *nodes, int32_t *uidx, double *value, double *stage,
                                    double *dt, double *P, int32_t *flag)
{
    if (!c) return C3SC_ERR_ARG;
    if (n == 0) return c3sc_hip_chain_transitions(c, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (!nodes) return fail(c, C3SC_ERR_ARG, "chain_transitions_host: null nodes");
    if (n > SIM_MAX_TRAJ) return fail(c, C3SC_ERR_ARG, "chain_transitions_host: sizes too large");
    if (c->d == 0) return fail(c, C3SC_ERR_ARG, "chain_transitions_host: set_grid first");
    const size_t d = (size_t)c->d, D = sizeof(double), I = sizeof(int32_t);
    return stage_host(c, STAGE_PER_CALL, "chain_transitions_host",
                      {{nodes, n * d * I, SEG_IN}, {uidx, n * I, SEG_OUT}, {value, n * D, SEG_OUT}, {stage, n * D, SEG_OUT},
                       {dt, n * D, SEG_OUT}, {P, n * 2 * d * D, SEG_OUT}, {flag, n * I, SEG_OUT}},
                      [&](const DevPtr *b) { return c3sc_hip_chain_transitions(c, n, b[0], b[1], b[2], b[3], b[4], b[5], b[6], nullptr); });
}

int c3sc_hip_simulate_chain(c3sc_hip_ctx *c, const c3sc_hip_chain_args *a, void *stream)
{
    const char *who = "simulate_chain";
    if (!c) return C3SC_ERR_ARG;
    if (!a) return failw(c, C3SC_ERR_ARG, who, ": null argument struct");
    KArgs A;
    const KernelEntry *e = nullptr;
    int rc = chain_setup(c, who, VARIANT_CHAIN_WALK, A, e);
    if (rc != C3SC_OK) return rc;
    if (a->nsteps > (size_t)1 << 30) return failw(c, C3SC_ERR_ARG, who, ": nsteps too large");
    if (a->n > SIM_MAX_TRAJ) return failw(c, C3SC_ERR_ARG, who, ": more than 2^31 walks in one call (split the batch, traj_offset)");
    if (a->save_every == 0 && (a->d_traj || a->d_uidx)) return failw(c, C3SC_ERR_ARG, who, ": d_traj / d_uidx need save_every > 0");
    if (a->save_every > a->nsteps && a->save_every > 1 && (a->d_traj || a->d_uidx))
        return failw(c, C3SC_ERR_ARG, who, ": save_every larger than nsteps");
    if (a->steps_per_launch < 0) return failw(c, C3SC_ERR_ARG, who, ": steps_per_launch < 0");
    const bool hz = c->hz_dt > 0.0; // horizon mode: one launch per step, step s decides on the cores of V_{s+1} (as c3sc_hip_simulate)
    if (hz) {
        if (c->hz_nstack == 0) return failw(c, C3SC_ERR_ARG, who, ": horizon mode needs the value stack (c3sc_hip_upload_value_stack)");
        if (a->nsteps + 1 > (size_t)c->hz_nstack) return failw(c, C3SC_ERR_ARG, who, ": nsteps exceeds the value stack (nstack - 1 stages)");
        if (c->hz_stack_static != c->static_doubles)
            return failw(c, C3SC_ERR_ARG, who, ": static data changed size after upload_value_stack; upload the stack again");
        for (size_t s = 0; s <= a->nsteps; s++)
            if (!find_sim_kernel(VARIANT_CHAIN_WALK, c->model, c->d, c->hz_rp[s]))
                return failw(c, C3SC_ERR_UNSUPPORTED, who, ": no chain instantiation for a stage's padded rank");
    }
    if (a->n == 0) return C3SC_OK;
    if (!a->d_node0) return failw(c, C3SC_ERR_ARG, who, ": null d_node0");
    const size_t n = a->n, d = (size_t)c->d;
    rc = chain_check_device_nodes(c, who, a->d_node0, n, stream);
    if (rc != C3SC_OK) return rc;
    // the state between launches: cost | disc | time | exit_step | node (the doubles first: every block stays aligned)
    rc = closed_loop_state(c, n * 4 * sizeof(double) + n * d * sizeof(int32_t));
    if (rc != C3SC_OK) return rc;
    ChainK S;
    std::memset(&S, 0, sizeof(S));
    S.n = (long)n;
    S.traj_offset = (long long)a->traj_offset;
    S.nsteps = (int)a->nsteps;
    S.save_every = (int)a->save_every;
    S.seed = a->seed;
    S.node0 = a->d_node0;
    S.uniform = a->d_uniform;
    S.cost = (double *)c->sim_state;
    S.disc = S.cost + n;
    S.time = S.disc + n;
    S.exit_step = (long long *)(S.time + n);
    S.node = (int32_t *)(S.exit_step + n);
    S.traj = a->d_traj;
    S.uidx = a->d_uidx;
    S.vend = a->d_vend;
    const int chunk = hz ? 1 : (a->steps_per_launch > 0 ? a->steps_per_launch : 64);
    if (hz) HIPCHK(c, hipMemcpyAsync(c->hz_stack, c->arena, c->static_doubles * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    int s0 = 0;
    do { // at least one launch: nsteps = 0 still tests xi_0 and evaluates V_end
        S.s0 = s0;
        S.s1 = (int)std::min<long long>((long long)s0 + chunk, (long long)a->nsteps);
        const KernelEntry *ek = e;
        const double *ro = c->arena;
        if (hz) { // the launch of step s0 (or the terminal-only launch of nsteps = 0) reads stage s1: V_{s0+1}, and V_nsteps at the end
            for (int m = 0; m < c->d; m++) A.core_off[m] = c->hz_core_off[(size_t)S.s1 * MAXD + m];
            ek = find_sim_kernel(VARIANT_CHAIN_WALK, c->model, c->d, c->hz_rp[S.s1]);
            ro = c->hz_stack;
        }
        LaunchIO io{ro, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream, &S};
        rc = launch_one(c, ek, A, io, "simulate_chain: the chain kernels take a candidate list");
        if (rc != C3SC_OK) return rc;
        s0 = S.s1;
    } while (s0 < (int)a->nsteps);
    rc = copy_back(c, a->d_cost, S.cost, n * sizeof(double), stream);
    if (rc == C3SC_OK) rc = copy_back(c, a->d_disc, S.disc, n * sizeof(double), stream);
    if (rc == C3SC_OK) rc = copy_back(c, a->d_time, S.time, n * sizeof(double), stream);
    if (rc == C3SC_OK) rc = copy_back(c, a->d_exit, S.exit_step, n * sizeof(int64_t), stream);
    if (rc == C3SC_OK) rc = copy_back(c, a->d_node, S.node, n * d * sizeof(int32_t), stream);
    return rc;
}

int c3sc_hip_simulate_chain_host(c3sc_hip_ctx *c, const c3sc_hip_chain_args *h)
{
    if (!c) return C3SC_ERR_ARG;
    if (!h) return fail(c, C3SC_ERR_ARG, "simulate_chain_host: null argument struct");
    if (h->n == 0) return c3sc_hip_simulate_chain(c, h, nullptr);
    if (!h->d_node0) return fail(c, C3SC_ERR_ARG, "simulate_chain_host: null node0");
    if (h->n > SIM_MAX_TRAJ || h->nsteps > ((size_t)1 << 30)) return fail(c, C3SC_ERR_ARG, "simulate_chain_host: sizes too large");
    if (h->save_every == 0 && (h->d_traj || h->d_uidx)) return fail(c, C3SC_ERR_ARG, "simulate_chain: d_traj / d_uidx need save_every > 0");
    if (c->d == 0) return fail(c, C3SC_ERR_ARG, "simulate_chain_host: set_grid first");
    const size_t n = h->n, d = (size_t)c->d, se = h->save_every, D = sizeof(double), I = sizeof(int32_t);
    const size_t nrow = se ? h->nsteps / se + 1 : 0, nurow = se ? (h->nsteps + se - 1) / se : 0;
    return stage_host(c, STAGE_PER_CALL, "simulate_chain_host",
                      {{h->d_node0, n * d * I, SEG_IN}, {h->d_uniform, h->d_uniform ? n * h->nsteps * D * ((ctx_form(c) & FORM_JUMP) ? 2 : 1) : 0, SEG_IN},
                       {h->d_cost, n * D, SEG_OUT}, {h->d_disc, n * D, SEG_OUT}, {h->d_time, n * D, SEG_OUT}, {h->d_vend, n * D, SEG_OUT},
                       {h->d_node, n * d * I, SEG_OUT}, {h->d_exit, n * sizeof(int64_t), SEG_OUT},
                       {h->d_traj, h->d_traj ? n * nrow * d * I : 0, SEG_OUT}, {h->d_uidx, h->d_uidx ? n * nurow * I : 0, SEG_OUT}},
                      [&](const DevPtr *b) {
                          c3sc_hip_chain_args a = *h;
                          a.d_node0 = b[0]; a.d_uniform = b[1]; a.d_cost = b[2]; a.d_disc = b[3]; a.d_time = b[4]; a.d_vend = b[5];
                          a.d_node = b[6]; a.d_exit = b[7]; a.d_traj = b[8]; a.d_uidx = b[9];
                          return c3sc_hip_simulate_chain(c, &a, nullptr);
                      });
}

// ------------------------------------------------------------------ closed-loop integration (kernel_rollout_ode.hpp)
static const size_t ODE_MAX_EVALS = (size_t)1 << 40; // controller evaluations per lane of one call (substep indices stay exact)

// nsub = dt_out / dt_int, an integer to 1e-9 relative (dt_int = 0: 1); 0 when it is not
static long long ode_nsub(double dt_out, double dt_int)
{
    if (dt_int == 0.0) return 1;
    const double r = dt_out / dt_int, q = std::nearbyint(r);
    if (!(q >= 1.0) || !(std::fabs(r - q) <= 1e-9 * q) || q > (double)(1 << 30)) return 0;
    return (long long)q;
}

// a stop box: host (lo[d], hi[d]); lo > hi or a NaN is an error
static bool ode_box_ok(const double *b, int d)
{
    if (!b) return true;
    for (int m = 0; m < d; m++)
        if (!(b[m] <= b[d + m])) return false;
    return true;
}

int c3sc_hip_integrate(c3sc_hip_ctx *c, const c3sc_hip_ode_args *a, void *stream)
{
    const char *who = "integrate";
    int rc = closed_loop_setup(c, who, a);
    if (rc != C3SC_OK) return rc;
    for (const FormRow &r : FORM_ROWS)
        if ((ctx_form(c) & r.bit) && !form_offered(r.bit, FORM_ROLLOUT_ODE))
            return fails(c, C3SC_ERR_UNSUPPORTED, std::string("integrate: deterministic closed loops are not offered ") + r.problems);
    KArgs A;
    rc = fill_args(c, 0, 0, A, false);
    if (rc != C3SC_OK) return rc;
    rc = check_bounds_set(c, "integrate: every dimension needs a boundary type");
    if (rc != C3SC_OK) return rc;
    if (!(a->dt_out > 0.0) || !std::isfinite(a->dt_out)) return fail(c, C3SC_ERR_ARG, "integrate: dt_out must be positive and finite");
    if (!(a->dt_int >= 0.0) || !std::isfinite(a->dt_int)) return fail(c, C3SC_ERR_ARG, "integrate: dt_int must be >= 0 and finite");
    const long long nsub = ode_nsub(a->dt_out, a->dt_int);
    if (nsub == 0) return fail(c, C3SC_ERR_ARG, "integrate: dt_out / dt_int is not an integer (to 1e-9 relative)");
    if (a->method != C3SC_ODE_FORWARD_EULER && a->method != C3SC_ODE_RK4)
        return fail(c, C3SC_ERR_ARG, "integrate: method must be C3SC_ODE_FORWARD_EULER or C3SC_ODE_RK4");
    const int nstage = a->method == C3SC_ODE_RK4 ? 4 : 1;
    if (a->nout > (size_t)1 << 30) return fail(c, C3SC_ERR_ARG, "integrate: nout too large");
    if ((size_t)nsub * a->nout * nstage > ODE_MAX_EVALS) return fail(c, C3SC_ERR_ARG, "integrate: more than 2^40 controller evaluations per trajectory");
    rc = closed_loop_sizes(c, who, a, a->nout, "integrate: more than 2^31 trajectories in one call (split the batch)",
                           "integrate: save_every larger than nout");
    if (rc != C3SC_OK) return rc;
    if (a->evals_per_launch < 0) return fail(c, C3SC_ERR_ARG, "integrate: evals_per_launch < 0");
    if (!ode_box_ok(a->goal, c->d) || !ode_box_ok(a->keep, c->d))
        return fail(c, C3SC_ERR_ARG, "integrate: a stop box has lo > hi (or a NaN)");
    const KernelEntry *e = find_sim_kernel(VARIANT_ROLLOUT_ODE, c->model, c->d, c->rp);
    if (!e) return fail(c, C3SC_ERR_UNSUPPORTED, "integrate: no integrate instantiation for this model at this padded rank");
    if (a->n == 0) return C3SC_OK;
    if (!a->d_x0) return fail(c, C3SC_ERR_ARG, "integrate: null d_x0");
    const int d = c->d;
    const size_t n = a->n;
    rc = closed_loop_state(c, n * (size_t)(d + 3) * sizeof(double)); // x | cost | stop_step | stop_reason
    if (rc != C3SC_OK) return rc;
    closed_loop_box(c, a->box, A);
    OdeK S;
    std::memset(&S, 0, sizeof(S));
    S.n = (long)n;
    S.nsub = (int)nsub;
    S.nout = (int)a->nout;
    S.nstage = nstage;
    S.save_every = (int)a->save_every;
    S.wrap = a->wrap_periodic ? 1 : 0;
    S.constelm = c->constelm;
    S.h = a->dt_int == 0.0 ? a->dt_out : a->dt_int;
    S.dt_out = a->dt_out;
    S.has_goal = a->goal ? 1 : 0;
    S.has_keep = a->keep ? 1 : 0;
    for (int m = 0; m < d; m++) {
        S.goal_lo[m] = a->goal ? a->goal[m] : 0.0;
        S.goal_hi[m] = a->goal ? a->goal[d + m] : 0.0;
        S.keep_lo[m] = a->keep ? a->keep[m] : -INFINITY;
        S.keep_hi[m] = a->keep ? a->keep[d + m] : INFINITY;
    }
    S.x0 = a->d_x0;
    S.x = (double *)c->sim_state;
    S.cost = S.x + n * d;
    S.stop_step = (long long *)(S.cost + n);
    S.stop_reason = (int32_t *)(S.stop_step + n);
    S.traj = a->d_traj;
    S.u = a->d_u;
    S.vend = a->d_vend;
    const long long ktot = nsub * (long long)a->nout;
    const long long chunk = std::max<long long>(1, (a->evals_per_launch > 0 ? a->evals_per_launch : 256) / nstage);
    long long k0 = 0;
    do { // at least one launch: nout = 0 still tests x_0 and evaluates V_end
        S.k0 = k0;
        S.k1 = std::min(k0 + chunk, ktot);
        LaunchIO io{c->arena, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream, &S};
        rc = launch_one(c, e, A, io, "integrate: this integrate kernel has no box minimiser");
        if (rc != C3SC_OK) return rc;
        k0 = S.k1;
    } while (k0 < ktot);
    rc = closed_loop_results(c, a, a->d_stop_step, stream);
    if (rc != C3SC_OK) return rc;
    return copy_back(c, a->d_stop_reason, S.stop_reason, n * sizeof(int32_t), stream);
}

int c3sc_hip_integrate_host(c3sc_hip_ctx *c, const c3sc_hip_ode_args *h)
{
    if (!c) return C3SC_ERR_ARG;
    if (!h) return fail(c, C3SC_ERR_ARG, "integrate_host: null argument struct");
    if (h->n == 0) return c3sc_hip_integrate(c, h, nullptr);
    HostShape sh;
    const int rc = closed_loop_host_shape(c, "integrate", h, h->nout, sh);
    if (rc != C3SC_OK) return rc;
    const size_t n = sh.n, d = sh.d, D = sizeof(double);
    return stage_host(c, STAGE_PER_CALL, "integrate_host",
                      {{h->d_x0, n * d * D, SEG_IN}, {h->d_traj, h->d_traj ? n * sh.nrow * d * D : 0, SEG_OUT},
                       {h->d_u, h->d_u ? n * sh.nurow * sh.du * D : 0, SEG_OUT}, {h->d_cost, n * D, SEG_OUT},
                       {h->d_stop_step, n * sizeof(int64_t), SEG_OUT}, {h->d_stop_reason, n * sizeof(int32_t), SEG_OUT},
                       {h->d_vend, n * D, SEG_OUT}, {h->d_xfinal, n * d * D, SEG_OUT}},
                      [&](const DevPtr *b) {
                          c3sc_hip_ode_args a = *h;
                          a.d_x0 = b[0]; a.d_traj = b[1]; a.d_u = b[2]; a.d_cost = b[3];
                          a.d_stop_step = b[4]; a.d_stop_reason = b[5]; a.d_vend = b[6]; a.d_xfinal = b[7];
                          return c3sc_hip_integrate(c, &a, nullptr);
                      });
}

int c3sc_hip_normals(uint64_t seed, uint64_t traj0, size_t ntraj, uint64_t step0, size_t nsteps, int dw, double *out)
{
    if (!out || dw < 1 || dw > MAXD) return C3SC_ERR_ARG;
    for (size_t t = 0; t < ntraj; t++)
        for (size_t k = 0; k < nsteps; k++)
            for (int j = 0; j < dw; j++)
                out[(t * nsteps + k) * dw + j] = philox_normal(seed, traj0 + t, (uint32_t)(step0 + k), (uint32_t)j);
    return C3SC_OK;
}

int c3sc_hip_jump_uniforms(uint64_t seed, uint64_t traj, uint64_t step, double *out)
{
    if (!out) return C3SC_ERR_ARG;
    philox_jump_uniforms(seed, traj, (uint32_t)step, out[0], out[1]);
    return C3SC_OK;
}

unsigned long long c3sc_hip_launch_count(void) { return g_launches; }
unsigned long long c3sc_hip_table3_launch_count(void) { return g_tab3_launches; }

int c3sc_hip_last_partition(c3sc_hip_ctx *c, int slot, int32_t *perm, size_t cap, size_t *F, int *nlive)
{
    if (!c) return C3SC_ERR_ARG;
    if (slot < 0 || slot > c3sc_hip_ctx::NSIDE || !F || !nlive) return fail(c, C3SC_ERR_ARG, "last_partition: bad arguments");
    const auto &lp = c->part_last[slot];
    if (!lp.perm) return fail(c, C3SC_ERR_ARG, "last_partition: no partition has run on this slot");
    *F = (size_t)lp.F;
    HIPCHK(c, hipStreamSynchronize(lp.stream));
    int32_t nl = 0;
    HIPCHK(c, hipMemcpy(&nl, lp.nlive, sizeof(nl), hipMemcpyDeviceToHost));
    *nlive = nl;
    if (perm) {
        if (cap < (size_t)lp.F) return fail(c, C3SC_ERR_ARG, "last_partition: perm holds fewer than F entries");
        HIPCHK(c, hipMemcpy(perm, lp.perm, (size_t)lp.F * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return C3SC_OK;
}

int c3sc_hip_debug_read(c3sc_hip_ctx *c, unsigned long long *out, size_t n)
{
    if (!c || !c->d_dbg || !out) return C3SC_ERR_ARG;
    HIPCHK(c, hipMemcpy(out, c->d_dbg, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return C3SC_OK;
}

int c3sc_hip_timer_start(c3sc_hip_ctx *c, void *stream)
{
    if (!c) return C3SC_ERR_ARG;
    HIPCHK(c, hipEventRecord(c->ev0, (hipStream_t)stream));
    return C3SC_OK;
}

int c3sc_hip_timer_stop(c3sc_hip_ctx *c, void *stream, float *ms)
{
    if (!c || !ms) return C3SC_ERR_ARG;
    HIPCHK(c, hipEventRecord(c->ev1, (hipStream_t)stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return C3SC_OK;
}

static int run_peak(c3sc_hip_ctx *c, bool mfma, double *tflops)
{
    if (!c || !tflops) return C3SC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const char *ev = getenv("C3SC_PEAK_BLOCKS_PER_CU");
    const int blocks = 256 * (ev ? atoi(ev) : 8), threads = 256, iters = 20000;
    int rc = ensure_scratch(c, (size_t)blocks * threads * sizeof(double));
    if (rc != C3SC_OK) return rc;
    float best = 1e30f;
    for (int rep = 0; rep < 4; rep++) {
        HIPCHK(c, hipEventRecord(c->ev0, nullptr));
        if (mfma) hipLaunchKernelGGL(k_peak_mfma, dim3(blocks), dim3(threads), 0, nullptr, (double *)c->scratch, iters);
        else hipLaunchKernelGGL(k_peak_fma, dim3(blocks), dim3(threads), 0, nullptr, (double *)c->scratch, iters);
        HIPCHK(c, hipEventRecord(c->ev1, nullptr));
        HIPCHK(c, hipEventSynchronize(c->ev1));
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        if (rep > 0 && ms < best) best = ms;
    }
    const double waves = (double)blocks * threads / 64.0;
    const double flop = mfma ? waves * iters * 4.0 * (2.0 * 16 * 16 * 4) : (double)blocks * threads * iters * 8.0 * 2.0;
    *tflops = flop / (best * 1e-3) / 1e12;
    return C3SC_OK;
}

int c3sc_hip_peak_fma_f64(c3sc_hip_ctx *c, double *tflops) { return run_peak(c, false, tflops); }
int c3sc_hip_peak_mfma_f64(c3sc_hip_ctx *c, double *tflops) { return run_peak(c, true, tflops); }

} // extern "C"
