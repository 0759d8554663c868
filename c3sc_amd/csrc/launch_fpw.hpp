// launch_fpw.hpp -- host launcher + registration macro for the fiber-per-wave kernels.
#pragma once
#include "kernel_fiber_per_wave.hpp"
#include "registry.hpp"

namespace c3sc {

// Launch geometry of k_fiber_per_wave, shared by the launchers below and the module launcher of run-time compiled models
// (rtc.hip): dynamic LDS = per-wave scratch of the 4 waves | staged varying core (STAGED) | candidate table (tbl_off), and one
// workgroup per 4 fibers up to the resident capacity.  cand_doubles: 0 for the stencil and table kernels.
struct FpwGeom {
    size_t shmem; // bytes of dynamic LDS
    int tbl_off;  // KArgs::tbl_off (doubles)
};
inline FpwGeom fpw_geometry(int D, int RP, int NPL, bool staged, int k, int N, size_t cand_doubles)
{
    const int WS = 4 * RP + 2 * D * RP + 64 * NPL;
    const bool kedge = (k == 0) || (k == D - 1);
    const size_t doubles = (size_t)(4 * WS + (staged ? N * kcore_stride(RP, kedge) : 0));
    return FpwGeom{(doubles + cand_doubles) * sizeof(double), (int)doubles};
}
// the varying core (N x RP^2 doubles) is staged in LDS when it fits the CU, otherwise read from L2 (RP >= 12 only)
constexpr size_t FPW_MAX_LDS = 160u * 1024u;
inline int fpw_grid(long F, int blocks_per_cu, int num_cu)
{
    const long want = (F + 3) / 4;
    const long cap = (long)num_cu * blocks_per_cu;
    const int grid = (int)(want < cap ? want : cap);
    return grid < 1 ? 1 : grid;
}
// doubles of the candidate table in LDS: rows of CandLds<Model>::CW (u, features, constant rates, obstacle flag)
constexpr int cand_row_doubles(int D, int DU, int NCF, unsigned uconst_mask)
{
    int nuc = 0;
    for (int m = 0; m < D; m++) nuc += (uconst_mask >> m) & 1u;
    return DU + (NCF > 0 ? NCF : 1) + 2 * (nuc > 0 ? nuc : 1) + 1; // CandRegs<Model>::NUC is at least 1
}
template <class Model, bool STENCIL>
inline size_t fpw_cand_doubles(int ncand)
{
    if constexpr (!STENCIL && !Model::IS_TABLE) {
        static_assert(CandLds<Model>::CW == cand_row_doubles(Model::D, Model::DU, Model::NCF, Model::UCONST_MASK));
        return (size_t)CandLds<Model>::doubles(ncand);
    } else {
        return 0;
    }
}

template <class Model, int RP, int NPL, bool STENCIL, bool BOX, bool STAGED>
hipError_t launch_fpw_impl(const KArgs &A, const LaunchIO &io)
{
    const FpwGeom g = fpw_geometry(Model::D, RP, NPL, STAGED, A.k, A.N, fpw_cand_doubles<Model, STENCIL>(A.ncand));
    KArgs B = A;
    B.tbl_off = g.tbl_off; // candidate table behind everything else
    auto kern = k_fiber_per_wave<Model, RP, NPL, STENCIL, BOX, STAGED>;
    static LaunchCache cache;
    int blocks_per_cu = 1, num_cu = 256;
    hipError_t e = cache.prepare((const void *)kern, 256, g.shmem, blocks_per_cu, num_cu);
    if (e != hipSuccess) return e;
    const int grid = fpw_grid(A.F, blocks_per_cu, num_cu);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), g.shmem, io.stream, B, io.ro, io.idx, io.out, io.uidx, io.absorbed,
                       io.nbf, io.nbv, io.tbl, io.tcost);
    return hipGetLastError();
}

template <class Model, int RP, int NPL, bool STENCIL, bool BOX = false>
hipError_t launch_fpw(const KArgs &A, const LaunchIO &io)
{
    if (A.cmode == 1 && !BOX) return hipErrorNotSupported; // this entry has no box-minimiser instantiation
    const size_t staged = fpw_geometry(Model::D, RP, NPL, true, A.k, A.N, fpw_cand_doubles<Model, STENCIL>(A.ncand)).shmem;
    if (staged <= FPW_MAX_LDS) return launch_fpw_impl<Model, RP, NPL, STENCIL, BOX, true>(A, io);
    if constexpr (RP >= 12) return launch_fpw_impl<Model, RP, NPL, STENCIL, BOX, false>(A, io);
    else return hipErrorOutOfMemory; // small ranks always fit for N <= 128
}

#define C3SC_CAT2(a, b) a##b
#define C3SC_CAT(a, b) C3SC_CAT2(a, b)

// MODEL may contain commas/angle brackets, hence the variadic tail
#define C3SC_REG_FPW(MODEL_ID, RP, NPL, ...)                                                                 \
    static Registrar C3SC_CAT(reg_fpw_, __COUNTER__)(KernelEntry{                                            \
        MODEL_ID, __VA_ARGS__::D, RP, NPL, C3SC_VARIANT_FIBER_PER_WAVE, 64 * NPL, -1,                          \
        &launch_fpw<__VA_ARGS__, RP, NPL, false>, "k_fiber_per_wave<" #__VA_ARGS__ "," #RP "," #NPL ">"});

// the same entry serving both the candidate-list kernel and the box minimiser (continuous controls)
template <class Model, int RP, int NPL>
hipError_t launch_fpw_both(const KArgs &A, const LaunchIO &io)
{
    return A.cmode == 1 ? launch_fpw<Model, RP, NPL, false, true>(A, io) : launch_fpw<Model, RP, NPL, false, false>(A, io);
}
#define C3SC_REG_FPW_BOX(MODEL_ID, RP, NPL, ...)                                                             \
    static Registrar C3SC_CAT(reg_fpwb_, __COUNTER__)(KernelEntry{                                           \
        MODEL_ID, __VA_ARGS__::D, RP, NPL, C3SC_VARIANT_FIBER_PER_WAVE, 64 * NPL, -1,                          \
        &launch_fpw_both<__VA_ARGS__, RP, NPL>, "k_fiber_per_wave<" #__VA_ARGS__ "," #RP "," #NPL ">"});

#define C3SC_REG_STENCIL(DIM, RP, NPL)                                                                       \
    static Registrar C3SC_CAT(reg_st_, __COUNTER__)(KernelEntry{                                             \
        0, DIM, RP, NPL, C3SC_VARIANT_FIBER_PER_WAVE, 64 * NPL, -1, &launch_fpw<NoModel<DIM>, RP, NPL, true>,    \
        "k_fiber_per_wave<stencil," #DIM "," #RP "," #NPL ">"});

} // namespace c3sc
