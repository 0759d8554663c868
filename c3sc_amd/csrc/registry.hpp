// registry.hpp -- table of compiled kernel instantiations (model, dim, padded rank, nodes per lane).
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>
#endif

#include "kernel_common.hpp"

namespace c3sc {

#ifndef __HIPCC_RTC__ // the launch side is host code; run-time compiled device code (rtc.hip) sees only the variant ids below
struct LaunchIO {
    const double *ro;
    const int32_t *idx;
    double *out; // bellman: [F][N]; stencil: [F][N][2d+1]
    int32_t *uidx;
    int32_t *absorbed;
    const int32_t *nbf; // stencil only: explicit fixed-dim neighbours [F][2(d-1)] or null
    const int32_t *nbv; // stencil only: explicit varying-dim neighbours [F][N][2] or null
    const double *tbl;   // TableModel only: [F][N][U][2d+1] host-evaluated callbacks
    const double *tcost; // TableModel only: [F][N][2] (boundcost, obscost)
    hipStream_t stream;
    const void *sim = nullptr; // rollout / off-grid stencil kernels only: their SimK argument block (kernel_rollout.hpp)
    // fiber-pair kernels only (fiber_partition.hpp): the batch order live fibers first, and the device-side count of live ones;
    // null = batch order
    const int32_t *perm = nullptr;
    const int32_t *nlive = nullptr;
    bool tab3 = false; // ... and the three-core product tables are built: a partitioned launch may run its three-core kernel
    bool parked = true; // ... and a K with a parked node split (kernel_fiber_pair.hpp: fpp_parked) runs it; false: the rank-split kernels
    // the context's switches (FORM_STOP | FORM_JUMP | FORM_IMPULSE | FORM_CORR, kernel_common.hpp): a run-time compiled model's kernels
    // of that form run.  The game and horizon bits travel in KArgs (game_gsz, hz_off), whose data the kernels read
    unsigned form = 0;
};
#endif

// KernelEntry::variant of the rollout, off-grid stencil and integrate kernels (c3sc_hip_simulate / c3sc_hip_stencil_points /
// c3sc_hip_integrate): not Bellman-operator kernels, so the fiber paths never select them (find_kernel, pick_rp)
constexpr int VARIANT_ROLLOUT = 100, VARIANT_STENCIL_POINTS = 101, VARIANT_ROLLOUT_ODE = 102;
// ... and of the Markov-chain kernels (c3sc_hip_simulate_chain / c3sc_hip_chain_transitions, kernel_chain_walk.hpp)
constexpr int VARIANT_CHAIN_WALK = 103, VARIANT_CHAIN_TRANSITIONS = 104;
__host__ __device__ constexpr bool is_fiber_variant(int v) { return v < VARIANT_ROLLOUT; }

#ifndef __HIPCC_RTC__
struct RtcLaunch; // rtc.hip: a kernel of a run-time compiled model (module function)

typedef hipError_t (*launch_fn)(const KArgs &A, const LaunchIO &io);

struct KernelEntry {
    int model;   // C3SC_MODEL_* or 0 for the stencil-only kernels
    int d;       // state dimension
    int rp;      // padded rank
    int npl;     // nodes per lane (fiber-per-wave) ; 0 = any
    int variant; // C3SC_VARIANT_*
    int max_n;   // largest N_k this instantiation handles
    int k;       // dim_vary this instantiation is compiled for, -1 = any
    launch_fn fn;
    const char *name;
    const RtcLaunch *rtc = nullptr; // set instead of fn for the kernels of a run-time compiled model (rtc_launch)
};

// the compiled-in instantiations; the kernels of run-time compiled models (ids >= C3SC_MODEL_USER) are kept apart, in
// rtc.hip (rtc_entries), because this vector is read without a lock and find_kernel hands out pointers into it
std::vector<KernelEntry> &kernel_registry();

// What a launcher has to find out once per (kernel, device, dynamic-LDS size): the opt-in to more than 64 KiB of dynamic
// LDS (hipFuncSetAttribute applies to the CURRENT device only), the resident workgroups per CU and the CU count.  One
// instance per kernel instantiation (a function-local static of the launcher), slots per device, guarded by a mutex: the
// C API allows contexts on several devices and calls from several threads.
struct LaunchCache {
    static constexpr int MAXDEV = 16;
    std::mutex mu;
    size_t attr_shmem[MAXDEV] = {0}, occ_shmem[MAXDEV] = {0};
    int blocks_per_cu[MAXDEV] = {0}, num_cu[MAXDEV] = {0};
    hipError_t prepare(const void *kern, int threads, size_t shmem, int &blocks, int &cus)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= MAXDEV) return hipErrorInvalidDevice;
        std::lock_guard<std::mutex> lk(mu);
        if (shmem > attr_shmem[dev]) {
            e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
            if (e != hipSuccess) return e;
            attr_shmem[dev] = shmem;
        }
        if (blocks_per_cu[dev] == 0 || shmem != occ_shmem[dev]) {
            int nb = 0;
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, shmem);
            if (e != hipSuccess) return e;
            blocks_per_cu[dev] = nb > 0 ? nb : 1;
            occ_shmem[dev] = shmem;
        }
        if (num_cu[dev] == 0) {
            hipDeviceProp_t prop;
            e = hipGetDeviceProperties(&prop, dev);
            if (e != hipSuccess) return e;
            num_cu[dev] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        }
        blocks = blocks_per_cu[dev];
        cus = num_cu[dev];
        return hipSuccess;
    }
};

struct Registrar {
    explicit Registrar(const KernelEntry &e) { kernel_registry().push_back(e); }
};

// kernel entries of the run-time compiled models (rtc.hip): a snapshot that stays valid (entries are never removed or moved)
struct RtcEntries {
    const KernelEntry *const *e;
    int n;
};
RtcEntries rtc_entries();
// launch an entry of either kind
hipError_t rtc_launch(const KernelEntry &e, const KArgs &A, const LaunchIO &io);
bool rtc_model_known(int model); // an id c3sc_hip_model_compile returned
bool rtc_model_info(int model, int &du); // its control dimension (false: unknown id)
bool rtc_model_chain(int model, int &njump); // compiled with the Markov-chain kernels (c3sc_hip_model_compile_mc, chain = 1); its marks
unsigned rtc_model_forms(int model); // the FORM_* bits of the features it was compiled with (0: none, or an unknown id)
inline hipError_t launch_entry(const KernelEntry &e, const KArgs &A, const LaunchIO &io) { return e.rtc ? rtc_launch(e, A, io) : e.fn(A, io); }
#endif

} // namespace c3sc
