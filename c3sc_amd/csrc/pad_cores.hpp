// pad_cores.hpp -- all cores of a value function into the rank-padded device layout in ONE launch (prepass.hip: k_pad_cores; the
// layout is k_pad_core's in c3sc_hip.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_common.hpp"

namespace c3sc {

struct PadJobs {
    const double *src[MAXD]; // cores[m][j*r0*r1 + a + b*r0] on the device
    long dst[MAXD];          // arena offsets
    int N[MAXD], r0[MAXD], r1[MAXD];
    int d;
};
// enqueue the padding of J's d cores at padded rank rp: gridx workgroups of 256 threads per core
hipError_t pad_cores_launch(double *arena, const PadJobs &J, int rp, unsigned gridx, hipStream_t stream);

} // namespace c3sc
