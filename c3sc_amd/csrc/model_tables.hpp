// model_tables.hpp -- the univariate functions of a state coordinate the device models read as tables (models.hpp: NTAB,
// tab_dim).  At grid nodes the host evaluates them once with libm and uploads the tables (c3sc_hip.hip: upload_static);
// the rollouts of c3sc_hip_simulate need them at arbitrary states and evaluate the SAME expressions on the device (device
// libm: within about an ulp of the host's).
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#include "../../include/c3sc_hip.h"

namespace c3sc {

__host__ __device__ inline int model_ntab(int model)
{
    if (model == C3SC_MODEL_SKID5D) return 2; // cos / sin of the orientation x2
    return model == C3SC_MODEL_DUBINS3D ? 2 : (model == C3SC_MODEL_SCAR4D ? 3 : ((model == C3SC_MODEL_CAR7D || model == C3SC_MODEL_PERCH7D) ? 4 : 0));
}
__host__ __device__ inline int model_tab_dim(int model, int t)
{
    if (model == C3SC_MODEL_PERCH7D) return t < 2 ? 2 : 3; // cos / sin of the pitch x2, cos / sin of the elevator angle x3
    if (model == C3SC_MODEL_CAR7D) return t == 2 ? 5 : (t == 3 ? 3 : 2);
    if (model == C3SC_MODEL_SCAR4D) return t == 2 ? 3 : 2;
    return 2;
}
__host__ __device__ inline double model_table_value(int model, int t, double xv)
{
    if (t == 0) return cos(xv);
    if (t == 1) return sin(xv);
    if (model == C3SC_MODEL_PERCH7D) return t == 2 ? cos(xv) : sin(xv);
    if (model == C3SC_MODEL_CAR7D && t == 2) return tan(xv);
    if (model == C3SC_MODEL_CAR7D && t == 3) return xv / (0.2 * (1.0 + xv / 8.0));
    if (model == C3SC_MODEL_SCAR4D && t == 2) return (1.0 / (1.0 + (xv / 8.0))) * (xv / 0.2); /* scar.c:68-71 with L = 0.2, vcar = 8 */
    return tan(xv);
}

} // namespace c3sc
