// fiber-pair (rank-split) instantiations for the other models (one kernel per varying dimension)
#include "launch_fpw.hpp"
#include "launch_fpp.hpp"
#include "models.hpp"
namespace c3sc {
#define REG3P(RP)                                        \
    C3SC_REG_FPP1(C3SC_MODEL_DUBINS3D, RP, 0, Dubins3D)  \
    C3SC_REG_FPP1(C3SC_MODEL_DUBINS3D, RP, 1, Dubins3D)  \
    C3SC_REG_FPP1(C3SC_MODEL_DUBINS3D, RP, 2, Dubins3D)
// K = 0: x and y both drift with theta alone; y is the only other uncontrolled dimension and merges into one vector right of K,
// theta keeps its pair: 3 vectors.  K = 2: both drifts read the varying dimension, nothing merges: 4.
static_assert(PairPark<Dubins3D, 0>::merged() == 0x2u && PairMap<Dubins3D, 0>::nv() == 3, "dubins3d: slot map of K = 0");
static_assert(PairPark<Dubins3D, 2>::merged() == 0x0u && PairMap<Dubins3D, 2>::nv() == 4, "dubins3d: slot map of K = 2");
REG3P(4)
REG3P(6)
REG3P(8)
#define REG3R(RP)                                          \
    C3SC_REG_FPP1(C3SC_MODEL_ROSSLER3D, RP, 0, Rossler3D)  \
    C3SC_REG_FPP1(C3SC_MODEL_ROSSLER3D, RP, 1, Rossler3D)  \
    C3SC_REG_FPP1(C3SC_MODEL_ROSSLER3D, RP, 2, Rossler3D)
REG3R(4)
REG3R(8)
#define REG4P(RP)                                    \
    C3SC_REG_FPP1(C3SC_MODEL_SCAR4D, RP, 0, Scar4D)  \
    C3SC_REG_FPP1(C3SC_MODEL_SCAR4D, RP, 1, Scar4D)  \
    C3SC_REG_FPP1(C3SC_MODEL_SCAR4D, RP, 2, Scar4D)  \
    C3SC_REG_FPP1(C3SC_MODEL_SCAR4D, RP, 3, Scar4D)
REG4P(4)
REG4P(8)
C3SC_REG_FPP1(C3SC_MODEL_LQGND, 4, 0, LqgNd<2>)
C3SC_REG_FPP1(C3SC_MODEL_LQGND, 4, 1, LqgNd<2>)
} // namespace c3sc
