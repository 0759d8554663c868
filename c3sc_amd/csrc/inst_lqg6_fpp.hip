// fiber-pair (rank-split) instantiations: 6-D LQG (examples/lqgnd)
#include "launch_fpw.hpp"
#include "launch_fpp.hpp"
#include "models.hpp"
namespace c3sc {
#define REG6P(RP)                                     \
    C3SC_REG_FPP1(C3SC_MODEL_LQGND, RP, 0, LqgNd<6>)  \
    C3SC_REG_FPP1(C3SC_MODEL_LQGND, RP, 1, LqgNd<6>)  \
    C3SC_REG_FPP1(C3SC_MODEL_LQGND, RP, 2, LqgNd<6>)  \
    C3SC_REG_FPP1(C3SC_MODEL_LQGND, RP, 3, LqgNd<6>)  \
    C3SC_REG_FPP1(C3SC_MODEL_LQGND, RP, 4, LqgNd<6>)  \
    C3SC_REG_FPP1(C3SC_MODEL_LQGND, RP, 5, LqgNd<6>)
// K = 1: the uncontrolled dimensions 2 and 4 (drifts x3, x5) merge into one vector right of K, 0 (drift x1) does not: 3 pairs + 1
static_assert(PairPark<LqgNd<6>, 1>::merged() == 0x14u && PairMap<LqgNd<6>, 1>::nv() == 7, "lqg6d: slot map of K = 1");
REG6P(4)
REG6P(8)
} // namespace c3sc
