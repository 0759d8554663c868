// fiber-pair (rank-split) instantiations: synthetic 7-D car, one kernel per varying dimension
#include "launch_fpw.hpp"
#include "launch_fpp.hpp"
#include "models.hpp"
namespace c3sc {
#define REG7P(RP)                                  \
    C3SC_REG_FPP1(C3SC_MODEL_CAR7D, RP, 0, Car7D)  \
    C3SC_REG_FPP1(C3SC_MODEL_CAR7D, RP, 1, Car7D)  \
    C3SC_REG_FPP1(C3SC_MODEL_CAR7D, RP, 2, Car7D)  \
    C3SC_REG_FPP1(C3SC_MODEL_CAR7D, RP, 3, Car7D)  \
    C3SC_REG_FPP1(C3SC_MODEL_CAR7D, RP, 4, Car7D)  \
    C3SC_REG_FPP1(C3SC_MODEL_CAR7D, RP, 5, Car7D)  \
    C3SC_REG_FPP1(C3SC_MODEL_CAR7D, RP, 6, Car7D)
// merged dimensions (bit m) and folded vectors per varying dimension, worked out by hand from Car7D::dep_mask: 48 vectors over
// a step instead of 7 x 12
#define CAR7_MAP(K, MERGED, NVEC)                                                                   \
    static_assert(PairPark<Car7D, K>::merged() == (MERGED), "car7d: merged dimensions of K = " #K); \
    static_assert(PairMap<Car7D, K>::nv() == (NVEC), "car7d: folded vectors of K = " #K);
CAR7_MAP(0, 0x1Eu, 5)  // 1,2,3,4
CAR7_MAP(1, 0x1Du, 6)  // 0 | 2,3,4
CAR7_MAP(2, 0x18u, 9)  // 3,4
CAR7_MAP(3, 0x04u, 11) // 2
CAR7_MAP(4, 0x0Bu, 7)  // 0,1,3
CAR7_MAP(5, 0x0Fu, 5)  // 0,1,2,3
CAR7_MAP(6, 0x17u, 5)  // 0,1,2,4
REG7P(4)
REG7P(10)
} // namespace c3sc
