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
// three-core product tables: rank 10 only; the plan of every K, of which fpp_table3_optout leaves K = 0, 1 to run
C3SC_FPP_TABLE3(Car7D, 10)
#define CAR7_PLAN3(K, ROUNDS, PRODUCTS)                                                                                  \
    static_assert(PairMap<Car7D, K, true, true>::plan().staged == (ROUNDS), "car7d: three-core staging rounds of K = " #K); \
    static_assert(PairMap<Car7D, K, true, true>::plan().products == (PRODUCTS), "car7d: three-core products of K = " #K);
CAR7_PLAN3(0, 3, 24)
CAR7_PLAN3(1, 2, 16)
CAR7_PLAN3(2, 1, 8)
CAR7_PLAN3(3, 0, 0)
CAR7_PLAN3(4, 1, 6)
CAR7_PLAN3(5, 2, 8)
CAR7_PLAN3(6, 3, 16)
// parked node split of the middle K at rank 10: the kernels stand in inst_car7d_fpp_pk.hip
C3SC_FPP_PARKED(Car7D, 10, 2)
C3SC_FPP_PARKED(Car7D, 10, 4)
REG7P(4)
REG7P(10)
} // namespace c3sc
