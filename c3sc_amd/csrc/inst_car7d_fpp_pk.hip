// fiber-pair kernels of the parked node split (kernel_fiber_pair.hpp: fpp_parked): synthetic 7-D car at rank 10, the middle K.
// A translation unit of its own: k_fiber_pair_pk / k_fiber_pair_part_pk keep their resource remarks in pk_res/, and
// inst_car7d_fpp.hip -- which registers these K and calls launch_fpp_parked -- compiles the kernels it compiled before.
#include "launch_fpp.hpp"
#include "models.hpp"
namespace c3sc {
// vectors in LDS / in registers, and the rows of a tile (64 doubles each): hand-over or L, R, VX, PX below the homes
#define CAR7_PARKED(K, P, HOME, ROWS)                                                                                       \
    static_assert(fpp_parked<Car7D, 10, K>() == (P), "car7d: parked vectors of K = " #K);                                  \
    static_assert(fpp_parked_home_row<Car7D, 10, K>() == (HOME) && fpp_parked_rows<Car7D, 10, K>() == (ROWS), "car7d: rows of K = " #K); \
    /* the footprint does not move: not above the rank-split rows, nor above the staged image of the 41-node grid */       \
    static_assert(fpp_tile_doubles<Car7D, 10, K>(true, true) <= fpp_tile_doubles<Car7D, 10, K>(false), "car7d: LDS of K = " #K); \
    static_assert(fpp_tile_doubles<Car7D, 10, K>(true, true) <= (size_t)41 * fpl_lds_stride(10 * 10), "car7d: staged image, K = " #K);
CAR7_PARKED(2, 3, 31, 61)
CAR7_PARKED(4, FPP_PARKED_K4, 31, 31 + 10 * FPP_PARKED_K4)
static_assert(fpp_parked<Car7D, 10, 0>() == 0 && fpp_parked<Car7D, 10, 1>() == 0 && fpp_parked<Car7D, 10, 3>() == 0 &&
              fpp_parked<Car7D, 10, 5>() == 0 && fpp_parked<Car7D, 10, 6>() == 0, "car7d: every other K keeps its form");
C3SC_FPP_PARKED_KERNELS(Car7D, 10, 2)
C3SC_FPP_PARKED_KERNELS(Car7D, 10, 4)
} // namespace c3sc
