// Markov-chain walk / transitions instantiations (kernel_chain_walk.hpp): 3-D Dubins car and 2-D LQG, at the padded ranks
// their rollout kernels register
#include "kernel_chain_walk.hpp"
#include "models.hpp"
namespace c3sc {
C3SC_CHAIN_KERNELS(C3SC_MODEL_DUBINS3D, 4, Dubins3D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_DUBINS3D, 6, Dubins3D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_DUBINS3D, 8, Dubins3D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_DUBINS3D, 12, Dubins3D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_DUBINS3D, 16, Dubins3D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_DUBINS3D, 20, Dubins3D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_LQGND, 4, LqgNd<2>)
C3SC_CHAIN_KERNELS(C3SC_MODEL_LQGND, 8, LqgNd<2>)
C3SC_CHAIN_KERNELS(C3SC_MODEL_LQGND, 12, LqgNd<2>)
C3SC_CHAIN_KERNELS(C3SC_MODEL_LQGND, 20, LqgNd<2>)
} // namespace c3sc
