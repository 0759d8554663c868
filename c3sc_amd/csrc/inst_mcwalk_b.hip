// Markov-chain walk / transitions instantiations (kernel_chain_walk.hpp): the 7-D car, at the padded ranks its rollout
// kernels register
#include "kernel_chain_walk.hpp"
#include "models.hpp"
namespace c3sc {
C3SC_CHAIN_KERNELS(C3SC_MODEL_CAR7D, 4, Car7D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_CAR7D, 10, Car7D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_CAR7D, 12, Car7D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_CAR7D, 16, Car7D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_CAR7D, 20, Car7D)
} // namespace c3sc
