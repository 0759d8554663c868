// Markov-chain walk / transitions instantiations (kernel_chain_walk.hpp): the 6-D co-thrust vehicle, at the padded ranks its
// rollout kernels register
#include "kernel_chain_walk.hpp"
#include "models.hpp"
namespace c3sc {
C3SC_CHAIN_KERNELS(C3SC_MODEL_COTHRUST6D, 4, Cothrust6D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_COTHRUST6D, 8, Cothrust6D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_COTHRUST6D, 12, Cothrust6D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_COTHRUST6D, 16, Cothrust6D)
C3SC_CHAIN_KERNELS(C3SC_MODEL_COTHRUST6D, 20, Cothrust6D)
} // namespace c3sc
