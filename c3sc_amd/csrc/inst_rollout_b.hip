// rollout / off-grid stencil instantiations (kernel_rollout.hpp): synthetic 7-D car and the 6-D quadcopter of
// examples/cothrust2 (per-candidate features; candidate lists and the control box), at the padded ranks their Bellman
// kernels register
#include "kernel_rollout.hpp"
#include "models.hpp"
namespace c3sc {
C3SC_REG_ROLLOUT(C3SC_MODEL_CAR7D, 4, false, Car7D)
C3SC_REG_ROLLOUT(C3SC_MODEL_CAR7D, 10, false, Car7D)
C3SC_REG_ROLLOUT(C3SC_MODEL_CAR7D, 12, false, Car7D)
C3SC_REG_ROLLOUT(C3SC_MODEL_CAR7D, 16, false, Car7D)
C3SC_REG_ROLLOUT(C3SC_MODEL_CAR7D, 20, false, Car7D)
C3SC_REG_ROLLOUT(C3SC_MODEL_COTHRUST6D, 4, true, Cothrust6D)
C3SC_REG_ROLLOUT(C3SC_MODEL_COTHRUST6D, 8, true, Cothrust6D)
C3SC_REG_ROLLOUT(C3SC_MODEL_COTHRUST6D, 12, true, Cothrust6D)
C3SC_REG_ROLLOUT(C3SC_MODEL_COTHRUST6D, 16, true, Cothrust6D)
C3SC_REG_ROLLOUT(C3SC_MODEL_COTHRUST6D, 20, true, Cothrust6D)
C3SC_REG_STENCIL_POINTS(6, 4)
C3SC_REG_STENCIL_POINTS(6, 8)
C3SC_REG_STENCIL_POINTS(6, 12)
C3SC_REG_STENCIL_POINTS(6, 16)
C3SC_REG_STENCIL_POINTS(6, 20)
C3SC_REG_STENCIL_POINTS(7, 4)
C3SC_REG_STENCIL_POINTS(7, 10)
C3SC_REG_STENCIL_POINTS(7, 12)
C3SC_REG_STENCIL_POINTS(7, 16)
C3SC_REG_STENCIL_POINTS(7, 20)
} // namespace c3sc
