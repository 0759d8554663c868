// closed-loop integration instantiations (kernel_rollout_ode.hpp): glider perching and the quadcopter (both with the control
// box), at the padded ranks of their examples and tests
#include "kernel_rollout_ode.hpp"
#include "models.hpp"
namespace c3sc {
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_PERCH7D, 4, true, Perch7D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_PERCH7D, 16, true, Perch7D) // the example's maxrank is 15
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_COTHRUST6D, 4, true, Cothrust6D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_COTHRUST6D, 8, true, Cothrust6D)
} // namespace c3sc
