// closed-loop integration instantiations (kernel_rollout_ode.hpp): the cars (synthetic 7-D, both skidding cars) and the 6-D
// LQG, at the padded ranks of their examples and tests; BOX where the model's Bellman kernels serve the control box
#include "kernel_rollout_ode.hpp"
#include "models.hpp"
namespace c3sc {
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_CAR7D, 4, false, Car7D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_CAR7D, 10, false, Car7D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_SCAR4D, 4, false, Scar4D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_SCAR4D, 20, false, Scar4D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_SKID5D, 4, false, Skid5D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_SKID5D, 16, false, Skid5D) // the example's maxrank is 15
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_LQGND, 4, true, LqgNd<6>)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_LQGND, 8, true, LqgNd<6>)
} // namespace c3sc
