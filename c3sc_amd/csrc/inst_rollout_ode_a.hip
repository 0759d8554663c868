// closed-loop integration instantiations (kernel_rollout_ode.hpp): the 2-D / 3-D models and the chain at small d, at the padded
// ranks of their examples and tests; BOX where the model's Bellman kernels serve the control box
#include "kernel_rollout_ode.hpp"
#include "models.hpp"
namespace c3sc {
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_DUBINS3D, 4, false, Dubins3D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_DUBINS3D, 6, false, Dubins3D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_DUBINS3D, 8, false, Dubins3D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_LQGND, 4, true, LqgNd<2>)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_LQGND, 8, true, LqgNd<2>)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_LQGND, 20, true, LqgNd<2>)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_CHAIN, 4, false, Chain<2>)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_CHAIN, 4, false, Chain<4>)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_ROSSLER3D, 4, true, Rossler3D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_ROSSLER3D, 8, true, Rossler3D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_TPROB3D, 4, true, Tprob3D)
C3SC_REG_ROLLOUT_ODE(C3SC_MODEL_TPROB3D, 12, true, Tprob3D)
} // namespace c3sc
