// rollout / off-grid stencil instantiations (kernel_rollout.hpp): 3-D Dubins car (periodic heading, obstacle) and 2-D LQG
// (candidate lists and the control box), at the padded ranks their Bellman kernels register
#include "kernel_rollout.hpp"
#include "models.hpp"
namespace c3sc {
C3SC_REG_ROLLOUT(C3SC_MODEL_DUBINS3D, 4, false, Dubins3D)
C3SC_REG_ROLLOUT(C3SC_MODEL_DUBINS3D, 6, false, Dubins3D)
C3SC_REG_ROLLOUT(C3SC_MODEL_DUBINS3D, 8, false, Dubins3D)
C3SC_REG_ROLLOUT(C3SC_MODEL_DUBINS3D, 12, false, Dubins3D)
C3SC_REG_ROLLOUT(C3SC_MODEL_DUBINS3D, 16, false, Dubins3D)
C3SC_REG_ROLLOUT(C3SC_MODEL_DUBINS3D, 20, false, Dubins3D)
C3SC_REG_ROLLOUT(C3SC_MODEL_LQGND, 4, true, LqgNd<2>)
C3SC_REG_ROLLOUT(C3SC_MODEL_LQGND, 8, true, LqgNd<2>)
C3SC_REG_ROLLOUT(C3SC_MODEL_LQGND, 12, true, LqgNd<2>)
C3SC_REG_ROLLOUT(C3SC_MODEL_LQGND, 20, true, LqgNd<2>)
C3SC_REG_STENCIL_POINTS(2, 4)
C3SC_REG_STENCIL_POINTS(2, 8)
C3SC_REG_STENCIL_POINTS(2, 12)
C3SC_REG_STENCIL_POINTS(2, 20)
C3SC_REG_STENCIL_POINTS(3, 4)
C3SC_REG_STENCIL_POINTS(3, 6)
C3SC_REG_STENCIL_POINTS(3, 8)
C3SC_REG_STENCIL_POINTS(3, 12)
C3SC_REG_STENCIL_POINTS(3, 16)
C3SC_REG_STENCIL_POINTS(3, 20)
} // namespace c3sc
