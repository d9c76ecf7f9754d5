// The forward-dynamics additions of the facade (Robot::forwardDynamics, impulseDynamics, stepForwardEuler) and of the C ABI
// (idocp_rbd_fd_io_t, idocp_rbd_forward_dynamics_batch, idocp_rbd_rollout): compiles against include/ alone and, without a GPU, exercises the
// argument checks that need no device.
//   usage: forward_dynamics_surface
#include <cstdio>
#include <cstring>
#include <vector>

#include "idocp/robot/robot.hpp"

int main() {
  // the member functions exist with these signatures
  void (idocp::Robot::*fd)(const Eigen::VectorXd&, const Eigen::VectorXd&, const Eigen::VectorXd&, const idocp::ContactStatus&, const double, Eigen::VectorXd&,
                           std::vector<Eigen::Vector3d>&) = &idocp::Robot::forwardDynamics;
  void (idocp::Robot::*id)(const Eigen::VectorXd&, const Eigen::VectorXd&, const idocp::ImpulseStatus&, Eigen::VectorXd&, std::vector<Eigen::Vector3d>&) =
      &idocp::Robot::impulseDynamics;
  void (idocp::Robot::*st)(const Eigen::VectorXd&, const Eigen::VectorXd&, const Eigen::VectorXd&, const idocp::ContactStatus&, const double, const double,
                           Eigen::VectorXd&, Eigen::VectorXd&) = &idocp::Robot::stepForwardEuler;
  if (!fd || !id || !st) return 1;
  idocp_rbd_fd_io_t io;
  std::memset(&io, 0, sizeof(io));
  const int active[4] = {1, 1, 1, 1};
  int bad = 0;
  bad += idocp_rbd_forward_dynamics_batch(nullptr, IDOCP_RBD_STAGE, 1, active, 0.05, 0.01, &io) != IDOCP_E_ARG;
  bad += std::strlen(idocp_last_error()) == 0;
  bad += idocp_rbd_forward_dynamics_batch_device(nullptr, IDOCP_RBD_IMPULSE, 1, active, 0.0, 0.0, &io) != IDOCP_E_ARG;
  bad += idocp_rbd_rollout(nullptr, 1, 1, active, 0.05, 0.01, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != IDOCP_E_ARG;
  bad += idocp_rbd_rollout_device(nullptr, 1, 0, active, 0.05, 0.01, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) != IDOCP_E_ARG;
  std::printf(bad ? "forward dynamics surface: %d wrong\n" : "forward dynamics surface: ok\n", bad);
  return bad;
}
