// The closed-loop additions of the facade (Robot::stateFeedbackTorques) and of the C ABI (idocp_rbd_policy_t, idocp_rbd_feedback_torques_batch,
// idocp_rbd_rollout_policy): compiles against include/ alone and, without a GPU, exercises the argument checks that need no device.
//   usage: closed_loop_surface
#include <cstdio>
#include <cstring>

#include "idocp/robot/robot.hpp"

int main() {
  // the member function exists with this signature
  void (idocp::Robot::*sf)(const Eigen::VectorXd&, const Eigen::VectorXd&, const Eigen::VectorXd&, const Eigen::VectorXd&, const Eigen::VectorXd&,
                           const Eigen::MatrixXd&, const Eigen::MatrixXd&, Eigen::VectorXd&) = &idocp::Robot::stateFeedbackTorques;
  if (!sf) return 1;
  idocp_rbd_policy_t pol;
  std::memset(&pol, 0, sizeof(pol));
  pol.shared_gains = 1; pol.shared_ref = 1;
  const int active[4] = {1, 1, 1, 1};
  const double x[19] = {};
  double u[12] = {};
  int bad = 0;
  bad += idocp_rbd_feedback_torques_batch(nullptr, 1, x, x, &pol, u) != IDOCP_E_ARG;
  bad += std::strstr(idocp_last_error(), "idocp_rbd_feedback_torques_batch") == nullptr;
  bad += idocp_rbd_feedback_torques_batch_device(nullptr, 1, x, x, &pol, u) != IDOCP_E_ARG;
  bad += std::strstr(idocp_last_error(), "idocp_rbd_feedback_torques_batch_device") == nullptr;
  bad += idocp_rbd_rollout_policy(nullptr, 1, 1, active, 0.05, 0.01, &pol, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1) != IDOCP_E_ARG;
  bad += std::strstr(idocp_last_error(), "idocp_rbd_rollout_policy") == nullptr;
  bad += idocp_rbd_rollout_policy_device(nullptr, 1, 1, active, 0.05, 0.01, &pol, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) != IDOCP_E_ARG;
  bad += std::strstr(idocp_last_error(), "idocp_rbd_rollout_policy_device") == nullptr;
  std::printf(bad ? "closed loop surface: %d wrong\n" : "closed loop surface: ok\n", bad);
  return bad;
}
