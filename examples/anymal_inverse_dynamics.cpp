// ANYmal standing still: gravity-compensation torques and the contact residual, through idocp::Robot.
// Robot::RNEA with the weight shared by the four feet gives the joint torques that hold the standing posture (the u_ref of a
// torque cost); Robot::computeBaumgarteResidual at rest with the feet on their own footholds is zero.  Each call is one n = 1 launch
// of the batched rigid-body API (idocp_rbd_contact_dynamics_batch in idocp_hip.h takes many states at once).
//   usage: anymal_inverse_dynamics <anymal.urdf>
#include <cmath>

#include "common.hpp"

int main(int argc, char** argv) {
  idocp::Robot robot(ex::needUrdf(argc, argv), ex::anymalFeet());
  const ex::Vec q = ex::anymalStanding();
  const ex::Vec zero = ex::Vec::Zero(robot.dimv());

  idocp::ContactStatus standing = robot.createContactStatus();
  standing.activateContacts();
  robot.updateKinematics(q, zero, zero);
  robot.setContactPoints(standing);
  // the weight in the local frame of each foot: the world's z axis there
  std::vector<ex::V3> f;
  for (const int frame : robot.contactFramesIndices()) {
    const Eigen::Matrix3d R = robot.frameRotation(frame);
    const double share = robot.totalWeight() / robot.maxPointContacts();
    f.push_back(ex::V3(share * R(2, 0), share * R(2, 1), share * R(2, 2)));
  }
  robot.setContactForces(standing, f);
  ex::Vec tau(robot.dimv());
  robot.RNEA(q, zero, zero, tau);
  std::cout << "generalized forces at rest (base wrench, then u_ref of the 12 joints):\n  " << tau << "\n";
  double base = 0.0;
  for (int k = 0; k < 3; ++k) base = std::fmax(base, std::fabs(tau[k]));
  std::cout << "largest unbalanced force on the base: " << base << " N\n";

  ex::Vec C(standing.dimf());
  robot.computeBaumgarteResidual(standing, 0.05, standing.contactPoints(), C);
  double worst = 0.0;
  for (int k = 0; k < C.size(); ++k) worst = std::fmax(worst, std::fabs(C[k]));
  std::cout << "Baumgarte residual of the four feet: max |C| = " << worst << "\n";
  return 0;
}
