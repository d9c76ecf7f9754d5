// ANYmal standing, in closed loop against dynamics the solver did not predict: the stage-0 torques of idocp::OCPSolver drive the plant, and
// the plant is Robot::forwardDynamics / stepForwardEuler -- accelerations and contact forces from the torques, then the explicit Euler step of the
// OCP's own discretisation, each ONE n = 1 launch of idocp_rbd_forward_dynamics_batch (idocp_hip.h takes many states at once, and
// idocp_rbd_rollout chains the steps on the GPU).  The reference has no forward dynamics; its drivers advance the solver's own prediction.
// Prints, per step, the base height, the norm of the base quaternion, the largest acceleration and the vertical force on each foot.
//   usage: anymal_forward_simulation <anymal.urdf> [steps = 5]
#include <cmath>
#include <cstdio>

#include "common.hpp"
#include "idocp/cost/configuration_space_cost.hpp"
#include "idocp/ocp/ocp_solver.hpp"

int main(int argc, char** argv) {
  idocp::Robot robot(ex::needUrdf(argc, argv, "[steps]"), ex::anymalFeet());
  const int steps = ex::argInt(argc, argv, 2, 5);
  const ex::Vec stand = ex::anymalStanding();
  const double T = 0.5, dt = 0.025;      // the plant steps with the solver's own stage length, which is also its Baumgarte time step
  const int N = 20;

  auto pose_cost = std::make_shared<idocp::ConfigurationSpaceCost>(robot);
  pose_cost->set_q_ref(stand);
  ex::attachWeights(*pose_cost, ex::filled(18, 10), ex::filled(18, 1), ex::filled(18, 0.01), false);
  const ex::V3 share(0, 0, 70);
  auto cost = std::make_shared<idocp::CostFunction>();
  cost->push_back(pose_cost);
  cost->push_back(ex::forceCost(robot, ex::V3(0.001, 0.001, 0.001), false, &share));
  idocp::OCPSolver solver(robot, cost, ex::jointLimits(robot, 0.7, false, true), T, N, 4, 4);
  ex::Schedule standing(ex::footholds(robot, stand));
  standing.add({0, 1, 2, 3}, 0.0);
  standing.install(solver, robot);
  ex::restingGuess(solver, robot, stand);
  solver.initConstraints(0.0);

  idocp::ContactStatus feet = robot.createContactStatus();
  feet.activateContacts();
  robot.updateFrameKinematics(stand);
  robot.setContactPoints(feet);

  ex::Vec q = stand, v = ex::Vec::Zero(robot.dimv()), a(robot.dimv());
  std::vector<ex::V3> f;
  for (int it = 0; it < 10; ++it) solver.updateSolution(0.0, q, v);      // converge once at the initial state
  for (int k = 0; k < steps; ++k) {
    solver.updateSolution(0.0, q, v);                                     // one Newton step per control period at the MEASURED state
    const ex::Vec u = solver.getSolution(0).u;
    robot.forwardDynamics(q, v, u, feet, dt, a, f);
    robot.stepForwardEuler(q, v, u, feet, dt, dt, q, v);
    double amax = 0.0;
    for (int i = 0; i < robot.dimv(); ++i) amax = std::fmax(amax, std::fabs(a[i]));
    const double qn = std::sqrt(q[3] * q[3] + q[4] * q[4] + q[5] * q[5] + q[6] * q[6]);
    std::printf("step %d: base height = %.9f quaternion norm = %.17g max |a| = %.6e fz = %.4f %.4f %.4f %.4f\n", k, q[2], qn,
                amax, f[0][2], f[1][2], f[2][2], f[3][2]);
  }
  return 0;
}
