// ANYmal standing: the time-varying affine policy of idocp::OCPSolver -- stage torques u_k, stage states (q_k, v_k) and the Riccati gains K_k --
// run on many perturbed plants at once, entirely on the GPU: idocp_rbd_rollout_policy evaluates u = u_k + K_k [q (-) q_k ; v - v_k] in front of
// every forward-dynamics step, with no host round trip (anymal_forward_simulation.cpp does the same loop at n = 1 through host calls).  One
// policy, shared by all plants; 256 initial states perturbed around q_0; once with the gains and once without (K = NULL: the open-loop
// torques).  Prints the largest final |x (-) x_ref| of both runs and their ratio.
//   usage: anymal_closed_loop_rollout <anymal.urdf> [steps = 10] [perturbation = 0.02]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "common.hpp"
#include "idocp/cost/configuration_space_cost.hpp"
#include "idocp/ocp/ocp_solver.hpp"

int main(int argc, char** argv) {
  idocp::Robot robot(ex::needUrdf(argc, argv, "[steps] [perturbation]"), ex::anymalFeet());
  const double T = 0.5, dt = 0.025;      // the plant steps with the solver's own stage length, which is also its Baumgarte time step
  const int N = 20, n = 256;
  const int steps = ex::argInt(argc, argv, 2, 10);
  const double eps = argc > 3 ? std::atof(argv[3]) : 0.02;
  if (steps < 1 || steps >= N) { std::fprintf(stderr, "steps must be in [1, %d)\n", N); return 2; }
  const ex::Vec stand = ex::anymalStanding();

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
  const ex::Vec v0 = ex::Vec::Zero(robot.dimv());
  for (int it = 0; it < 20; ++it) solver.updateSolution(0.0, stand, v0);      // to convergence at the nominal state

  // the policy of the first stages, shared by every plant: u_ff [steps][n][nu], K [steps][nu * 2 nv] = [Kq | Kv], q_ref [steps][nq], v_ref [steps][nv]
  const int nq = robot.dimq(), nv = robot.dimv(), nu = robot.dimu();
  std::vector<double> u_ff((size_t)steps * n * nu), K((size_t)steps * nu * 2 * nv), q_ref((size_t)steps * nq), v_ref((size_t)steps * nv);
  Eigen::MatrixXd Kq, Kv;
  for (int k = 0; k < steps; ++k) {
    const idocp::SplitSolution& s = solver.getSolution(k);
    solver.getStateFeedbackGain(k, Kq, Kv);
    for (int i = 0; i < n; ++i) for (int j = 0; j < nu; ++j) u_ff[((size_t)k * n + i) * nu + j] = s.u[j];
    for (int c = 0; c < nv; ++c) for (int r = 0; r < nu; ++r) {
      K[(size_t)k * nu * 2 * nv + (size_t)c * nu + r] = Kq(r, c);
      K[(size_t)k * nu * 2 * nv + (size_t)(nv + c) * nu + r] = Kv(r, c);
    }
    for (int j = 0; j < nq; ++j) q_ref[(size_t)k * nq + j] = s.q[j];
    for (int j = 0; j < nv; ++j) v_ref[(size_t)k * nv + j] = s.v[j];
  }
  const ex::Vec q_end = solver.getSolution(steps).q, v_end = solver.getSolution(steps).v;

  // the plants: q_0 (+) d, every tangent coordinate of d uniform in [-eps, eps] (a fixed sequence), at rest; the feet are held at the nominal footholds
  std::vector<double> q0((size_t)n * nq), pts((size_t)steps * n * 12);
  std::vector<int> active((size_t)steps * 4, 1);
  unsigned long long seed = 88172645463325252ull;
  auto uniform = [&seed]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
  ex::Vec d(nv), qi(nq);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < nv; ++j) d[j] = eps * uniform();
    robot.integrateConfiguration(stand, d, 1.0, qi);
    for (int j = 0; j < nq; ++j) q0[(size_t)i * nq + j] = qi[j];
  }
  robot.updateFrameKinematics(stand);
  std::vector<ex::V3> feet;
  robot.getContactPoints(feet);
  for (size_t e = 0; e < (size_t)steps * n; ++e) for (int c = 0; c < 4; ++c) for (int k = 0; k < 3; ++k) pts[e * 12 + 3 * c + k] = feet[c][k];

  idocp_rbd_t* h = nullptr;
  if (idocp_rbd_create(&robot.model(), 0, &h) != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); return 1; }
  idocp_rbd_policy_t pol = idocp_rbd_policy_t();
  pol.u_ff = u_ff.data(); pol.q_ref = q_ref.data(); pol.v_ref = v_ref.data();
  pol.shared_gains = 1; pol.shared_ref = 1;
  double worst[2] = {0.0, 0.0};
  for (int run = 0; run < 2; ++run) {
    pol.K = run == 0 ? K.data() : nullptr;
    std::vector<double> q_traj((size_t)(steps + 1) * n * nq), v_traj((size_t)(steps + 1) * n * nv, 0.0);
    for (size_t e = 0; e < q0.size(); ++e) q_traj[e] = q0[e];
    if (idocp_rbd_rollout_policy(h, n, steps, active.data(), dt, dt, &pol, pts.data(), q_traj.data(), v_traj.data(), nullptr, nullptr, nullptr, 0) != IDOCP_OK) {
      std::fprintf(stderr, "%s\n", idocp_last_error()); return 1;
    }
    for (int i = 0; i < n; ++i) {
      ex::Vec q(nq), diff(nv);
      for (int j = 0; j < nq; ++j) q[j] = q_traj[((size_t)steps * n + i) * nq + j];
      robot.subtractConfiguration(q, q_end, diff);
      double s = 0.0;
      for (int j = 0; j < nv; ++j) { const double dv = v_traj[((size_t)steps * n + i) * nv + j] - v_end[j]; s += diff[j] * diff[j] + dv * dv; }
      worst[run] = std::fmax(worst[run], std::sqrt(s));
      if (!std::isfinite(s)) worst[run] = s;
    }
  }
  idocp_rbd_destroy(h);
  std::printf("%d plants, %d steps of %.3f s, perturbation %.3g\n", n, steps, dt, eps);
  std::printf("closed loop: max final |x (-) x_ref| = %.6e\n", worst[0]);
  std::printf("open loop:   max final |x (-) x_ref| = %.6e\n", worst[1]);
  std::printf("ratio closed / open = %.4f\n", worst[0] / worst[1]);
  return (std::isfinite(worst[0]) && std::isfinite(worst[1])) ? 0 : 1;
}
