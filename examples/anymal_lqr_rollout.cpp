// ANYmal standing, the workload of anymal_closed_loop_rollout.cpp: the feed-forward torques of idocp::OCPSolver are rolled out on the nominal
// plant (idocp_rbd_rollout), that rollout is linearised (idocp_rbd_linearize_rollout) and idocp_rbd_lqr_backward turns A_k, B_k into time-varying
// LQR gains ABOUT THE ROLLOUT, with the example's own cost: x_weight = dt [q_weight; v_weight], u_weight = dt u_weight (zero here, so a small
// regularisation keeps Quu definite: with four feet on the ground only six directions of the torques move the plant), xf_weight = [qf_weight;
// vf_weight].  The a_weight and f_weight terms of the cost have no place in a diagonal x_weight / u_weight and are left out.
// 256 perturbed plants then run three ways on the GPU: the torques alone, the solver's Riccati gains about the solver's states, and the LQR
// gains about the rollout.  Prints, for each, the mean final distance |x (-) x_nominal| from the end of the nominal rollout over the plants
// that stayed finite, and the number that did not; and the largest difference between the LQR run and the nominal rollout anywhere on the
// trajectory, which is exactly 0 at perturbation 0 (K 0 adds nothing).  No ranking of the three is claimed.
//   usage: anymal_lqr_rollout <anymal.urdf> [steps = 10] [perturbation = 0.02]
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
  const double q_weight = 10, v_weight = 1, a_weight = 0.01, u_weight = 0, regularization = 1e-6;      // (qf_weight = q_weight, vf_weight = v_weight: attachWeights)

  auto pose_cost = std::make_shared<idocp::ConfigurationSpaceCost>(robot);
  pose_cost->set_q_ref(stand);
  ex::attachWeights(*pose_cost, ex::filled(18, q_weight), ex::filled(18, v_weight), ex::filled(18, a_weight), false);
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

  // the solver's policy of the first stages: u_ff [steps][n][nu], K [steps][nu * 2 nv] = [Kq | Kv], q_ref [steps][nq], v_ref [steps][nv]
  const int nq = robot.dimq(), nv = robot.dimv(), nu = robot.dimu(), nx = 2 * nv;
  std::vector<double> u_ff((size_t)steps * n * nu), u_nom((size_t)steps * nu), K_ric((size_t)steps * nu * nx), q_sol((size_t)steps * nq), v_sol((size_t)steps * nv);
  Eigen::MatrixXd Kq, Kv;
  for (int k = 0; k < steps; ++k) {
    const idocp::SplitSolution& s = solver.getSolution(k);
    solver.getStateFeedbackGain(k, Kq, Kv);
    for (int j = 0; j < nu; ++j) u_nom[(size_t)k * nu + j] = s.u[j];
    for (int i = 0; i < n; ++i) for (int j = 0; j < nu; ++j) u_ff[((size_t)k * n + i) * nu + j] = s.u[j];
    for (int c = 0; c < nv; ++c) for (int r = 0; r < nu; ++r) {
      K_ric[(size_t)k * nu * nx + (size_t)c * nu + r] = Kq(r, c);
      K_ric[(size_t)k * nu * nx + (size_t)(nv + c) * nu + r] = Kv(r, c);
    }
    for (int j = 0; j < nq; ++j) q_sol[(size_t)k * nq + j] = s.q[j];
    for (int j = 0; j < nv; ++j) v_sol[(size_t)k * nv + j] = s.v[j];
  }

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
  auto ok = [](int rc) { if (rc != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); std::exit(1); } };
  ok(idocp_rbd_create(&robot.model(), 0, &h));

  // ---- 1. the nominal plant under the solver's torques, 2. its linearisation, 3. the LQR gains about it ----
  std::vector<double> q_nom((size_t)(steps + 1) * nq), v_nom((size_t)(steps + 1) * nv, 0.0);
  for (int j = 0; j < nq; ++j) q_nom[j] = stand[j];
  std::vector<double> pts1((size_t)steps * 12);
  for (int k = 0; k < steps; ++k) for (int e = 0; e < 12; ++e) pts1[(size_t)k * 12 + e] = pts[(size_t)k * n * 12 + e];
  ok(idocp_rbd_rollout(h, 1, steps, active.data(), dt, dt, u_nom.data(), pts1.data(), q_nom.data(), v_nom.data(), nullptr, nullptr, 0));
  std::vector<double> A((size_t)steps * nx * nx), B((size_t)steps * nx * nu), K_lqr((size_t)steps * nu * nx);
  ok(idocp_rbd_linearize_rollout(h, 1, steps, active.data(), dt, dt, u_nom.data(), pts1.data(), q_nom.data(), v_nom.data(), A.data(), B.data(), 0));
  std::vector<double> wx(nx), wu(nu, dt * u_weight), wxf(nx);
  for (int j = 0; j < nv; ++j) { wx[j] = dt * q_weight; wx[nv + j] = dt * v_weight; wxf[j] = q_weight; wxf[nv + j] = v_weight; }
  int status = 0;
  idocp_rbd_lqr_io_t lqr = idocp_rbd_lqr_io_t();
  lqr.A_traj = A.data(); lqr.B_traj = B.data(); lqr.x_weight = wx.data(); lqr.u_weight = wu.data(); lqr.xf_weight = wxf.data();
  lqr.regularization = regularization; lqr.K_traj = K_lqr.data(); lqr.status = &status;
  ok(idocp_rbd_lqr_backward(h, 1, steps, &lqr));
  if (status >= 0) { std::fprintf(stderr, "the LQR backward pass failed at step %d\n", status); return 1; }

  // ---- 4. the perturbed plants three ways ----
  const char* const names[3] = {"no gains", "solver's Riccati gains", "LQR gains about the rollout"};
  double mean[3] = {0.0, 0.0, 0.0}, off_nominal = 0.0;
  int lost[3] = {0, 0, 0};
  ex::Vec q_end(nq);
  for (int j = 0; j < nq; ++j) q_end[j] = q_nom[(size_t)steps * nq + j];
  for (int run = 0; run < 3; ++run) {
    idocp_rbd_policy_t pol = idocp_rbd_policy_t();
    pol.u_ff = u_ff.data(); pol.shared_gains = 1; pol.shared_ref = 1;
    if (run == 1) { pol.K = K_ric.data(); pol.q_ref = q_sol.data(); pol.v_ref = v_sol.data(); }
    if (run == 2) { pol.K = K_lqr.data(); pol.q_ref = q_nom.data(); pol.v_ref = v_nom.data(); }
    std::vector<double> q_traj((size_t)(steps + 1) * n * nq), v_traj((size_t)(steps + 1) * n * nv, 0.0);
    for (size_t e = 0; e < q0.size(); ++e) q_traj[e] = q0[e];
    ok(idocp_rbd_rollout_policy(h, n, steps, active.data(), dt, dt, &pol, pts.data(), q_traj.data(), v_traj.data(), nullptr, nullptr, nullptr, 0));
    int kept = 0;
    for (int i = 0; i < n; ++i) {
      ex::Vec q(nq), diff(nv);
      for (int j = 0; j < nq; ++j) q[j] = q_traj[((size_t)steps * n + i) * nq + j];
      robot.subtractConfiguration(q, q_end, diff);
      double s = 0.0;
      for (int j = 0; j < nv; ++j) { const double dv = v_traj[((size_t)steps * n + i) * nv + j] - v_nom[(size_t)steps * nv + j]; s += diff[j] * diff[j] + dv * dv; }
      if (std::isfinite(s)) { mean[run] += std::sqrt(s); ++kept; } else { ++lost[run]; }
    }
    mean[run] = kept ? mean[run] / kept : NAN;
    if (run == 2)
      for (int k = 0; k <= steps; ++k) for (int i = 0; i < n; ++i) {
        for (int j = 0; j < nq; ++j) { const double g = std::fabs(q_traj[((size_t)k * n + i) * nq + j] - q_nom[(size_t)k * nq + j]); off_nominal = (g > off_nominal || !std::isfinite(g)) ? g : off_nominal; }
        for (int j = 0; j < nv; ++j) { const double g = std::fabs(v_traj[((size_t)k * n + i) * nv + j] - v_nom[(size_t)k * nv + j]); off_nominal = (g > off_nominal || !std::isfinite(g)) ? g : off_nominal; }
      }
  }
  idocp_rbd_destroy(h);
  std::printf("%d plants, %d steps of %.3f s, perturbation %.3g\n", n, steps, dt, eps);
  for (int run = 0; run < 3; ++run) std::printf("%s: mean final distance = %.6e, plants lost = %d\n", names[run], mean[run], lost[run]);
  std::printf("LQR run against the nominal rollout: max difference = %.6e\n", off_nominal);
  return (std::isfinite(mean[0]) && std::isfinite(mean[1]) && std::isfinite(mean[2])) ? 0 : 1;
}
