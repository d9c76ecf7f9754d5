// ANYmal trotting: the solver's torques and Riccati gains of the first stages, rolled out closed loop on 256 perturbed plants over a window
// that contains the first lift-off and the first touchdown -- once with footholds LATCHED per plant (idocp_rbd_rollout_footholds: a contact
// that closes is anchored where that plant's foot is), once with the NOMINAL's footholds forced on every plant (idocp_rbd_rollout_policy with
// the contact points of the nominal plant's latched run, the workaround the latched rollout replaces).  The set-up is the one of
// anymal_trotting.cpp, iterated a few times.  The schedule of the plant is time-driven: step k takes the stance of t = k dt.
// Prints, for both runs: the spread of the touchdown points over the plants (largest distance from their mean, in metres), the mean
// tangential (world x-y) contact force at the first step after the touchdown, and the mean final distance |x (-) x_ref| to the solver's state,
// each over the plants that stayed finite, whose number is printed first.  Exit status 1: a figure is not finite or no plant stayed finite.
//   usage: anymal_foothold_rollout <anymal.urdf> [steps = 22] [perturbation = 0.001] [iterations = 5]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "common.hpp"
#include "idocp/cost/trotting_configuration_space_cost.hpp"
#include "idocp/ocp/ocp_solver.hpp"

int main(int argc, char** argv) {
  idocp::Robot robot(ex::needUrdf(argc, argv, "[steps] [perturbation] [iterations]"), ex::anymalFeet());
  const double step = 0.15, t0 = 0.5, period = 0.5;
  const int touch_downs = 2, horizon = 30, n = 256;
  const double T = t0 + touch_downs * period + 0.05, dt = T / horizon;
  const int steps = ex::argInt(argc, argv, 2, 22);
  const double eps = argc > 3 ? std::atof(argv[3]) : 0.001;
  const int iterations = ex::argInt(argc, argv, 4, 5);
  if (steps < 1 || steps >= horizon) { std::fprintf(stderr, "steps must be in [1, %d)\n", horizon); return 2; }
  const ex::Vec stand = ex::anymalStanding();

  auto gait_cost = std::make_shared<idocp::TrottingConfigurationSpaceCost>(robot);
  idocp::TrottingSwingAngles swing;
  swing.front_swing_knee = swing.hip_swing_knee = 1.7;
  gait_cost->set_ref(t0, period, stand, step, swing);
  ex::attachWeights(*gait_cost, ex::filled(18, 10), ex::runs({{6, 1}, {12, 0.1}}), ex::runs({{6, 0.1}, {12, 0.01}}), true);
  auto cost = std::make_shared<idocp::CostFunction>();
  cost->push_back(gait_cost);
  cost->push_back(ex::forceCost(robot, ex::V3(0.001, 0.001, 0.001), true, nullptr));
  idocp::OCPSolver solver(robot, cost, ex::jointLimits(robot, 0.7, true), T, horizon, touch_downs + 1, 4);
  ex::Schedule gait(ex::footholds(robot, stand));
  gait.add({0, 1, 2, 3}, 0.0);
  gait.add({1, 2}, t0);
  gait.advance({0, 3}, 0.5 * step); gait.add({0, 3}, t0 + period);
  gait.advance({1, 2}, step); gait.add({1, 2}, t0 + 2 * period);
  gait.install(solver, robot);
  ex::restingGuess(solver, robot, stand);
  solver.initConstraints(0.0);
  const ex::Vec v0 = ex::Vec::Zero(robot.dimv());
  for (int it = 0; it < iterations; ++it) solver.updateSolution(0.0, stand, v0);

  // the plant's schedule: the stance of the gait table at t = k dt; the first step at which a contact opens / closes
  const int nq = robot.dimq(), nv = robot.dimv(), nu = robot.dimu();
  std::vector<int> active((size_t)steps * 4, 0);
  int lift_off = -1, touchdown = -1;
  for (int k = 0; k < steps; ++k) {
    size_t row = 0;
    for (size_t r = 0; r < gait.rows.size(); ++r) if (gait.rows[r].since <= k * dt + 1e-9) row = r;
    for (int c : gait.rows[row].stance) active[(size_t)k * 4 + c] = 1;
    for (int c = 0; c < 4 && k > 0; ++c) {
      if (lift_off < 0 && active[(size_t)(k - 1) * 4 + c] && !active[(size_t)k * 4 + c]) lift_off = k;
      if (touchdown < 0 && !active[(size_t)(k - 1) * 4 + c] && active[(size_t)k * 4 + c]) touchdown = k;
    }
  }

  // the policy of the first stages, shared by every plant (the layout of idocp_ocp_get_riccati: K = [Kq | Kv], column-major)
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

  // the plants: plant 0 is the nominal, the others q_0 (+) d with every tangent coordinate of d uniform in [-eps, eps] (a fixed sequence), at rest
  std::vector<double> q0((size_t)n * nq);
  unsigned long long seed = 88172645463325252ull;
  auto uniform = [&seed]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
  ex::Vec d(nv), qi(nq);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < nv; ++j) d[j] = i == 0 ? 0.0 : eps * uniform();
    robot.integrateConfiguration(stand, d, 1.0, qi);
    for (int j = 0; j < nq; ++j) q0[(size_t)i * nq + j] = qi[j];
  }

  idocp_rbd_t* h = nullptr;
  if (idocp_rbd_create(&robot.model(), 0, &h) != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); return 1; }
  idocp_rbd_policy_t pol = idocp_rbd_policy_t();
  pol.u_ff = u_ff.data(); pol.K = K.data(); pol.q_ref = q_ref.data(); pol.v_ref = v_ref.data();
  pol.shared_gains = 1; pol.shared_ref = 1;
  std::vector<double> u_max(robot.model().u_max, robot.model().u_max + nu), u_min(nu);      // the torque limits of the model clamp the feedback
  for (int j = 0; j < nu; ++j) u_min[j] = -u_max[j];
  pol.u_min = u_min.data(); pol.u_max = u_max.data();

  std::printf("%d plants, %d steps of %.4f s, perturbation %.3g, %d solver iterations; first lift-off at step %d, first touchdown at step %d\n", n,
              steps, dt, eps, iterations, lift_off, touchdown);
  const char* names[2] = {"latched footholds", "nominal footholds"};
  std::vector<double> pts((size_t)steps * n * 12, 0.0), nominal_pts;
  bool finite = true;
  for (int run = 0; run < 2; ++run) {
    std::vector<double> q_traj((size_t)(steps + 1) * n * nq), v_traj((size_t)(steps + 1) * n * nv, 0.0), f_traj((size_t)steps * n * 12);
    for (size_t e = 0; e < q0.size(); ++e) q_traj[e] = q0[e];
    int rc;
    if (run == 0) {
      idocp_rbd_foothold_rollout_t io = idocp_rbd_foothold_rollout_t();
      io.policy = &pol; io.contact_points = pts.data(); io.q_traj = q_traj.data(); io.v_traj = v_traj.data(); io.f_traj = f_traj.data();
      rc = idocp_rbd_rollout_footholds(h, n, steps, active.data(), dt, dt, &io, 1, 1);      // (latch_first: every plant starts on its own feet)
      nominal_pts = pts;
    } else {
      // the points of plant 0 of the latched run on every plant
      for (int k = 0; k < steps; ++k) for (int i = 0; i < n; ++i) for (int e = 0; e < 12; ++e)
        pts[((size_t)k * n + i) * 12 + e] = nominal_pts[(size_t)k * n * 12 + e];
      rc = idocp_rbd_rollout_policy(h, n, steps, active.data(), dt, dt, &pol, pts.data(), q_traj.data(), v_traj.data(), nullptr, nullptr, f_traj.data(), 1);
    }
    if (rc != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); return 1; }
    // a plant whose rollout left the finite numbers (it fell over and the contact solve lost definiteness) is counted and left out of the figures
    std::vector<char> up(n, 1);
    int first_bad = -1;
    for (int k = 0; k <= steps; ++k) for (int i = 0; i < n; ++i) for (int j = 0; j < nq; ++j)
      if (!std::isfinite(q_traj[((size_t)k * n + i) * nq + j])) { up[i] = 0; if (first_bad < 0) first_bad = k; }
    int alive = 0;
    for (int i = 0; i < n; ++i) alive += up[i];
    // the spread of the touchdown points and the tangential force behind the touchdown, over the contacts that closed there
    double spread = 0.0, tangential = 0.0;
    int closed = 0;
    if (touchdown > 0) {
      std::vector<double> rot((size_t)n * 36);
      idocp_rbd_kin_io_t kin = idocp_rbd_kin_io_t();
      kin.q = &q_traj[(size_t)touchdown * n * nq]; kin.rotation = rot.data();
      if (idocp_rbd_contact_kinematics_batch(h, n, &kin) != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); return 1; }
      for (int c = 0; c < 4; ++c) {
        if (!active[(size_t)touchdown * 4 + c] || active[(size_t)(touchdown - 1) * 4 + c]) continue;
        ++closed;
        double mean[3] = {0, 0, 0};
        for (int i = 0; i < n; ++i) for (int e = 0; e < 3 && up[i]; ++e) mean[e] += pts[((size_t)touchdown * n + i) * 12 + 3 * c + e] / alive;
        for (int i = 0; i < n; ++i) {
          if (!up[i]) continue;
          double s = 0.0;
          for (int e = 0; e < 3; ++e) { const double x = pts[((size_t)touchdown * n + i) * 12 + 3 * c + e] - mean[e]; s += x * x; }
          spread = std::fmax(spread, std::sqrt(s));
          if (!std::isfinite(s)) spread = s;
          // the world force: rotation [c] times the local coordinates of f_traj
          const double* R = &rot[((size_t)i * 4 + c) * 9];
          const double* f = &f_traj[((size_t)touchdown * n + i) * 12 + 3 * c];
          const double fx = R[0] * f[0] + R[1] * f[1] + R[2] * f[2], fy = R[3] * f[0] + R[4] * f[1] + R[5] * f[2];
          tangential += std::sqrt(fx * fx + fy * fy) / alive;
        }
      }
      if (closed) tangential /= closed;
    }
    double distance = 0.0;
    for (int i = 0; i < n; ++i) {
      if (!up[i]) continue;
      ex::Vec q(nq), diff(nv);
      for (int j = 0; j < nq; ++j) q[j] = q_traj[((size_t)steps * n + i) * nq + j];
      robot.subtractConfiguration(q, q_end, diff);
      double s = 0.0;
      for (int j = 0; j < nv; ++j) { const double dv = v_traj[((size_t)steps * n + i) * nv + j] - v_end[j]; s += diff[j] * diff[j] + dv * dv; }
      distance += std::sqrt(s) / alive;
    }
    std::printf("%s: finite plants = %d   touchdown spread = %.6e m   mean tangential force = %.6e N   mean final |x (-) x_ref| = %.6e\n", names[run],
                alive, spread, tangential, distance);
    if (first_bad >= 0) std::printf("%s: the first plant left the finite numbers at step %d\n", names[run], first_bad);
    finite = finite && alive > 0 && std::isfinite(spread) && std::isfinite(tangential) && std::isfinite(distance);
  }
  idocp_rbd_destroy(h);
  return finite ? 0 : 1;
}
