// The setting of anymal_ilqr_constrained.cpp -- 256 ANYmal plants a little off the standing pose under zero torques, the workload's cost, the joint
// limits, a tight acceleration box and a friction cone with a small coefficient -- improved three ways from the same start:
//   cost      idocp_rbd_ilqr_iterate_gn_device, which sees the cost alone;
//   penalty   idocp_rbd_ilqr_iterate_penalty_device with that example's schedule, mu raised by a factor per iteration;
//   AL        idocp_rbd_ilqr_iterate_al_device at the schedule's FIRST mu held fixed, idocp_rbd_ilqr_al_update_device after every second iteration,
//             the same total number of iterations.
// Prints per run the mean cost, the mean UNSHIFTED sq_violation, the largest infeasibility (the largest unshifted row of any plant) and the count
// of plants that fail (a backward pass that failed in the last iteration, or a score that is not finite; they are left out of the means).  Nothing
// is hidden.  Exit status 1 only when every plant failed in every run.
//   usage: anymal_ilqr_al <anymal.urdf> [steps = 10] [iterations = 5] [perturbation = 0.02] [plants = 256] [mu = 10] [factor = 4]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "common.hpp"
#include "idocp/cost/configuration_space_cost.hpp"
#include "idocp/cost/contact_force_cost.hpp"
#include "idocp/cost/cost_function.hpp"

namespace {

struct DeviceBuffer {
  double* p = nullptr;
  explicit DeviceBuffer(size_t doubles, const double* host = nullptr) {
    void* v = nullptr;
    if (idocp_device_alloc(&v, (doubles ? doubles : 1) * sizeof(double)) != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); std::exit(1); }
    p = static_cast<double*>(v);
    if (host && idocp_device_upload(p, host, doubles * sizeof(double)) != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); std::exit(1); }
  }
  ~DeviceBuffer() { idocp_device_free(p); }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
};

void must(int rc) { if (rc != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); std::exit(1); } }

}  // namespace

int main(int argc, char** argv) {
  idocp::Robot robot(ex::needUrdf(argc, argv, "[steps] [iterations] [perturbation] [plants] [mu] [factor]"), ex::anymalFeet());
  const double dt = 0.025;      // the stage length, which is also the Baumgarte time step
  const int steps = ex::argInt(argc, argv, 2, 10), iterations = ex::argInt(argc, argv, 3, 5);
  const double eps = argc > 4 ? std::atof(argv[4]) : 0.02;
  const int n = ex::argInt(argc, argv, 5, 256);
  const double mu0 = argc > 6 ? std::atof(argv[6]) : 10.0, factor = argc > 7 ? std::atof(argv[7]) : 4.0;
  if (steps < 1 || iterations < 1 || n < 1 || !(mu0 > 0.0)) { std::fprintf(stderr, "steps, iterations, plants and mu must be positive\n"); return 2; }
  const ex::Vec stand = ex::anymalStanding();

  auto pose_cost = std::make_shared<idocp::ConfigurationSpaceCost>(robot);
  pose_cost->set_q_ref(stand);
  ex::attachWeights(*pose_cost, ex::filled(18, 10), ex::runs({{6, 1.0}, {12, 0.1}}), ex::runs({{6, 0.1}, {12, 0.01}}), false);
  idocp::CostFunction cost;
  cost.push_back(pose_cost);
  cost.push_back(ex::forceCost(robot, ex::V3(0.001, 0.001, 0.001), false, nullptr));

  const int nq = robot.dimq(), nv = robot.dimv(), nu = robot.dimu();
  const size_t S = (size_t)steps, Nn = (size_t)n;
  std::vector<double> q_init((S + 1) * Nn * nq, 0.0), pts(S * Nn * 12);
  const std::vector<double> v_init((S + 1) * Nn * nv, 0.0), u_init(S * Nn * nu, 0.0);
  std::vector<int> active(S * 4, 1);
  unsigned long long seed = 88172645463325252ull;
  auto uniform = [&seed]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
  ex::Vec d(nv), qi(nq);
  for (size_t i = 0; i < Nn; ++i) {
    for (int j = 0; j < nv; ++j) d[j] = eps * uniform();
    robot.integrateConfiguration(stand, d, 1.0, qi);
    for (int j = 0; j < nq; ++j) q_init[i * nq + j] = qi[j];
  }
  robot.updateFrameKinematics(stand);
  std::vector<ex::V3> feet;
  robot.getContactPoints(feet);
  for (size_t e = 0; e < S * Nn; ++e) for (int c = 0; c < 4; ++c) for (int k = 0; k < 3; ++k) pts[e * 12 + 3 * c + k] = feet[c][k];

  idocp_rbd_t* h = nullptr;
  must(idocp_rbd_create(&robot.model(), 0, &h));
  const idocp_cost_t native_cost = cost.native();
  idocp_constraints_t native_constraints = ex::jointLimits(robot, 0.05)->native();
  native_constraints.joint_acceleration_lower_limit = native_constraints.joint_acceleration_upper_limit = 1;
  for (int j = 0; j < nu; ++j) { native_constraints.a_min[j] = -2.0; native_constraints.a_max[j] = 2.0; }
  idocp_rbd_objective_t* objective = nullptr;
  must(idocp_rbd_objective_create(h, &native_cost, &native_constraints, 0.0, dt, steps, &objective));
  const size_t L = (size_t)idocp_rbd_objective_multiplier_rows(objective);
  std::printf("%d plants, %d steps of %.3f s, %d iterations, perturbation %.3g, %d multiplier rows per (step, plant), mu %.3g (penalty: x %.3g per iteration; AL: fixed)\n",
              n, steps, dt, iterations, eps, (int)L, mu0, factor);

  int all_failed = 1;
  const char* const names[3] = {"cost", "penalty", "AL"};
  for (int run = 0; run < 3; ++run) {
    DeviceBuffer d_q(q_init.size(), q_init.data()), d_v(v_init.size(), v_init.data()), d_u(u_init.size(), u_init.data()), d_pts(pts.size(), pts.data());
    DeviceBuffer d_a(S * Nn * nv), d_f(S * Nn * 12), d_cost(Nn), d_viol(Nn), d_l1(Nn), d_sq(Nn), d_alpha(Nn), d_expected(2 * Nn), d_status((Nn + 1) / 2);
    DeviceBuffer d_inf(Nn), d_change(Nn);
    const std::vector<double> zeros(S * Nn * L, 0.0);
    DeviceBuffer d_lambda(S * Nn * L, zeros.data()), d_scratch(S * Nn * L);
    const unsigned long long bytes = run == 0 ? idocp_rbd_ilqr_gn_workspace_bytes(h, n, steps) : idocp_rbd_ilqr_penalty_workspace_bytes(h, objective, n, steps);
    DeviceBuffer d_work((size_t)(bytes / sizeof(double)));
    must(idocp_rbd_rollout_device(h, n, steps, active.data(), dt, dt, d_u.p, d_pts.p, d_q.p, d_v.p, d_a.p, d_f.p, 0));
    idocp_rbd_score_io_t score = idocp_rbd_score_io_t();
    score.q_traj = d_q.p; score.v_traj = d_v.p; score.u_traj = d_u.p; score.a_traj = d_a.p; score.f_traj = d_f.p; score.cost = d_cost.p; score.violation = d_l1.p;
    std::vector<double> c(Nn), sq(Nn), inf(Nn), alpha(Nn);
    std::vector<int> status(Nn + 1, -1);
    int failed_last = 0;
    // the scores of what the run holds now: the cost, the UNSHIFTED sq_violation, and the infeasibility (the multiplier update with lambda = NULL
    // into a scratch array: its statistic is the largest unshifted row); returns the plants counted as failed
    auto report = [&](const char* when) {
      must(idocp_rbd_score_rollout_device(h, objective, n, 0, steps, active.data(), 1, 0, &score));
      must(idocp_rbd_score_penalty_device(h, objective, n, 0, steps, active.data(), 0, d_q.p, d_v.p, d_u.p, d_a.p, d_f.p, d_sq.p));
      must(idocp_rbd_multiplier_update_device(h, objective, n, 0, steps, active.data(), 0, d_q.p, d_v.p, d_u.p, d_a.p, d_f.p, mu0, nullptr, d_scratch.p, d_inf.p, nullptr));
      must(idocp_rbd_synchronize(h));
      must(idocp_device_download(c.data(), d_cost.p, Nn * sizeof(double)));
      must(idocp_device_download(sq.data(), d_sq.p, Nn * sizeof(double)));
      must(idocp_device_download(inf.data(), d_inf.p, Nn * sizeof(double)));
      double sc = 0.0, ss = 0.0, worst = 0.0;
      int bad = 0;
      for (size_t i = 0; i < Nn; ++i) {
        if (!(std::isfinite(c[i]) && std::isfinite(sq[i]) && std::isfinite(inf[i])) || (failed_last && status[i] != -1)) { ++bad; continue; }
        sc += c[i]; ss += sq[i]; worst = std::fmax(worst, inf[i]);
      }
      const int good = n - bad;
      std::printf("  %s %s: mean cost = %.6e  mean sq_violation = %.6e  largest infeasibility = %.6e  (over %d plants, %d failed)\n", names[run], when,
                  good ? sc / good : 0.0, good ? ss / good : 0.0, worst, good, bad);
      return bad;
    };
    report("before");
    // `violation` of the iteration: sq_violation for the penalty run and for AL (lambda = 0: sq_shifted is sq_violation); unused by the cost run
    must(idocp_device_upload(d_viol.p, sq.data(), Nn * sizeof(double)));
    idocp_rbd_ilqr_io_t io = idocp_rbd_ilqr_io_t();
    io.q_traj = d_q.p; io.v_traj = d_v.p; io.u_traj = d_u.p; io.a_traj = d_a.p; io.f_traj = d_f.p; io.cost = d_cost.p; io.violation = d_viol.p;
    io.regularization = 1e-6; io.armijo = 1e-4; io.shrink = 0.5; io.alpha_min = 1e-3; io.penalty = 0.0; io.trials = 6;
    io.alpha_accepted = d_alpha.p; io.lqr_status = reinterpret_cast<int*>(d_status.p); io.expected = d_expected.p; io.workspace = d_work.p;
    double mu = mu0;
    for (int it = 0; it < iterations; ++it) {
      if (run == 0) must(idocp_rbd_ilqr_iterate_gn_device(h, objective, n, steps, active.data(), dt, dt, d_pts.p, &io, 0));
      else if (run == 1) { io.penalty = mu; must(idocp_rbd_ilqr_iterate_penalty_device(h, objective, n, steps, active.data(), dt, dt, d_pts.p, &io, 0)); mu *= factor; }
      else {
        io.penalty = mu0;
        must(idocp_rbd_ilqr_iterate_al_device(h, objective, n, steps, active.data(), dt, dt, d_pts.p, &io, d_lambda.p, 0));
        if (it % 2 == 1)
          must(idocp_rbd_ilqr_al_update_device(h, objective, n, steps, active.data(), d_q.p, d_v.p, d_u.p, d_a.p, d_f.p, mu0, mu0, d_lambda.p, d_viol.p, d_inf.p, d_change.p));
      }
      must(idocp_rbd_synchronize(h));
      must(idocp_device_download(alpha.data(), d_alpha.p, Nn * sizeof(double)));
      must(idocp_device_download(status.data(), d_status.p, (Nn + 1) / 2 * sizeof(double)));
      int accepted = 0, failed = 0;
      for (size_t i = 0; i < Nn; ++i) { if (alpha[i] > 0.0) ++accepted; if (status[i] != -1) ++failed; }
      failed_last = failed;
      std::printf("  %s iteration %d: accepted = %d  backward pass failed = %d%s\n", names[run], it, accepted, failed,
                  run == 2 && it % 2 == 1 ? "  (multipliers updated)" : "");
    }
    const int bad = report("after");
    if (bad < n) all_failed = 0;
  }
  idocp_rbd_objective_destroy(objective);
  idocp_rbd_destroy(h);
  return all_failed;
}
