// ANYmal standing under the ANYmal workload's own cost AND constraints: 256 plants started a little off the standing pose under zero torques are
// improved by idocp_rbd_ilqr_iterate_penalty_device -- the joint limits, a tight acceleration box and a friction cone with a SMALL coefficient enter
// as a squared-hinge penalty (idocp_hip.h has the definition) whose weight mu the caller raises by a factor per iteration -- and, from the same
// start, by idocp_rbd_ilqr_iterate_gn_device, which sees the cost alone.  Prints for both runs, before and after, the mean cost, the mean
// sq_violation and the mean of the score's own L1 violation, and per iteration the plants that accepted a step.  Nothing is hidden: a plant whose
// backward pass failed or whose scores are not finite is COUNTED and printed (and left out of the means, which says so).  Exit status 1 only
// when every plant failed.
//   usage: anymal_ilqr_constrained <anymal.urdf> [steps = 10] [iterations = 5] [perturbation = 0.02] [plants = 256] [mu = 10] [factor = 4]
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
    if (idocp_device_alloc(&v, doubles * sizeof(double)) != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); std::exit(1); }
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
  if (steps < 1 || iterations < 1 || n < 1) { std::fprintf(stderr, "steps, iterations and plants must be positive\n"); return 2; }
  const ex::Vec stand = ex::anymalStanding();

  // the cost of the ANYmal workloads: q 10, v (1 on the base, 0.1 on the joints), a (0.1, 0.01), f 0.001 about the weight share, u_weight = 0
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
  // the plants: stand (+) d, every tangent coordinate of d uniform in [-eps, eps] (a fixed sequence), at rest; the feet are held at the nominal footholds
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
  // the joint limits of the model, a friction cone with a small coefficient and a tight acceleration box
  idocp_constraints_t native_constraints = ex::jointLimits(robot, 0.05)->native();
  native_constraints.joint_acceleration_lower_limit = native_constraints.joint_acceleration_upper_limit = 1;
  for (int j = 0; j < nu; ++j) { native_constraints.a_min[j] = -2.0; native_constraints.a_max[j] = 2.0; }
  idocp_rbd_objective_t* objective = nullptr;
  must(idocp_rbd_objective_create(h, &native_cost, &native_constraints, 0.0, dt, steps, &objective));
  std::printf("%d plants, %d steps of %.3f s, %d iterations, perturbation %.3g, %d cost rows and %d constraint rows per stage, mu %.3g x %.3g per iteration\n",
              n, steps, dt, iterations, eps, idocp_rbd_objective_residual_rows(objective), idocp_rbd_objective_constraint_rows(objective), mu0, factor);

  int all_failed = 1;
  for (int run = 0; run < 2; ++run) {
    const bool penalty = run == 0;
    DeviceBuffer d_q(q_init.size(), q_init.data()), d_v(v_init.size(), v_init.data()), d_u(u_init.size(), u_init.data()), d_pts(pts.size(), pts.data());
    DeviceBuffer d_a(S * Nn * nv), d_f(S * Nn * 12), d_cost(Nn), d_viol(Nn), d_l1(Nn), d_sq(Nn), d_alpha(Nn), d_expected(2 * Nn), d_status((Nn + 1) / 2);
    const unsigned long long bytes = penalty ? idocp_rbd_ilqr_penalty_workspace_bytes(h, objective, n, steps) : idocp_rbd_ilqr_gn_workspace_bytes(h, n, steps);
    DeviceBuffer d_work((size_t)(bytes / sizeof(double)));
    must(idocp_rbd_rollout_device(h, n, steps, active.data(), dt, dt, d_u.p, d_pts.p, d_q.p, d_v.p, d_a.p, d_f.p, 0));
    idocp_rbd_score_io_t score = idocp_rbd_score_io_t();
    score.q_traj = d_q.p; score.v_traj = d_v.p; score.u_traj = d_u.p; score.a_traj = d_a.p; score.f_traj = d_f.p; score.cost = d_cost.p; score.violation = d_l1.p;
    std::vector<double> c(Nn), l1(Nn), sq(Nn), alpha(Nn);
    std::vector<int> status(Nn + 1, -1);
    // the three scores of what the run holds now; returns the number of plants with a non-finite score
    auto report = [&](const char* when) {
      must(idocp_rbd_score_rollout_device(h, objective, n, 0, steps, active.data(), 1, 0, &score));
      must(idocp_rbd_score_penalty_device(h, objective, n, 0, steps, active.data(), 0, d_q.p, d_v.p, d_u.p, d_a.p, d_f.p, d_sq.p));
      must(idocp_rbd_synchronize(h));
      must(idocp_device_download(c.data(), d_cost.p, Nn * sizeof(double)));
      must(idocp_device_download(l1.data(), d_l1.p, Nn * sizeof(double)));
      must(idocp_device_download(sq.data(), d_sq.p, Nn * sizeof(double)));
      double sc = 0.0, sl = 0.0, ss = 0.0;
      int bad = 0;
      for (size_t i = 0; i < Nn; ++i) {
        if (!(std::isfinite(c[i]) && std::isfinite(l1[i]) && std::isfinite(sq[i]))) { ++bad; continue; }
        sc += c[i]; sl += l1[i]; ss += sq[i];
      }
      const int good = n - bad;
      std::printf("  %s: mean cost = %.6e  mean sq_violation = %.6e  mean L1 violation = %.6e  (over %d plants, %d not finite)\n", when,
                  good ? sc / good : 0.0, good ? ss / good : 0.0, good ? sl / good : 0.0, good, bad);
      return bad;
    };
    std::printf("%s\n", penalty ? "idocp_rbd_ilqr_iterate_penalty_device:" : "idocp_rbd_ilqr_iterate_gn_device (the cost alone):");
    report("before");
    // `violation` of the iteration: sq_violation for the penalty run, the L1 violation (with penalty = 0: unused) for the other
    must(idocp_device_upload(d_viol.p, penalty ? sq.data() : l1.data(), Nn * sizeof(double)));
    idocp_rbd_ilqr_io_t io = idocp_rbd_ilqr_io_t();
    io.q_traj = d_q.p; io.v_traj = d_v.p; io.u_traj = d_u.p; io.a_traj = d_a.p; io.f_traj = d_f.p; io.cost = d_cost.p; io.violation = d_viol.p;
    io.regularization = 1e-6; io.armijo = 1e-4; io.shrink = 0.5; io.alpha_min = 1e-3; io.penalty = 0.0; io.trials = 6;
    io.alpha_accepted = d_alpha.p; io.lqr_status = reinterpret_cast<int*>(d_status.p); io.expected = d_expected.p; io.workspace = d_work.p;
    double mu = mu0;
    int failed_last = 0;
    for (int it = 0; it < iterations; ++it, mu *= factor) {
      if (penalty) {
        io.penalty = mu;
        must(idocp_rbd_ilqr_iterate_penalty_device(h, objective, n, steps, active.data(), dt, dt, d_pts.p, &io, 0));
      } else {
        must(idocp_rbd_ilqr_iterate_gn_device(h, objective, n, steps, active.data(), dt, dt, d_pts.p, &io, 0));
      }
      must(idocp_rbd_synchronize(h));
      must(idocp_device_download(alpha.data(), d_alpha.p, Nn * sizeof(double)));
      must(idocp_device_download(status.data(), d_status.p, (Nn + 1) / 2 * sizeof(double)));
      int accepted = 0, failed = 0;
      for (size_t i = 0; i < Nn; ++i) { if (alpha[i] > 0.0) ++accepted; if (status[i] != -1) ++failed; }
      failed_last = failed;
      if (penalty) std::printf("  iteration %d (mu %.3g): accepted = %d  backward pass failed = %d\n", it, mu, accepted, failed);
      else std::printf("  iteration %d: accepted = %d  backward pass failed = %d\n", it, accepted, failed);
    }
    const int bad = report("after");
    if (bad < n && failed_last < n) all_failed = 0;
  }
  idocp_rbd_objective_destroy(objective);
  idocp_rbd_destroy(h);
  return all_failed;
}
