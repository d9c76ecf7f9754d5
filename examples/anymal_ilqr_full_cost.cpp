// ANYmal standing under the ANYmal workload's OWN cost: 256 plants, each started a little off the standing pose and under zero torques (they sag),
// are improved by iLQR on the cost the solvers use -- pose and velocity weights, an ACCELERATION weight, a contact-FORCE weight about every foot's
// share of the weight, and NO torque weight, so that Quu is positive definite through the acceleration rows alone.  One iteration is
// idocp_rbd_ilqr_iterate_gn_device:
//   idocp_rbd_linearize_rollout_cost_device   A_k, B_k, the residual rows G_k of the acceleration and force terms, the full gradients lx, lu
//   idocp_rbd_lqr_backward_gn_device          gains K_k and the feed-forward step k_k with G_k^T G_k in the stage Hessian
//   trials x (u + alpha k, idocp_rbd_rollout_policy_device, idocp_rbd_score_rollout_device, accept)
// on the handle's stream with no synchronisation in between (anymal_ilqr.cpp is the same loop on a cost without these terms, which is all
// idocp_rbd_ilqr_iterate_device takes).  Prints the mean cost before, per iteration the mean cost, the plants that accepted a step and the largest
// |e0|, and the mean cost after.  Exit status 1 only for non-finite output.
//   usage: anymal_ilqr_full_cost <anymal.urdf> [steps = 10] [iterations = 5] [perturbation = 0.02] [plants = 256]
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
  idocp::Robot robot(ex::needUrdf(argc, argv, "[steps] [iterations] [perturbation] [plants]"), ex::anymalFeet());
  const double dt = 0.025;      // the stage length, which is also the Baumgarte time step
  const int steps = ex::argInt(argc, argv, 2, 10), iterations = ex::argInt(argc, argv, 3, 5);
  const double eps = argc > 4 ? std::atof(argv[4]) : 0.02;
  const int n = ex::argInt(argc, argv, 5, 256);
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
  idocp_rbd_objective_t* objective = nullptr;
  must(idocp_rbd_objective_create(h, &native_cost, nullptr, 0.0, dt, steps, &objective));

  DeviceBuffer d_q(q_init.size(), q_init.data()), d_v(v_init.size(), v_init.data()), d_u(u_init.size(), u_init.data()), d_pts(pts.size(), pts.data());
  DeviceBuffer d_a(S * Nn * nv), d_f(S * Nn * 12), d_cost(Nn), d_viol(Nn), d_alpha(Nn), d_expected(2 * Nn), d_status((Nn + 1) / 2);
  DeviceBuffer d_work((size_t)(idocp_rbd_ilqr_gn_workspace_bytes(h, n, steps) / sizeof(double)));

  // the first rollout and its score, once
  must(idocp_rbd_rollout_device(h, n, steps, active.data(), dt, dt, d_u.p, d_pts.p, d_q.p, d_v.p, d_a.p, d_f.p, 0));
  idocp_rbd_score_io_t score = idocp_rbd_score_io_t();
  score.q_traj = d_q.p; score.v_traj = d_v.p; score.u_traj = d_u.p; score.a_traj = d_a.p; score.f_traj = d_f.p; score.cost = d_cost.p; score.violation = d_viol.p;
  must(idocp_rbd_score_rollout_device(h, objective, n, 0, steps, active.data(), 1, 0, &score));

  idocp_rbd_ilqr_io_t io = idocp_rbd_ilqr_io_t();
  io.q_traj = d_q.p; io.v_traj = d_v.p; io.u_traj = d_u.p; io.a_traj = d_a.p; io.f_traj = d_f.p; io.cost = d_cost.p; io.violation = d_viol.p;
  io.regularization = 1e-6; io.armijo = 1e-4; io.shrink = 0.5; io.alpha_min = 1e-3; io.penalty = 0.0; io.trials = 6;
  io.alpha_accepted = d_alpha.p; io.lqr_status = reinterpret_cast<int*>(d_status.p); io.expected = d_expected.p; io.workspace = d_work.p;

  std::printf("%d plants, %d steps of %.3f s, %d iterations, perturbation %.3g, %d residual rows per stage\n", n, steps, dt, iterations, eps,
              idocp_rbd_objective_residual_rows(objective));
  std::vector<double> c(Nn), alpha(Nn), expected(2 * Nn);
  auto meanCost = [&]() { must(idocp_device_download(c.data(), d_cost.p, Nn * sizeof(double))); double s = 0.0; for (double x : c) s += x; return s / n; };
  must(idocp_rbd_synchronize(h));
  double mean = meanCost();
  bool finite = std::isfinite(mean);
  std::printf("mean cost before = %.6e\n", mean);
  for (int it = 0; it < iterations; ++it) {
    must(idocp_rbd_ilqr_iterate_gn_device(h, objective, n, steps, active.data(), dt, dt, d_pts.p, &io, 0));
    must(idocp_rbd_synchronize(h));
    mean = meanCost();
    must(idocp_device_download(alpha.data(), d_alpha.p, Nn * sizeof(double)));
    must(idocp_device_download(expected.data(), d_expected.p, 2 * Nn * sizeof(double)));
    int accepted = 0;
    double e0 = 0.0;
    for (size_t i = 0; i < Nn; ++i) {
      if (alpha[i] > 0.0) ++accepted;
      if (std::isfinite(expected[2 * i]) && std::fabs(expected[2 * i]) > e0) e0 = std::fabs(expected[2 * i]);
    }
    finite = finite && std::isfinite(mean);
    std::printf("iteration %d: mean cost = %.6e  accepted = %d  max |e0| = %.6e\n", it, mean, accepted, e0);
  }
  std::printf("mean cost after = %.6e\n", mean);
  idocp_rbd_objective_destroy(objective);
  idocp_rbd_destroy(h);
  return finite ? 0 : 1;
}
