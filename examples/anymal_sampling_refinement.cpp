// ANYmal standing: a torque sequence repaired by sampling, every stage on the GPU.  The nominal sequence starts from the converged solution of
// idocp::OCPSolver PLUS a fixed offset on every joint, so there is something to repair.  One iteration is the MPPI update -- the softmin-weighted
// mean of sampled torque sequences --
//   idocp_rbd_perturb_torques_device     n sequences around the nominal (sample 0 is the nominal itself)
//   idocp_rbd_rollout_policy_device      every sequence on the plant (no gains: u_ff = the samples)
//   idocp_rbd_score_rollout_device       the solver's own cost and constraint violation per sequence
//   idocp_rbd_importance_weights_device  exp(-(s - s_min) / temperature)
//   idocp_rbd_weighted_mean_device       of the torques applied, straight into the nominal
// on the handle's stream with no synchronisation in between; per iteration only the five statistics and cost[0], the nominal's own cost, come back
// to the host.  Prints them per iteration, and the nominal's cost after the last update.  Exit status 1 only for non-finite output.
//   usage: anymal_sampling_refinement <anymal.urdf> [steps = 10] [iterations = 6] [sigma = 1.0] [temperature = 2.0] [offset = 2.0] [plants = 256]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "common.hpp"
#include "idocp/cost/configuration_space_cost.hpp"
#include "idocp/ocp/ocp_solver.hpp"

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
  idocp::Robot robot(ex::needUrdf(argc, argv, "[steps] [iterations] [sigma] [temperature] [offset] [plants]"), ex::anymalFeet());
  const double T = 0.5, dt = 0.025;      // the plant steps with the solver's own stage length, which is also its Baumgarte time step
  const int N = 20;
  const int steps = ex::argInt(argc, argv, 2, 10), iterations = ex::argInt(argc, argv, 3, 6);
  const double sigma = argc > 4 ? std::atof(argv[4]) : 1.0, temperature = argc > 5 ? std::atof(argv[5]) : 2.0, offset = argc > 6 ? std::atof(argv[6]) : 2.0;
  const int n = ex::argInt(argc, argv, 7, 256);
  const double penalty = 10.0;           // of the constraint violation in a sample's score
  if (steps < 1 || steps >= N || iterations < 1 || n < 1) { std::fprintf(stderr, "steps must be in [1, %d), iterations and plants positive\n", N); return 2; }
  const ex::Vec stand = ex::anymalStanding();

  auto pose_cost = std::make_shared<idocp::ConfigurationSpaceCost>(robot);
  pose_cost->set_q_ref(stand);
  ex::attachWeights(*pose_cost, ex::filled(18, 10), ex::filled(18, 1), ex::filled(18, 0.01), false);
  const ex::V3 share(0, 0, 70);
  auto cost = std::make_shared<idocp::CostFunction>();
  cost->push_back(pose_cost);
  cost->push_back(ex::forceCost(robot, ex::V3(0.001, 0.001, 0.001), false, &share));
  auto constraints = ex::jointLimits(robot, 0.7, false, true);
  idocp::OCPSolver solver(robot, cost, constraints, T, N, 4, 4);
  ex::Schedule standing(ex::footholds(robot, stand));
  standing.add({0, 1, 2, 3}, 0.0);
  standing.install(solver, robot);
  ex::restingGuess(solver, robot, stand);
  solver.initConstraints(0.0);
  const ex::Vec v0 = ex::Vec::Zero(robot.dimv());
  for (int it = 0; it < 20; ++it) solver.updateSolution(0.0, stand, v0);      // to convergence at the nominal state

  // the nominal torque sequence [steps][nu]: the solver's, pushed off by `offset` N m on every joint
  const int nq = robot.dimq(), nv = robot.dimv(), nu = robot.dimu();
  std::vector<double> nominal((size_t)steps * nu), sig(nu, sigma);
  for (int k = 0; k < steps; ++k) for (int j = 0; j < nu; ++j) nominal[(size_t)k * nu + j] = solver.getSolution(k).u[j] + offset;

  // every plant starts standing at rest; the feet are held at the nominal footholds
  const size_t S = (size_t)steps, Nn = (size_t)n;
  std::vector<double> q_init((S + 1) * Nn * nq, 0.0), pts(S * Nn * 12);
  const std::vector<double> v_init((S + 1) * Nn * nv, 0.0);
  std::vector<int> active(S * 4, 1);
  for (size_t i = 0; i < Nn; ++i) for (int j = 0; j < nq; ++j) q_init[i * nq + j] = stand[j];
  robot.updateFrameKinematics(stand);
  std::vector<ex::V3> feet;
  robot.getContactPoints(feet);
  for (size_t e = 0; e < S * Nn; ++e) for (int c = 0; c < 4; ++c) for (int k = 0; k < 3; ++k) pts[e * 12 + 3 * c + k] = feet[c][k];

  idocp_rbd_t* h = nullptr;
  must(idocp_rbd_create(&robot.model(), 0, &h));
  const idocp_cost_t native_cost = cost->native();
  const idocp_constraints_t native_constraints = constraints->native();
  idocp_rbd_objective_t* objective = nullptr;
  must(idocp_rbd_objective_create(h, &native_cost, &native_constraints, 0.0, dt, steps, &objective));

  DeviceBuffer d_nominal(nominal.size(), nominal.data()), d_sigma(sig.size(), sig.data()), d_pts(pts.size(), pts.data());
  DeviceBuffer d_samples(S * Nn * nu), d_q(q_init.size(), q_init.data()), d_v(v_init.size(), v_init.data());
  DeviceBuffer d_u(S * Nn * nu), d_a(S * Nn * nv), d_f(S * Nn * 12), d_cost(Nn), d_viol(Nn), d_w(Nn), d_stats(IDOCP_RBD_WEIGHT_STATS);
  idocp_rbd_policy_t pol = idocp_rbd_policy_t();
  pol.u_ff = d_samples.p;
  idocp_rbd_score_io_t io = idocp_rbd_score_io_t();
  io.q_traj = d_q.p; io.v_traj = d_v.p; io.u_traj = d_u.p; io.a_traj = d_a.p; io.f_traj = d_f.p;
  io.cost = d_cost.p; io.violation = d_viol.p;
  std::printf("%d plants, %d steps of %.3f s, %d iterations, sigma %.3g, temperature %.3g, offset %.3g\n", n, steps, dt, iterations, sigma, temperature, offset);
  const unsigned long long seed = 88172645463325252ull;
  bool finite = true;
  // slice 0 of q and v stays what it is: every rollout starts from it and writes slices 1 .. steps
  for (int it = 0; it <= iterations; ++it) {
    must(idocp_rbd_perturb_torques_device(h, n, 0, steps, d_nominal.p, d_sigma.p, nullptr, nullptr, seed, (unsigned)it, d_samples.p));
    must(idocp_rbd_rollout_policy_device(h, n, steps, active.data(), dt, dt, &pol, d_pts.p, d_q.p, d_v.p, d_u.p, d_a.p, d_f.p, 0));
    must(idocp_rbd_score_rollout_device(h, objective, n, 0, steps, active.data(), 1, 0, &io));
    if (it < iterations) {
      must(idocp_rbd_importance_weights_device(h, n, d_cost.p, d_viol.p, penalty, temperature, d_w.p, d_stats.p));
      must(idocp_rbd_weighted_mean_device(h, n, steps, nu, d_w.p, d_u.p, d_nominal.p));
    }
    must(idocp_rbd_synchronize(h));
    double nominal_cost = 0.0, stats[IDOCP_RBD_WEIGHT_STATS] = {0, 0, 0, 0, 0};
    must(idocp_device_download(&nominal_cost, d_cost.p, sizeof(double)));
    finite = finite && std::isfinite(nominal_cost);
    if (it == iterations) {
      std::printf("final: nominal cost = %.6e\n", nominal_cost);
      break;
    }
    must(idocp_device_download(stats, d_stats.p, sizeof(stats)));
    for (double x : stats) finite = finite && std::isfinite(x);
    std::printf("iteration %d: nominal cost = %.6e  s_min = %.6e  effective samples = %.2f  finite = %d\n", it, nominal_cost, stats[1], stats[4], (int)stats[0]);
  }
  idocp_rbd_objective_destroy(objective);
  idocp_rbd_destroy(h);
  return finite ? 0 : 1;
}
