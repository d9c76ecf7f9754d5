// ANYmal standing: the converged policy of idocp::OCPSolver on 256 perturbed plants, with and without its Riccati gains, and each plant's
// trajectory SCORED on the GPU under the very cost and constraints the solver was given -- idocp_rbd_rollout_policy_device followed by
// idocp_rbd_score_rollout_device on the device arrays the rollout wrote, with no download of a trajectory.  The references of the policy are the
// objective's own tables (idocp_rbd_objective_reference_device: the standing reference of the cost at every step).  Prints mean and worst cost
// and violation per variant; only the 2 x 256 scores come back to the host.
//   usage: anymal_rollout_scoring <anymal.urdf> [steps = 10] [perturbation = 0.02]
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
  auto constraints = ex::jointLimits(robot, 0.7, false, true);
  idocp::OCPSolver solver(robot, cost, constraints, T, N, 4, 4);
  ex::Schedule standing(ex::footholds(robot, stand));
  standing.add({0, 1, 2, 3}, 0.0);
  standing.install(solver, robot);
  ex::restingGuess(solver, robot, stand);
  solver.initConstraints(0.0);
  const ex::Vec v0 = ex::Vec::Zero(robot.dimv());
  for (int it = 0; it < 20; ++it) solver.updateSolution(0.0, stand, v0);      // to convergence at the nominal state

  // the policy of the first stages, shared by every plant: u_ff [steps][n][nu], K [steps][nu * 2 nv] = [Kq | Kv]
  const int nq = robot.dimq(), nv = robot.dimv(), nu = robot.dimu();
  std::vector<double> u_ff((size_t)steps * n * nu), K((size_t)steps * nu * 2 * nv);
  Eigen::MatrixXd Kq, Kv;
  for (int k = 0; k < steps; ++k) {
    const idocp::SplitSolution& s = solver.getSolution(k);
    solver.getStateFeedbackGain(k, Kq, Kv);
    for (int i = 0; i < n; ++i) for (int j = 0; j < nu; ++j) u_ff[((size_t)k * n + i) * nu + j] = s.u[j];
    for (int c = 0; c < nv; ++c) for (int r = 0; r < nu; ++r) {
      K[(size_t)k * nu * 2 * nv + (size_t)c * nu + r] = Kq(r, c);
      K[(size_t)k * nu * 2 * nv + (size_t)(nv + c) * nu + r] = Kv(r, c);
    }
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
  must(idocp_rbd_create(&robot.model(), 0, &h));
  // the objective: the solver's own cost and constraints on the grid of the rollout
  const idocp_cost_t native_cost = cost->native();
  const idocp_constraints_t native_constraints = constraints->native();
  idocp_rbd_objective_t* objective = nullptr;
  must(idocp_rbd_objective_create(h, &native_cost, &native_constraints, 0.0, dt, steps, &objective));
  const double *d_q_ref = nullptr, *d_v_ref = nullptr;
  must(idocp_rbd_objective_reference_device(objective, &d_q_ref, &d_v_ref));

  const size_t S = (size_t)steps, Nn = (size_t)n;
  std::vector<double> q_init((S + 1) * Nn * nq, 0.0);
  for (size_t e = 0; e < q0.size(); ++e) q_init[e] = q0[e];
  const std::vector<double> v_init((S + 1) * Nn * nv, 0.0);
  DeviceBuffer d_u_ff(u_ff.size(), u_ff.data()), d_K(K.size(), K.data()), d_pts(pts.size(), pts.data());
  DeviceBuffer d_q(q_init.size()), d_v(v_init.size()), d_u(S * Nn * nu), d_a(S * Nn * nv), d_f(S * Nn * 12), d_cost(Nn), d_viol(Nn);
  idocp_rbd_policy_t pol = idocp_rbd_policy_t();
  pol.u_ff = d_u_ff.p; pol.q_ref = d_q_ref; pol.v_ref = d_v_ref;
  pol.shared_gains = 1; pol.shared_ref = 1;
  idocp_rbd_score_io_t io = idocp_rbd_score_io_t();
  io.q_traj = d_q.p; io.v_traj = d_v.p; io.u_traj = d_u.p; io.a_traj = d_a.p; io.f_traj = d_f.p;
  io.cost = d_cost.p; io.violation = d_viol.p;
  std::printf("%d plants, %d steps of %.3f s, perturbation %.3g\n", n, steps, dt, eps);
  const char* names[2] = {"with gains:   ", "without gains:"};
  double mean_cost[2];
  bool finite = true;
  for (int run = 0; run < 2; ++run) {
    pol.K = run == 0 ? d_K.p : nullptr;
    must(idocp_device_upload(d_q.p, q_init.data(), q_init.size() * sizeof(double)));
    must(idocp_device_upload(d_v.p, v_init.data(), v_init.size() * sizeof(double)));
    must(idocp_rbd_rollout_policy_device(h, n, steps, active.data(), dt, dt, &pol, d_pts.p, d_q.p, d_v.p, d_u.p, d_a.p, d_f.p, 0));
    must(idocp_rbd_score_rollout_device(h, objective, n, 0, steps, active.data(), 1, 0, &io));
    must(idocp_rbd_synchronize(h));
    std::vector<double> c(n), g(n);
    must(idocp_device_download(c.data(), d_cost.p, Nn * sizeof(double)));
    must(idocp_device_download(g.data(), d_viol.p, Nn * sizeof(double)));
    double sc = 0, sg = 0, wc = 0, wg = 0;
    for (int i = 0; i < n; ++i) {
      sc += c[i]; sg += g[i]; wc = std::fmax(wc, c[i]); wg = std::fmax(wg, g[i]);
      finite = finite && std::isfinite(c[i]) && std::isfinite(g[i]);
    }
    mean_cost[run] = sc / n;
    std::printf("%s cost mean = %.6e worst = %.6e   violation mean = %.6e worst = %.6e\n", names[run], sc / n, wc, sg / n, wg);
  }
  std::printf("ratio of the mean costs, with / without gains = %.4f\n", mean_cost[0] / mean_cost[1]);
  idocp_rbd_objective_destroy(objective);
  idocp_rbd_destroy(h);
  return finite ? 0 : 1;
}
