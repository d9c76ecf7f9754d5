// ANYmal standing: the policy of idocp::OCPSolver rolled out closed loop on a few perturbed plants (as anymal_closed_loop_rollout.cpp does on
// many), then LINEARISED along what was stored: idocp_rbd_linearize_rollout gives A_k, B_k of every step about the torques that were applied.
// Prints, over the plants,
//   the largest |prod_k A_k|_inf (open loop: the torques held) and |prod_k (A_k + B_k K_k)|_inf (closed loop: the solver's gains; K_k acts on
//   q (-) q_ref, whose tangent is taken as dq itself -- exact to first order in the distance from the reference),
//   and the gap between a re-rollout from x_0 (+) (+-eps) d under the SAME torques (idocp_rbd_rollout) and the linear prediction
//   (+-eps) prod_k A_k d, for eps and eps / 10: the gap is of second order, so it falls by about 100.
//   usage: anymal_rollout_linearisation <anymal.urdf> [steps = 10] [perturbation = 0.02] [eps = 1e-3]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "common.hpp"
#include "idocp/cost/configuration_space_cost.hpp"
#include "idocp/ocp/ocp_solver.hpp"

namespace {

typedef std::vector<double> Mat;      // column-major, nx x nx unless said otherwise

// C (rows x cols) = A (rows x inner) B (inner x cols)
Mat mul(const Mat& A, const Mat& B, int rows, int inner, int cols) {
  Mat C((size_t)rows * cols, 0.0);
  for (int c = 0; c < cols; ++c) for (int k = 0; k < inner; ++k) { const double b = B[(size_t)c * inner + k]; for (int r = 0; r < rows; ++r) C[(size_t)c * rows + r] += A[(size_t)k * rows + r] * b; }
  return C;
}

double normInf(const Mat& A, int rows, int cols) {
  double worst = 0.0;
  for (int r = 0; r < rows; ++r) { double s = 0.0; for (int c = 0; c < cols; ++c) s += std::fabs(A[(size_t)c * rows + r]); worst = (s > worst || !std::isfinite(s)) ? s : worst; }
  return worst;
}

}  // namespace

int main(int argc, char** argv) {
  idocp::Robot robot(ex::needUrdf(argc, argv, "[steps] [perturbation] [eps]"), ex::anymalFeet());
  const double T = 0.5, dt = 0.025;      // the plant steps with the solver's own stage length, which is also its Baumgarte time step
  const int N = 20, n = 4;
  const int steps = ex::argInt(argc, argv, 2, 10);
  const double spread = argc > 3 ? std::atof(argv[3]) : 0.02, eps0 = argc > 4 ? std::atof(argv[4]) : 1e-3;
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

  // ---- 1. the standing policy rolled out on a few perturbed plants ----
  const int nq = robot.dimq(), nv = robot.dimv(), nu = robot.dimu(), nx = 2 * nv;
  std::vector<double> u_ff((size_t)steps * n * nu), K((size_t)steps * nu * nx), q_ref((size_t)steps * nq), v_ref((size_t)steps * nv);
  Eigen::MatrixXd Kq, Kv;
  for (int k = 0; k < steps; ++k) {
    const idocp::SplitSolution& s = solver.getSolution(k);
    solver.getStateFeedbackGain(k, Kq, Kv);
    for (int i = 0; i < n; ++i) for (int j = 0; j < nu; ++j) u_ff[((size_t)k * n + i) * nu + j] = s.u[j];
    for (int c = 0; c < nv; ++c) for (int r = 0; r < nu; ++r) {
      K[(size_t)k * nu * nx + (size_t)c * nu + r] = Kq(r, c);
      K[(size_t)k * nu * nx + (size_t)(nv + c) * nu + r] = Kv(r, c);
    }
    for (int j = 0; j < nq; ++j) q_ref[(size_t)k * nq + j] = s.q[j];
    for (int j = 0; j < nv; ++j) v_ref[(size_t)k * nv + j] = s.v[j];
  }
  unsigned long long seed = 88172645463325252ull;
  auto uniform = [&seed]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (double)(seed >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
  std::vector<double> q_traj((size_t)(steps + 1) * n * nq), v_traj((size_t)(steps + 1) * n * nv, 0.0), u_traj((size_t)steps * n * nu);
  ex::Vec d(nv), qi(nq);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < nv; ++j) d[j] = spread * uniform();
    robot.integrateConfiguration(stand, d, 1.0, qi);
    for (int j = 0; j < nq; ++j) q_traj[(size_t)i * nq + j] = qi[j];
  }
  robot.updateFrameKinematics(stand);
  std::vector<ex::V3> feet;
  robot.getContactPoints(feet);
  auto pointsFor = [&](int samples) {
    std::vector<double> pts((size_t)steps * samples * 12);
    for (size_t e = 0; e < (size_t)steps * samples; ++e) for (int c = 0; c < 4; ++c) for (int k = 0; k < 3; ++k) pts[e * 12 + 3 * c + k] = feet[c][k];
    return pts;
  };
  const std::vector<double> pts = pointsFor(n);
  std::vector<int> active((size_t)steps * 4, 1);
  idocp_rbd_t* h = nullptr;
  auto ok = [](int rc) { if (rc != IDOCP_OK) { std::fprintf(stderr, "%s\n", idocp_last_error()); std::exit(1); } };
  ok(idocp_rbd_create(&robot.model(), 0, &h));
  idocp_rbd_policy_t pol = idocp_rbd_policy_t();
  pol.u_ff = u_ff.data(); pol.K = K.data(); pol.q_ref = q_ref.data(); pol.v_ref = v_ref.data();
  pol.shared_gains = 1; pol.shared_ref = 1;
  ok(idocp_rbd_rollout_policy(h, n, steps, active.data(), dt, dt, &pol, pts.data(), q_traj.data(), v_traj.data(), u_traj.data(), nullptr, nullptr, 0));

  // ---- 2. linearise what was stored, about the torques that were applied ----
  std::vector<double> A((size_t)steps * n * nx * nx), B((size_t)steps * n * nx * nu);
  ok(idocp_rbd_linearize_rollout(h, n, steps, active.data(), dt, dt, u_traj.data(), pts.data(), q_traj.data(), v_traj.data(), A.data(), B.data(), 0));

  // ---- 3. the products: open loop and closed loop ----
  std::vector<Mat> open(n);
  double norm_open = 0.0, norm_closed = 0.0;
  for (int i = 0; i < n; ++i) {
    Mat Po((size_t)nx * nx, 0.0), Pc;
    for (int r = 0; r < nx; ++r) Po[(size_t)r * nx + r] = 1.0;
    Pc = Po;
    for (int k = 0; k < steps; ++k) {
      const Mat Ak(A.begin() + ((size_t)k * n + i) * nx * nx, A.begin() + ((size_t)k * n + i + 1) * nx * nx);
      const Mat Bk(B.begin() + ((size_t)k * n + i) * nx * nu, B.begin() + ((size_t)k * n + i + 1) * nx * nu);
      const Mat Kk(K.begin() + (size_t)k * nu * nx, K.begin() + (size_t)(k + 1) * nu * nx);
      Mat Ac = mul(Bk, Kk, nx, nu, nx);
      for (size_t e = 0; e < Ac.size(); ++e) Ac[e] += Ak[e];
      Po = mul(Ak, Po, nx, nx, nx);
      Pc = mul(Ac, Pc, nx, nx, nx);
    }
    norm_open = std::fmax(norm_open, normInf(Po, nx, nx));
    norm_closed = std::fmax(norm_closed, normInf(Pc, nx, nx));
    if (!std::isfinite(normInf(Po, nx, nx)) || !std::isfinite(normInf(Pc, nx, nx))) norm_open = norm_closed = NAN;
    open[i] = Po;
  }

  // ---- 4. the re-rollout from x_0 (+) (+-eps) d under the same torques against the linear prediction ----
  Mat dir(nx);
  double len = 0.0;
  for (int j = 0; j < nx; ++j) { dir[j] = uniform(); len += dir[j] * dir[j]; }
  for (int j = 0; j < nx; ++j) dir[j] /= std::sqrt(len);
  double gap[2] = {0.0, 0.0};
  const double epss[2] = {eps0, eps0 / 10};
  const int m = 2 * n;                      // per eps: every plant with + and with -
  const std::vector<double> pts2 = pointsFor(m);
  for (int e = 0; e < 2; ++e) {
    std::vector<double> qt((size_t)(steps + 1) * m * nq), vt((size_t)(steps + 1) * m * nv), ut((size_t)steps * m * nu);
    for (int i = 0; i < n; ++i) for (int sg = 0; sg < 2; ++sg) {
      const double s = sg ? -epss[e] : epss[e];
      const int at = 2 * i + sg;
      ex::Vec q(nq), dq(nv), qp(nq);
      for (int j = 0; j < nq; ++j) q[j] = q_traj[(size_t)i * nq + j];
      for (int j = 0; j < nv; ++j) dq[j] = dir[j];
      robot.integrateConfiguration(q, dq, s, qp);
      for (int j = 0; j < nq; ++j) qt[(size_t)at * nq + j] = qp[j];
      for (int j = 0; j < nv; ++j) vt[(size_t)at * nv + j] = v_traj[(size_t)i * nv + j] + s * dir[nv + j];
      for (int k = 0; k < steps; ++k) for (int j = 0; j < nu; ++j) ut[((size_t)k * m + at) * nu + j] = u_traj[((size_t)k * n + i) * nu + j];
    }
    ok(idocp_rbd_rollout(h, m, steps, active.data(), dt, dt, ut.data(), pts2.data(), qt.data(), vt.data(), nullptr, nullptr, 0));
    for (int i = 0; i < n; ++i) {
      const Mat lin = mul(open[i], dir, nx, nx, 1);
      ex::Vec qn(nq), qs(nq), diff(nv);
      for (int j = 0; j < nq; ++j) qn[j] = q_traj[((size_t)steps * n + i) * nq + j];
      for (int sg = 0; sg < 2; ++sg) {
        const double s = sg ? -epss[e] : epss[e];
        const int at = 2 * i + sg;
        for (int j = 0; j < nq; ++j) qs[j] = qt[((size_t)steps * m + at) * nq + j];
        robot.subtractConfiguration(qs, qn, diff);
        for (int j = 0; j < nv; ++j) {
          const double gq = diff[j] - s * lin[j];
          const double gv = vt[((size_t)steps * m + at) * nv + j] - v_traj[((size_t)steps * n + i) * nv + j] - s * lin[nv + j];
          const double g = std::fmax(std::fabs(gq), std::fabs(gv));
          gap[e] = (g > gap[e] || !std::isfinite(g)) ? g : gap[e];
        }
      }
    }
  }
  idocp_rbd_destroy(h);
  std::printf("%d plants, %d steps of %.3f s, perturbation %.3g\n", n, steps, dt, spread);
  std::printf("open loop:   max |prod A|_inf = %.6e\n", norm_open);
  std::printf("closed loop: max |prod (A + B K)|_inf = %.6e\n", norm_closed);
  std::printf("gap of the linear prediction at eps = %.3e: %.6e\n", epss[0], gap[0]);
  std::printf("gap of the linear prediction at eps = %.3e: %.6e\n", epss[1], gap[1]);
  std::printf("gap ratio = %.3f\n", gap[0] / gap[1]);
  return (std::isfinite(norm_open) && std::isfinite(norm_closed) && std::isfinite(gap[0]) && std::isfinite(gap[1])) ? 0 : 1;
}
