// Robot::RNEA, RNEADerivatives, computeBaumgarteResidual / Derivatives of the facade on ANYmal with two active contacts: prints the inputs and
// the results as hexadecimal floats (exact), one named line each, for tests/test_rbd_batch_gpu.py to compare with the C ABI call.
//   usage: robot_dynamics <anymal.urdf>
#include <cmath>
#include <cstdio>
#include <vector>

#include "idocp/robot/robot.hpp"

static void line(const char* name, const double* x, int n) {
  std::printf("%s:", name);
  for (int i = 0; i < n; ++i) std::printf(" %a", x[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: robot_dynamics <anymal.urdf>\n"); return 2; }
  idocp::Robot robot(argv[1], {14, 24, 34, 44});
  const int nq = robot.dimq(), nv = robot.dimv();
  Eigen::VectorXd q(nq), v(nv), a(nv), tau(nv);
  const double quat[4] = {0.05, -0.1, 0.2, 0.97};
  double norm = 0.0;
  for (double x : quat) norm += x * x;
  norm = std::sqrt(norm);
  q[0] = 0.1; q[1] = -0.2; q[2] = 0.48;
  for (int k = 0; k < 4; ++k) q[3 + k] = quat[k] / norm;
  for (int k = 7; k < nq; ++k) q[k] = 0.3 * std::sin(1.0 + k);
  for (int k = 0; k < nv; ++k) { v[k] = 0.5 * std::cos(0.7 * k); a[k] = 1.5 * std::sin(0.3 * k + 0.2); }
  idocp::ContactStatus status = robot.createContactStatus();
  status.activateContacts({1, 2});
  std::vector<Eigen::Vector3d> f, points;
  for (int c = 0; c < 4; ++c) {
    f.push_back(Eigen::Vector3d(3.0 + c, -2.0 * c, 40.0 + 5.0 * c));
    points.push_back(Eigen::Vector3d(0.3 - 0.2 * c, 0.1 * c, 0.01 * c));
  }
  const double time_step = 0.025;
  const int dimf = status.dimf();

  robot.setContactForces(status, f);
  robot.RNEA(q, v, a, tau);
  Eigen::MatrixXd dq(nv, nv), dv(nv, nv), da(nv, nv);
  robot.RNEADerivatives(q, v, a, dq, dv, da);
  robot.updateKinematics(q, v, a);
  const idocp::Robot copy(robot);                      // (a copy creates its own handle)
  Eigen::VectorXd C(dimf);
  copy.computeBaumgarteResidual(status, time_step, points, C);
  Eigen::MatrixXd Cq(dimf, nv), Cv(dimf, nv), Ca(dimf, nv);
  robot.computeBaumgarteDerivatives(status, time_step, Cq, Cv, Ca);

  double act[4], fl[12], pl[12];
  for (int c = 0; c < 4; ++c) {
    act[c] = status.isContactActive(c) ? 1.0 : 0.0;
    for (int k = 0; k < 3; ++k) { fl[3 * c + k] = f[c][k]; pl[3 * c + k] = points[c][k]; }
  }
  line("q", q.data(), nq); line("v", v.data(), nv); line("a", a.data(), nv);
  line("f", fl, 12); line("points", pl, 12); line("active", act, 4); line("time_step", &time_step, 1);
  line("tau", tau.data(), nv);
  line("dtau_dq", dq.data(), nv * nv); line("dtau_dv", dv.data(), nv * nv); line("dtau_da", da.data(), nv * nv);
  line("C", C.data(), dimf);
  line("dCdq", Cq.data(), dimf * nv); line("dCdv", Cv.data(), dimf * nv); line("dCda", Ca.data(), dimf * nv);
  return 0;
}
