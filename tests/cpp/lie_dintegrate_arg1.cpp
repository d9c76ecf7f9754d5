// lieDIntegrateArg1 (idocp_amd/csrc/dev_lie.hpp), the right Jacobian of exp6, held on the CPU on both sides of its 0.05 rad switch between the
// series and the closed form, at zero and at large angles, to a form that shares nothing with it: the inverse of Jlog6 at exp6(v)
// (lieJlog6, lieBlockInverse), since Jlog6(exp6(v)) Jexp6(v) = I.  tests/test_rbd_fd_derivatives_host.py builds and runs it.
#define IDOCP_NO_HIP_RUNTIME
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "dev_lie.hpp"

using namespace idocp_dev;

int main() {
  const double angles[] = {0.0, 1e-9, 1e-4, 1e-2, 0.0499, 0.04999999, 0.05, 0.05000001, 0.0501, 0.3, 1.5, 3.0};
  const double axis[3] = {0.6, -0.3, 0.7416198487095663}, lin[3] = {0.3, -0.5, 0.7};
  double worst = 0.0, jump = 0.0, prev[36] = {};
  int failures = 0;
  for (double t : angles) {
    double v[6], R[9], p[3], J[36], Jl[36], Ji[36];
    for (int k = 0; k < 3; ++k) { v[k] = lin[k]; v[3 + k] = t * axis[k]; }
    lieDIntegrateArg1(v, J);
    lieExp6(v, R, p); lieJlog6(R, p, Jl); lieBlockInverse(Jl, Ji);
    double err = 0.0;
    for (int i = 0; i < 36; ++i) { if (!std::isfinite(J[i])) ++failures; err = std::fmax(err, std::fabs(J[i] - Ji[i])); }
    // Jlog6's own closed forms cancel between 1e-4 and 1e-2 rad (its beta-dot: 2 / t^4 against its neighbour); 1e-9 covers that and is far below
    // any error of sign, order or coefficient in the block Q, which is of the size of |lin| = 0.9
    std::printf("t = %.8g: |Jexp6 - Jlog6^-1| = %.2e\n", t, err);
    if (!(err < 1e-9)) ++failures;
    worst = std::fmax(worst, err);
    if (t == 0.05) { for (int i = 0; i < 36; ++i) jump = std::fmax(jump, std::fabs(J[i] - prev[i])); }      // against 0.04999999: the series side
    for (int i = 0; i < 36; ++i) prev[i] = J[i];
    if (t == 0.0) for (int i = 0; i < 36; ++i) {
      // at zero rotation: [[I, -skew(lin) / 2], [0, I]]
      const int r = i % 6, c = i / 6;
      double want = r == c ? 1.0 : 0.0;
      if (r < 3 && c >= 3) { double S[9]; lieSkew(lin, S); want = -0.5 * S[3 * r + (c - 3)]; }
      if (std::fabs(J[i] - want) > 1e-15) ++failures;
    }
  }
  std::printf("across the switch: %.2e\n", jump);
  if (!(jump < 1e-8)) ++failures;      // (the argument itself moves by 1e-8)
  if (failures) { std::printf("lie dintegrate arg1: %d failures\n", failures); return EXIT_FAILURE; }
  std::printf("lie dintegrate arg1: ok (worst %.2e)\n", worst);
  return EXIT_SUCCESS;
}
