// The augmented-Lagrangian form of the residual kernel (idocp_rbd_linearize_rollout_al; include/idocp_hip.h has the definition): the penalty form
// of rbd_residual_penalty_kernel.hip with every constraint row taken at its SHIFTED value.  With lambda the multiplier of the row and mu > 0:
//   q, v, u boxes (per sample and column):   y = x + lambda / mu,  b~ = max(0, y - hi) - max(0, lo - y);  D = dt mu [b~ != 0], gradient + dt mu b~
//   acceleration box of joint j:             the same y on a_j;    sigma = s b~,  row = s [b~ != 0] da_j/d(q, v, u),      s = sqrt(dt mu)
//   cone row of an active contact:           g~ = g + lambda / mu; sigma = s max(0, g~),  row = s [g~ > 0] (dg/df) df_c/d(q, v, u)
// The shift is applied at the two places where the penalty form computes its per-(sample, column) box value and its per-(sample, row) sigma; the
// quotient is rounded, then the sum (fp contract(off) there).  Every multiplier is read ONCE, by the lane that forms its row or column, straight
// from the pass's slice [count][L] in global memory: the form keeps no LDS beyond the penalty form's, so the workgroups per CU are the same.  A
// non-finite multiplier flags its sample like any other input.  lambda == NULL: no shift, the penalty form's bits.  Rows of kinds switched off and
// of inactive contacts do not read their multiplier.  The same template (rbd_residual_kernel.hpp) with Args = RbdResidualAlArgs, instantiated HERE so
// that the cost form and the penalty form keep their code.
#include "rbd_residual_kernel.hpp"

namespace idocp_dev {

namespace {

template <int NV, int NF, int NU, int S>
void launchResidualAl(const RbdResidualAlArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((rbd_residual_kernel<NV, NF, NU, S, RbdResidualAlArgs>), dim3((unsigned)((a.count + S - 1) / S)), dim3(THREADS), 0, st, a);
}

}  // namespace

bool rbdResidualAl(int nv, bool quadruped, const RbdResidualAlArgs& a, hipStream_t st) {
  constexpr int SC = RBD_RESIDUAL_SAMPLES_CHAIN;
  if (quadruped) { launchResidualAl<LeggedDims<4, 3>::NV, 12, LeggedDims<4, 3>::NV - 6, RBD_RESIDUAL_SAMPLES>(a, st); return true; }
  switch (nv) {
    case 2: launchResidualAl<2, 0, 2, SC>(a, st); break;
    case 3: launchResidualAl<3, 0, 3, SC>(a, st); break;
    case 4: launchResidualAl<4, 0, 4, SC>(a, st); break;
    case 5: launchResidualAl<5, 0, 5, SC>(a, st); break;
    case 6: launchResidualAl<6, 0, 6, SC>(a, st); break;
    case 7: launchResidualAl<7, 0, 7, SC>(a, st); break;
    case 8: launchResidualAl<8, 0, 8, SC>(a, st); break;
    default: return false;
  }
  return true;
}

}  // namespace idocp_dev
