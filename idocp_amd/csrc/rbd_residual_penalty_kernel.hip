// The penalty form of the residual kernel (idocp_rbd_linearize_rollout_penalty; include/idocp_hip.h has the definition): ONE launch per pass loads
// the scratch blocks of rbd_residual_kernel.hip into LDS once and writes, per sample, G [R + Rc][nz] -- the cost rows of the cost form bit for bit,
// the constraint rows behind them --, rho [R + Rc] (sigma on the constraint rows), D [nz] and the gradient of merit = cost + mu sq_violation.
//   acceleration box of joint j:  sigma = s b,  row = s [b != 0] da_j/d(q, v, u),                         s = sqrt(dt mu)
//   cone row of an active contact: sigma = s max(0, g),  row = s [g > 0] (dg/df) df_c/d(q, v, u)
//   q, v, u boxes: no dense row -- D = dt mu [b != 0] and the gradient term dt mu b at the joint's own column.
// Between the loads and the stores the form adds: the box values of the columns (q, v, u read from the rollout, one entry per lane), sigma and the
// at most three coefficients of every constraint row, kept in LDS (RbdResidualPenaltyLds: 2.3 KiB on the quadruped at S = 2, on top of the
// 25.6 KiB of the cost form).  An entry of a constraint row is the coefficient times the block entry, a cone row the three products summed by
// fused multiply-adds in the order x, y, z.  G^T rho runs over the cost rows first, then the constraint rows, in index order; the diagonal term is
// added last.  The same template (rbd_residual_kernel.hpp) with Args = RbdResidualPenaltyArgs, instantiated HERE so that the cost form keeps its code.
#include "rbd_residual_kernel.hpp"

namespace idocp_dev {

namespace {

template <int NV, int NF, int NU, int S>
void launchResidualPenalty(const RbdResidualPenaltyArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((rbd_residual_kernel<NV, NF, NU, S, RbdResidualPenaltyArgs>), dim3((unsigned)((a.count + S - 1) / S)), dim3(THREADS), 0, st, a);
}

}  // namespace

bool rbdResidualPenalty(int nv, bool quadruped, const RbdResidualPenaltyArgs& a, hipStream_t st) {
  constexpr int SC = RBD_RESIDUAL_SAMPLES_CHAIN;
  if (quadruped) { launchResidualPenalty<LeggedDims<4, 3>::NV, 12, LeggedDims<4, 3>::NV - 6, RBD_RESIDUAL_SAMPLES>(a, st); return true; }
  switch (nv) {
    case 2: launchResidualPenalty<2, 0, 2, SC>(a, st); break;
    case 3: launchResidualPenalty<3, 0, 3, SC>(a, st); break;
    case 4: launchResidualPenalty<4, 0, 4, SC>(a, st); break;
    case 5: launchResidualPenalty<5, 0, 5, SC>(a, st); break;
    case 6: launchResidualPenalty<6, 0, 6, SC>(a, st); break;
    case 7: launchResidualPenalty<7, 0, 7, SC>(a, st); break;
    case 8: launchResidualPenalty<8, 0, 8, SC>(a, st); break;
    default: return false;
  }
  return true;
}

}  // namespace idocp_dev
