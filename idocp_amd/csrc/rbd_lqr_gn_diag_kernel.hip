// The Gauss-Newton form of the LQR backward pass with a per-sample per-stage diagonal (idocp_rbd_lqr_backward_gn_diag; include/idocp_hip.h):
// the recursion of rbd_lqr_gn_kernel.hip, and entry (c, c) of the stage Hessian gains D_k[c] right where wx / wu are added, as the tiles of H
// are stored: Qxx = (H + wx) + D, Quu = (H + wu) + D.  D_k [nz] is read once per step, entry c on lane c, into nz doubles of LDS of this form's
// own; a negative or non-finite entry fails the sample at step k.  The same kernel template (rbd_lqr_kernel.hpp) with Args = RbdLqrGnDiagArgs,
// instantiated HERE so that the code of the two other forms stays what it was.
#include "rbd_lqr_kernel.hpp"

namespace idocp_dev {

void rbdLqrBackwardGnDiag(bool quadruped, const RbdLqrGnDiagArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.n + RBD_LQR_WAVES - 1) / RBD_LQR_WAVES)), block(64 * RBD_LQR_WAVES);
  if (quadruped) hipLaunchKernelGGL((rbd_lqr_kernel<36, 12, RbdLqrGnDiagArgs>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((rbd_lqr_kernel<16, 8, RbdLqrGnDiagArgs>), grid, block, 0, st, a);
}

}  // namespace idocp_dev
