// The Gauss-Newton form of the LQR backward pass (idocp_rbd_lqr_backward_gn; include/idocp_hip.h): the recursion of rbd_lqr_kernel.hip with
// G_k^T G_k added to the stage Hessian H = Z^T P Z before it is stored.  G_k [g_rows][nz] is row-major in global memory; for the four rows
// 4 j .. 4 j + 3, lane l loads G[4 j + l / 16][16 t + l % 16] for each tile index t -- 16 consecutive doubles per row, coalesced -- and that
// value is both the A operand of tile column t and the B operand of tile row t of v_mfma_f64_16x16x4_f64, so G^T G accumulates into the H
// tiles in registers without LDS, in row order, the next four rows in flight while these multiply.  A non-finite entry of G_k fails the
// sample at step k.  The same kernel template (rbd_lqr_kernel.hpp) with Args = RbdLqrGnArgs, instantiated HERE so that the code of the form
// without rows stays what it was.
#include "rbd_lqr_kernel.hpp"

namespace idocp_dev {

void rbdLqrBackwardGn(bool quadruped, const RbdLqrGnArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.n + RBD_LQR_WAVES - 1) / RBD_LQR_WAVES)), block(64 * RBD_LQR_WAVES);
  if (quadruped) hipLaunchKernelGGL((rbd_lqr_kernel<36, 12, RbdLqrGnArgs>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((rbd_lqr_kernel<16, 8, RbdLqrGnArgs>), grid, block, 0, st, a);
}

}  // namespace idocp_dev
