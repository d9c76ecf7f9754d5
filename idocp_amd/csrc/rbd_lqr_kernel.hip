// The backward pass of time-varying LQR / iLQR over a linearised rollout, per sample (idocp_rbd_lqr_backward; include/idocp_hip.h has the
// recursion as the definition).  An ADDITION like the rest of the idocp_rbd_* block: the reference has no counterpart.
//
//   P = Wxf, p = lx[steps];   for k = steps - 1 .. 0, with Z = [A_k | B_k] (nx x (nx + nu)):
//     [Qx; Qu] = [lx_k; lu_k] + Z^T p
//     H = Z^T (P Z) = [A^T P A, .; B^T P A, B^T P B]:   Qxx = Wx + H_xx,  Qux = H_ux,  Quu = Wu + reg I + H_uu (lower triangle, mirrored)
//     [K_k | k_k] = -Quu^-1 [Qux | Qu]                  (Cholesky, L D L^T in registers: choleskySolveRows)
//     X = Qxx + Qux^T K_k,  P <- (X + X^T) / 2,  p <- Qx + Qux^T k_k
//
// ONE wavefront owns a sample's chain, one sample per workgroup (RBD_LQR_WAVES = 1: nothing is shared between samples, and the LDS of a sample
// -- 31.7 kB on the quadruped -- then packs five to a CU instead of four).  P, p and the block column of P Z in flight live in LDS for the whole
// horizon and never touch HBM between the steps; A_k, B_k are read once, K_k, k_k written once.  The products run on v_mfma_f64_16x16x4_f64
// through mfmaTileColumnTN (dev_dense.hpp): P Z is formed one block column of 16 at a time (three row tiles into Gc) and consumed at once by
// the tiles Z^T Gc of that column, whose accumulators -- the whole of H, 9 tiles on the quadruped -- stay in registers until Z is dead; the Qux,
// Quu, [K | k] blocks then reuse Z's room.  The 12 x 12 (chains: up to 8 x 8) solve takes all nx + 1 right-hand sides at once, one per lane.
// The chain over the steps is dependent, so step k - 1's A, B are fetched into registers (16-byte loads, lane l on pairs l, l + 64, ...)
// before step k computes and go to LDS when it is done.  Every sum has a fixed order and there are no atomics: a sample's bits depend neither
// on n nor on the outputs asked for.  Chains (nx <= 16, nu <= 8) run the same code with one row tile.
//
// Failure is per sample: a non-finite entry among what step k reads of the sample (A_k, B_k, lx_k, lu_k; lx[steps] counts for the last step)
// or a pivot of Quu that is not positive ends the sample's chain at k -- K, k of the steps <= k, P0, p0 and expected become NaN, status = k.
#include "rbd_lqr_kernel.hpp"

namespace idocp_dev {

void rbdLqrBackward(bool quadruped, const RbdLqrArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.n + RBD_LQR_WAVES - 1) / RBD_LQR_WAVES)), block(64 * RBD_LQR_WAVES);
  if (quadruped) hipLaunchKernelGGL((rbd_lqr_kernel<36, 12>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((rbd_lqr_kernel<16, 8>), grid, block, 0, st, a);
}

}  // namespace idocp_dev
