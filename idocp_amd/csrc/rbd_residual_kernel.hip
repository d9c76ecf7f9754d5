// The residual rows of the acceleration and contact-force terms of an objective (idocp_rbd_linearize_rollout_cost; include/idocp_hip.h has the
// definition): per sample of one pass of one step, from the forward solution a, f and the column-major blocks da_dq, da_dv, da_du, df_dq, df_dv, df_du
// that the derivative composition left in scratch,
//   G [R][nz] row-major = s_r [d/dq | d/dv | d/du] of row r,   rho [R] = s_r a_r  or  s_r (f - f_ref),   lx += Gx^T rho,  lu += Gu^T rho,
// the rows of inactive contacts and the padding rows zero.  An ADDITION: the reference differentiates these terms inside its solvers only.
//
// Bandwidth work, a transposition through LDS.  A workgroup of RBD_RESIDUAL_THREADS lanes owns S consecutive samples (S even: 2 on the quadruped, 16
// on a chain).  Because every scratch array is [count][its size], the S samples' share of each array is ONE contiguous run that starts at an even
// number of doubles:
//   1. the eight runs go into LDS with 16-byte loads, lane l on the pairs l, l + 256, ... of each run (contiguous over the lanes); every entry is
//      looked at on its way, and a non-finite one raises the flag of the sample it belongs to.  In LDS a block keeps its column-major form with the
//      leading dimension padded to an odd number of doubles, the three blocks of a kind side by side: Da [nz][nv | 1], Df [nz][nf | 1];
//   2. rho, one (sample, row) per lane;
//   3. the run of G -- S R nz doubles, contiguous -- is written with 16-byte stores, lane l on the pairs l, l + 256, ...: each entry is ONE rounded
//      product of s_r and the block entry read from LDS at [c][r];
//   4. G^T rho, one (sample, column) per lane: the sum over the rows in index order, fused multiply-adds from 0 on the same rounded products, added
//      to the diagonal part that lx, lu hold.
// Every sum has a fixed order, there are no atomics and no scratch memory; a flagged sample stores NaN everywhere.  A caller's G that is only 8-byte
// aligned takes 8-byte stores (a uniform branch).  The kernel template lives in rbd_residual_kernel.hpp; the form here is Args = RbdResidualArgs.
#include "rbd_residual_kernel.hpp"

namespace idocp_dev {

namespace {

template <int NV, int NF, int NU, int S>
void launchResidual(const RbdResidualArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((rbd_residual_kernel<NV, NF, NU, S>), dim3((unsigned)((a.count + S - 1) / S)), dim3(THREADS), 0, st, a);
}

}  // namespace

bool rbdResidual(int nv, bool quadruped, const RbdResidualArgs& a, hipStream_t st) {
  constexpr int SC = RBD_RESIDUAL_SAMPLES_CHAIN;
  if (quadruped) { launchResidual<LeggedDims<4, 3>::NV, 12, LeggedDims<4, 3>::NV - 6, RBD_RESIDUAL_SAMPLES>(a, st); return true; }
  switch (nv) {
    case 2: launchResidual<2, 0, 2, SC>(a, st); break;
    case 3: launchResidual<3, 0, 3, SC>(a, st); break;
    case 4: launchResidual<4, 0, 4, SC>(a, st); break;
    case 5: launchResidual<5, 0, 5, SC>(a, st); break;
    case 6: launchResidual<6, 0, 6, SC>(a, st); break;
    case 7: launchResidual<7, 0, 7, SC>(a, st); break;
    case 8: launchResidual<8, 0, 8, SC>(a, st); break;
    default: return false;
  }
  return true;
}

}  // namespace idocp_dev
