// Batched contact-frame kinematics on plain arrays (idocp_rbd_contact_kinematics_batch, the latch step of idocp_rbd_rollout_footholds;
// include/idocp_hip.h): what Robot::updateFrameKinematics + getContactPoints, frameRotation and getFrameJacobian give the reference for one
// state, for n states in one launch.  An addition: the library had no forward kinematics on the device.
//
// The arithmetic of a sample is one quaternion -> rotation and four chains of LJ revolute joints, so a wavefront per sample (the other rbd
// kernels) would idle 60 lanes.  ONE LANE PER (sample, leg): lane 4 i + c of the grid serves contact c of sample i, 16 samples per wavefront,
// RBD_KIN_THREADS / 4 per workgroup.  No LDS, no cross-lane exchange, no barrier: a lane past the last sample leaves at once, and a sample's
// arithmetic is one straight instruction stream that depends neither on n nor on which outputs were asked for (the Jacobian columns are
// computed in ONE place, for the Jacobian and the velocity alike; only the stores are conditional).
//   points, velocity   a wavefront stores 64 x 3 contiguous doubles
//   rotation           64 x 9 contiguous doubles
//   jacobian           column-major 12 x 18 per sample: the four lanes of a sample store the 12 contiguous rows of a column, 3 each
//   q, v               every lane reads its sample's whole row (the non-finite rule needs all of it); the 16 rows of a wavefront are one
//                      contiguous run of 16 x 19 (18) doubles, the four lanes of a sample read the same addresses
//
// The Jacobian is the WORLD-frame one, written geometrically: column r of contact c is d/d eps p_c(q (+) eps e_r), i.e. the world linear
// velocity of the frame origin under the unit tangent e_r:
//   base linear r    R_b e_r                               (the retraction moves the base by R_b v_lin)
//   base angular r   (R_b e_r) x (p_c - p_b)
//   joint j of leg c a_j x (p_c - o_j),  a_j the world axis and o_j the world origin of the joint
//   joints of the other legs: zero (stored, not skipped)
// velocity = sum over the columns in that order of column * v_r.
//
// The latch entry (rbdLatchQuadruped) is this kernel with `points` alone and a carry mask: a lane whose bit is set copies its three doubles
// from prev (or, without prev, leaves them alone) instead of computing them.
#include <hip/hip_runtime.h>

#include "dev_lie.hpp"
#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

template <typename D>
__global__ __launch_bounds__(RBD_KIN_THREADS) void rbd_kinematics_kernel(const DevModel* __restrict__ m, const RbdFrames* __restrict__ P,
                                                                         idocp_rbd_kin_io_t io, const double* prev, int carry_mask, int n) {
  constexpr int NV = D::NV, NQ = D::NQ, NL = D::NL, LJ = D::LJ, NF = D::NF;
  const long gid = (long)blockIdx.x * RBD_KIN_THREADS + threadIdx.x;
  const long sample = gid / NL;
  if (sample >= n) return;
  const int leg = (int)(gid - sample * NL);
  if ((carry_mask >> leg) & 1) {
    // carried bit for bit; without prev the entry is the caller's and stays as it is
    if (prev) {
#pragma unroll
      for (int r = 0; r < 3; ++r) io.points[sample * NF + 3 * leg + r] = prev[sample * NF + 3 * leg + r];
    }
    return;
  }
  const double* __restrict__ q = io.q + sample * NQ;
  const double* __restrict__ v = io.v ? io.v + sample * NV : nullptr;
  const bool want_cols = io.jacobian || io.velocity;

  // a non-finite entry anywhere in the row: 0 * x is NaN exactly then
  double zq = 0.0;
#pragma unroll
  for (int i = 0; i < NQ; ++i) zq += 0.0 * q[i];
  const bool bad_q = !(zq == 0.0);

  // ---- outward: base, then the LJ joints of this lane's leg ----
  double Rb[9], Rw[9], pw[3], org[LJ][3], axw[LJ][3];
  lieQuatToR(q + 3, Rb);
#pragma unroll
  for (int i = 0; i < 9; ++i) Rw[i] = Rb[i];
  const double pb[3] = {q[0], q[1], q[2]};
  pw[0] = pb[0]; pw[1] = pb[1]; pw[2] = pb[2];
#pragma unroll
  for (int j = 0; j < LJ; ++j) {
    const int ji = 1 + leg * LJ + j;
    double sj, cj;
    sincos(q[7 + leg * LJ + j], &sj, &cj);
    Mat3<double> R;
    revoluteRotation<double>(m->R[ji], m->axis[ji], cj, sj, R);
    const double* p = m->p[ji];
    const double* u = m->axis[ji];
    double t[3];
    lieMatvec3(Rw, p, t);
    pw[0] += t[0]; pw[1] += t[1]; pw[2] += t[2];
    org[j][0] = pw[0]; org[j][1] = pw[1]; org[j][2] = pw[2];
    lieMatmul3(Rw, R.m, Rw);
    lieMatvec3(Rw, u, axw[j]);
  }
  // ---- the contact frame in the tip joint ----
  double pf[3], Rf[9];
  {
    double t[3];
    lieMatvec3(Rw, P->p[leg], t);
    pf[0] = pw[0] + t[0]; pf[1] = pw[1] + t[1]; pf[2] = pw[2] + t[2];
    lieMatmul3(Rw, P->R[leg], Rf);
  }
  const double nan = __builtin_nan("");
  if (io.points) {
#pragma unroll
    for (int r = 0; r < 3; ++r) io.points[sample * NF + 3 * leg + r] = bad_q ? nan : pf[r];
  }
  if (io.rotation) {
#pragma unroll
    for (int r = 0; r < 9; ++r) io.rotation[(sample * NL + leg) * 9 + r] = bad_q ? nan : Rf[r];
  }
  if (!want_cols) return;

  // ---- the columns of the world Jacobian that this contact has: 6 of the base, LJ of its leg ----
  double col[6 + LJ][3];
  const double d[3] = {pf[0] - pb[0], pf[1] - pb[1], pf[2] - pb[2]};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double e[3] = {Rb[r], Rb[3 + r], Rb[6 + r]};      // R_b e_r
    col[r][0] = e[0]; col[r][1] = e[1]; col[r][2] = e[2];
    col[3 + r][0] = e[1] * d[2] - e[2] * d[1];
    col[3 + r][1] = e[2] * d[0] - e[0] * d[2];
    col[3 + r][2] = e[0] * d[1] - e[1] * d[0];
  }
#pragma unroll
  for (int j = 0; j < LJ; ++j) {
    const double* a = axw[j];
    const double o[3] = {pf[0] - org[j][0], pf[1] - org[j][1], pf[2] - org[j][2]};
    col[6 + j][0] = a[1] * o[2] - a[2] * o[1];
    col[6 + j][1] = a[2] * o[0] - a[0] * o[2];
    col[6 + j][2] = a[0] * o[1] - a[1] * o[0];
  }
  if (io.jacobian) {
    double* __restrict__ J = io.jacobian + sample * (NF * NV) + 3 * leg;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      // column c of this contact: the base's, this leg's, or the zero of another leg
      const int l = c < 6 ? leg : (c - 6) / LJ, k = c < 6 ? c : 6 + (c - 6) % LJ;
      const bool mine = (l == leg);
#pragma unroll
      for (int r = 0; r < 3; ++r) J[c * NF + r] = bad_q ? nan : (mine ? col[k][r] : 0.0);
    }
  }
  if (io.velocity) {
    double zv = 0.0;
#pragma unroll
    for (int i = 0; i < NV; ++i) zv += 0.0 * v[i];
    const bool bad = bad_q || !(zv == 0.0);
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6 + LJ; ++k) {
      const double vk = k < 6 ? v[k] : v[6 + leg * LJ + (k - 6)];
#pragma unroll
      for (int r = 0; r < 3; ++r) acc[r] += col[k][r] * vk;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) io.velocity[sample * NF + 3 * leg + r] = bad ? nan : acc[r];
  }
}

void launchKinematics(const DevModel* m, const RbdFrames* frames, const idocp_rbd_kin_io_t& io, const double* prev, int carry_mask, int n,
                      hipStream_t st) {
  using D = LeggedDims<4, 3>;
  const long long lanes = (long long)n * D::NL;
  const dim3 grid((unsigned)((lanes + RBD_KIN_THREADS - 1) / RBD_KIN_THREADS)), block(RBD_KIN_THREADS);
  hipLaunchKernelGGL((rbd_kinematics_kernel<D>), grid, block, 0, st, m, frames, io, prev, carry_mask, n);
}

}  // namespace

void rbdKinematicsQuadruped(const DevModel* m, const RbdFrames* frames, const idocp_rbd_kin_io_t& io, int n, hipStream_t st) {
  launchKinematics(m, frames, io, nullptr, 0, n, st);
}

void rbdLatchQuadruped(const DevModel* m, const RbdFrames* frames, const double* q, const double* prev, double* points, int carry_mask, int n,
                       hipStream_t st) {
  idocp_rbd_kin_io_t io = idocp_rbd_kin_io_t();
  io.q = q; io.points = points;
  launchKinematics(m, frames, io, prev, carry_mask, n, st);
}

}  // namespace idocp_dev
