// The score of a rollout on plain arrays (idocp_rbd_score_rollout; include/idocp_hip.h): per sample the solvers' stage and terminal cost and the
// violation sum_k dt sum_rows max(0, g_row) of the constraint rows switched on, from the step-major slices idocp_rbd_rollout writes.  An ADDITION:
// the reference evaluates these sums for the solver's own iterate only.
//
// One wavefront per sample, RBD_WAVES samples per workgroup, no workgroup barrier (a wavefront past the last sample leaves at once), like the other
// rbd kernels; one launch per call.  A wavefront is cut into GROUPS = 64 / ROWS groups of ROWS lanes (32 on the quadruped, 8 on a chain), and each
// group takes one step at a time, so a wavefront works on GROUPS consecutive steps at once.  Inside a group lane l < NV holds row l of the tangent
// space -- q (-) q_ref, v - v_ref, a, and on an actuated row the torque term and the joint-limit rows --, lane NV + 3 c + x entry x of the force
// of contact c, and lane NV + 3 c also the cone rows of contact c.  Every load of a step is one contiguous run of doubles over the lanes of a group.
//
// The SE(3) logarithm (rows 0 .. 5 on the quadruped) is the only expensive term of a step.  It is NOT computed where it is used: before a chunk of 64
// steps is folded, lane l of the wavefront computes the logarithm of step l of the chunk (lieRelative, lieLog6 of dev_lie.hpp, the functions the
// policy kernel and idocp_model_subtract_configuration run) and leaves its six values in the wavefront's LDS slice, so a window of s steps costs
// ceil(s / 64) logarithms of latency per wavefront, not s.
//
// The order of summation is fixed.  The partial sums of a step are folded over the ROWS lanes of its group by the xor tree ROWS / 2, ..., 2, 1 (every
// lane ends with the same sum: a + b is commutative); the steps are then added to the running cost and violation IN INDEX ORDER, the terminal term
// last.  The running sums start from zero or, with `accumulate`, from what cost / violation hold -- the very additions a longer window would have
// made --, so a sample's results do not depend on n, on the launch, or on the windowing.  No floating-point atomics.
//
// A non-finite entry in anything read of a sample makes both results NaN, decided by a ballot over the wavefront at the end, because max(0, NaN)
// would swallow it.  The f of a contact that is not active at a step is not read.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dev_dense.hpp"
#include "dev_lie.hpp"
#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

template <bool FLOATING>
struct RbdScoreLds {
  double e6[FLOATING ? 64 : 1][6];      // the base rows of q (-) q_ref for the 64 steps of a chunk
};

__device__ __forceinline__ double positivePart(double x) { return x > 0.0 ? x : 0.0; }

template <int NV, bool FLOATING>
__global__ __launch_bounds__(64 * RBD_WAVES) void rbd_score_kernel(RbdScoreArgs a, int n) {
  constexpr int NQ = FLOATING ? NV + 1 : NV, NU = FLOATING ? NV - 6 : NV, NC = FLOATING ? 4 : 0, NF = 3 * NC;
  constexpr int ROWS = FLOATING ? 32 : 8, GROUPS = 64 / ROWS;
  static_assert(NV + NF <= ROWS, "one lane of a group per row and per force entry");
  __shared__ RbdScoreLds<FLOATING> s_wave[RBD_WAVES];
  const int lane = threadIdx.x & 63, l = lane % ROWS, grp = lane / ROWS;
  const long sample = (long)blockIdx.x * RBD_WAVES + (threadIdx.x >> 6);
  if (sample >= n) return;                                // (no workgroup barrier below)
  RbdScoreLds<FLOATING>& L = s_wave[threadIdx.x >> 6];
  const idocp_host::RbdScoreBlock& W = *a.block;
  const size_t N = (size_t)n;
  const int slices = a.steps + (a.terminal ? 1 : 0);
  const double dt = W.dt;

  // what this lane's row needs of the block
  const bool row = l < NV, joint = row && l >= NV - NU, force = !row && l < NV + NF;
  const int j = l - (NV - NU), fx = l - NV, fc = fx / 3;
  double wq = 0, wv = 0, wa = 0, wqf = 0, wvf = 0, wu = 0, uref = 0, qmin = 0, qmax = 0, vmax = 0, umax = 0, amin = 0, amax = 0, wf = 0, fref = 0;
  if (row) { wq = W.q_weight[l]; wv = W.v_weight[l]; wa = W.a_weight[l]; wqf = W.qf_weight[l]; wvf = W.vf_weight[l]; }
  if (joint) { wu = W.u_weight[j]; uref = W.u_ref[j]; qmin = W.q_min[j]; qmax = W.q_max[j]; vmax = W.v_max[j]; umax = W.u_max[j]; amin = W.a_min[j]; amax = W.a_max[j]; }
  if (force) { wf = W.f_weight[fc][fx % 3]; fref = W.f_ref[fc][fx % 3]; }
  const int cone = W.cone;
  const double mu = W.mu, mu_lin = mu * 0.70710678118654752440;      // mu / sqrt 2 (linearized_friction_cone.cpp)
  const bool pos_lim = W.position_limits, vel_lim = W.velocity_limits, tau_lim = W.torque_limits, acc_lo = W.acceleration_lower, acc_hi = W.acceleration_upper;

  double cost = (a.accumulate && a.cost) ? a.cost[sample] : 0.0;
  double violation = (a.accumulate && a.violation) ? a.violation[sample] : 0.0;
  bool finite = true;

  for (int k0 = 0; k0 < slices; k0 += 64) {
    if (FLOATING) {
      waveLdsSync();                                       // (the previous chunk's values have been read)
      const int k = k0 + lane;
      if (k < slices) {
        const double* __restrict__ q = a.q + ((size_t)k * N + sample) * NQ;
        const double* __restrict__ qr = a.q_ref + (size_t)k * NQ;
        double qm[7], qp[7], R[9], p[3], d[6];
#pragma unroll
        for (int i = 0; i < 7; ++i) { qm[i] = qr[i]; qp[i] = q[i]; finite = finite && std::isfinite(qp[i]); }
        lieRelative(qm, qp, R, p);
        lieLog6(R, p, d);
#pragma unroll
        for (int i = 0; i < 6; ++i) L.e6[lane][i] = d[i];
      }
      waveLdsSync();
    }
    const int chunk = slices - k0 < 64 ? slices - k0 : 64;
    for (int kk = 0; kk < chunk; kk += GROUPS) {
      const int k = k0 + kk + grp;
      const bool valid = k < slices, term = k == a.steps;
      double c = 0.0, g = 0.0;
      if (valid && row) {
        const size_t at = (size_t)k * N + sample;
        const int iq = FLOATING ? l + 1 : l;
        double e, qj = 0.0;
        if (FLOATING && l < 6) e = L.e6[kk + grp][l];
        else { qj = a.q[at * NQ + iq]; finite = finite && std::isfinite(qj); e = qj - a.q_ref[(size_t)k * NQ + iq]; }
        const double vj = a.v[at * NV + l];
        finite = finite && std::isfinite(vj);
        const double dv = vj - a.v_ref[(size_t)k * NV + l];
        if (term) {
          c = wqf * e * e + wvf * dv * dv;
        } else {
          c = wq * e * e + wv * dv * dv;
          double aj = 0.0, uj = 0.0;
          if (a.a) { aj = a.a[at * NV + l]; finite = finite && std::isfinite(aj); c += wa * aj * aj; }
          if (joint) {
            if (a.u) { uj = a.u[at * NU + j]; finite = finite && std::isfinite(uj); c += wu * (uj - uref) * (uj - uref); }
            if (pos_lim) g += positivePart(qmin - qj) + positivePart(qj - qmax);
            if (vel_lim) g += positivePart(-vmax - vj) + positivePart(vj - vmax);
            if (tau_lim && a.u) g += positivePart(-umax - uj) + positivePart(uj - umax);
            if (acc_lo && a.a) g += positivePart(amin - aj);
            if (acc_hi && a.a) g += positivePart(aj - amax);
          }
        }
      } else if (valid && force && !term && a.f) {
        const unsigned mask = (a.masks[k >> 3] >> (4 * (k & 7))) & 15u;
        if (mask >> fc & 1u) {
          const double* __restrict__ f = a.f + ((size_t)k * N + sample) * NF + 3 * fc;
          const double fj = f[fx % 3];
          finite = finite && std::isfinite(fj);
          c = wf * (fj - fref) * (fj - fref);
          if (cone && fx % 3 == 0) {
            const double fy = f[1], fz = f[2];                 // (this lane's own entry is fx; lanes + 1, + 2 check fy, fz)
            if (cone == 1) {
              g = positivePart(-fz) + positivePart(fj - mu_lin * fz) + positivePart(-fj - mu_lin * fz) + positivePart(fy - mu_lin * fz) +
                  positivePart(-fy - mu_lin * fz);
            } else {
              g = positivePart(-fz) + positivePart(fj * fj + fy * fy - mu * mu * fz * fz);
            }
          }
        }
      }
      // the rows of a step: a fixed tree over the lanes of the group
#pragma unroll
      for (int off = ROWS / 2; off >= 1; off >>= 1) { c += __shfl_xor(c, off); g += __shfl_xor(g, off); }
      c = (term ? 1.0 : dt) * (0.5 * c);
      g = dt * g;
      if (valid && l == 0 && a.stage_cost) a.stage_cost[(size_t)k * N + sample] = c;
      // the steps, in index order
#pragma unroll
      for (int s = 0; s < GROUPS; ++s) {
        const double cs = __shfl(c, s * ROWS), gs = __shfl(g, s * ROWS);
        if (k0 + kk + s < slices) {
          cost += cs;
          if (k0 + kk + s != a.steps) violation += gs;
        }
      }
    }
  }
  const bool all_finite = __ballot(!finite) == 0;
  if (lane == 0) {
    if (a.cost) a.cost[sample] = all_finite ? cost : __builtin_nan("");
    if (a.violation) a.violation[sample] = all_finite ? violation : __builtin_nan("");
  }
}

template <int NV, bool FLOATING>
void launchScore(const RbdScoreArgs& a, int n, hipStream_t st) {
  hipLaunchKernelGGL((rbd_score_kernel<NV, FLOATING>), dim3((unsigned)((n + RBD_WAVES - 1) / RBD_WAVES)), dim3(64 * RBD_WAVES), 0, st, a, n);
}

}  // namespace

void rbdScore(int nv, bool quadruped, const RbdScoreArgs& a, int n, hipStream_t st) {
  if (quadruped) { launchScore<LeggedDims<4, 3>::NV, true>(a, n, st); return; }
  switch (nv) {
    case 2: launchScore<2, false>(a, n, st); break;
    case 3: launchScore<3, false>(a, n, st); break;
    case 4: launchScore<4, false>(a, n, st); break;
    case 5: launchScore<5, false>(a, n, st); break;
    case 6: launchScore<6, false>(a, n, st); break;
    case 7: launchScore<7, false>(a, n, st); break;
    case 8: launchScore<8, false>(a, n, st); break;
    default: break;
  }
}

}  // namespace idocp_dev
