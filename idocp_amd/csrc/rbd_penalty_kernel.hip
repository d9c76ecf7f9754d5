// The squared-hinge penalty of a rollout (idocp_rbd_score_penalty; include/idocp_hip.h has the definition): per sample
//   sq_violation = sum_k dt 1/2 sum_rows max(0, g_row)^2
// over the very rows the score (rbd_score_kernel.hip) sums into `violation`, a lower / upper pair on one quantity taken as ONE signed row
// b = max(0, x - hi) - max(0, lo - x).  An ADDITION: the reference has slacks and a barrier in place of a penalty.
//
// One wavefront per sample, RBD_WAVES samples per workgroup, no workgroup barrier, one launch per call.  Lane kind * NU + j, kind = 0 .. 3, holds
// the q, v, u or a box of actuated joint j, lane 4 NU + c the cone rows of contact c; every load of a step is a contiguous run over the lanes of a
// kind.  An array is read only where an enabled row needs it, and the f of a contact that is not active at a step is not read.
//
// The order of summation is fixed: a lane squares its own row (a cone lane adds its rows' squares in row order), the 64 lanes of a step are folded
// by the xor tree 32, ..., 2, 1, and the steps are added to the running sum IN INDEX ORDER, from zero or, with `accumulate`, from what sq_violation
// holds.  So a sample's result depends neither on n nor on the windowing.  A non-finite entry in anything read of a sample makes its result NaN,
// decided by a ballot at the end; no floating-point atomics.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

__device__ __forceinline__ double penaltyPositivePart(double x) { return x > 0.0 ? x : 0.0; }

template <int NV, bool FLOATING>
__global__ __launch_bounds__(64 * RBD_WAVES) void rbd_penalty_kernel(RbdPenaltyArgs a, int n) {
  constexpr int NQ = FLOATING ? NV + 1 : NV, NU = FLOATING ? NV - 6 : NV, NC = FLOATING ? 4 : 0, NF = 3 * NC;
  static_assert(4 * NU + NC <= 64, "one lane per box and per contact");
  const int lane = threadIdx.x & 63;
  const long sample = (long)blockIdx.x * RBD_WAVES + (threadIdx.x >> 6);
  if (sample >= n) return;                                // (no workgroup barrier below)
  const idocp_host::RbdScoreBlock& W = *a.block;
  const size_t N = (size_t)n;
  const double dt = W.dt;

  // what this lane's row needs of the block
  const int kind = lane / NU, j = lane - kind * NU, fc = lane - 4 * NU;
  const bool contact = NC > 0 && fc >= 0 && fc < NC;
  bool lower = false, upper = false;
  double lo = 0.0, hi = 0.0;
  if (kind == 0) { lower = upper = W.position_limits; lo = W.q_min[j]; hi = W.q_max[j]; }
  else if (kind == 1) { lower = upper = W.velocity_limits; lo = -W.v_max[j]; hi = W.v_max[j]; }
  else if (kind == 2) { lower = upper = W.torque_limits; lo = -W.u_max[j]; hi = W.u_max[j]; }
  else if (kind == 3) { lower = W.acceleration_lower; upper = W.acceleration_upper; lo = W.a_min[j]; hi = W.a_max[j]; }
  const double* __restrict__ src = kind == 0 ? a.q : (kind == 1 ? a.v : (kind == 2 ? a.u : a.a));
  const int width = kind == 0 ? NQ : (kind == 2 ? NU : NV);
  const int at = kind == 0 ? (NQ - NU) + j : (kind == 2 ? j : (NV - NU) + j);
  const bool box = kind < 4 && (lower || upper) && src != nullptr;
  const int cone = contact && a.f ? W.cone : 0;
  const double mu = W.mu, mu_lin = mu * 0.70710678118654752440;      // mu / sqrt 2, as the score takes it

  double sq = (a.accumulate) ? a.sq[sample] : 0.0;
  bool finite = true;
  for (int k = 0; k < a.steps; ++k) {
    double t = 0.0;
    if (box) {
      const double x = src[((size_t)k * N + sample) * width + at];
      finite = finite && std::isfinite(x);
      const double b = (upper ? penaltyPositivePart(x - hi) : 0.0) - (lower ? penaltyPositivePart(lo - x) : 0.0);
      t = b * b;
    } else if (cone) {
      const unsigned mask = (a.masks[k >> 3] >> (4 * (k & 7))) & 15u;
      if (mask >> fc & 1u) {
        const double* __restrict__ f = a.f + ((size_t)k * N + sample) * NF + 3 * fc;
        const double fx = f[0], fy = f[1], fz = f[2];
        finite = finite && std::isfinite(fx) && std::isfinite(fy) && std::isfinite(fz);
        const double h0 = penaltyPositivePart(-fz);
        t = h0 * h0;
        if (cone == 1) {
          const double h1 = penaltyPositivePart(fx - mu_lin * fz), h2 = penaltyPositivePart(-fx - mu_lin * fz);
          const double h3 = penaltyPositivePart(fy - mu_lin * fz), h4 = penaltyPositivePart(-fy - mu_lin * fz);
          t += h1 * h1; t += h2 * h2; t += h3 * h3; t += h4 * h4;
        } else {
          const double h1 = penaltyPositivePart(fx * fx + fy * fy - mu * mu * fz * fz);
          t += h1 * h1;
        }
      }
    }
    // the rows of a step: a fixed tree over the wavefront
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
    sq += dt * (0.5 * t);
  }
  const bool all_finite = __ballot(!finite) == 0;
  if (lane == 0) a.sq[sample] = all_finite ? sq : __builtin_nan("");
}

template <int NV, bool FLOATING>
void launchPenalty(const RbdPenaltyArgs& a, int n, hipStream_t st) {
  hipLaunchKernelGGL((rbd_penalty_kernel<NV, FLOATING>), dim3((unsigned)((n + RBD_WAVES - 1) / RBD_WAVES)), dim3(64 * RBD_WAVES), 0, st, a, n);
}

}  // namespace

bool rbdPenalty(int nv, bool quadruped, const RbdPenaltyArgs& a, int n, hipStream_t st) {
  if (quadruped) { launchPenalty<LeggedDims<4, 3>::NV, true>(a, n, st); return true; }
  switch (nv) {
    case 2: launchPenalty<2, false>(a, n, st); break;
    case 3: launchPenalty<3, false>(a, n, st); break;
    case 4: launchPenalty<4, false>(a, n, st); break;
    case 5: launchPenalty<5, false>(a, n, st); break;
    case 6: launchPenalty<6, false>(a, n, st); break;
    case 7: launchPenalty<7, false>(a, n, st); break;
    case 8: launchPenalty<8, false>(a, n, st); break;
    default: return false;
  }
  return true;
}

}  // namespace idocp_dev
