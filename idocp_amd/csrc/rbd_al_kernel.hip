// The augmented Lagrangian of the constraint rows (idocp_rbd_score_al, idocp_rbd_multiplier_update; include/idocp_hip.h has the definition): the
// squared hinge of rbd_penalty_kernel.hip on SHIFTED rows, and the first-order multiplier update.  With one multiplier per row, mu > 0:
//   box (ONE signed row per lower / upper pair):  y = x + lambda / mu,   b~ = max(0, y - hi) - max(0, lo - y)
//   cone row:                                     g~ = g + lambda / mu,  h~ = max(0, g~),  g as the penalty kernel computes it
//   sq_shifted = sum_k dt 1/2 sum_rows b~^2 | h~^2          lambda+ = mu b~ | mu h~
// The quotient is rounded, then the sum; lambda+ is one rounded product (fp contract(off) around the shift and the update, so that a host
// computes the same numbers; g is the penalty kernel's expression, and the sums of squares are written as the fused multiply-adds that kernel
// compiles to, so that lambda = 0 reproduces its bits).
// An ADDITION: the reference has slacks and a barrier.
//
// The shape is the penalty kernel's: one wavefront per sample, RBD_WAVES samples per workgroup, no workgroup barrier, no LDS, one launch per call.
// Lane kind * NU + j holds the q, v, u or a box of actuated joint j and multiplier row kind * NU + j: the 4 NU box rows of a (step, sample) are
// one contiguous run over the lanes, in and out.  Lane 4 NU + c holds contact c and its ncone consecutive rows 4 NU + ncone c + r.  Rows of
// kinds switched off and of contacts inactive at a step are not read; the update writes 0 there.
//
// Score: the summation order of the penalty kernel (lane, xor tree 32 .. 1, steps in index order from zero or from what sq holds).  Update: a lane
// writes its own rows after reading them, so lambda_out may alias lambda; the two statistics are maxima -- over a lane's steps, then over the
// wavefront by the xor tree, then, with accumulate, with what the arrays hold -- and a maximum has no order.  A non-finite entry in anything read
// of a sample makes its score and its statistics NaN, and the update writes NaN to all rows of the (step, sample) where it was read; no other
// sample is touched.  No atomics, no scratch memory.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

__device__ __forceinline__ double alPositivePart(double x) { return x > 0.0 ? x : 0.0; }

// lambda / mu of one row; lambda == nullptr: all zeros
__device__ __forceinline__ double alShift(const double* __restrict__ lambda, size_t at, double mu, double* value, bool* finite) {
#pragma clang fp contract(off)
  if (!lambda) { *value = 0.0; return 0.0; }
  const double l = lambda[at];
  *finite = *finite && std::isfinite(l);
  *value = l;
  return l / mu;
}

template <int NV, bool FLOATING, bool UPDATE>
__global__ __launch_bounds__(64 * RBD_WAVES) void rbd_al_kernel(RbdAlArgs a, int n) {
  constexpr int NQ = FLOATING ? NV + 1 : NV, NU = FLOATING ? NV - 6 : NV, NC = FLOATING ? 4 : 0, NF = 3 * NC;
  static_assert(4 * NU + NC <= 64, "one lane per box and per contact");
  const int lane = threadIdx.x & 63;
  const long sample = (long)blockIdx.x * RBD_WAVES + (threadIdx.x >> 6);
  if (sample >= n) return;                                // (no workgroup barrier below)
  const idocp_host::RbdScoreBlock& W = *a.block;
  const size_t N = (size_t)n;
  const double dt = W.dt, pen = a.penalty;

  // what this lane's row needs of the block: as in the penalty kernel
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
  // the multiplier rows: L per (step, sample); this lane's first row and its count
  const int ncone = NC == 0 ? 0 : (W.cone == 1 ? 5 : (W.cone == 2 ? 2 : 0));
  const int L = 4 * NU + ncone * NC;
  const int row0 = kind < 4 ? lane : 4 * NU + ncone * fc, nrows = kind < 4 ? 1 : (contact ? ncone : 0);
  const double nan = __builtin_nan("");

  double sq = (!UPDATE && a.accumulate) ? a.sq[sample] : 0.0;
  double worst = 0.0, moved = 0.0;
  bool finite = true;
  for (int k = 0; k < a.steps; ++k) {
    const size_t base = ((size_t)k * N + sample) * (size_t)L + row0;
    double t = 0.0;
    double out[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    bool finite_k = true;
    if (box) {
      const double x = src[((size_t)k * N + sample) * width + at];
      finite_k = std::isfinite(x);
      double l;
      const double shift = alShift(a.lambda, base, pen, &l, &finite_k);
      double bs;
      {
#pragma clang fp contract(off)
        const double y = x + shift;
        bs = (upper ? alPositivePart(y - hi) : 0.0) - (lower ? alPositivePart(lo - y) : 0.0);
        if (UPDATE) {
          const double b = (upper ? alPositivePart(x - hi) : 0.0) - (lower ? alPositivePart(lo - x) : 0.0);
          out[0] = pen * bs;
          worst = fmax(worst, fabs(b));
          moved = fmax(moved, fabs(out[0] - l));
        }
      }
      t = bs * bs;
    } else if (cone) {
      const unsigned mask = (a.masks[k >> 3] >> (4 * (k & 7))) & 15u;
      if (mask >> fc & 1u) {
        const double* __restrict__ f = a.f + ((size_t)k * N + sample) * NF + 3 * fc;
        const double fx = f[0], fy = f[1], fz = f[2];
        finite_k = std::isfinite(fx) && std::isfinite(fy) && std::isfinite(fz);
        double g[5];
        g[0] = -fz;
        if (cone == 1) { g[1] = fx - mu_lin * fz; g[2] = -fx - mu_lin * fz; g[3] = fy - mu_lin * fz; g[4] = -fy - mu_lin * fz; }
        else { g[1] = fx * fx + fy * fy - mu * mu * fz * fz; g[2] = g[3] = g[4] = 0.0; }
        double hs[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
          hs[r] = 0.0;
          if (r < ncone) {
#pragma clang fp contract(off)
            double l;
            const double shift = alShift(a.lambda, base + r, pen, &l, &finite_k);
            hs[r] = alPositivePart(g[r] + shift);
            if (UPDATE) {
              out[r] = pen * hs[r];
              worst = fmax(worst, alPositivePart(g[r]));
              moved = fmax(moved, fabs(out[r] - l));
            }
          }
        }
        // the squares as the penalty kernel sums them, its fused multiply-adds written out: h0^2 rounded, every further square fused into the sum
        t = hs[0] * hs[0];
        if (cone == 1) { t = __builtin_fma(hs[1], hs[1], t); t = __builtin_fma(hs[2], hs[2], t); t = __builtin_fma(hs[3], hs[3], t); t = __builtin_fma(hs[4], hs[4], t); }
        else t = __builtin_fma(hs[1], hs[1], t);
      }
    }
    finite = finite && finite_k;
    if (UPDATE) {
      const bool step_finite = __ballot(!finite_k) == 0;
#pragma unroll
      for (int r = 0; r < 5; ++r)
        if (r < nrows) a.lambda_out[base + r] = step_finite ? out[r] : nan;
    } else {
      // the rows of a step: a fixed tree over the wavefront
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off);
      sq = __builtin_fma(dt, 0.5 * t, sq);      // (as the penalty kernel's sq += dt * (0.5 * t) compiles)
    }
  }
  const bool all_finite = __ballot(!finite) == 0;
  if (UPDATE) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { worst = fmax(worst, __shfl_xor(worst, off)); moved = fmax(moved, __shfl_xor(moved, off)); }
    if (lane == 0) {
      double* const stat[2] = {a.infeasibility, a.change};
      const double value[2] = {worst, moved};
      for (int i = 0; i < 2; ++i) {
        if (!stat[i]) continue;
        double x = all_finite ? value[i] : nan;
        if (a.accumulate) { const double before = stat[i][sample]; x = (before != before || x != x) ? nan : fmax(before, x); }
        stat[i][sample] = x;
      }
    }
  } else if (lane == 0) a.sq[sample] = all_finite ? sq : nan;
}

template <int NV, bool FLOATING, bool UPDATE>
void launchAl(const RbdAlArgs& a, int n, hipStream_t st) {
  hipLaunchKernelGGL((rbd_al_kernel<NV, FLOATING, UPDATE>), dim3((unsigned)((n + RBD_WAVES - 1) / RBD_WAVES)), dim3(64 * RBD_WAVES), 0, st, a, n);
}

template <bool UPDATE>
bool rbdAl(int nv, bool quadruped, const RbdAlArgs& a, int n, hipStream_t st) {
  if (quadruped) { launchAl<LeggedDims<4, 3>::NV, true, UPDATE>(a, n, st); return true; }
  switch (nv) {
    case 2: launchAl<2, false, UPDATE>(a, n, st); break;
    case 3: launchAl<3, false, UPDATE>(a, n, st); break;
    case 4: launchAl<4, false, UPDATE>(a, n, st); break;
    case 5: launchAl<5, false, UPDATE>(a, n, st); break;
    case 6: launchAl<6, false, UPDATE>(a, n, st); break;
    case 7: launchAl<7, false, UPDATE>(a, n, st); break;
    case 8: launchAl<8, false, UPDATE>(a, n, st); break;
    default: return false;
  }
  return true;
}

}  // namespace

bool rbdAlScore(int nv, bool quadruped, const RbdAlArgs& a, int n, hipStream_t st) { return rbdAl<false>(nv, quadruped, a, n, st); }
bool rbdAlUpdate(int nv, bool quadruped, const RbdAlArgs& a, int n, hipStream_t st) { return rbdAl<true>(nv, quadruped, a, n, st); }

}  // namespace idocp_dev
