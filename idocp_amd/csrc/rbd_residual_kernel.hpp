// The kernel template of rbd_residual_kernel.hip, rbd_residual_penalty_kernel.hip and rbd_residual_al_kernel.hip (their heads have the method).  It
// lives in a header so that each form is instantiated in a translation unit of its own: the code of the cost form does not depend on whether the
// penalty form is built beside it, nor that of the penalty form on the augmented-Lagrangian form.
#ifndef IDOCP_RBD_RESIDUAL_KERNEL_HPP_
#define IDOCP_RBD_RESIDUAL_KERNEL_HPP_

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

constexpr int THREADS = RBD_RESIDUAL_THREADS;

template <int NV, int NF, int NU, int S>
struct RbdResidualLds {
  static constexpr int NX = 2 * NV, NZ = NX + NU, R = (NV + NF + 3) / 4 * 4;
  static constexpr int LDA = NV | 1, LDF = NF | 1;
  double Da[S][NZ * LDA];
  double Df[S][NF ? NZ * LDF : 1];
  double a[S][NV], f[S][NF ? NF : 1], rho[S][R];
  double table[2 * R];
  int bad[S];
};

// What the penalty form keeps besides: per (sample, constraint row) sigma and the three coefficients of the row on the block rows it combines
// (an acceleration row: one coefficient; a cone row: s [active] times the gradient of g in (fx, fy, fz)), and per (sample, column) the signed
// box value b of the column's own quantity.  RCM: the most constraint rows, roundup4(NU + 5 NF / 3).
template <int NF, int NU, int NZ, int S>
struct RbdResidualPenaltyLds {
  static constexpr int RCM = (NU + 5 * (NF / 3) + 3) / 4 * 4;
  double sigma[S][RCM];
  double w[S][RCM][3];
  double b[S][NZ];
};

// the one LDS instance of T of the workgroup (the penalty form reaches its extra arrays through this, so the cost form declares nothing more)
template <class T>
__device__ __forceinline__ T& residualShared() { __shared__ T x; return x; }

// the doubles [0, total) of src, two per lane and load where a pair is whole; put(e, x) takes entry e
template <typename Put>
__device__ __forceinline__ void residualLoadRun(const double* __restrict__ src, int total, int tid, Put put) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  for (int e = 2 * tid; e < total; e += 2 * THREADS) {
    if (e + 1 < total) { const d2 x = *reinterpret_cast<const d2*>(src + e); put(e, x.x); put(e + 1, x.y); }
    else put(e, src[e]);
  }
}

// Args = RbdResidualArgs: the cost rows at the head of rbd_residual_kernel.hip.  Args = RbdResidualPenaltyArgs (idocp_rbd_linearize_rollout_penalty):
// the same blocks in LDS also give the constraint rows behind the cost rows, the diagonal D and the gradient of the merit.  Args = RbdResidualAlArgs
// (idocp_rbd_linearize_rollout_al): the penalty form with every constraint row taken at its shifted value x + lambda / mu, g + lambda / mu; a
// multiplier is read once, by the lane that forms its row, straight from global memory -- no LDS beyond the penalty form's.
template <int NV, int NF, int NU, int S, class Args = RbdResidualArgs>
__global__ __launch_bounds__(THREADS) void rbd_residual_kernel(Args a) {
  using Lds = RbdResidualLds<NV, NF, NU, S>;
  typedef double d2 __attribute__((ext_vector_type(2)));
  constexpr bool AL = std::is_same<Args, RbdResidualAlArgs>::value;
  constexpr bool PEN = std::is_same<Args, RbdResidualPenaltyArgs>::value || AL;
  constexpr int NX = Lds::NX, NZ = Lds::NZ, R = Lds::R, LDA = Lds::LDA, LDF = Lds::LDF;
  static_assert(S % 2 == 0 && (R * NZ) % 2 == 0, "the runs of a workgroup start at an even number of doubles");
  __shared__ Lds L;
  const int tid = threadIdx.x;
  const size_t s0 = (size_t)blockIdx.x * S;
  const int cnt = a.count - (int)s0 < S ? a.count - (int)s0 : S;      // >= 1 by the size of the grid
  const int mask = a.mask;

  if (tid < S) L.bad[tid] = 0;
  if (tid < 2 * R) L.table[tid] = a.table[tid];
  __syncthreads();

  // ---- 1. the runs of the inputs
  auto flag = [&](int sample, double x) { if (!std::isfinite(x)) L.bad[sample] = 1; };
  residualLoadRun(a.a + s0 * NV, cnt * NV, tid, [&](int e, double x) { const int s = e / NV; L.a[s][e - s * NV] = x; flag(s, x); });
  auto block = [&](const double* src, int rows, int cols, int ld, int col0, bool forces) {
    const int size = rows * cols;
    residualLoadRun(src + s0 * size, cnt * size, tid, [&](int e, double x) {
      const int s = e / size, i = e - s * size, c = i / rows, r = i - c * rows;
      if (forces) L.Df[s][(col0 + c) * ld + r] = x; else L.Da[s][(col0 + c) * ld + r] = x;
      flag(s, x);
    });
  };
  block(a.da_dq, NV, NV, LDA, 0, false);
  block(a.da_dv, NV, NV, LDA, NV, false);
  block(a.da_du, NV, NU, LDA, NX, false);
  if (NF) {
    residualLoadRun(a.f + s0 * NF, cnt * NF, tid, [&](int e, double x) { const int s = e / NF; L.f[s][e - s * NF] = x; flag(s, x); });
    block(a.df_dq, NF, NV, LDF, 0, true);
    block(a.df_dv, NF, NV, LDF, NV, true);
    block(a.df_du, NF, NU, LDF, NX, true);
  }
  if constexpr (PEN) {
    // the signed box value of every column's own quantity: q, v, u of the actuated joints where their limits are switched on
    auto& P = residualShared<RbdResidualPenaltyLds<NF, NU, NZ, S>>();
    const idocp_host::RbdScoreBlock& W = *a.block;
    constexpr int NQ = NF ? NV + 1 : NV;
    for (int t = tid; t < cnt * NZ; t += THREADS) {
      const int s = t / NZ, c = t - s * NZ;
      const int kind = c < NV ? 0 : (c < NX ? 1 : 2), j = kind == 0 ? c - (NV - NU) : (kind == 1 ? c - NV - (NV - NU) : c - NX);
      double b = 0.0;
      if (j >= 0) {
        const bool on = kind == 0 ? W.position_limits : (kind == 1 ? W.velocity_limits : W.torque_limits);
        const double* src = kind == 0 ? a.q : (kind == 1 ? a.v : a.u);
        if (on && src) {
          const double x = kind == 0 ? src[(s0 + s) * NQ + (NQ - NU) + j] : (kind == 1 ? src[(s0 + s) * NV + (NV - NU) + j] : src[(s0 + s) * NU + j]);
          const double lo = kind == 0 ? W.q_min[j] : (kind == 1 ? -W.v_max[j] : -W.u_max[j]);
          const double hi = kind == 0 ? W.q_max[j] : (kind == 1 ? W.v_max[j] : W.u_max[j]);
          flag(s, x);
          if constexpr (AL) {
            // the multiplier row kind * NU + j of the sample shifts the value: the quotient rounded, then the sum
            if (a.lambda) {
#pragma clang fp contract(off)
              const int rows = 4 * NU + (NF ? (W.cone == 1 ? 5 : (W.cone == 2 ? 2 : 0)) * (NF / 3) : 0);
              const double l = a.lambda[(s0 + s) * (size_t)rows + kind * NU + j];
              flag(s, l);
              const double y = x + l / a.penalty;
              b = (y - hi > 0.0 ? y - hi : 0.0) - (lo - y > 0.0 ? lo - y : 0.0);
            } else {
              b = (x - hi > 0.0 ? x - hi : 0.0) - (lo - x > 0.0 ? lo - x : 0.0);
            }
          } else {
            b = (x - hi > 0.0 ? x - hi : 0.0) - (lo - x > 0.0 ? lo - x : 0.0);
          }
        }
      }
      P.b[s][c] = b;
    }
  }
  __syncthreads();

  // row r of the rows in use: a force row of an inactive contact and a padding row are not
  auto live = [&](int r) { return r < NV || (r < NV + NF && ((mask >> ((r - NV) / 3)) & 1)); };

  // ---- 2. rho
  for (int t = tid; t < cnt * R; t += THREADS) {
    const int s = t / R, r = t - s * R;
    double v = 0.0;
    if (r < NV) v = L.table[r] * L.a[s][r];
    else if (live(r)) { const double d = L.f[s][r - NV] - L.table[R + r]; v = L.table[r] * d; }
    L.rho[s][r] = v;
  }
  if constexpr (PEN) {
    // sigma and the coefficients of the constraint rows
    auto& P = residualShared<RbdResidualPenaltyLds<NF, NU, NZ, S>>();
    const idocp_host::RbdScoreBlock& W = *a.block;
    const double sc = a.scale;
    const int cone = NF ? W.cone : 0, ncone = cone == 1 ? 5 : (cone == 2 ? 2 : 0);
    const double mu = W.mu, m = mu * 0.70710678118654752440;
    // (AL) lambda / mu of multiplier row `row` of sample s; a non-finite multiplier flags the sample -- the barrier below stands before the stores
    auto shift = [&](int s, int row) {
#pragma clang fp contract(off)
      double q = 0.0;
      if constexpr (AL) {
        if (a.lambda) { const double l = a.lambda[(s0 + s) * (size_t)(4 * NU + ncone * (NF / 3)) + row]; flag(s, l); q = l / a.penalty; }
      }
      return q;
    };
    for (int t = tid; t < cnt * a.rc; t += THREADS) {
      const int s = t / a.rc, r = t - s * a.rc;
      double g = 0.0, w0 = 0.0, w1 = 0.0, w2 = 0.0;
      if (r < NU) {
        double x = L.a[s][NV - NU + r];
        if constexpr (AL) {
#pragma clang fp contract(off)
          if (W.acceleration_upper || W.acceleration_lower) x = x + shift(s, 3 * NU + r);
        }
        g = (W.acceleration_upper && x - W.a_max[r] > 0.0 ? x - W.a_max[r] : 0.0) - (W.acceleration_lower && W.a_min[r] - x > 0.0 ? W.a_min[r] - x : 0.0);
        w0 = g != 0.0 ? sc : 0.0;      // (the signed row: its gradient is that of x on either side)
      } else if (NF && r < NU + ncone * (NF / 3)) {
        const int c = (r - NU) / ncone, i = (r - NU) - c * ncone;
        if ((mask >> c) & 1) {
          const double fx = L.f[s][3 * c], fy = L.f[s][3 * c + 1], fz = L.f[s][3 * c + 2];
          double j0, j1, j2;
          if (i == 0) { g = -fz; j0 = 0.0; j1 = 0.0; j2 = -1.0; }
          else if (cone == 1) {
            j0 = i == 1 ? 1.0 : (i == 2 ? -1.0 : 0.0); j1 = i == 3 ? 1.0 : (i == 4 ? -1.0 : 0.0); j2 = -m;
            g = (i < 3 ? j0 * fx : j1 * fy) - m * fz;
          } else { g = fx * fx + fy * fy - mu * mu * fz * fz; j0 = 2.0 * fx; j1 = 2.0 * fy; j2 = -2.0 * (mu * mu) * fz; }
          if constexpr (AL) {
#pragma clang fp contract(off)
            g = g + shift(s, 4 * NU + ncone * c + i);
          }
          if (g > 0.0) { w0 = sc * j0; w1 = sc * j1; w2 = sc * j2; } else g = 0.0;
        }
      }
      P.sigma[s][r] = sc * g;
      P.w[s][r][0] = w0; P.w[s][r][1] = w1; P.w[s][r][2] = w2;
    }
  }
  __syncthreads();

  const double nan = __builtin_nan("");
  // entry (r, c) of sample s: ONE rounded product
  auto entry = [&](int s, int r, int c) {
    if (r < NV) return L.table[r] * L.Da[s][c * LDA + r];
    if (live(r)) return L.table[r] * L.Df[s][c * LDF + (r - NV)];
    return 0.0;
  };

  if constexpr (PEN) {
    auto& P = residualShared<RbdResidualPenaltyLds<NF, NU, NZ, S>>();
    // entry (r, c) of the constraint rows: the coefficient times the block row, a cone row the three products summed by fused multiply-adds
    auto centry = [&](int s, int r, int c) {
      if (r < NU) return P.w[s][r][0] * L.Da[s][c * LDA + (NV - NU + r)];
      if constexpr (NF > 0) {
        const int ncone = (*a.block).cone == 1 ? 5 : 2, fc = (r - NU) / ncone;
        if (fc < NF / 3) {
          const double* d = &L.Df[s][c * LDF + 3 * fc];
          return __builtin_fma(P.w[s][r][2], d[2], __builtin_fma(P.w[s][r][1], d[1], P.w[s][r][0] * d[0]));
        }
      }
      return 0.0;
    };
    const int RT = R + a.rc;      // rows of G per sample: the cost rows, the constraint rows behind them
    // ---- 3. the run of G, both kinds of rows
    if (a.G) {
      double* __restrict__ G = a.G + s0 * ((size_t)RT * NZ);
      const bool wide = (reinterpret_cast<uintptr_t>(a.G) & 15u) == 0;
      for (int e = 2 * tid; e < cnt * RT * NZ; e += 2 * THREADS) {
        const int s = e / (RT * NZ), i = e - s * (RT * NZ);
        const int r0 = i / NZ, c0 = i - r0 * NZ;
        const int r1 = (i + 1) / NZ, c1 = (i + 1) - r1 * NZ;
        d2 v;
        v.x = L.bad[s] ? nan : (r0 < R ? entry(s, r0, c0) : centry(s, r0 - R, c0));
        v.y = L.bad[s] ? nan : (r1 < R ? entry(s, r1, c1) : centry(s, r1 - R, c1));
        if (wide) *reinterpret_cast<d2*>(G + e) = v; else { G[e] = v.x; G[e + 1] = v.y; }
      }
    }
    if (a.rho) {
      double* __restrict__ rho = a.rho + s0 * RT;
      for (int t = tid; t < cnt * RT; t += THREADS) {
        const int s = t / RT, r = t - s * RT;
        rho[t] = L.bad[s] ? nan : (r < R ? L.rho[s][r] : P.sigma[s][r - R]);
      }
    }
    // ---- 4. G^T rho over the cost rows, then over the constraint rows, on top of the diagonal part; D and the diagonal gradient
    for (int t = tid; t < cnt * NZ; t += THREADS) {
      const int s = t / NZ, c = t - s * NZ;
      double acc = 0.0;
      for (int r = 0; r < NV + NF; ++r)
        if (live(r)) acc = __builtin_fma(entry(s, r, c), L.rho[s][r], acc);
      for (int r = 0; r < a.rc; ++r) acc = __builtin_fma(centry(s, r, c), P.sigma[s][r], acc);
      const double b = P.b[s][c];
      double* const out = c < NX ? (a.lx ? a.lx + (s0 + s) * NX + c : nullptr) : (a.lu ? a.lu + (s0 + s) * NU + (c - NX) : nullptr);
      if (out) { const double d = *out; *out = L.bad[s] ? nan : (d + acc) + a.dtmu * b; }
      if (a.D) a.D[(s0 + s) * NZ + c] = L.bad[s] ? nan : (b != 0.0 ? a.dtmu : 0.0);
    }
  } else {
    // ---- 3. the run of G
    if (a.G) {
      double* __restrict__ G = a.G + s0 * (R * NZ);
      const bool wide = (reinterpret_cast<uintptr_t>(a.G) & 15u) == 0;
      for (int e = 2 * tid; e < cnt * R * NZ; e += 2 * THREADS) {
        const int s = e / (R * NZ), i = e - s * (R * NZ);
        const int r0 = i / NZ, c0 = i - r0 * NZ;
        const int r1 = (i + 1) / NZ, c1 = (i + 1) - r1 * NZ;
        d2 v;
        v.x = L.bad[s] ? nan : entry(s, r0, c0);
        v.y = L.bad[s] ? nan : entry(s, r1, c1);
        if (wide) *reinterpret_cast<d2*>(G + e) = v; else { G[e] = v.x; G[e + 1] = v.y; }
      }
    }
    if (a.rho) {
      double* __restrict__ rho = a.rho + s0 * R;
      for (int t = tid; t < cnt * R; t += THREADS) { const int s = t / R; rho[t] = L.bad[s] ? nan : L.rho[s][t - s * R]; }
    }

    // ---- 4. G^T rho on top of the diagonal part
    if (a.lx || a.lu) {
      for (int t = tid; t < cnt * NZ; t += THREADS) {
        const int s = t / NZ, c = t - s * NZ;
        double acc = 0.0;
        for (int r = 0; r < NV + NF; ++r)
          if (live(r)) acc = __builtin_fma(entry(s, r, c), L.rho[s][r], acc);
        double* const out = c < NX ? (a.lx ? a.lx + (s0 + s) * NX + c : nullptr) : (a.lu ? a.lu + (s0 + s) * NU + (c - NX) : nullptr);
        if (out) { const double d = *out; *out = L.bad[s] ? nan : d + acc; }
      }
    }
  }
}

}  // namespace

}  // namespace idocp_dev
#endif  // IDOCP_RBD_RESIDUAL_KERNEL_HPP_
