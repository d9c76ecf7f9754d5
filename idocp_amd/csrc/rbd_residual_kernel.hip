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
// aligned takes 8-byte stores (a uniform branch).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

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

// the doubles [0, total) of src, two per lane and load where a pair is whole; put(e, x) takes entry e
template <typename Put>
__device__ __forceinline__ void residualLoadRun(const double* __restrict__ src, int total, int tid, Put put) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  for (int e = 2 * tid; e < total; e += 2 * THREADS) {
    if (e + 1 < total) { const d2 x = *reinterpret_cast<const d2*>(src + e); put(e, x.x); put(e + 1, x.y); }
    else put(e, src[e]);
  }
}

template <int NV, int NF, int NU, int S>
__global__ __launch_bounds__(THREADS) void rbd_residual_kernel(RbdResidualArgs a) {
  using Lds = RbdResidualLds<NV, NF, NU, S>;
  typedef double d2 __attribute__((ext_vector_type(2)));
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
  __syncthreads();

  const double nan = __builtin_nan("");
  // entry (r, c) of sample s: ONE rounded product
  auto entry = [&](int s, int r, int c) {
    if (r < NV) return L.table[r] * L.Da[s][c * LDA + r];
    if (live(r)) return L.table[r] * L.Df[s][c * LDF + (r - NV)];
    return 0.0;
  };

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
