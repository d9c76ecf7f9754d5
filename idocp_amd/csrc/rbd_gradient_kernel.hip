// Gradients of an objective along a rollout (idocp_rbd_objective_gradients; include/idocp_hip.h has the definition): per slice k and sample i
//   lx[0:nv] = s J^T (wq o e),  lx[nv:2nv] = s wv o (v - v_ref_k),  lu = dt wu o (u - u_ref),
// e = q (-) q_ref(t_k), s = dt with the stage weights, s = 1 with the terminal weights on the terminal slice; J is Jlog6 of the relative base
// placement on the six base rows of the quadruped and the identity elsewhere.  An ADDITION: the reference forms this product for the solver's own
// iterate only (configuration_space_cost.cpp:292-328, lq += dt J^T W diff with Robot::dSubtractdConfigurationPlus).
//
// An item is one (slice, sample) pair; the items are independent.  Because the arrays are step-major, item t = k n + i owns the doubles
// [t NQ, (t + 1) NQ) of q, [t NV, ..) of v, [t NU, ..) of u (stage slices only) and writes [t 2NV, ..) of lx and [t NU, ..) of lu: a RUN of consecutive
// items is a contiguous run of every array, across sample and slice boundaries alike.  One wavefront (one workgroup) takes RBD_GRADIENT_ITEMS = 64
// consecutive items:
//   1. the runs of q, v and u go into LDS, lane l loading the doubles l, l + 64, ... of each run (contiguous over the lanes), and every lane that
//      meets a non-finite entry raises the flag of the item it belongs to;
//   2. lane l takes item l: its slice index k = t / n, and on the quadruped the ONE logarithm and the ONE Jlog6 of the item -- lieRelative, lieLog6
//      (the functions the score kernel runs) and lieJlog6 of dev_lie.hpp -- and g = J^T (w o e) over the six base rows, summed over the rows in
//      index order; g goes to LDS;
//   3. the runs of lx and lu are written, lane l storing the doubles l, l + 64, ... of each run: a base row takes g, every other row is one
//      subtraction and two products from LDS; a flagged item stores NaN.
// No atomics, no scratch; the weights travel through LDS once per workgroup.  The LDS reads of step 2 walk items NQ = 19 doubles apart: with
// ds_read_b64 the 32 lanes of a half hit 32 different even banks.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dev_lie.hpp"
#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

constexpr int ITEMS = RBD_GRADIENT_ITEMS;

template <int NV, bool FLOATING>
struct RbdGradientLds {
  static constexpr int NQ = FLOATING ? NV + 1 : NV, NU = FLOATING ? NV - 6 : NV;
  double q[ITEMS * NQ], v[ITEMS * NV], u[ITEMS * NU];
  double g[FLOATING ? ITEMS * 6 : 1];
  double wq[NV], wv[NV], wqf[NV], wvf[NV], wu[NU], uref[NU];
  int k[ITEMS], bad[ITEMS];
};

template <int NV, bool FLOATING>
__global__ __launch_bounds__(64) void rbd_gradient_kernel(RbdGradientArgs a) {
  using Lds = RbdGradientLds<NV, FLOATING>;
  constexpr int NQ = Lds::NQ, NU = Lds::NU, NX = 2 * NV;
  __shared__ Lds L;
  const int lane = threadIdx.x;
  const int total = (a.steps + (a.terminal ? 1 : 0)) * a.n, stage_items = a.steps * a.n;      // (fits an int: the planner refuses otherwise)
  const int t0 = (int)blockIdx.x * ITEMS;
  const int items = total - t0 < ITEMS ? total - t0 : ITEMS;                                    // >= 1 by the size of the grid
  const int u_items = stage_items - t0 < 0 ? 0 : (stage_items - t0 < items ? stage_items - t0 : items);
  const idocp_host::RbdScoreBlock& W = *a.block;
  const double dt = W.dt;

  // ---- 1. the runs of the inputs, the weights
  L.bad[lane] = 0;
  if (lane < NV) { L.wq[lane] = W.q_weight[lane]; L.wv[lane] = W.v_weight[lane]; L.wqf[lane] = W.qf_weight[lane]; L.wvf[lane] = W.vf_weight[lane]; }
  if (lane < NU) { L.wu[lane] = W.u_weight[lane]; L.uref[lane] = W.u_ref[lane]; }
  __syncthreads();
  {
    const double* __restrict__ q = a.q + (size_t)t0 * NQ;
#pragma unroll
    for (int m = 0; m < NQ; ++m) {
      const int j = lane + 64 * m;
      if (j < items * NQ) { const double x = q[j]; L.q[j] = x; if (!std::isfinite(x)) L.bad[j / NQ] = 1; }
    }
    const double* __restrict__ v = a.v + (size_t)t0 * NV;
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int j = lane + 64 * m;
      if (j < items * NV) { const double x = v[j]; L.v[j] = x; if (!std::isfinite(x)) L.bad[j / NV] = 1; }
    }
    if (a.u) {
      const double* __restrict__ u = a.u + (size_t)t0 * NU;
#pragma unroll
      for (int m = 0; m < NU; ++m) {
        const int j = lane + 64 * m;
        if (j < u_items * NU) { const double x = u[j]; L.u[j] = x; if (!std::isfinite(x)) L.bad[j / NU] = 1; }
      }
    }
  }
  __syncthreads();

  // ---- 2. one item per lane: its slice, and the base rows of the quadruped
  if (lane < items) {
    const int k = (t0 + lane) / a.n;
    L.k[lane] = k;
    if (FLOATING && a.lx) {
      const bool term = k == a.steps;
      const double* __restrict__ qr = a.q_ref + (size_t)k * NQ;
      double qm[7], qp[7], R[9], p[3], e[6], J[36];
#pragma unroll
      for (int i = 0; i < 7; ++i) { qm[i] = qr[i]; qp[i] = L.q[lane * NQ + i]; }
      lieRelative(qm, qp, R, p);
      lieLog6(R, p, e);
      lieJlog6(R, p, J);
#pragma unroll
      for (int r = 0; r < 6; ++r) e[r] = (term ? L.wqf[r] : L.wq[r]) * e[r];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) acc += J[r + 6 * c] * e[r];      // (J^T (W e))[c], the rows in index order
        L.g[lane * 6 + c] = acc;
      }
    }
  }
  __syncthreads();

  // ---- 3. the runs of the outputs
  const double nan = __builtin_nan("");
  if (a.lx) {
    double* __restrict__ lx = a.lx + (size_t)t0 * NX;
#pragma unroll 4
    for (int m = 0; m < NX; ++m) {
      const int j = lane + 64 * m;
      if (j < items * NX) {
        const int item = j / NX, r = j - item * NX, k = L.k[item];
        const bool term = k == a.steps;
        const double s = term ? 1.0 : dt;
        double val;
        if (FLOATING && r < 6) {
          val = s * L.g[item * 6 + r];
        } else if (r < NV) {
          const int iq = FLOATING ? r + 1 : r;
          val = s * ((term ? L.wqf[r] : L.wq[r]) * (L.q[item * NQ + iq] - a.q_ref[(size_t)k * NQ + iq]));
        } else {
          const int rv = r - NV;
          val = s * ((term ? L.wvf[rv] : L.wv[rv]) * (L.v[item * NV + rv] - a.v_ref[(size_t)k * NV + rv]));
        }
        lx[j] = L.bad[item] ? nan : val;
      }
    }
  }
  if (a.lu) {
    double* __restrict__ lu = a.lu + (size_t)t0 * NU;
#pragma unroll
    for (int m = 0; m < NU; ++m) {
      const int j = lane + 64 * m;
      if (j < u_items * NU) {
        const int item = j / NU, jj = j - item * NU;
        const double val = a.u ? dt * (L.wu[jj] * (L.u[j] - L.uref[jj])) : 0.0;
        lu[j] = L.bad[item] ? nan : val;
      }
    }
  }
}

template <int NV, bool FLOATING>
void launchGradient(const RbdGradientArgs& a, hipStream_t st) {
  const long long total = ((long long)a.steps + (a.terminal ? 1 : 0)) * a.n;
  hipLaunchKernelGGL((rbd_gradient_kernel<NV, FLOATING>), dim3((unsigned)((total + ITEMS - 1) / ITEMS)), dim3(64), 0, st, a);
}

}  // namespace

void rbdGradient(int nv, bool quadruped, const RbdGradientArgs& a, hipStream_t st) {
  if (quadruped) { launchGradient<LeggedDims<4, 3>::NV, true>(a, st); return; }
  switch (nv) {
    case 2: launchGradient<2, false>(a, st); break;
    case 3: launchGradient<3, false>(a, st); break;
    case 4: launchGradient<4, false>(a, st); break;
    case 5: launchGradient<5, false>(a, st); break;
    case 6: launchGradient<6, false>(a, st); break;
    case 7: launchGradient<7, false>(a, st); break;
    case 8: launchGradient<8, false>(a, st); break;
    default: break;
  }
}

}  // namespace idocp_dev
