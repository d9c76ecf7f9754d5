// The line-search step of iLQR on plain arrays (idocp_rbd_ilqr_step_torques, idocp_rbd_ilqr_accept; include/idocp_hip.h has the rules).  ADDITIONS:
// the reference has no counterpart.  Both kernels are bandwidth work on the step-major arrays of the rollouts.
//
// Step torques: u_ff = u + alpha[i] k, one 16-byte piece (two doubles of one sample, nu even and the pointers aligned) or one double per lane,
// contiguous over the lanes.  The product is rounded before the sum (no contraction into a fused multiply-add), and alpha[i] == 0 selects u itself.
//
// Accept: a workgroup owns RBD_ILQR_GROUP consecutive samples.  Its first lanes decide them -- every value a decision reads is read before the
// barrier, every value it writes is written behind it, and no other workgroup touches these samples --, then all lanes walk the arrays slice by
// slice: the group's part of a slice is ONE contiguous run of RBD_ILQR_GROUP * width doubles, copied in 16-byte pieces where both doubles of a piece
// belong to accepted samples, as single doubles at the edges of an accepted sample.  Nothing of a rejected or finished sample is written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

__global__ __launch_bounds__(256) void rbd_ilqr_step_kernel(const double* __restrict__ u, const double* __restrict__ k, const double* __restrict__ alpha,
                                                            double* __restrict__ out, int n, int nu, long long count, int wide) {
#pragma clang fp contract(off)
  const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
  if (wide) {      // nu even: the two doubles of a piece belong to one sample
    if (2 * at >= count) return;
    const int i = (int)((2 * at / nu) % n);
    const double al = alpha[i];
    const double2 uu = reinterpret_cast<const double2*>(u)[at], kk = reinterpret_cast<const double2*>(k)[at];
    double2 r;
    r.x = al == 0.0 ? uu.x : uu.x + al * kk.x;
    r.y = al == 0.0 ? uu.y : uu.y + al * kk.y;
    reinterpret_cast<double2*>(out)[at] = r;
  } else {
    if (at >= count) return;
    const int i = (int)((at / nu) % n);
    const double al = alpha[i];
    out[at] = al == 0.0 ? u[at] : u[at] + al * k[at];
  }
}

// the doubles of `dst` the group owns in one slice, [lo, lo + len), from `src` where the owning sample was accepted; width doubles per sample.
// wide: both pointers are 16-byte aligned, so an even index is a 16-byte boundary
__device__ __forceinline__ void copyAccepted(double* __restrict__ dst, const double* __restrict__ src, size_t lo, int len, int width, const int* accepted,
                                             bool wide, int tid) {
  if (!wide) {
    for (int e = tid; e < len; e += 256) if (accepted[e / width]) dst[lo + e] = src[lo + e];
    return;
  }
  const int head = (int)(lo & 1);                          // a leading double in front of the first 16-byte boundary
  if (tid == 0 && head && accepted[0]) dst[lo] = src[lo];
  const int pairs = (len - head) / 2;
  for (int p = tid; p < pairs; p += 256) {
    const int e = head + 2 * p;
    const bool a0 = accepted[e / width], a1 = accepted[(e + 1) / width];
    if (a0 && a1) *reinterpret_cast<double2*>(dst + lo + e) = *reinterpret_cast<const double2*>(src + lo + e);
    else if (a0) dst[lo + e] = src[lo + e];
    else if (a1) dst[lo + e + 1] = src[lo + e + 1];
  }
  const int tail = head + 2 * pairs;
  if (tid == 0 && tail < len && accepted[tail / width]) dst[lo + tail] = src[lo + tail];
}

__global__ __launch_bounds__(256) void rbd_ilqr_accept_kernel(RbdIlqrAcceptArgs a) {
#pragma clang fp contract(off)
  constexpr int G = RBD_ILQR_GROUP;
  __shared__ int s_accepted[G];
  const int tid = threadIdx.x, i0 = (int)blockIdx.x * G;
  const int group = a.n - i0 < G ? a.n - i0 : G;
  if (tid < G) {
    bool accept = false;
    const int i = i0 + tid;
    if (tid < group && a.done[i] == 0) {
      const double c = a.cost[i], g = a.violation[i], ct = a.trial_cost[i], gt = a.trial_violation[i], al = a.alpha[i];
      const double e0 = a.expected[2 * (size_t)i], e1 = a.expected[2 * (size_t)i + 1];
      const double merit = c + a.penalty * g, merit_trial = ct + a.penalty * gt;
      accept = std::isfinite(ct) && std::isfinite(gt) && merit_trial <= merit + a.armijo * (al * e0 + (al * al) * e1);
      if (accept) {
        a.cost[i] = ct; a.violation[i] = gt; a.done[i] = 1; a.alpha_accepted[i] = al;
      } else {
        double next = al * a.shrink;
        if (next < a.alpha_min) next = 0.0;
        a.alpha[i] = next;
      }
    }
    s_accepted[tid] = accept;
  }
  __syncthreads();
  bool any = false;
  for (int s = 0; s < group; ++s) any = any || s_accepted[s];
  if (!any) return;
  const size_t N = (size_t)a.n;
  for (int c = 0; c < 5; ++c) {
    if (!a.dst[c] || !a.src[c] || !a.width[c]) continue;
    const int w = a.width[c], slices = a.steps + (c < 2 ? 1 : 0);      // q, v carry the slice behind the last step
    const bool wide = (a.wide >> c) & 1;
    for (int k = 0; k < slices; ++k) copyAccepted(a.dst[c], a.src[c], ((size_t)k * N + i0) * w, group * w, w, s_accepted, wide, tid);
  }
}

__global__ __launch_bounds__(256) void rbd_ilqr_init_kernel(double* __restrict__ alpha, int* __restrict__ done, double* __restrict__ alpha_accepted, int n) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { alpha[i] = 1.0; done[i] = 0; alpha_accepted[i] = 0.0; }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

void rbdIlqrStepTorques(const double* u, const double* k, const double* alpha, double* out, int n, int steps, int nu, hipStream_t st) {
  const long long count = (long long)steps * n * nu;
  const int wide = nu % 2 == 0 && aligned16(u) && aligned16(k) && aligned16(out);
  const long long pieces = wide ? count / 2 : count;
  hipLaunchKernelGGL(rbd_ilqr_step_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, u, k, alpha, out, n, nu, count, wide);
}

void rbdIlqrAccept(RbdIlqrAcceptArgs a, hipStream_t st) {
  a.wide = 0;
  for (int c = 0; c < 5; ++c) if (aligned16(a.dst[c]) && aligned16(a.src[c])) a.wide |= 1 << c;
  hipLaunchKernelGGL(rbd_ilqr_accept_kernel, dim3((unsigned)((a.n + RBD_ILQR_GROUP - 1) / RBD_ILQR_GROUP)), dim3(256), 0, st, a);
}

void rbdIlqrInit(double* alpha, int* done, double* alpha_accepted, int n, hipStream_t st) {
  hipLaunchKernelGGL(rbd_ilqr_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, alpha, done, alpha_accepted, n);
}

}  // namespace idocp_dev
