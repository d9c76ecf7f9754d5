// The time-varying affine feedback policy of the solvers on plain arrays (idocp_rbd_feedback_torques_batch, idocp_rbd_rollout_policy;
// include/idocp_hip.h):
//   u = clamp(u_ff + K [q (-) q_ref ; v - v_ref]),   K: nu x 2 nv column-major, columns [dq | dv]
// -- the layout idocp_ocp_get_riccati and getStateFeedbackGain ([Kq | Kv]) return.  q (-) q_ref is the tangent of
// idocp_model_subtract_configuration(q_plus = q, q_minus = q_ref): on a floating base the SE(3) log of the relative base placement (lieRelative,
// lieLog6 of dev_lie.hpp, the very functions that call runs on the host) in rows 0 .. 5, plain differences elsewhere.  An ADDITION like the forward
// dynamics: the reference only evaluates the inverse direction.
//
// One wavefront per sample, RBD_WAVES samples per workgroup, no workgroup barrier (a wavefront past the last sample leaves at once), like the
// other rbd kernels.  Lane c < 2 nv forms row c of the state difference; the SE(3) log runs on lane 0 and its six values reach the others through
// the wavefront's LDS slice.  The gain block is read ONCE, lane l on doubles l, l + 64, ... of the column-major block (coalesced), each entry
// multiplied by its column's difference and left in LDS; lane j < nu then adds row j in column order -- the same order whatever n is, so a
// sample's torques do not depend on the launch it is part of.  Per-sample and shared gains / references differ by a STRIDE argument alone
// (0 = shared), not by a code path.  The clamp is the last operation.  A non-finite input of a sample (q, v, the references, the gains, u_ff)
// makes all of that sample's torques NaN -- decided by a ballot over the wavefront, because min / max would turn a NaN into a bound.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dev_dense.hpp"
#include "dev_lie.hpp"
#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

template <int NV, bool FLOATING>
struct RbdPolicyLds {
  static constexpr int NQ = FLOATING ? NV + 1 : NV, NU = FLOATING ? NV - 6 : NV, NX = 2 * NV;
  double prod[NU * NX];         // K(j, c) dx(c), column-major like K
  double dx[NX];                // [q (-) q_ref ; v - v_ref]
};

template <int NV, bool FLOATING>
__global__ __launch_bounds__(64 * RBD_WAVES) void rbd_policy_kernel(RbdPolicyArgs a, int n) {
  using W = RbdPolicyLds<NV, FLOATING>;
  constexpr int NQ = W::NQ, NU = W::NU, NX = W::NX;
  static_assert(NX <= 64, "one lane per row of the state difference");
  __shared__ W s_wave[RBD_WAVES];
  const int lane = threadIdx.x & 63;
  const long sample = (long)blockIdx.x * RBD_WAVES + (threadIdx.x >> 6);
  if (sample >= n) return;                                // (no workgroup barrier below)
  W& L = s_wave[threadIdx.x >> 6];
  bool finite = true;
  double acc = 0.0;
  if (a.K) {
    const double* __restrict__ q = a.q + sample * NQ;
    const double* __restrict__ v = a.v + sample * NV;
    const double* __restrict__ qr = a.q_ref + sample * a.q_ref_stride;
    const double* __restrict__ vr = a.v_ref + sample * a.v_ref_stride;
    if (lane >= NV && lane < NX) {
      const double x = v[lane - NV], r = vr[lane - NV];
      finite = std::isfinite(x) && std::isfinite(r);
      L.dx[lane] = x - r;
    } else if (lane < NV && (!FLOATING || lane >= 6)) {
      const int iq = FLOATING ? lane + 1 : lane;
      const double x = q[iq], r = qr[iq];
      finite = std::isfinite(x) && std::isfinite(r);
      L.dx[lane] = x - r;
    }
    if (FLOATING && lane == 0) {
      double qm[7], qp[7], R[9], p[3], d[6];
#pragma unroll
      for (int i = 0; i < 7; ++i) { qm[i] = qr[i]; qp[i] = q[i]; finite = finite && std::isfinite(qm[i]) && std::isfinite(qp[i]); }
      lieRelative(qm, qp, R, p);
      lieLog6(R, p, d);
#pragma unroll
      for (int i = 0; i < 6; ++i) L.dx[i] = d[i];
    }
    waveLdsSync();
    const double* __restrict__ Ks = a.K + sample * a.k_stride;
    for (int e = lane; e < NU * NX; e += 64) {
      const double k = Ks[e];
      finite = finite && std::isfinite(k);
      L.prod[e] = k * L.dx[e / NU];
    }
    waveLdsSync();
    if (lane < NU) {
#pragma unroll
      for (int c = 0; c < NX; ++c) acc += L.prod[lane + NU * c];
    }
  }
  double ff = 0.0;
  if (lane < NU && a.u_ff) {
    ff = a.u_ff[sample * NU + lane];
    finite = finite && std::isfinite(ff);
  }
  const bool all_finite = __ballot(!finite) == 0;
  if (lane < NU) {
    double u = ff + acc;
    if (a.u_min) { const double lo = a.u_min[lane]; u = u < lo ? lo : u; }
    if (a.u_max) { const double hi = a.u_max[lane]; u = u > hi ? hi : u; }
    a.u[sample * NU + lane] = all_finite ? u : __builtin_nan("");
  }
}

template <int NV, bool FLOATING>
void launchPolicy(const RbdPolicyArgs& a, int n, hipStream_t st) {
  hipLaunchKernelGGL((rbd_policy_kernel<NV, FLOATING>), dim3((unsigned)((n + RBD_WAVES - 1) / RBD_WAVES)), dim3(64 * RBD_WAVES), 0, st, a, n);
}

}  // namespace

void rbdPolicy(int nv, bool quadruped, const RbdPolicyArgs& a, int n, hipStream_t st) {
  if (quadruped) { launchPolicy<LeggedDims<4, 3>::NV, true>(a, n, st); return; }
  switch (nv) {
    case 2: launchPolicy<2, false>(a, n, st); break;
    case 3: launchPolicy<3, false>(a, n, st); break;
    case 4: launchPolicy<4, false>(a, n, st); break;
    case 5: launchPolicy<5, false>(a, n, st); break;
    case 6: launchPolicy<6, false>(a, n, st); break;
    case 7: launchPolicy<7, false>(a, n, st); break;
    case 8: launchPolicy<8, false>(a, n, st); break;
    default: break;
  }
}

}  // namespace idocp_dev
