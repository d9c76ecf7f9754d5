// Derivatives of the batched forward dynamics and the linearised Euler step (idocp_rbd_forward_dynamics_derivatives_batch; include/idocp_hip.h):
// an addition the reference does not have.  A COMPOSITION of the kernels that are already held to independent answers: rbd_forward_kernel gives the
// forward solution (a, f), rbd_batch_kernel at (q, v, a, f) gives dID/d(q, v), dC/d(q, v) and MJtJinv = [M J^T; J 0]^-1 into scratch the handle
// owns, and the kernel here reads that scratch and forms, over the packed nv + dimf active rows,
//   d[a; -f]/dtheta = -MJtJinv [dID/dtheta ; dC/dtheta]   (theta = q in the tangent q (+) eps e_r, or v),     d[a; -f]/du = MJtJinv[:, 6 : nv]
// with ONE correction: dC/dtheta of the inverse call is the reference's formula, which is not the derivative of C in the term of w x v_lin (see the
// kernel); the difference, 2 skew(v_lin) dw of the LOCAL frame velocity, is taken off here by a velocity-only sweep of the active legs.  Then the
// Jacobians A, B of x_next = (q (+) dt v, v + dt a) on the tangent [dq; dv] (IMPULSE: of (q, v + dv)).  The top rows of A on the floating
// base are the two Jacobians of the retraction (dev_lie.hpp: lieDIntegrateArg0 of exp6(dt v), dt lieDIntegrateArg1(dt v)).
//
// Quadruped: one wavefront per sample, RBD_WAVES samples per workgroup, no workgroup barrier, like the two kernels in front of it.  The products
// are plain FMAs out of LDS in a fixed order of summation (k ascending); no atomics.  A sample whose forward solution or MJtJinv is not finite
// (M or J M^-1 J^T not positive definite, a non-finite input) gets NaN in every output.  Every value is computed whether or not its output was
// asked for, so a sample's bits depend on neither.
//
// Fixed-base chains: one lane per sample; M = dID/da from the chain sweep at (q, v, a), its Cholesky factor in registers, one solve per column.
#include <hip/hip_runtime.h>

#include "dev_dense.hpp"
#include "dev_lie.hpp"
#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

template <typename D>
struct RbdFddLds {
  static constexpr int NV = D::NV, NVF = D::NVF, NF = D::NF;
  static constexpr int LDC = NVF | 1;      // odd column stride, like the kernels in front
  double kinv[NVF * NVF];                  // MJtJinv, packed (nv + dimf)^2 column-major
  double rhs[2][NV][LDC];                  // theta = q, v; column c: rows [dID/dtheta (NV) ; dC/dtheta over the packed active rows (dimf)]
  double lie[2][36];                       // the base blocks of dq_next/dq and dq_next/dv (6 x 6 column-major)
  int prow[NF];                            // packed contact row -> row of the contact outputs
};

template <typename D, bool IMPULSE>
__global__ __launch_bounds__(64 * RBD_WAVES) void rbd_fd_derivatives_kernel(const DevModel* __restrict__ m, const RbdFrames* __restrict__ P, RbdFddArgs g, int n,
                                                                            int active_mask) {
  using W = RbdFddLds<D>;
  constexpr int NV = D::NV, NQ = D::NQ, NL = D::NL, LJ = D::LJ, NF = D::NF, NVF = D::NVF, NU = D::NU, NX = 2 * NV;
  __shared__ W s_wave[RBD_WAVES];
  const int lane = threadIdx.x & 63;
  const long sample = (long)blockIdx.x * RBD_WAVES + (threadIdx.x >> 6);
  if (sample >= n) return;                                // (no workgroup barrier below)
  W& L = s_wave[threadIdx.x >> 6];
  active_mask &= (1 << NL) - 1;
  const int dimf = 3 * __builtin_popcount(active_mask), np = NV + dimf;
  const double scale = IMPULSE ? 1.0 : g.dt;              // x_next's velocity: v + dt a, or v + dv
  if (lane == 0) {
    int row = 0;
    for (int c = 0; c < NL; ++c)
      if ((active_mask >> c) & 1) { L.prow[row] = 3 * c; L.prow[row + 1] = 3 * c + 1; L.prow[row + 2] = 3 * c + 2; row += 3; }
  }
  bool mine_bad = false;
  {
    const double* __restrict__ kin = g.MJtJinv + sample * (NVF * NVF);
    for (int e = lane; e < np * np; e += 64) { const double x = kin[e]; L.kinv[e] = x; mine_bad = mine_bad || !isfinite(x); }
    const double* __restrict__ dq = g.dtau_dq + sample * (NV * NV);
    const double* __restrict__ dv = g.dtau_dv + sample * (NV * NV);
    for (int e = lane; e < NV * NV; e += 64) { const int c = e / NV, r = e - c * NV; L.rhs[0][c][r] = dq[e]; L.rhs[1][c][r] = dv[e]; }
  }
  if (lane < NV) mine_bad = mine_bad || !isfinite(g.a[sample * NV + lane]);
  if (lane < NF) mine_bad = mine_bad || !isfinite(g.f[sample * NF + lane]);
  const bool bad = __ballot(mine_bad) != 0;
  waveLdsSync();
  {
    const double* __restrict__ cq = g.dCdq + sample * (NF * NV);
    const double* __restrict__ cv = g.dCdv + sample * (NF * NV);
    for (int e = lane; e < NV * dimf; e += 64) {
      const int c = e / dimf, i = e - c * dimf, src = c * NF + L.prow[i];
      L.rhs[0][c][NV + i] = cq[src]; L.rhs[1][c][NV + i] = cv[src];
    }
  }
  // (IMPULSE mode needs no such correction: its constraint is the LOCAL linear velocity itself, without a w x v_lin term)
  if (!IMPULSE && dimf > 0) {
    // dCdq and dCdv of the inverse call are the reference's (point_contact.hxx:117-143), which carry the term of w x v_lin as
    // +skew(v_lin) dw; the derivative of the residual has -skew(v_lin) dw there.  The forward solution moves with the TRUE derivative, so
    // 2 skew(v_lin) dw is taken off: v_lin, w the LOCAL velocity of the contact frame, dw its tangent along the seeds that reach it -- the
    // base's angular velocity and the leg's joint velocities (theta = v), the leg's joint angles (theta = q).  One velocity-only outward
    // sweep of the leg per seed, 9 seeds per leg, one round of the wavefront.
    waveLdsSync();
    typedef Dual T;
    const int leg = lane / 9, sd = lane - 9 * leg;
    if (leg < NL && ((active_mask >> leg) & 1)) {
      const int th = sd < 6 ? 1 : 0;
      const int k = sd < 3 ? 3 + sd : 6 + leg * LJ + (sd < 6 ? sd - 3 : sd - 6);      // velocity index of the seed
      const double* __restrict__ qs = g.q + sample * NQ;
      const double* __restrict__ vs = g.v + sample * NV;
      auto seedV = [&](int i) { return T(vs[i], (th == 1 && k == i) ? 1.0 : 0.0); };
      Vec3<T> v = mk<T>(seedV(0), seedV(1), seedV(2)), w = mk<T>(seedV(3), seedV(4), seedV(5));
#pragma unroll 1
      for (int j = 0; j < LJ; ++j) {
        const int ji = 1 + leg * LJ + j, dof = 6 + leg * LJ + j;
        const bool mine = (k == dof);
        double sj, cj;
        sincos(qs[1 + dof], &sj, &cj);
        const T cqi(cj, (mine && th == 0) ? -sj : 0.0), sqi(sj, (mine && th == 0) ? cj : 0.0);
        const T qdi(vs[dof], (mine && th == 1) ? 1.0 : 0.0);
        Mat3<T> R;
        revoluteRotation<T>(m->R[ji], m->axis[ji], cqi, sqi, R);
        const double* p = m->p[ji];
        const double* u = m->axis[ji];
        const Vec3<T> wc = mulT(R, w);
        const Vec3<T> vc = mulT(R, v + crossVC<T>(w, p));
        w = wc + mk<T>(u[0] * qdi, u[1] * qdi, u[2] * qdi);
        v = vc;
      }
      const double* Rc = P->R[leg];
      const double* pc = P->p[leg];
      auto rotT = [&](Vec3<T> x) {
        return mk<T>(Rc[0] * x.x + Rc[3] * x.y + Rc[6] * x.z, Rc[1] * x.x + Rc[4] * x.y + Rc[7] * x.z, Rc[2] * x.x + Rc[5] * x.y + Rc[8] * x.z);
      };
      const Vec3<T> fv = rotT(v + crossVC<T>(w, pc)), fw = rotT(w);
      double* __restrict__ row = &L.rhs[th][k][NV + 3 * __builtin_popcount(active_mask & ((1 << leg) - 1))];
      row[0] -= 2.0 * (fv.y.v * fw.z.d - fv.z.v * fw.y.d);
      row[1] -= 2.0 * (fv.z.v * fw.x.d - fv.x.v * fw.z.d);
      row[2] -= 2.0 * (fv.x.v * fw.y.d - fv.y.v * fw.x.d);
    }
  }
  // (single-lane scalar code like the other users of dev_lie.hpp; without A, L.lie stays unwritten and is not read: only the stores under Ao do)
  if (g.A && !IMPULSE && lane == 0) {
    // q_next = q (+) dt v: d/dq in the tangent at q_next is the action of exp6(dt v)^-1, d/dv is dt times the right Jacobian of exp6 at dt v
    double xi[6], R[9], p[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) xi[i] = g.dt * g.v[sample * NV + i];
    lieExp6(xi, R, p);
    lieDIntegrateArg0(R, p, L.lie[0]);
    lieDIntegrateArg1(xi, L.lie[1]);
  }
  waveLdsSync();
  const double nan = __builtin_nan("");
  // ---- the forward solution itself ----
  if (g.a_out && lane < NV) g.a_out[sample * NV + lane] = bad ? nan : g.a[sample * NV + lane];
  if (g.f_out && lane < NF) g.f_out[sample * NF + lane] = bad ? nan : g.f[sample * NF + lane];
  // ---- rows of inactive contacts ----
  {
    double* const con[2] = {g.df_dq ? g.df_dq + sample * (NF * NV) : nullptr, g.df_dv ? g.df_dv + sample * (NF * NV) : nullptr};
    for (int e = lane; e < NF * NV; e += 64) {
      const int r = e % NF;
      if ((active_mask >> (r / 3)) & 1) continue;
      if (con[0]) con[0][e] = bad ? nan : 0.0;
      if (con[1]) con[1][e] = bad ? nan : 0.0;
    }
    if (g.df_du) {
      double* __restrict__ o = g.df_du + sample * (NF * NU);
      for (int e = lane; e < NF * NU; e += 64) {
        const int r = e % NF;
        if (!((active_mask >> (r / 3)) & 1)) o[e] = bad ? nan : 0.0;
      }
    }
  }
  // ---- d[a; -f]/dtheta = -MJtJinv [dID/dtheta; dC/dtheta]: np x NV per theta ----
  double* __restrict__ Ao = g.A ? g.A + sample * (NX * NX) : nullptr;
  for (int e = lane; e < 2 * NV * np; e += 64) {
    const int th = e / (NV * np), rem = e - th * (NV * np), c = rem / np, r = rem - c * np;
    const double* __restrict__ col = &L.rhs[th][c][0];
    double acc = 0.0;
    for (int k = 0; k < np; ++k) acc = __builtin_fma(L.kinv[r + np * k], col[k], acc);
    if (r < NV) {
      const double val = bad ? nan : -acc;
      double* da = th == 0 ? g.da_dq : g.da_dv;
      if (da) da[sample * (NV * NV) + c * NV + r] = val;
      // bottom rows of A: [dt da_dq, I + dt da_dv]
      if (Ao) Ao[(NV + r) + NX * (th * NV + c)] = bad ? nan : ((th == 1 && r == c) ? 1.0 : 0.0) + scale * -acc;
    } else {
      double* df = th == 0 ? g.df_dq : g.df_dv;
      if (df) df[sample * (NF * NV) + c * NF + L.prow[r - NV]] = bad ? nan : acc;      // (the sign of f, not of -f)
    }
  }
  // ---- d[a; -f]/du = MJtJinv[:, 6 : nv] ----
  double* __restrict__ Bo = g.B ? g.B + sample * (NX * NU) : nullptr;
  if (!IMPULSE) {
    for (int e = lane; e < NU * np; e += 64) {
      const int j = e / np, r = e - j * np;
      const double x = L.kinv[r + np * (6 + j)];
      if (r < NV) {
        if (g.da_du) g.da_du[sample * (NV * NU) + j * NV + r] = bad ? nan : x;
        if (Bo) { Bo[r + NX * j] = bad ? nan : 0.0; Bo[(NV + r) + NX * j] = bad ? nan : scale * x; }
      } else if (g.df_du) {
        g.df_du[sample * (NF * NU) + j * NF + L.prow[r - NV]] = bad ? nan : -x;
      }
    }
  }
  // ---- top rows of A: dq_next/d(q, v) ----
  if (Ao) {
    for (int e = lane; e < NV * NX; e += 64) {
      const int c = e / NV, r = e - c * NV, th = c >= NV, cc = c - th * NV;
      double val;
      if (IMPULSE) val = (th == 0 && r == cc) ? 1.0 : 0.0;
      else {
        const double blk = (r < 6 && cc < 6) ? L.lie[th][r + 6 * cc] : ((r == cc) ? 1.0 : 0.0);
        val = th ? g.dt * blk : blk;
      }
      Ao[r + NX * c] = bad ? nan : val;
    }
  }
}

// One lane per sample.  M [n][NV * NV] column-major (only the lower triangle is read), dtau_dq, dtau_dv alike; a [n][NV] the forward solution.
template <int NV>
__global__ __launch_bounds__(64) void rbd_fd_derivatives_chain_kernel(RbdFddArgs g, int n) {
  const long s = (long)blockIdx.x * 64 + threadIdx.x;
  if (s >= n) return;
  constexpr int NX = 2 * NV;
  double Lm[NV][NV];
  const double* __restrict__ Ms = g.MJtJinv + s * (NV * NV);
  bool ok = true;
#pragma unroll
  for (int c = 0; c < NV; ++c)
#pragma unroll
    for (int r = c; r < NV; ++r) Lm[r][c] = Ms[r + NV * c];
#pragma unroll
  for (int i = 0; i < NV; ++i) ok = ok && isfinite(g.a[s * NV + i]);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double p = Lm[k][k];
#pragma unroll
    for (int j = 0; j < k; ++j) p -= Lm[k][j] * Lm[k][j];
    ok = ok && (p > 0.0);
    const double d = sqrt(p), id = 1.0 / d;
    Lm[k][k] = d;
#pragma unroll
    for (int r = k + 1; r < NV; ++r) {
      double t = Lm[r][k];
#pragma unroll
      for (int j = 0; j < k; ++j) t -= Lm[r][j] * Lm[k][j];
      Lm[r][k] = t * id;
    }
  }
  const double nan = __builtin_nan("");
  double* __restrict__ Ao = g.A ? g.A + s * (NX * NX) : nullptr;
  double* __restrict__ Bo = g.B ? g.B + s * (NX * NV) : nullptr;
#pragma unroll
  for (int i = 0; i < NV; ++i) if (g.a_out) g.a_out[s * NV + i] = ok ? g.a[s * NV + i] : nan;
  // columns of [dtau_dq | dtau_dv | I]: da_dq = -M^-1 dtau_dq, da_dv = -M^-1 dtau_dv, da_du = M^-1
#pragma unroll 1
  for (int col = 0; col < 3 * NV; ++col) {
    const int kind = col / NV, c = col - kind * NV;
    const double* __restrict__ src = (kind == 0 ? g.dtau_dq : g.dtau_dv) + s * (NV * NV) + c * NV;
    double x[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) x[i] = kind == 2 ? (i == c ? 1.0 : 0.0) : src[i];
#pragma unroll
    for (int i = 0; i < NV; ++i) {          // L z = r
      double t = x[i];
#pragma unroll
      for (int j = 0; j < i; ++j) t -= Lm[i][j] * x[j];
      x[i] = t / Lm[i][i];
    }
#pragma unroll
    for (int i = NV - 1; i >= 0; --i) {     // L^T y = z
      double t = x[i];
#pragma unroll
      for (int j = i + 1; j < NV; ++j) t -= Lm[j][i] * x[j];
      x[i] = t / Lm[i][i];
    }
    double* out = kind == 0 ? g.da_dq : (kind == 1 ? g.da_dv : g.da_du);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const double val = kind == 2 ? x[i] : -x[i];
      if (out) out[s * (NV * NV) + c * NV + i] = ok ? val : nan;
      if (kind < 2) {
        if (Ao) {
          Ao[i + NX * col] = ok ? ((i == c) ? (kind ? g.dt : 1.0) : 0.0) : nan;                      // top rows: [I, dt I]
          Ao[(NV + i) + NX * col] = ok ? ((kind == 1 && i == c) ? 1.0 : 0.0) + g.dt * val : nan;    // bottom rows: [dt da_dq, I + dt da_dv]
        }
      } else if (Bo) {
        Bo[i + NX * c] = ok ? 0.0 : nan;
        Bo[(NV + i) + NX * c] = ok ? g.dt * val : nan;
      }
    }
  }
}

// A = E A, B = E B in place: one wavefront per sample, everything of the sample in LDS before the first store
constexpr int FDD_NX_MAX = 36, FDD_NU_MAX = 12;
__global__ __launch_bounds__(64) void rbd_fdd_impulse_product_kernel(int nx, int nu, const double* __restrict__ E, double* A, double* B, int n) {
  __shared__ double s_e[FDD_NX_MAX * FDD_NX_MAX], s_x[FDD_NX_MAX * (FDD_NX_MAX + FDD_NU_MAX)];
  const long sample = blockIdx.x;
  const int lane = threadIdx.x;
  if (sample >= n) return;
  const int na = A ? nx * nx : 0, nb = B ? nx * nu : 0;
  for (int e = lane; e < nx * nx; e += 64) s_e[e] = E[sample * (nx * nx) + e];
  for (int e = lane; e < na; e += 64) s_x[e] = A[sample * (nx * nx) + e];
  for (int e = lane; e < nb; e += 64) s_x[nx * nx + e] = B[sample * (nx * nu) + e];
  waveLdsSync();
  for (int e = lane; e < na + nb; e += 64) {
    const bool inB = e >= na;
    const int o = inB ? e - na : e, c = o / nx, r = o - c * nx;
    const double* __restrict__ col = s_x + (inB ? nx * nx : 0) + c * nx;
    double acc = 0.0;
    for (int k = 0; k < nx; ++k) acc = __builtin_fma(s_e[r + nx * k], col[k], acc);
    if (inB) B[sample * (nx * nu) + o] = acc; else A[sample * (nx * nx) + o] = acc;
  }
}

template <int NV>
void launchFddChain(const RbdFddArgs& a, int n, hipStream_t st) {
  hipLaunchKernelGGL((rbd_fd_derivatives_chain_kernel<NV>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a, n);
}

}  // namespace

void rbdFddQuadruped(const DevModel* m, const RbdFrames* frames, const RbdFddArgs& a, int n, int mode, int active_mask, hipStream_t st) {
  using D = LeggedDims<4, 3>;
  const dim3 grid((unsigned)((n + RBD_WAVES - 1) / RBD_WAVES)), block(64 * RBD_WAVES);
  if (mode == IDOCP_RBD_IMPULSE) hipLaunchKernelGGL((rbd_fd_derivatives_kernel<D, true>), grid, block, 0, st, m, frames, a, n, active_mask);
  else hipLaunchKernelGGL((rbd_fd_derivatives_kernel<D, false>), grid, block, 0, st, m, frames, a, n, active_mask);
}

void rbdFddImpulseProduct(int nx, int nu, const double* E, double* A, double* B, int n, hipStream_t st) {
  if (nx > FDD_NX_MAX || nu > FDD_NU_MAX || n <= 0) return;
  hipLaunchKernelGGL(rbd_fdd_impulse_product_kernel, dim3((unsigned)n), dim3(64), 0, st, nx, nu, E, A, B, n);
}

void rbdFddChain(int nv, const RbdFddArgs& a, int n, hipStream_t st) {
  switch (nv) {
    case 2: launchFddChain<2>(a, n, st); break;
    case 3: launchFddChain<3>(a, n, st); break;
    case 4: launchFddChain<4>(a, n, st); break;
    case 5: launchFddChain<5>(a, n, st); break;
    case 6: launchFddChain<6>(a, n, st); break;
    case 7: launchFddChain<7>(a, n, st); break;
    case 8: launchFddChain<8>(a, n, st); break;
    default: break;
  }
}

}  // namespace idocp_dev
