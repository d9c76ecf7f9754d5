// The kernel template of rbd_lqr_kernel.hip and rbd_lqr_gn_kernel.hip (their heads have the method).  It lives in a header so that each form is
// instantiated in a translation unit of its own: the code of one form does not depend on whether the other is built beside it.
#ifndef IDOCP_RBD_LQR_KERNEL_HPP_
#define IDOCP_RBD_LQR_KERNEL_HPP_

#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "dev_dense.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

template <int NXM, int NUM>
struct RbdLqrLds {
  static constexpr int NZM = NXM + NUM;
  static constexpr int LDP = NXM + 2, LDZ = NXM + 2, LDU = NUM + 2;      // even (16-byte operand reads), and 16 columns apart hit 16 different bank groups
  static constexpr int PAD = 8;                                          // the tile reads run up to 8 ceil(K / 8) entries into a column: room behind the last one
  static constexpr int U_SIZE = LDU * NXM + PAD, KK_SIZE = LDU * (NXM + 1) + PAD, Q_SIZE = NUM * NUM;
  static constexpr int U_AT = 0, KK_AT = U_SIZE, Q_AT = U_SIZE + KK_SIZE;      // inside Z, once Z is dead
  double Pm[LDP * NXM + PAD];       // P, then Qxx, then X, then the new P: column-major
  double Z[LDZ * NZM + PAD];        // [A | B] column-major; from the store of H to the end of the step: Qux (ld LDU), [K | k] (ld LDU), Quu (ld NUM)
  double Gc[LDZ * 16 + PAD];        // one block column of P Z
  double pv[NXM];                   // p
  double qxu[NZM];                  // [Qx; Qu]
  double wx[NXM], wu[NUM];          // diag Wx, diag Wu + reg
  int ok;
  static_assert(LDP % 2 == 0 && LDU % 2 == 0 && U_SIZE % 2 == 0 && KK_SIZE % 2 == 0, "16-byte operand reads");
  static_assert(Q_AT + Q_SIZE <= LDZ * NZM + PAD, "Qux, [K | k] and Quu fit in Z");
};

// the LDS of the DIAG form alone: D_k of the step (the other forms declare nothing more)
static_assert(RBD_LQR_WAVES == 1, "the LDS of the kernel, lqrDiagShared included, is one sample's: one wavefront per workgroup");
template <int NZM>
__device__ __forceinline__ double* lqrDiagShared() { __shared__ double d[NZM]; return d; }

__device__ __forceinline__ bool finite2(double x, double y) { return std::isfinite(x) && std::isfinite(y); }

// Args = RbdLqrArgs: the recursion at the head of rbd_lqr_kernel.hip.  Args = RbdLqrGnArgs (the GN form, idocp_rbd_lqr_backward_gn): H gains G_k^T G_k before it is stored.
// Args = RbdLqrGnDiagArgs (idocp_rbd_lqr_backward_gn_diag): the GN form, and the diagonal of H also gains D_k where wx / wu are added.
template <int NXM, int NUM, class Args = RbdLqrArgs>
__global__ __launch_bounds__(64 * RBD_LQR_WAVES) void rbd_lqr_kernel(Args a) {
  using W = RbdLqrLds<NXM, NUM>;
  constexpr bool GN = std::is_base_of<RbdLqrGnArgs, Args>::value, DIAG = std::is_same<Args, RbdLqrGnDiagArgs>::value;
  typedef double d2 __attribute__((ext_vector_type(2), aligned(8)));      // (a caller's device pointer need not be 16-byte aligned)
  constexpr int LDP = W::LDP, LDZ = W::LDZ, LDU = W::LDU;
  constexpr int RT = (NXM + 15) / 16, ZT = (NXM + NUM + 15) / 16, KT = (NXM + 1 + 15) / 16;
  constexpr int NA2 = (NXM * NXM / 2 + 63) / 64, NB2 = (NXM * NUM / 2 + 63) / 64;
  static_assert(NXM % 2 == 0 && NXM + 1 <= 64 && NXM + NUM <= 64 && NUM <= 16, "one lane per column of [K | k] and per entry of [Qx; Qu]");
  __shared__ W L;
  const int lane = threadIdx.x;
  const size_t sample = blockIdx.x;
  const int nx = a.nx, nu = a.nu, nz = nx + nu, steps = a.steps, h = nx / 2;      // (nx = 2 nv is even)
  const size_t N = (size_t)a.n, nxx = (size_t)nx * nx, nxu = (size_t)nx * nu;
  const bool grad = a.lx != nullptr;
  const double nan = __builtin_nan("");
  double* const U = L.Z + W::U_AT;
  double* const KK = L.Z + W::KK_AT;
  double* const Q = L.Z + W::Q_AT;

  // where pair l + 64 t of A (of B) goes in Z; -1: beyond the block
  int zA[NA2], zB[NB2];
#pragma unroll
  for (int t = 0; t < NA2; ++t) { const int e = lane + 64 * t, c = e / h; zA[t] = e < nx * h ? 2 * (e - c * h) + LDZ * c : -1; }
#pragma unroll
  for (int t = 0; t < NB2; ++t) { const int e = lane + 64 * t, c = e / h; zB[t] = e < nu * h ? 2 * (e - c * h) + LDZ * (nx + c) : -1; }
  d2 ra[NA2], rb[NB2];
  auto fetch = [&](int k) {
    const double* __restrict__ Ak = a.A + ((size_t)k * N + sample) * nxx;
    const double* __restrict__ Bk = a.B + ((size_t)k * N + sample) * nxu;
#pragma unroll
    for (int t = 0; t < NA2; ++t) if (zA[t] >= 0) ra[t] = *reinterpret_cast<const d2*>(Ak + 2 * (lane + 64 * t));
#pragma unroll
    for (int t = 0; t < NB2; ++t) if (zB[t] >= 0) rb[t] = *reinterpret_cast<const d2*>(Bk + 2 * (lane + 64 * t));
  };
  // the fetched step into Z; true: an entry of this lane's is not finite
  auto stash = [&]() {
    bool bad = false;
#pragma unroll
    for (int t = 0; t < NA2; ++t) if (zA[t] >= 0) { bad = bad || !finite2(ra[t].x, ra[t].y); L.Z[zA[t]] = ra[t].x; L.Z[zA[t] + 1] = ra[t].y; }
#pragma unroll
    for (int t = 0; t < NB2; ++t) if (zB[t] >= 0) { bad = bad || !finite2(rb[t].x, rb[t].y); L.Z[zB[t]] = rb[t].x; L.Z[zB[t] + 1] = rb[t].y; }
    return bad;
  };

  fetch(steps - 1);
  // P = Wxf, p = lx[steps], the weights
  for (int e = lane; e < LDP * NXM + W::PAD; e += 64) L.Pm[e] = 0.0;
  waveLdsSync();
  bool bad = false;
  if (lane < nx) {
    L.Pm[lane + LDP * lane] = a.xf_weight[lane];
    L.wx[lane] = a.x_weight[lane];
    const double p = grad ? a.lx[((size_t)steps * N + sample) * nx + lane] : 0.0;
    bad = !std::isfinite(p);
    L.pv[lane] = p;
  }
  if (lane < nu) L.wu[lane] = a.u_weight[lane] + a.regularization;
  double e0 = 0.0, e1 = 0.0;      // lane nx: the two sums of `expected`
  int failed = -1;

  for (int k = steps - 1; k >= 0; --k) {
    bad = stash() || bad;
    double g = 0.0;
    if (grad && lane < nz) {
      g = lane < nx ? a.lx[((size_t)k * N + sample) * nx + lane] : a.lu[((size_t)k * N + sample) * nu + (lane - nx)];
      bad = bad || !std::isfinite(g);
    }
    if (__ballot(bad) != 0) { failed = k; break; }
    if constexpr (DIAG) {
      // D_k, entry c on lane c: it must be finite and not negative, else the sample fails here.  (The reads of the previous step's are behind a
      // waveLdsSync; the one below orders this write before the reads.)
      double* const Dk = lqrDiagShared<NXM + NUM>();
      bool dbad = false;
      if (lane < nz) { const double d = a.D[((size_t)k * N + sample) * nz + lane]; dbad = !(d >= 0.0) || !std::isfinite(d); Dk[lane] = d; }
      if (__ballot(dbad) != 0) { failed = k; break; }
    }
    if (k > 0) fetch(k - 1);
    if (lane == 0) L.ok = 1;
    waveLdsSync();

    // [Qx; Qu] = [lx; lu] + Z^T p, entry j on lane j, in row order
    if (lane < nz) {
      const double* z = L.Z + LDZ * lane;
      double acc = g;
      for (int r = 0; r < nx; ++r) acc = __builtin_fma(z[r], L.pv[r], acc);
      L.qxu[lane] = acc;
    }

    // H = Z^T (P Z), one block column at a time
    mfma_d4 H[ZT][ZT];
#pragma unroll
    for (int ct = 0; ct < ZT; ++ct) {
      if (16 * ct < nz) {
        const int yc = nz - 16 * ct < 16 ? nz - 16 * ct : 16;
        mfma_d4 G[RT];
        mfmaTileColumnTN<NXM, RT>(L.Pm, nx, L.Z + LDZ * 16 * ct, yc, LDP, LDZ, nx, lane, G);      // (P is symmetric: P Z = P^T Z)
#pragma unroll
        for (int t = 0; t < RT; ++t) mfmaTileStore(G[t], 16 * t, 0, nx, 16, lane, [&](int r, int c, double v) { L.Gc[r + LDZ * c] = v; });
        waveLdsSync();
        mfma_d4 Hc[ZT];
        mfmaTileColumnTN<NXM, ZT>(L.Z, nz, L.Gc, yc, LDZ, LDZ, nx, lane, Hc);
#pragma unroll
        for (int t = 0; t < ZT; ++t) H[t][ct] = Hc[t];
        waveLdsSync();      // (Gc is read before the next column overwrites it)
      }
    }
    if constexpr (GN) {
      // H += G^T G straight from global memory, no LDS: for four rows 4 j .. 4 j + 3 of G, lane l holds G[4 j + l / 16][16 t + l % 16], which is
      // both the A operand of tile column t and the B operand of tile row t.  The rows of the next four are in flight while these multiply.
      const int li = lane & 15, g4 = lane >> 4;
      const double* __restrict__ Gk = a.G + ((size_t)k * N + sample) * ((size_t)a.g_rows * nz) + (size_t)g4 * nz;
      auto rows = [&](int j, double (&x)[ZT]) {
#pragma unroll
        for (int t = 0; t < ZT; ++t) { const int c = 16 * t + li; x[t] = c < nz ? Gk[(size_t)j * nz + c] : 0.0; }
      };
      double cur[ZT], nxt[ZT];
      bool gbad = false;
      rows(0, cur);
      for (int j = 0; j < a.g_rows; j += 4) {
#pragma unroll
        for (int t = 0; t < ZT; ++t) nxt[t] = 0.0;
        if (j + 4 < a.g_rows) rows(j + 4, nxt);
#pragma unroll
        for (int t = 0; t < ZT; ++t) gbad = gbad || !std::isfinite(cur[t]);
#pragma unroll
        for (int ct = 0; ct < ZT; ++ct)
#pragma unroll
          for (int t = 0; t < ZT; ++t)
            if (16 * ct < nz && 16 * t < nz) H[t][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[ct], cur[t], H[t][ct], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < ZT; ++t) cur[t] = nxt[t];
      }
      if (__ballot(gbad) != 0) { failed = k; break; }
    }
    // the DIAG form: entry (r, r) of the Hessian gains D_k[r] on top of its weight; the other forms: nothing
    auto diag = [&](int r, int c, double q) {
      if constexpr (DIAG) return r == c ? q + lqrDiagShared<NXM + NUM>()[r] : q;
      else { (void)r; (void)c; return q; }
    };
    // Z and P are dead: Qxx over P, Qux and Quu (the lower triangle, mirrored) into Z's room
#pragma unroll
    for (int ct = 0; ct < ZT; ++ct)
#pragma unroll
      for (int t = 0; t < ZT; ++t)
        if (16 * ct < nz && 16 * t < nz)
          mfmaTileStore(H[t][ct], 16 * t, 16 * ct, nz, nz, lane, [&](int r, int c, double v) {
            if (r < nx) { if (c < nx) L.Pm[r + LDP * c] = diag(r, c, v + (r == c ? L.wx[r] : 0.0)); }
            else if (c < nx) U[(r - nx) + LDU * c] = v;
            else if (r >= c) { const int i = r - nx, j = c - nx; const double q = diag(r, c, v + (i == j ? L.wu[i] : 0.0)); Q[i + NUM * j] = q; Q[j + NUM * i] = q; }
          });
    waveLdsSync();

    // [K | k] = -Quu^-1 [Qux | Qu]: column c on lane c
    double x[NUM];
    {
      const int col = lane < nx ? lane : nx - 1;
#pragma unroll
      for (int i = 0; i < NUM; ++i) {
        const int ii = i < nu ? i : nu - 1;
        const double ux = U[ii + LDU * col], qu = L.qxu[nx + ii];
        x[i] = i < nu ? (lane < nx ? ux : (lane == nx ? qu : 0.0)) : 0.0;
      }
    }
    choleskySolveRows<NUM>(Q, NUM, lane, &L.ok, x, nu);
    waveLdsSync();
    if (!L.ok) { failed = k; break; }
#pragma unroll
    for (int i = 0; i < NUM; ++i) x[i] = -x[i];
    if (lane <= nx) {
#pragma unroll
      for (int i = 0; i < NUM; ++i) if (i < nu) KK[i + LDU * lane] = x[i];
    }
    if (a.K && lane < nx) {
      double* Kk = a.K + ((size_t)k * N + sample) * nxu + (size_t)nu * lane;
#pragma unroll
      for (int i = 0; i < NUM; ++i) if (i < nu) Kk[i] = x[i];
    }
    if (grad && lane == nx) {
      if (a.k) {
        double* kk = a.k + ((size_t)k * N + sample) * nu;
#pragma unroll
        for (int i = 0; i < NUM; ++i) if (i < nu) kk[i] = x[i];
      }
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int i = 0; i < NUM; ++i) {
        if (i < nu) {
          double qk = 0.0;
#pragma unroll
          for (int j = 0; j < NUM; ++j) if (j < nu) qk = __builtin_fma(Q[i + NUM * j], x[j], qk);
          s0 = __builtin_fma(x[i], L.qxu[nx + i], s0);
          s1 = __builtin_fma(x[i], qk, s1);
        }
      }
      e0 += s0; e1 += 0.5 * s1;
    }
    waveLdsSync();

    // X = Qxx + Qux^T K in place, p = Qx + Qux^T k (column nx of the product)
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) {
      if (16 * ct < nx + 1) {
        const int yc = nx + 1 - 16 * ct < 16 ? nx + 1 - 16 * ct : 16;
        mfma_d4 T[RT];
        mfmaTileColumnTN<NUM, RT>(U, nx, KK + LDU * 16 * ct, yc, LDU, LDU, nu, lane, T);
#pragma unroll
        for (int t = 0; t < RT; ++t)
          mfmaTileStore(T[t], 16 * t, 16 * ct, nx, nx + 1, lane, [&](int r, int c, double v) {
            if (c < nx) L.Pm[r + LDP * c] += v; else L.pv[r] = L.qxu[r] + v;
          });
      }
    }
    waveLdsSync();
    // P = (X + X^T) / 2: lane j owns the pairs (i, j), i < j
    if (lane < nx) {
      for (int i = 0; i < lane; ++i) {
        const double s = 0.5 * (L.Pm[i + LDP * lane] + L.Pm[lane + LDP * i]);
        L.Pm[i + LDP * lane] = s; L.Pm[lane + LDP * i] = s;
      }
    }
    waveLdsSync();
  }

  if (failed >= 0) {
    for (int s = failed; s >= 0; --s) {
      if (a.K) { double* Ks = a.K + ((size_t)s * N + sample) * nxu; for (int e = lane; e < nx * nu; e += 64) Ks[e] = nan; }
      if (a.k && lane < nu) a.k[((size_t)s * N + sample) * nu + lane] = nan;
    }
  }
  if (a.P0) {
    double* P0 = a.P0 + sample * nxx;
    if (lane < nx) for (int c = 0; c < nx; ++c) P0[lane + (size_t)nx * c] = failed >= 0 ? nan : L.Pm[lane + LDP * c];
  }
  if (a.p0 && lane < nx) a.p0[sample * nx + lane] = failed >= 0 ? nan : L.pv[lane];
  if (a.expected && lane == nx) { a.expected[2 * sample] = failed >= 0 ? nan : e0; a.expected[2 * sample + 1] = failed >= 0 ? nan : e1; }
  if (a.status && lane == 0) a.status[sample] = failed;
}

}  // namespace

}  // namespace idocp_dev
#endif  // IDOCP_RBD_LQR_KERNEL_HPP_
