// Batched forward dynamics with contacts on plain arrays (idocp_rbd_forward_dynamics_batch, idocp_rbd_rollout; include/idocp_hip.h): an addition
// the reference does not have -- it only evaluates the inverse direction (Robot::RNEA, computeBaumgarteResidual, computeMJtJinv).  Defined
// through rbd_batch_kernel.hip's terms:
//   STAGE    [M J^T; J 0] [a; -f]       = [S^T u - h; -b],   h = ID(q, v, 0, 0),  M = dID/da,  b = C(q, v, 0),  J = dC/da over the active rows
//   IMPULSE  [M J^T; J 0] [dv; -lambda] = [0; -J v]           (no gravity, no velocity in the dynamics; J v = the impulse-velocity residual at v)
//
// Quadruped: one wavefront per sample, RBD_WAVES samples per workgroup, no workgroup barrier, like rbd_batch_kernel.  The sweep is that
// kernel's, cut down to what this one needs and kept SELF-CONTAINED here (sharing it through a header would re-shape the batch kernel's
// instantiations): the four nominal items and the 36 a-seed items -- its RBD_ITEMS_A set, one round of 40 lanes --
// at a = 0, f = 0; in impulse mode a second, kinematic pass at v.  The 42 x 42 inverse is never formed: M^-1 by blockArrowInverse, y = M^-1 r,
// T = M^-1 J^T, S = J T over the packed active rows, ONE Cholesky solve S g = J y + b in registers (choleskySolveRows), a = y - T g, f = -g.
// The Euler step is the OCP's own (state_equation.hxx): q (+) dt v by lieIntegrateBase (dev_lie.hpp), v + dt a.
//
// Fixed-base chains: the chain sweep (UnLaunch<NV>::rneaDerivatives at a = 0) gives h and M; rbd_forward_chain_kernel solves and steps.
#include <hip/hip_runtime.h>

#include "dev_dense.hpp"
#include "dev_lie.hpp"
#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

template <typename D>
struct RbdForwardLds {
  static constexpr int NV = D::NV, NVF = D::NVF, NL = D::NL, LJ = D::LJ, NF = D::NF, NQ = D::NQ;
  static constexpr int A_PER_LEG = 6 + LJ, NSEED = NL * A_PER_LEG;
  // column stride: odd, so that the lanes of the round, which write the same row of different columns, fall on different LDS banks
  static constexpr int LDC = NVF | 1;
  double out[NV + 1][LDC];      // column of each a seed: rows [M (NV) ; J (NF, the rows of contact c at 3 c)]; column NV: what the nominal items leave
  double bt[NSEED][6];          // tangent of the force each seed item's leg transmits to the base
  double bown[6][6];            // tangent of the base's own inertial force, per base seed
  double bn[NL + 1][6];         // nominal base force: own, then per leg
  double idc[NVF];              // nominal [h ; b]
  double cs[D::NU][2];          // cos / sin of the leg joint angles
  double q[NQ], v[NV];          // the sample's state (read completely before anything is stored: q_next / v_next may be q / v)
  double vp[NV];                // velocity of the current pass
  double minv[NV * NV];         // M, then M^-1 (column-major, ld NV)
  double r[NV], y[NV];          // right-hand side S^T u - h, y = M^-1 r
  double Tm[NV * NF];           // T = M^-1 J^T (ld NV)
  double Sm[NF * NF];           // S = J T (ld NF)
  double g[NF];                 // J y + b, then g = S^-1 (J y + b) = -f (packed active rows)
  double acc[NV];               // the answer a (dv)
  int prow[NF];                 // packed contact row -> row of `out` behind NV
  int ok;
};

template <typename D, bool IMPULSE>
__global__ __launch_bounds__(64 * RBD_WAVES, 2) void rbd_forward_kernel(const DevModel* __restrict__ m, const RbdFrames* __restrict__ P,
                                                                        idocp_rbd_fd_io_t io, int n, int active_mask, double time_step, double dt) {
  using W = RbdForwardLds<D>;
  constexpr int NV = D::NV, NQ = D::NQ, NL = D::NL, LJ = D::LJ, NF = D::NF, NVF = D::NVF, NU = D::NU;
  constexpr int A_PER_LEG = W::A_PER_LEG, NIDX = NL + W::NSEED;
  static_assert(NIDX <= 64, "the nominal and the a-seed items are one round of the wavefront");
  static_assert(NF <= 16, "the contact Schur complement is solved on the rows of 16 lanes");
  typedef Dual T;
  __shared__ W s_wave[RBD_WAVES];
  const int lane = threadIdx.x & 63;
  const long sample = (long)blockIdx.x * RBD_WAVES + (threadIdx.x >> 6);
  if (sample >= n) return;                                // (no workgroup barrier below)
  W& L = s_wave[threadIdx.x >> 6];
  active_mask &= (1 << NL) - 1;
  const int dimf = 3 * __builtin_popcount(active_mask);
  const double* __restrict__ cpin = io.contact_points ? io.contact_points + sample * NF : nullptr;
  const bool want_solve = io.a || io.f || io.v_next;      // (q_next alone needs no dynamics)
  if (lane < NQ) L.q[lane] = io.q[sample * NQ + lane];
  if (lane < NV) L.v[lane] = io.v[sample * NV + lane];
  if (lane == 0) {
    L.ok = 1;
    int row = 0;
    for (int c = 0; c < NL; ++c)
      if ((active_mask >> c) & 1) { L.prow[row] = 3 * c; L.prow[row + 1] = 3 * c + 1; L.prow[row + 2] = 3 * c + 2; row += 3; }
  }
  waveLdsSync();
  if (want_solve) {
    if (lane < NU) {
      double sj, cj;
      sincos(L.q[7 + lane], &sj, &cj);
      L.cs[lane][0] = cj; L.cs[lane][1] = sj;
    }
    // zero the rows a seed does not reach (the joints of the other legs, the rows of inactive contacts)
    for (int e = lane; e < (NV + 1) * W::LDC; e += 64) (&L.out[0][0])[e] = 0.0;
    if (lane < NVF) L.idc[lane] = 0.0;
    const double gz = IMPULSE ? 0.0 : m->gravity[2];
    const double wv = 2.0 / time_step, wp = 1.0 / (time_step * time_step);
    double Rn[9];
    lieQuatToR(&L.q[3], Rn);

    constexpr int npass = IMPULSE ? 2 : 1;
#pragma unroll 1
    for (int pass = 0; pass < npass; ++pass) {
      // impulse: pass 0 is the dynamics at (v, a, g) = (0, 0, 0), i.e. M alone; pass 1 the kinematics at the velocity v: J and J v
      const bool do_dyn = (pass == 0), do_con = IMPULSE ? (pass == 1) : (dimf > 0);
      if (IMPULSE && pass == 1 && dimf == 0) break;
      waveLdsSync();
      if (lane < NV) L.vp[lane] = (IMPULSE && pass == 0) ? 0.0 : L.v[lane];
      waveLdsSync();
      if (lane < NIDX) {
        // lanes 0 .. NL - 1: the nominal item of each leg; then per leg the 6 base a seeds and its LJ joint a seeds
        const bool nominal = lane < NL;
        const int e = nominal ? 0 : lane - NL;
        const int leg = nominal ? lane : e / A_PER_LEG, rs = e - leg * A_PER_LEG;
        const bool base_seed = !nominal && rs < 6;
        const int k = nominal ? -1 : (base_seed ? rs : 6 + leg * LJ + (rs - 6));      // velocity index of the seed
        double* __restrict__ col = &L.out[nominal ? NV : k][0];
        // in the kinematic pass of the impulse mode the seeds are velocity seeds (dC/ddv = dC/dv)
        const bool vseed = IMPULSE && pass == 1, aseed = !vseed;
        const bool active = (active_mask >> leg) & 1;
        Mat3<T> Rw;                                       // world pose of the current frame (starts at the base)
#pragma unroll
        for (int i = 0; i < 9; ++i) Rw.m[i] = T(Rn[i]);
        Vec3<T> pw = mk<T>(T(L.q[0]), T(L.q[1]), T(L.q[2]));
        auto seedV = [&](int i) { return T(L.vp[i], (vseed && k == i) ? 1.0 : 0.0); };
        auto seedA = [&](int i) { return T(0.0, (aseed && k == i) ? 1.0 : 0.0); };
        Vec3<T> v = mk<T>(seedV(0), seedV(1), seedV(2)), w = mk<T>(seedV(3), seedV(4), seedV(5));
        // a_gf = a_joint + R^T (0, 0, -g_z)  (base acceleration in the gravity field)
        Vec3<T> bl = mk<T>(seedA(0) - gz * Rw.m[6], seedA(1) - gz * Rw.m[7], seedA(2) - gz * Rw.m[8]);
        Vec3<T> bw = mk<T>(seedA(3), seedA(4), seedA(5));
        if (do_dyn && leg == 0 && (base_seed || nominal)) {
          // the base's own inertial force: once per base seed and once for the nominal value
          Vec3<T> hl, hn, f, nn;
          inertiaMul<T>(m, 0, v, w, hl, hn);
          inertiaMul<T>(m, 0, bl, bw, f, nn);
          const Vec3<T> Fbl = f + cross(w, hl);
          const Vec3<T> Fbn = nn + cross(w, hn) + cross(v, hl);
          if (nominal) { double* on = &L.bn[0][0]; on[0] = Fbl.x.v; on[1] = Fbl.y.v; on[2] = Fbl.z.v; on[3] = Fbn.x.v; on[4] = Fbn.y.v; on[5] = Fbn.z.v; }
          else { double* o = &L.bown[rs][0]; o[0] = Fbl.x.d; o[1] = Fbl.y.d; o[2] = Fbl.z.d; o[3] = Fbn.x.d; o[4] = Fbn.y.d; o[5] = Fbn.z.d; }
        }
        // ---- the leg of this item, outward ----
#pragma unroll 1
        for (int j = 0; j < LJ; ++j) {
          const int ji = 1 + leg * LJ + j, dof = 6 + leg * LJ + j, ci = leg * LJ + j;
          const bool mine = (k == dof);
          const T cqi(L.cs[ci][0]), sqi(L.cs[ci][1]);
          const T qdi(L.vp[dof], (mine && vseed) ? 1.0 : 0.0);
          const T qddi(0.0, (mine && aseed) ? 1.0 : 0.0);
          Mat3<T> R;
          revoluteRotation<T>(m->R[ji], m->axis[ji], cqi, sqi, R);
          const double* p = m->p[ji];
          const double* u = m->axis[ji];
          pw = pw + mul(Rw, mk<T>(T(p[0]), T(p[1]), T(p[2])));
          {
            Mat3<T> Rn2;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
              for (int c = 0; c < 3; ++c) Rn2.m[3 * r + c] = Rw.m[3 * r] * R.m[c] + Rw.m[3 * r + 1] * R.m[3 + c] + Rw.m[3 * r + 2] * R.m[6 + c];
            Rw = Rn2;
          }
          const Vec3<T> wc = mulT(R, w);
          const Vec3<T> vc = mulT(R, v + crossVC<T>(w, p));
          const Vec3<T> bwc = mulT(R, bw);
          const Vec3<T> blc = mulT(R, bl + crossVC<T>(bw, p));
          const Vec3<T> vJ = mk<T>(u[0] * qdi, u[1] * qdi, u[2] * qdi);
          w = wc + vJ;
          v = vc;
          bw = bwc + mk<T>(u[0] * qddi, u[1] * qddi, u[2] * qddi) + cross(w, vJ);
          bl = blc + cross(v, vJ);
        }
        // ---- contact frame at the foot (tip joint of this leg) ----
        if (active && do_con) {
          const double* Rc = P->R[leg];
          const double* pc = P->p[leg];
          const int row = NV + 3 * leg;
          // frame spatial velocity / acceleration (acceleration WITHOUT gravity: a = a_gf + R_w^T g)
          const Vec3<T> al_ng = mk<T>(bl.x + gz * Rw.m[6], bl.y + gz * Rw.m[7], bl.z + gz * Rw.m[8]);
          const Vec3<T> vj = v + crossVC<T>(w, pc);
          const Vec3<T> aj = al_ng + crossVC<T>(bw, pc);
          auto rotT = [&](Vec3<T> x) {
            return mk<T>(Rc[0] * x.x + Rc[3] * x.y + Rc[6] * x.z, Rc[1] * x.x + Rc[4] * x.y + Rc[7] * x.z, Rc[2] * x.x + Rc[5] * x.y + Rc[8] * x.z);
          };
          const Vec3<T> fv = rotT(vj), fw = rotT(w), fa = rotT(aj);
          const Vec3<T> pf = pw + mul(Rw, mk<T>(T(pc[0]), T(pc[1]), T(pc[2])));
          double cx, cy, cz, dx, dy, dz;
          if (IMPULSE) {
            // impulse-velocity constraint (point_contact.hxx:145-175): LOCAL linear velocity of the frame
            cx = fv.x.v; cy = fv.y.v; cz = fv.z.v;
            dx = fv.x.d; dy = fv.y.d; dz = fv.z.d;
          } else {
            const double px = cpin ? cpin[3 * leg] : 0.0, py = cpin ? cpin[3 * leg + 1] : 0.0, pz = cpin ? cpin[3 * leg + 2] : 0.0;
            // Baumgarte residual (point_contact.hxx:67-87) and its derivative with respect to a (point_contact.hxx:117-143, the a seed alone)
            cx = fa.x.v + (fw.y.v * fv.z.v - fw.z.v * fv.y.v) + wv * fv.x.v + wp * (pf.x.v - px);
            cy = fa.y.v + (fw.z.v * fv.x.v - fw.x.v * fv.z.v) + wv * fv.y.v + wp * (pf.y.v - py);
            cz = fa.z.v + (fw.x.v * fv.y.v - fw.y.v * fv.x.v) + wv * fv.z.v + wp * (pf.z.v - pz);
            dx = fa.x.d; dy = fa.y.d; dz = fa.z.d;
          }
          col[row] = dx; col[row + 1] = dy; col[row + 2] = dz;
          if (nominal) { L.idc[row] = cx; L.idc[row + 1] = cy; L.idc[row + 2] = cz; }
        }
        if (do_dyn) {
          // ---- inward sweep: accumulate forces, emit tau, undo the kinematic steps (no contact force: f = 0) ----
          Vec3<T> Fl = mk<T>(T(0.0), T(0.0), T(0.0)), Fn = Fl;
#pragma unroll 1
          for (int j = LJ - 1; j >= 0; --j) {
            const int ji = 1 + leg * LJ + j, dof = 6 + leg * LJ + j, ci = leg * LJ + j;
            const double* u = m->axis[ji];
            Vec3<T> hl, hn, f, nn;
            inertiaMul<T>(m, ji, v, w, hl, hn);
            inertiaMul<T>(m, ji, bl, bw, f, nn);
            Fl = Fl + f + cross(w, hl);
            Fn = Fn + nn + cross(w, hn) + cross(v, hl);
            const T ti = u[0] * Fn.x + u[1] * Fn.y + u[2] * Fn.z;
            col[dof] = ti.d;
            if (nominal) L.idc[dof] = ti.v;
            const bool mine = (k == dof);
            const T cqi(L.cs[ci][0]), sqi(L.cs[ci][1]);
            Mat3<T> R;
            revoluteRotation<T>(m->R[ji], m->axis[ji], cqi, sqi, R);
            const double* p = m->p[ji];
            const Vec3<T> Rf = mul(R, Fl);
            Fn = mul(R, Fn) + crossC<T>(p, Rf);
            Fl = Rf;
            if (j > 0) {
              const T qdi(L.vp[dof], (mine && vseed) ? 1.0 : 0.0);
              const T qddi(0.0, (mine && aseed) ? 1.0 : 0.0);
              const Vec3<T> vJ = mk<T>(u[0] * qdi, u[1] * qdi, u[2] * qdi);
              const Vec3<T> bwc = bw - mk<T>(u[0] * qddi, u[1] * qddi, u[2] * qddi) - cross(w, vJ);
              const Vec3<T> blc = bl - cross(v, vJ);
              const Vec3<T> wc = w - vJ;
              w = mul(R, wc);
              v = mul(R, v) - crossVC<T>(w, p);
              bw = mul(R, bwc);
              bl = mul(R, blc) - crossVC<T>(bw, p);
            }
          }
          if (nominal) { double* on = &L.bn[1 + leg][0]; on[0] = Fl.x.v; on[1] = Fl.y.v; on[2] = Fl.z.v; on[3] = Fn.x.v; on[4] = Fn.y.v; on[5] = Fn.z.v; }
          else { double* o = &L.bt[e][0]; o[0] = Fl.x.d; o[1] = Fl.y.d; o[2] = Fl.z.d; o[3] = Fn.x.d; o[4] = Fn.y.d; o[5] = Fn.z.d; }
        }
      }
      if (do_dyn) {
        waveLdsSync();
        // base rows: tau[0:6] = total spatial force on the base (S = identity): own term + legs, in leg order
        for (int e = lane; e < NV * 6; e += 64) {
          const int c = e / 6, r = e - 6 * c;
          double acc;
          if (c < 6) {
            acc = L.bown[c][r];
            for (int leg = 0; leg < NL; ++leg) acc += L.bt[leg * A_PER_LEG + c][r];
          } else {
            const int leg = (c - 6) / LJ;
            acc = L.bt[leg * A_PER_LEG + 6 + (c - 6 - leg * LJ)][r];
          }
          L.out[c][r] = acc;
        }
        if (lane < 6) {
          double acc = L.bn[0][lane];
          for (int leg = 0; leg < NL; ++leg) acc += L.bn[1 + leg][lane];
          L.idc[lane] = acc;
        }
      }
    }
    waveLdsSync();
    // ---- y = M^-1 (S^T u - h) ----
    for (int e = lane; e < NV * NV; e += 64) { const int c = e / NV, r = e - c * NV; L.minv[e] = L.out[c][r]; }
    if (lane < NV) {
      const double ui = (!IMPULSE && io.u && lane >= 6) ? io.u[sample * NU + (lane - 6)] : 0.0;
      L.r[lane] = ui - L.idc[lane];
    }
    waveLdsSync();
    blockArrowInverse<6, NL, LJ>(L.minv, NV, lane, &L.ok);
    if (lane < NV) {
      double acc = 0.0;
      for (int kk = 0; kk < NV; ++kk) acc += L.minv[lane + NV * kk] * L.r[kk];
      L.y[lane] = acc;
    }
    double x[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) x[i] = 0.0;
    if (dimf > 0) {
      // ---- the contact Schur complement over the packed active rows: S g = J y + b, g = -f ----
      for (int e = lane; e < NV * dimf; e += 64) {                       // T = M^-1 J^T
        const int i = e / NV, r = e - i * NV, jr = NV + L.prow[i];
        double acc = 0.0;
        for (int kk = 0; kk < NV; ++kk) acc += L.minv[r + NV * kk] * L.out[kk][jr];
        L.Tm[r + NV * i] = acc;
      }
      waveLdsSync();
      for (int e = lane; e < dimf * dimf; e += 64) {                     // S = J T
        const int j = e / dimf, i = e - j * dimf, jr = NV + L.prow[i];
        double acc = 0.0;
        for (int kk = 0; kk < NV; ++kk) acc += L.out[kk][jr] * L.Tm[kk + NV * j];
        L.Sm[i + NF * j] = acc;
      }
      if (lane < dimf) {
        const int jr = NV + L.prow[lane];
        double acc = L.idc[jr];
        for (int kk = 0; kk < NV; ++kk) acc += L.out[kk][jr] * L.y[kk];
        L.g[lane] = acc;
      }
      waveLdsSync();
#pragma unroll
      for (int i = 0; i < NF; ++i) x[i] = i < dimf ? L.g[i] : 0.0;        // (every lane keeps the right-hand side; the padding rows stay zero)
      choleskySolveRows<NF>(L.Sm, NF, lane, &L.ok, x, dimf);
      waveLdsSync();
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NF; ++i) L.g[i] = x[i];
      }
    }
    if (lane < NV) {
      double acc = L.y[lane];
#pragma unroll
      for (int i = 0; i < NF; ++i) if (i < dimf) acc -= L.Tm[lane + NV * i] * x[i];
      L.acc[lane] = acc;
    }
    waveLdsSync();
  }
  // ---- the requested outputs ----
  const double nan = __builtin_nan("");
  const bool ok = L.ok != 0;
  if (io.a && lane < NV) io.a[sample * NV + lane] = ok ? L.acc[lane] : nan;
  if (io.f && lane < NF) {
    const int c = lane / 3;
    const bool on = (active_mask >> c) & 1;
    const int pk = 3 * __builtin_popcount(active_mask & ((1 << c) - 1)) + (lane - 3 * c);
    io.f[sample * NF + lane] = ok ? (on ? -L.g[pk] : 0.0) : nan;
  }
  if (io.v_next && lane < NV) io.v_next[sample * NV + lane] = ok ? L.v[lane] + (IMPULSE ? 1.0 : dt) * L.acc[lane] : nan;
  if (io.q_next) {
    double* qn = io.q_next + sample * NQ;
    if (IMPULSE) { if (lane < NQ) qn[lane] = ok ? L.q[lane] : nan; }
    else {
      if (lane == 0) {
        double qb[7];
        lieIntegrateBase(L.q, L.v, dt, qb);
#pragma unroll
        for (int i = 0; i < 7; ++i) qn[i] = ok ? qb[i] : nan;
      }
      if (lane >= 6 && lane < NV) qn[lane + 1] = ok ? L.q[lane + 1] + dt * L.v[lane] : nan;
    }
  }
}

// One lane per sample: Cholesky solve of the NV x NV SPD M (column-major, only the lower triangle is read) for u - h, then the step.
template <int NV>
__global__ __launch_bounds__(64) void rbd_forward_chain_kernel(int n, const double* __restrict__ h, const double* __restrict__ M, const double* q, const double* v,
                                                               const double* __restrict__ u, double dt, double* __restrict__ a, double* q_next, double* v_next) {
  const long s = (long)blockIdx.x * 64 + threadIdx.x;
  if (s >= n) return;
  double qs[NV], vs[NV], x[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { qs[i] = q[s * NV + i]; vs[i] = v[s * NV + i]; }
  bool ok = true;
  if (a || v_next) {
    double Lm[NV][NV];
    const double* __restrict__ Ms = M + s * (NV * NV);
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
      for (int r = c; r < NV; ++r) Lm[r][c] = Ms[r + NV * c];
#pragma unroll
    for (int i = 0; i < NV; ++i) x[i] = (u ? u[s * NV + i] : 0.0) - h[s * NV + i];
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
#pragma unroll
    for (int i = 0; i < NV; ++i) {          // L z = r
      double t = x[i];
#pragma unroll
      for (int j = 0; j < i; ++j) t -= Lm[i][j] * x[j];
      x[i] = t / Lm[i][i];
    }
#pragma unroll
    for (int i = NV - 1; i >= 0; --i) {     // L^T a = z
      double t = x[i];
#pragma unroll
      for (int j = i + 1; j < NV; ++j) t -= Lm[j][i] * x[j];
      x[i] = t / Lm[i][i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < NV; ++i) x[i] = 0.0;
  }
  const double nan = __builtin_nan("");
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (a) a[s * NV + i] = ok ? x[i] : nan;
    if (v_next) v_next[s * NV + i] = ok ? vs[i] + dt * x[i] : nan;
    if (q_next) q_next[s * NV + i] = ok ? qs[i] + dt * vs[i] : nan;
  }
}

template <int NV>
void launchChain(int n, const double* h, const double* M, const double* q, const double* v, const double* u, double dt, double* a, double* q_next,
                 double* v_next, hipStream_t st) {
  hipLaunchKernelGGL((rbd_forward_chain_kernel<NV>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, n, h, M, q, v, u, dt, a, q_next, v_next);
}

}  // namespace

void rbdForwardQuadruped(const DevModel* m, const RbdFrames* frames, const idocp_rbd_fd_io_t& io, int n, int mode, int active_mask,
                         double time_step, double dt, hipStream_t st) {
  using D = LeggedDims<4, 3>;
  const dim3 grid((unsigned)((n + RBD_WAVES - 1) / RBD_WAVES)), block(64 * RBD_WAVES);
  if (mode == IDOCP_RBD_IMPULSE) hipLaunchKernelGGL((rbd_forward_kernel<D, true>), grid, block, 0, st, m, frames, io, n, active_mask, time_step, dt);
  else hipLaunchKernelGGL((rbd_forward_kernel<D, false>), grid, block, 0, st, m, frames, io, n, active_mask, time_step, dt);
}

void rbdForwardChainSolve(int nv, int n, const double* h, const double* M, const double* q, const double* v, const double* u, double dt,
                          double* a, double* q_next, double* v_next, hipStream_t st) {
  switch (nv) {
    case 2: launchChain<2>(n, h, M, q, v, u, dt, a, q_next, v_next, st); break;
    case 3: launchChain<3>(n, h, M, q, v, u, dt, a, q_next, v_next, st); break;
    case 4: launchChain<4>(n, h, M, q, v, u, dt, a, q_next, v_next, st); break;
    case 5: launchChain<5>(n, h, M, q, v, u, dt, a, q_next, v_next, st); break;
    case 6: launchChain<6>(n, h, M, q, v, u, dt, a, q_next, v_next, st); break;
    case 7: launchChain<7>(n, h, M, q, v, u, dt, a, q_next, v_next, st); break;
    case 8: launchChain<8>(n, h, M, q, v, u, dt, a, q_next, v_next, st); break;
    default: break;
  }
}

}  // namespace idocp_dev
