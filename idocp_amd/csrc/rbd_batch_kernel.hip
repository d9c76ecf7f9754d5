// Batched rigid-body terms of a quadruped on plain arrays: inverse dynamics with contact forces, its derivatives, the Baumgarte /
// impulse-velocity constraint with its derivatives, and MJtJinv -- what Robot::RNEA, RNEADerivatives, computeBaumgarteResidual /
// Derivatives, RNEAImpulse(+Derivatives), computeImpulseVelocityResidual / Derivatives and computeMJtJinv give the reference
// (include/idocp/robot/robot.hxx:85-91, 262-283, 444-540, 576-615), for n independent samples (idocp_rbd_contact_dynamics_batch).
//
// One wavefront per sample, RBD_WAVES samples per workgroup, no workgroup barrier (a wavefront past the last sample leaves at once).
// The sweep is the one-tangent-per-lane form of ocp_rnea_kernel.hip: an ITEM = (seed, leg) carries the dual number (value, d / d seed)
// through one leg in registers, the columns meet in the wavefront's slice of LDS.  The items a call needs are chosen from what it asks
// for: the q and v seeds only for d / dq, d / dv outputs, the a seeds only for d / da outputs and MJtJinv, and a call that wants tau or C
// alone runs the four nominal items.  MJtJinv = [M J^T; J 0]^-1 over the active rows: M^-1 by the block-arrow inverse of dev_dense.hpp,
// the contact Schur complement (J M^-1 J^T)^-1 by its Cholesky inverse, the four blocks assembled on the way out.
#include <hip/hip_runtime.h>

#include "dev_dense.hpp"
#include "ocp_device.hpp"
#include "rbd_launch.hpp"

namespace idocp_dev {

namespace {

__device__ __forceinline__ void rbdQuatToRot(const double* __restrict__ qt, double* R) {
  const double x = qt[0], y = qt[1], z = qt[2], w = qt[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
}

template <typename D>
struct RbdWaveLds {
  static constexpr int NV = D::NV, NVF = D::NVF, NL = D::NL, LJ = D::LJ, NF = D::NF;
  static constexpr int IPL = 18 + 3 * LJ, NITEMS = NL * IPL;
  // column stride: odd, so that the lanes of a round, which write the same row of different columns, fall on different LDS banks
  // (NVF = 30 doubles would put 64 lanes on 16 bank pairs)
  static constexpr int LDC = NVF | 1;
  double out[3 * NV][LDC];      // column of each seed: rows [dID (NV) ; dC (NF, the rows of contact c at 3 c)]
  double bt[NITEMS][6];         // tangent of the force each item's leg transmits to the base   } dead once the columns are assembled:
  double bown[18][6];           // tangent of the base's own inertial force, per base seed       } the workspace of the MJtJinv blocks
  double bn[NL + 1][6];         // nominal base force: own, then per leg
  double idc[NVF];              // nominal [ID ; C]
  double cs[D::NU][2];          // cos / sin of the leg joint angles
  double v[NV], a[NV];          // velocity / acceleration inputs of the current pass
  int prow[NF];                 // packed contact row -> row of `out` behind NV
  int ok;
  // workspace of the MJtJinv blocks in bt .. bown (doubles): T = M^-1 J^T (NV x NF), S = J T (NF x NF), W of its inverse, T S^-1;
  // M^-1 itself lies over the q-seed columns of `out`, stored by then (only the a-seed columns, M and J, are read after that)
  static constexpr int W_T = 0, W_S = W_T + NV * NF, W_W = W_S + NF * NF, W_TS = W_W + NF * NF, W_END = W_TS + NV * NF;
  static_assert(W_END <= (NITEMS + 18) * 6, "the MJtJinv workspace fits the dead force tangents");
  static_assert(NV * NV <= NV * LDC, "M^-1 fits the q-seed columns");
};

// which items a call runs: all of them | the a seeds and the nominal items | the nominal items
enum { RBD_ITEMS_ALL = 0, RBD_ITEMS_A = 1, RBD_ITEMS_NOMINAL = 2 };

// registers capped at two wavefronts per SIMD, which is also what the LDS allows (four workgroups per CU): measured faster than the
// spill-free build at one wavefront per SIMD (-DIDOCP_RBD_WAVES_PER_SIMD=1; DESIGN.md 3.2b has both)
#ifndef IDOCP_RBD_WAVES_PER_SIMD
#define IDOCP_RBD_WAVES_PER_SIMD 2
#endif

template <typename D, bool IMPULSE>
__global__ __launch_bounds__(64 * RBD_WAVES, IDOCP_RBD_WAVES_PER_SIMD) void rbd_batch_kernel(const DevModel* __restrict__ m, const RbdFrames* __restrict__ P,
                                                                    idocp_rbd_io_t io, int n, int active_mask, double time_step) {
  using W = RbdWaveLds<D>;
  constexpr int NV = D::NV, NQ = D::NQ, NL = D::NL, LJ = D::LJ, NF = D::NF, NVF = D::NVF;
  constexpr int IPL = W::IPL, NITEMS = W::NITEMS, A_PER_LEG = 6 + LJ;
  typedef Dual T;
  __shared__ W s_wave[RBD_WAVES];
  const int lane = threadIdx.x & 63;
  const long sample = (long)blockIdx.x * RBD_WAVES + (threadIdx.x >> 6);
  if (sample >= n) return;                                // (no workgroup barrier below)
  W& L = s_wave[threadIdx.x >> 6];
  const double* __restrict__ q = io.q + sample * NQ;
  const double* __restrict__ vin = io.v + sample * NV;
  const double* __restrict__ ain = io.a + sample * NV;
  const double* __restrict__ fin = io.f ? io.f + sample * NF : nullptr;
  const double* __restrict__ cpin = io.contact_points ? io.contact_points + sample * NF : nullptr;
  const bool want_qv = io.dtau_dq || io.dtau_dv || io.dCdq || io.dCdv;
  const bool want_a = io.dtau_da || io.dCda || io.MJtJinv;
  const bool want_con = io.C || io.dCdq || io.dCdv || io.dCda || io.MJtJinv;
  const int items = want_qv ? RBD_ITEMS_ALL : (want_a ? RBD_ITEMS_A : RBD_ITEMS_NOMINAL);
  const int nidx = items == RBD_ITEMS_ALL ? NITEMS : (items == RBD_ITEMS_A ? NL + NL * A_PER_LEG : NL);
  if (lane < D::NU) {
    double sj, cj;
    sincos(q[7 + lane], &sj, &cj);
    L.cs[lane][0] = cj; L.cs[lane][1] = sj;
  }
  // zero the C rows of inactive contacts / rows a seed does not reach
  for (int r = lane; r < 3 * NV * W::LDC; r += 64) (&L.out[0][0])[r] = 0.0;
  if (lane < NVF) L.idc[lane] = 0.0;
  if (lane == 0) {
    L.ok = 1;
    int row = 0;
    for (int c = 0; c < NL; ++c)
      if ((active_mask >> c) & 1) { L.prow[row] = 3 * c; L.prow[row + 1] = 3 * c + 1; L.prow[row + 2] = 3 * c + 2; row += 3; }
  }
  const double gz = IMPULSE ? 0.0 : m->gravity[2];
  const double wv = 2.0 / time_step, wp = 1.0 / (time_step * time_step);
  double Rn[9];
  rbdQuatToRot(q + 3, Rn);

  constexpr int npass = IMPULSE ? 2 : 1;
#pragma unroll 1
  for (int pass = 0; pass < npass; ++pass) {
    // impulse: pass 0 is the dynamics at (v, a, g) = (0, dv, 0), pass 1 the kinematics at the velocity v + dv
    const bool do_dyn = (pass == 0), do_con = IMPULSE ? (pass == 1) : want_con;
    if (IMPULSE && pass == 1 && !want_con) break;
    waveLdsSync();
    if (lane < NV) {
      L.v[lane] = IMPULSE ? (pass == 0 ? 0.0 : vin[lane] + ain[lane]) : vin[lane];
      L.a[lane] = IMPULSE ? (pass == 0 ? ain[lane] : 0.0) : ain[lane];
    }
    waveLdsSync();
#pragma unroll 1
    for (int idx = lane; idx < nidx; idx += 64) {
      int item;
      if (items == RBD_ITEMS_ALL) item = idx;
      else if (idx < NL) item = idx * IPL;                                         // the nominal item of each leg (q seed of base coordinate 0)
      else { const int e = idx - NL, leg = e / A_PER_LEG, r = e - leg * A_PER_LEG; item = leg * IPL + (r < 6 ? 12 + r : 18 + 2 * LJ + (r - 6)); }
      const int leg = item / IPL, j0 = item - leg * IPL;
      const bool base_seed = j0 < 18;
      const int kind = base_seed ? j0 / 6 : (j0 - 18) / LJ;                           // 0: q, 1: v, 2: a
      const int k = base_seed ? j0 - 6 * kind : 6 + leg * LJ + (j0 - 18 - LJ * kind);   // velocity index of the seed
      double* __restrict__ col = &L.out[kind * NV + k][0];
      // velocity seeds: the v seeds; in the kinematic pass of the impulse mode also the a seeds (dC/ddv = dC/dv)
      const bool vseed = (kind == 1) || (IMPULSE && pass == 1 && kind == 2);
      const bool aseed = (kind == 2) && !(IMPULSE && pass == 1);
      const bool active = (active_mask >> leg) & 1;
      // ---- base (free-flyer): tangent of q (+) e_k on the manifold: dp = R e_lin, dR = R skew(e_ang) ----
      const double el[3] = {(kind == 0 && k == 0) ? 1.0 : 0.0, (kind == 0 && k == 1) ? 1.0 : 0.0, (kind == 0 && k == 2) ? 1.0 : 0.0};
      const double ea[3] = {(kind == 0 && k == 3) ? 1.0 : 0.0, (kind == 0 && k == 4) ? 1.0 : 0.0, (kind == 0 && k == 5) ? 1.0 : 0.0};
      Mat3<T> Rw;                                       // world pose of the current frame (starts at the base)
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        Rw.m[3 * r + 0] = T(Rn[3 * r + 0], Rn[3 * r + 1] * ea[2] - Rn[3 * r + 2] * ea[1]);
        Rw.m[3 * r + 1] = T(Rn[3 * r + 1], Rn[3 * r + 2] * ea[0] - Rn[3 * r + 0] * ea[2]);
        Rw.m[3 * r + 2] = T(Rn[3 * r + 2], Rn[3 * r + 0] * ea[1] - Rn[3 * r + 1] * ea[0]);
      }
      Vec3<T> pw = mk<T>(T(q[0], Rn[0] * el[0] + Rn[1] * el[1] + Rn[2] * el[2]), T(q[1], Rn[3] * el[0] + Rn[4] * el[1] + Rn[5] * el[2]),
                         T(q[2], Rn[6] * el[0] + Rn[7] * el[1] + Rn[8] * el[2]));
      auto seedV = [&](int i) { return T(L.v[i], (vseed && k == i) ? 1.0 : 0.0); };
      auto seedA = [&](int i) { return T(L.a[i], (aseed && k == i) ? 1.0 : 0.0); };
      Vec3<T> v = mk<T>(seedV(0), seedV(1), seedV(2)), w = mk<T>(seedV(3), seedV(4), seedV(5));
      // a_gf = a_joint + R^T (0, 0, -g_z)  (base acceleration in the gravity field)
      Vec3<T> bl = mk<T>(seedA(0) - gz * Rw.m[6], seedA(1) - gz * Rw.m[7], seedA(2) - gz * Rw.m[8]);
      Vec3<T> bw = mk<T>(seedA(3), seedA(4), seedA(5));
      if (do_dyn && leg == 0 && base_seed) {
        // the base's own inertial force: once per base seed (and once for the nominal value)
        Vec3<T> hl, hn, f, nn;
        inertiaMul<T>(m, 0, v, w, hl, hn);
        inertiaMul<T>(m, 0, bl, bw, f, nn);
        const Vec3<T> Fbl = f + cross(w, hl);
        const Vec3<T> Fbn = nn + cross(w, hn) + cross(v, hl);
        double* o = &L.bown[j0][0];
        o[0] = Fbl.x.d; o[1] = Fbl.y.d; o[2] = Fbl.z.d; o[3] = Fbn.x.d; o[4] = Fbn.y.d; o[5] = Fbn.z.d;
        if (j0 == 0) { double* on = &L.bn[0][0]; on[0] = Fbl.x.v; on[1] = Fbl.y.v; on[2] = Fbl.z.v; on[3] = Fbn.x.v; on[4] = Fbn.y.v; on[5] = Fbn.z.v; }
      }
      // ---- the leg of this item, outward ----
#pragma unroll 1
      for (int j = 0; j < LJ; ++j) {
        const int ji = 1 + leg * LJ + j, dof = 6 + leg * LJ + j, ci = leg * LJ + j;
        const bool mine = (k == dof);
        const T cqi(L.cs[ci][0], (mine && kind == 0) ? -L.cs[ci][1] : 0.0);
        const T sqi(L.cs[ci][1], (mine && kind == 0) ? L.cs[ci][0] : 0.0);
        const T qdi(L.v[dof], (mine && vseed) ? 1.0 : 0.0);
        const T qddi(L.a[dof], (mine && aseed) ? 1.0 : 0.0);
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
      Vec3<T> fel = mk<T>(T(0.0), T(0.0), T(0.0)), fen = fel;     // contact force as a spatial force on the tip joint
      if (active) {
        const double* Rc = P->R[leg];
        const double* pc = P->p[leg];
        const int row = NV + 3 * leg;
        if (do_con) {
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
            // contact-velocity constraint (point_contact.hxx:145-175): LOCAL linear velocity of the frame
            cx = fv.x.v; cy = fv.y.v; cz = fv.z.v;
            dx = fv.x.d; dy = fv.y.d; dz = fv.z.d;
          } else {
            const double px = cpin ? cpin[3 * leg] : 0.0, py = cpin ? cpin[3 * leg + 1] : 0.0, pz = cpin ? cpin[3 * leg + 2] : 0.0;
            // nominal residual (point_contact.hxx:67-87)
            cx = fa.x.v + (fw.y.v * fv.z.v - fw.z.v * fv.y.v) + wv * fv.x.v + wp * (pf.x.v - px);
            cy = fa.y.v + (fw.z.v * fv.x.v - fw.x.v * fv.z.v) + wv * fv.y.v + wp * (pf.y.v - py);
            cz = fa.z.v + (fw.x.v * fv.y.v - fw.y.v * fv.x.v) + wv * fv.z.v + wp * (pf.z.v - pz);
            // derivative column (point_contact.hxx:117-143): da_lin + skew(w) dv_lin + skew(v_lin) dw + (2/D) dv_lin + (1/D^2) dp_world
            dx = fa.x.d + (fw.y.v * fv.z.d - fw.z.v * fv.y.d) + (fv.y.v * fw.z.d - fv.z.v * fw.y.d) + wv * fv.x.d + wp * pf.x.d;
            dy = fa.y.d + (fw.z.v * fv.x.d - fw.x.v * fv.z.d) + (fv.z.v * fw.x.d - fv.x.v * fw.z.d) + wv * fv.y.d + wp * pf.y.d;
            dz = fa.z.d + (fw.x.v * fv.y.d - fw.y.v * fv.x.d) + (fv.x.v * fw.y.d - fv.y.v * fw.x.d) + wv * fv.z.d + wp * pf.z.d;
          }
          col[row] = dx; col[row + 1] = dy; col[row + 2] = dz;
          if (j0 == 0) { L.idc[row] = cx; L.idc[row + 1] = cy; L.idc[row + 2] = cz; }
        }
        if (fin) {
          // PointContact::computeJointForceFromContactForce (point_contact.hxx:15-20): jXf.act(Force(f, 0))
          const double* f = fin + 3 * leg;
          const double fx = Rc[0] * f[0] + Rc[1] * f[1] + Rc[2] * f[2], fy = Rc[3] * f[0] + Rc[4] * f[1] + Rc[5] * f[2],
                       fz = Rc[6] * f[0] + Rc[7] * f[1] + Rc[8] * f[2];
          fel = mk<T>(T(fx), T(fy), T(fz));
          fen = mk<T>(T(pc[1] * fz - pc[2] * fy), T(pc[2] * fx - pc[0] * fz), T(pc[0] * fy - pc[1] * fx));
        }
      }
      if (!do_dyn) continue;                          // kinematic pass of the impulse mode: no forces
      // ---- inward sweep: accumulate forces, emit tau, undo the kinematic steps ----
      Vec3<T> Fl = mk<T>(T(0.0), T(0.0), T(0.0)) - fel, Fn = mk<T>(T(0.0), T(0.0), T(0.0)) - fen;
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
        if (j0 == 0) L.idc[dof] = ti.v;
        const bool mine = (k == dof);
        const T cqi(L.cs[ci][0], (mine && kind == 0) ? -L.cs[ci][1] : 0.0);
        const T sqi(L.cs[ci][1], (mine && kind == 0) ? L.cs[ci][0] : 0.0);
        Mat3<T> R;
        revoluteRotation<T>(m->R[ji], m->axis[ji], cqi, sqi, R);
        const double* p = m->p[ji];
        const Vec3<T> Rf = mul(R, Fl);
        Fn = mul(R, Fn) + crossC<T>(p, Rf);
        Fl = Rf;
        if (j > 0) {
          const T qdi(L.v[dof], (mine && vseed) ? 1.0 : 0.0);
          const T qddi(L.a[dof], (mine && aseed) ? 1.0 : 0.0);
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
      {
        double* o = &L.bt[item][0];
        o[0] = Fl.x.d; o[1] = Fl.y.d; o[2] = Fl.z.d; o[3] = Fn.x.d; o[4] = Fn.y.d; o[5] = Fn.z.d;
        if (j0 == 0) { double* on = &L.bn[1 + leg][0]; on[0] = Fl.x.v; on[1] = Fl.y.v; on[2] = Fl.z.v; on[3] = Fn.x.v; on[4] = Fn.y.v; on[5] = Fn.z.v; }
      }
    }
    if (do_dyn) {
      waveLdsSync();
      // base rows: tau[0:6] = total spatial force on the base (S = identity): own term + legs, in leg order; only the kinds that ran
      const int kind0 = items == RBD_ITEMS_ALL ? 0 : 2, kind1 = items == RBD_ITEMS_NOMINAL ? 2 : 3;
      for (int e = kind0 * NV * 6 + lane; e < kind1 * NV * 6; e += 64) {
        const int c = e / 6, r = e - 6 * c, kind = c / NV, k = c - kind * NV;
        double acc;
        if (k < 6) {
          acc = L.bown[kind * 6 + k][r];
          for (int leg = 0; leg < NL; ++leg) acc += L.bt[leg * IPL + kind * 6 + k][r];
        } else {
          const int leg = (k - 6) / LJ;
          acc = L.bt[leg * IPL + 18 + LJ * kind + (k - 6 - leg * LJ)][r];
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
  // ---- the requested outputs, coalesced ----
  if (io.tau && lane < NV) io.tau[sample * NV + lane] = L.idc[lane];
  if (io.C && lane < NF) io.C[sample * NF + lane] = L.idc[NV + lane];
  auto storeDyn = [&](double* __restrict__ dst, int kind, bool zero) {
    if (!dst) return;
    dst += sample * (NV * NV);
    for (int e = lane; e < NV * NV; e += 64) { const int c = e / NV, r = e - c * NV; dst[e] = zero ? 0.0 : L.out[kind * NV + c][r]; }
  };
  auto storeCon = [&](double* __restrict__ dst, int kind) {
    if (!dst) return;
    dst += sample * (NF * NV);
    for (int e = lane; e < NF * NV; e += 64) { const int c = e / NF, r = e - c * NF; dst[e] = L.out[kind * NV + c][NV + r]; }
  };
  storeDyn(io.dtau_dq, 0, false);
  storeDyn(io.dtau_dv, 1, IMPULSE);       // (the impulse dynamics see no velocity)
  storeDyn(io.dtau_da, 2, false);
  storeCon(io.dCdq, 0);
  storeCon(io.dCdv, 1);
  storeCon(io.dCda, 2);
  if (!io.MJtJinv) return;
  // ---- MJtJinv = [M J^T; J 0]^-1 over the dimf active rows, packed (NV + dimf)^2 column-major ----
  const int dimf = 3 * __builtin_popcount(active_mask & ((1 << NL) - 1));
  double* __restrict__ ws = &L.bt[0][0];
  double *Tm = ws + W::W_T, *Sm = ws + W::W_S, *Wb = ws + W::W_W, *TS = ws + W::W_TS;
  double* __restrict__ minv = &L.out[0][0];
  waveLdsSync();                                                     // (the stores above have read the q-seed columns)
  for (int e = lane; e < NV * NV; e += 64) { const int c = e / NV, r = e - c * NV; minv[e] = L.out[2 * NV + c][r]; }
  waveLdsSync();
  blockArrowInverse<6, NL, LJ>(minv, NV, lane, &L.ok);
  for (int e = lane; e < NV * dimf; e += 64) {                       // T = M^-1 J^T
    const int i = e / NV, r = e - i * NV, jr = NV + L.prow[i];
    double acc = 0.0;
    for (int kk = 0; kk < NV; ++kk) acc += minv[r + NV * kk] * L.out[2 * NV + kk][jr];
    Tm[r + NV * i] = acc;
  }
  waveLdsSync();
  for (int e = lane; e < dimf * dimf; e += 64) {                     // S = J T
    const int j = e / dimf, i = e - j * dimf, jr = NV + L.prow[i];
    double acc = 0.0;
    for (int kk = 0; kk < NV; ++kk) acc += L.out[2 * NV + kk][jr] * Tm[kk + NV * j];
    Sm[i + NF * j] = acc;
  }
  waveLdsSync();
  if (dimf > 0) spdInverseCholDpp<NF>(Sm, NF, dimf, lane, &L.ok, Wb, NF);
  waveLdsSync();
  for (int e = lane; e < NV * dimf; e += 64) {                       // T S^-1: the off-diagonal blocks
    const int j = e / NV, r = e - j * NV;
    double acc = 0.0;
    for (int i = 0; i < dimf; ++i) acc += Tm[r + NV * i] * Sm[i + NF * j];
    TS[r + NV * j] = acc;
  }
  waveLdsSync();
  const int np = NV + dimf;
  double* __restrict__ o = io.MJtJinv + sample * (NVF * NVF);
  for (int e = lane; e < np * np; e += 64) {
    const int c = e / np, r = e - c * np;
    double val;
    if (r < NV && c < NV) {                                          // M^-1 - (T S^-1) T^T
      val = minv[r + NV * c];
      for (int i = 0; i < dimf; ++i) val -= TS[r + NV * i] * Tm[c + NV * i];
    } else if (r < NV) val = TS[r + NV * (c - NV)];
    else if (c < NV) val = TS[c + NV * (r - NV)];
    else val = -Sm[(r - NV) + NF * (c - NV)];
    o[e] = L.ok ? val : __builtin_nan("");
  }
}

}  // namespace

void rbdBatchQuadruped(const DevModel* m, const RbdFrames* frames, const idocp_rbd_io_t& io, int n, int mode, int active_mask,
                       double time_step, hipStream_t st) {
  using D = LeggedDims<4, 3>;
  const dim3 grid((unsigned)((n + RBD_WAVES - 1) / RBD_WAVES)), block(64 * RBD_WAVES);
  if (mode == IDOCP_RBD_IMPULSE) hipLaunchKernelGGL((rbd_batch_kernel<D, true>), grid, block, 0, st, m, frames, io, n, active_mask, time_step);
  else hipLaunchKernelGGL((rbd_batch_kernel<D, false>), grid, block, 0, st, m, frames, io, n, active_mask, time_step);
}

}  // namespace idocp_dev
