// ParNMPC: the event stages of a horizon with discrete events (ParNMPCDiscretizer chain, see ocp_capi.hip).
//
//   lift stage      an ordinary backward-Euler stage with its own time step: K5a / K5b<BWD> / K9w as they are
//   aux stage       ordinary stage + the switching constraint P(q) = 0 of the impulse that follows (switching_constraint.hxx:
//                   8-21): K5s produces P, Pq; K5b<BWD> adds Pq^T xi; its KKT matrix has dimi more constraint rows
//                   (SplitKKTMatrixInverter::invert with Pq, split_kkt_matrix_inverter.hxx:110-166)  -> K9w's general instantiation (parnmpc_kkt_wave_kernel.hip)
//   impulse stage   ImpulseSplitParNMPC::linearizeOCP (impulse_split_parnmpc.hxx:33-60): impulse cost + impulse friction cone,
//                   linearizeImpulseBackwardEuler / condenseImpulseBackwardEuler (impulse_state_equation.hxx:59-111),
//                   ImpulseDynamicsBackwardEuler::linearizeImpulseDynamics / condenseImpulseDynamics
//                   (impulse_dynamics_backward_euler.hxx:20-97)                                  -> K9i below
//                   and its KKT matrix in (lmd, gmm, mu | f, q, v) (ImpulseSplitKKTMatrixInverter::invert,
//                   impulse_split_kkt_matrix_inverter.hxx:34-80)                                  -> K9w's general instantiation
//
// K9i writes the impulse stage into the SAME records as a regular stage, re-using their blocks
//   kkt:  K_QXX = Qxx, K_QXU = [Qqf; 0] (NX x ni), K_QUU = Qff (ni x ni), K_FQQ = Fqq6, K_FVQ = Fvq, K_FVV = -I,
//         K_FVU = Fvf (NV x ni), K_LX = (lq, lv), K_LU = lf, K_FX = (Fq, Fv)
//   swc:  W_P = V (contact-velocity residual), W_PHIX = [Vq Vv]
//   exp:  what K6 / K7 need for computeCondensed{Primal,Dual}Direction of the impulse stage
// so that the general inverse treats aux and impulse stages alike:  J = [F ; C], C = the W_PHIX rows on the (q, v) columns,
// Q over (w, q, v) with w = u (aux) or f (impulse).
#include <hip/hip_runtime.h>

#include "dev_dense.hpp"
#include "dev_lie.hpp"
#include "ocp_device.hpp"
#include "ocp_launch.hpp"

namespace idocp_dev {

// ---------------------------------------------------------------------------------------------------- K9i ----
// MERIT (with RESIDUAL): the line search's evaluation of a trial iterate on the impulse stage -- ImpulseSplitParNMPC::stageCost and
// constraintViolation (impulse_split_parnmpc.hxx:147-194): B.sol is the trial iterate, the lin / lie records have been rebuilt on it.
template <typename D, bool RESIDUAL, bool MERIT = false>
__global__ __launch_bounds__(256) void parnmpc_impulse_condense_kernel(OcpBuffers B, const double* __restrict__ q0, const double* __restrict__ v0) {
  using L = OcpLayout<D>;
  constexpr int NV = D::NV, NQ = D::NQ, NX = D::NX, NF = D::NF, NVF = D::NVF, NU = D::NU, NC = D::NC;
  __shared__ double Mi[NV * NV], Fvq[NV * NV], Fvf[NV * NF], Vq[NF * NV], Vv[NF * NV], dIq[NV * NV];
  __shared__ double lq[NV], lv[NV], ldv[NV], lf[NF], Fq[NV], Fv[NV], ImD[NV], Vr[NF], MiI[NV], qdd[NV], mu_p[NF], f_p[NF], err[256];
  __shared__ double Qff[NF * NF], Jq6[36], Fqq6[36], FqqI[36], FqqP[36], Fq6[6];
  __shared__ int s_ok;
  const OcpProblem* __restrict__ P = B.prob;
  const int tid = threadIdx.x;
  const int n_imp = gridDim.y;
  (void)n_imp;
  const long b = blockIdx.x;
  const int pos = B.impulse_pos[blockIdx.y];
  const OcpNode* __restrict__ nd = B.nodes + pos;
  const int ni = nd->dimf;
  const long rec = b * B.NS + nd->slot;
  const double* __restrict__ s = B.sol + rec * L::SOL;
  const double* __restrict__ sn = B.sol + (b * B.NS + nd->next) * L::SOL;
  const double* __restrict__ sp = nd->prev >= 0 ? B.sol + (b * B.NS + nd->prev) * L::SOL : nullptr;
  const double* __restrict__ lin = B.lin + rec * L::LIN;
  const double* __restrict__ zz = B.lie + rec * L::LIE;
  const double* __restrict__ qref = B.q_ref + (long)pos * NQ;
  const double* __restrict__ slack = B.slack + rec * L::CON;
  const double* __restrict__ dual = B.dual + rec * L::CON;
  const bool cone = P->use_impulse_friction_cone != 0;
  const double vref_on = nd->vref_on;
  if (tid == 0) s_ok = 1;
  // ---- load: dImD/dq, M, Vq, Vv, ImD, V (lin record of the impulse pass of K5a), the Lie-group blocks ----
  for (int e = tid; e < NV * NV; e += 256) { const int c = e / NV, r = e - c * NV; dIq[e] = lin[L::L_DIDC + r + NVF * c]; Mi[e] = lin[L::L_M + e]; }
  for (int e = tid; e < ni * NV; e += 256) {
    const int c = e / ni, j = e - c * ni;
    Vq[j + NF * c] = lin[L::L_DIDC + (NV + j) + NVF * c];
    Vv[j + NF * c] = lin[L::L_DIDC + (NV + j) + NVF * (NV + c)];
  }
  if (tid < NV) ImD[tid] = lin[L::L_IDC + tid];
  if (tid < ni) Vr[tid] = lin[L::L_IDC + NV + tid];
  if (tid < 36) { Jq6[tid] = zz[L::Z_JQ + tid]; FqqP[tid] = zz[L::Z_FQQP + tid]; FqqI[tid] = zz[L::Z_FQQI + tid]; Fqq6[tid] = zz[L::Z_FQQ + tid]; }
  if (tid < 6) { Fq6[tid] = zz[L::Z_FQ6 + tid]; qdd[tid] = zz[L::Z_QDIFF + tid]; }
  if (tid < NC && nd->active[tid]) for (int x = 0; x < 3; ++x) { mu_p[nd->row_of[tid] + x] = s[L::S_MU + 3 * tid + x]; f_p[nd->row_of[tid] + x] = s[L::S_F + 3 * tid + x]; }
  for (int e = tid; e < NF * NF; e += 256) Qff[e] = 0.0;
  blockLdsSync();
  // ---- impulse cost, state equation, multipliers of the impulse dynamics and of the velocity constraint: gradients ----
  if (tid < NV) {
    const int r = tid;
    const double q_r = s[L::S_Q + (r < 6 ? r : r + 1)];
    (void)q_r;
    const double vr = s[L::S_V + r], dvr = s[L::S_A + r];
    const double lmd = s[L::S_LMD + r], gmm = s[L::S_GMM + r], lmdn = sn[L::S_LMD + r], gmmn = sn[L::S_GMM + r];
    const double vpr = sp ? sp[L::S_V + r] : v0[b * NV + r];
    double a_q, a_v, a_dv;
    if (r < 6) {
      a_q = 0.0;
      for (int m2 = 0; m2 < 6; ++m2) a_q += Jq6[m2 + 6 * r] * P->qi_weight[m2] * qdd[m2];
      double t1 = 0.0;
      for (int m2 = 0; m2 < 6; ++m2) t1 += Fqq6[m2 + 6 * r] * sn[L::S_LMD + m2] + FqqP[m2 + 6 * r] * s[L::S_LMD + m2];
      a_q += t1;
      Fq[r] = Fq6[r];
    } else {
      const double qpr = sp ? sp[L::S_Q + r + 1] : q0[b * NQ + r + 1];
      a_q = P->qi_weight[r] * (s[L::S_Q + r + 1] - qref[r + 1]) + lmdn - lmd;
      Fq[r] = qpr - s[L::S_Q + r + 1];
    }
    a_v = P->vi_weight[r] * (vr - vref_on * P->v_ref[r]) - gmm + gmmn;
    a_dv = P->dvi_weight[r] * dvr + gmm;
    Fv[r] = vpr - vr + dvr;
    // + dImD/dq^T beta, + M^T beta, + Vq^T mu, + Vv^T mu
    double dq = 0.0, dm = 0.0;
    for (int m = 0; m < NV; ++m) { dq += dIq[m + NV * r] * s[L::S_BETA + m]; dm += Mi[m + NV * r] * s[L::S_BETA + m]; }
    a_q += dq; a_dv += dm;
    if (B.ext) a_q += B.ext[rec * L::EXT + L::X_LQ + r];      // task-space cost with its impulse weights (ocp_ext_kernel.hip)
    double vq = 0.0, vv = 0.0;
    for (int j = 0; j < ni; ++j) { vq += Vq[j + NF * r] * mu_p[j]; vv += Vv[j + NF * r] * mu_p[j]; }
    a_q += vq; a_v += vv;
    lq[r] = a_q; lv[r] = a_v; ldv[r] = a_dv;
  }
  // lf of the contacts that touch down: impulse force cost + cone + (- Vv beta)
  double e_ipm = 0.0, m_cost = 0.0, m_viol = 0.0;
  if (tid >= 64 && tid < 64 + NC && nd->active[tid - 64]) {
    const int c = tid - 64, row = nd->row_of[c];
    // (Linearized)ImpulseFrictionCone, row by row (coneRow, ocp_device.hpp)
    const int ck = P->impulse_cone_kind, nr = coneRows(ck);
    const double fc[3] = {s[L::S_F + 3 * c], s[L::S_F + 3 * c + 1], s[L::S_F + 3 * c + 2]};
    double rr[5], ddv[5], Jr[5][3];
    for (int r = 0; r < 5; ++r) {
      if (r >= nr) { rr[r] = 0.0; ddv[r] = 0.0; Jr[r][0] = Jr[r][1] = Jr[r][2] = 0.0; continue; }
      const int idx = L::C_FRIC + 5 * c + r;
      const double g = coneRow(ck, P->mu, r, fc, Jr[r]);
      const double sl = slack[idx], du = dual[idx];
      const double res = g + sl, duality = sl * du - P->barrier;
      if (RESIDUAL) { rr[r] = du; ddv[r] = 0.0; e_ipm += res * res + duality * duality; if (MERIT && cone) m_viol += fabs(res); }
      else { rr[r] = du + (du * res - duality) / sl; ddv[r] = du / sl; }
    }
    for (int x = 0; x < 3; ++x) {
      double a = P->fi_weight[c][x] * (s[L::S_F + 3 * c + x] - P->fi_ref[c][x]);
      if (MERIT) m_cost += 0.5 * a * (s[L::S_F + 3 * c + x] - P->fi_ref[c][x]);      // ImpulseForceCost::computeImpulseCost
      if (cone) for (int r = 0; r < 5; ++r) a += Jr[r][x] * rr[r];
      double vb = 0.0;
      for (int m = 0; m < NV; ++m) vb += Vv[(row + x) + NF * m] * s[L::S_BETA + m];
      lf[row + x] = a - vb;
      if (!RESIDUAL) {
        for (int y = 0; y < 3; ++y) {
          double h = (x == y) ? P->fi_weight[c][x] : 0.0;
          if (cone) for (int r = 0; r < 5; ++r) h += Jr[r][x] * ddv[r] * Jr[r][y];
          Qff[(row + x) + NF * (row + y)] = h;
        }
      }
    }
    if (!cone) e_ipm = 0.0;
  }
  blockLdsSync();
  if (MERIT) {
    if (tid < NV) {
      const int r = tid;
      const double qd = r < 6 ? qdd[r] : s[L::S_Q + r + 1] - qref[r + 1];
      const double dvr = s[L::S_V + r] - vref_on * P->v_ref[r], ddv = s[L::S_A + r];
      m_cost += 0.5 * (P->qi_weight[r] * qd * qd + P->vi_weight[r] * dvr * dvr + P->dvi_weight[r] * ddv * ddv);
      m_viol += fabs(Fq[r]) + fabs(Fv[r]) + fabs(ImD[r]);
    }
    if (tid < ni) m_viol += fabs(Vr[tid]);
    if (tid == 0 && B.ext) m_cost += B.ext[rec * L::EXT + L::X_COST];
    err[tid] = m_cost;
    blockLdsSync();
    if (tid == 0) { double acc = 0.0; for (int t = 0; t < 256; ++t) acc += err[t]; B.merit_stage[rec * 4] = acc; }
    blockLdsSync();
    err[tid] = m_viol;
    blockLdsSync();
    if (tid == 0) { double acc = 0.0; for (int t = 0; t < 256; ++t) acc += err[t]; B.merit_stage[rec * 4 + 1] = acc; }
    return;
  }
  if (RESIDUAL) {
    // ImpulseSplitParNMPC::squaredNormKKTResidual (impulse_split_parnmpc.hxx:114-124)
    double e = e_ipm;
    if (tid < NV) e += lq[tid] * lq[tid] + lv[tid] * lv[tid] + ldv[tid] * ldv[tid] + Fq[tid] * Fq[tid] + Fv[tid] * Fv[tid] + ImD[tid] * ImD[tid];
    if (tid < ni) e += lf[tid] * lf[tid] + Vr[tid] * Vr[tid];
    err[tid] = e;
    blockLdsSync();
    if (tid == 0) { double acc = 0.0; for (int t = 0; t < 256; ++t) acc += err[t]; B.err_stage[rec] = acc; }
    return;
  }
  double* __restrict__ kk = B.kkt + rec * L::KKT;
  double* __restrict__ ee = B.exp + rec * L::EXP;
  double* __restrict__ W = B.swc + rec * L::SWC;
  // ---- condenseImpulseBackwardEuler: Fqq = Fqq_inv Fqq(q_prev, q), Fq.head(6) = Fqq_inv Fq.head(6) ----
  if (tid < 36) {
    const int c = tid / 6, r = tid - 6 * c;
    double acc = 0.0;
    for (int m = 0; m < 6; ++m) acc += FqqI[r + 6 * m] * FqqP[m + 6 * c];
    kk[L::K_FQQ + tid] = acc;
    kk[L::K_FQV + tid] = 0.0;
    ee[L::E_FQQPI + tid] = FqqI[tid];
  } else if (tid >= 64 && tid < 70) {
    const int r = tid - 64;
    double acc = 0.0;
    for (int m = 0; m < 6; ++m) acc += FqqI[r + 6 * m] * Fq6[m];
    Fq[r] = acc;
  }
  // ---- Minv (Robot::computeMinv), Fvq = -Minv dImD/dq, Fvf = Minv Vv^T, Minv ImD ----
  blockLdsSync();
  if (tid < 64) spdInverseRows<NV>(Mi, NV, NV, tid, &s_ok);
  blockLdsSync();
  for (int e = tid; e < NV * NV; e += 256) {
    const int c = e / NV, r = e - c * NV;
    double acc = 0.0;
    for (int m = 0; m < NV; ++m) acc += Mi[r + NV * m] * dIq[m + NV * c];
    Fvq[e] = -acc;
  }
  for (int e = tid; e < NV * ni; e += 256) {
    const int j = e / NV, r = e - j * NV;
    double acc = 0.0;
    for (int m = 0; m < NV; ++m) acc += Mi[r + NV * m] * Vv[j + NF * m];
    Fvf[r + NV * j] = acc;
  }
  if (tid >= 192 && tid < 192 + NV) {
    const int r = tid - 192;
    double acc = 0.0;
    for (int m = 0; m < NV; ++m) acc += Mi[r + NV * m] * ImD[m];
    MiI[r] = acc;
  }
  blockLdsSync();
  if (tid < NV) ldv[tid] -= P->dvi_weight[tid] * MiI[tid];            // data.ldv = ldv - Qdvdv Minv ImD
  blockLdsSync();
  // ---- condensed blocks (Qdvq = Qdvdv Fvq, Qdvf = Qdvdv Fvf) ----
  // Qxx = [Qqq 0; 0 Qvv]
  for (int e = tid; e < NX * NX; e += 256) {
    const int c = e / NX, r = e - c * NX;
    double v = 0.0;
    if (r < NV && c < NV) {
      if (r < 6 && c < 6) { for (int m2 = 0; m2 < 6; ++m2) v += Jq6[m2 + 6 * r] * P->qi_weight[m2] * Jq6[m2 + 6 * c]; }
      else if (r == c) v = P->qi_weight[r];
      double acc = 0.0;
      for (int m = 0; m < NV; ++m) acc += Fvq[m + NV * r] * (P->dvi_weight[m] * Fvq[m + NV * c]);
      v += acc;
      if (B.ext) {                                   // JJ^T diag(w_i) JJ of the task-space cost (the rows ocp_ext_kernel left)
        const double* __restrict__ xx = B.ext + rec * L::EXT;
        for (int k = 0; k < 6 * L::NT; ++k) v += xx[L::X_TW + k] * xx[L::X_TJ + k * NV + r] * xx[L::X_TJ + k * NV + c];      // (unused component slots: zero weights)
      }
    } else if (r == c) {
      v = P->vi_weight[r - NV];
    }
    if (r <= c) kk[L::K_QXX + L::xsym(r, c)] = v;
  }
  // Qxf = [Qqf; 0] in the place of Qxu, Qff in the place of Quu, Fvf in the place of Fvu
  for (int e = tid; e < NX * NU; e += 256) {
    const int j = e / NX, r = e - j * NX;
    double v = 0.0;
    if (r < NV && j < ni) for (int m = 0; m < NV; ++m) v += Fvq[m + NV * r] * (P->dvi_weight[m] * Fvf[m + NV * j]);
    kk[L::K_QXU + e] = v;
  }
  for (int e = tid; e < NU * NU; e += 256) {
    const int c = e / NU, r = e - c * NU;
    double v = 0.0;
    if (r < ni && c < ni) {
      v = Qff[r + NF * c];
      double acc = 0.0;
      for (int m = 0; m < NV; ++m) acc += Fvf[m + NV * r] * (P->dvi_weight[m] * Fvf[m + NV * c]);
      v += acc;
    } else if (r == c) v = 1.0;
    kk[L::K_QUU + e] = v;
  }
  for (int e = tid; e < NV * NV; e += 256) {
    const int c = e / NV, r = e - c * NV;
    kk[L::K_FVQ + e] = Fvq[e];
    kk[L::K_FVV + e] = (r == c) ? -1.0 : 0.0;
    if (r >= c) ee[L::E_MJ + r * (r + 1) / 2 + c] = Mi[e];      // Minv is symmetric: the exp record keeps the lower triangle (ocp_device.hpp)
  }
  for (int e = tid; e < NV * NU; e += 256) {
    const int j = e / NV;
    kk[L::K_FVU + e] = j < ni ? Fvf[e] : 0.0;
  }
  // gradients, residuals
  if (tid < NV) {
    const int r = tid;
    double aq = 0.0;
    for (int m = 0; m < NV; ++m) aq += Fvq[m + NV * r] * ldv[m];
    kk[L::K_LX + r] = lq[r] + aq;
    kk[L::K_LX + NV + r] = lv[r];
    kk[L::K_FX + r] = Fq[r];
    kk[L::K_FX + NV + r] = Fv[r] - MiI[r];
    ee[L::E_MJIDC + r] = MiI[r];
    ee[L::E_LAF + r] = ldv[r];
    ee[L::E_QAA + r] = P->dvi_weight[r];             // Qdvdv
  }
  if (tid >= 64 && tid < 64 + NU) {
    const int j = tid - 64;
    double v = 0.0;
    if (j < ni) { v = lf[j]; double af = 0.0; for (int m = 0; m < NV; ++m) af += Fvf[m + NV * j] * ldv[m]; v += af; }
    kk[L::K_LU + j] = v;
  }
  // the contact-velocity constraint rows
  if (tid >= 128 && tid < 128 + NF) W[L::W_P + tid - 128] = (tid - 128 < ni) ? Vr[tid - 128] : 0.0;
  for (int e = tid; e < NF * NX; e += 256) {
    const int c = e / NF, j = e - c * NF;
    W[L::W_PHIX + e] = j < ni ? (c < NV ? Vq[j + NF * c] : Vv[j + NF * (c - NV)]) : 0.0;
  }
  if (tid == 0 && !s_ok && B.status[b] == 0) B.status[b] = 2000 + pos;
}

template <typename D>
void OcpLaunch<D>::parnmpcImpulseCondense(const OcpBuffers& B, long batch, int n_impulse, bool residual, const double* q0, const double* v0,
                                          hipStream_t st) {
  if (n_impulse <= 0) return;
  if (residual) hipLaunchKernelGGL((parnmpc_impulse_condense_kernel<D, true>), dim3((unsigned)batch, (unsigned)n_impulse), dim3(256), 0, st, B, q0, v0);
  else hipLaunchKernelGGL((parnmpc_impulse_condense_kernel<D, false>), dim3((unsigned)batch, (unsigned)n_impulse), dim3(256), 0, st, B, q0, v0);
}

// line search: stage cost and l1 violation of the impulse stages of the trial iterate Btry.sol points at (after K5a's impulse pass and
// the Lie-group kernel on Btry; overwrites what the stage kernel left in merit_stage for these slots)
template <typename D>
void OcpLaunch<D>::parnmpcImpulseMerit(const OcpBuffers& Btry, long batch, int n_impulse, const double* q0, const double* v0, hipStream_t st) {
  if (n_impulse <= 0) return;
  hipLaunchKernelGGL((parnmpc_impulse_condense_kernel<D, true, true>), dim3((unsigned)batch, (unsigned)n_impulse), dim3(256), 0, st, Btry, q0, v0);
}

template void OcpLaunch<LeggedDims<4, 3>>::parnmpcImpulseCondense(const OcpBuffers&, long, int, bool, const double*, const double*, hipStream_t);
template void OcpLaunch<LeggedDims<4, 3>>::parnmpcImpulseMerit(const OcpBuffers&, long, int, const double*, const double*, hipStream_t);

}  // namespace idocp_dev
