// The model shapes the kernels of this build are compiled for, and the conversion of the flat model into the device block: shared by
// the C-ABI translation units (ocp_capi.hip, unocp_capi.hip, rbd_capi.hip), so that every entry point accepts and refuses the same models.
#ifndef IDOCP_MODEL_SHAPES_HPP_
#define IDOCP_MODEL_SHAPES_HPP_

#include <cmath>
#include <cstring>

#include "dev_rbd.hpp"
#include "idocp_hip.h"
#include "ocp_device.hpp"

namespace idocp_host {

inline void toDevModel(const idocp_model_t& m, idocp_dev::DevModel& d) {
  std::memset(&d, 0, sizeof(d));
  d.njoints = m.njoints; d.nq = m.nq; d.nv = m.nv; d.nu = m.nu; d.has_floating_base = m.has_floating_base;
  for (int i = 0; i < m.njoints; ++i) {
    d.parent[i] = m.parent[i]; d.jtype[i] = m.jtype[i]; d.idx_q[i] = m.idx_q[i]; d.idx_v[i] = m.idx_v[i];
    std::memcpy(d.axis[i], m.axis[i], sizeof(double) * 3);
    std::memcpy(d.R[i], m.plc_R[i], sizeof(double) * 9);
    std::memcpy(d.p[i], m.plc_p[i], sizeof(double) * 3);
    d.mass[i] = m.mass[i];
    const double* c = m.com[i];
    const double* I = m.inertia[i];
    const double ms = m.mass[i];
    for (int k = 0; k < 3; ++k) d.mc[i][k] = ms * c[k];
    // Io = Ic + m (c.c 1 - c c^T)   (inertia about the joint-frame origin)
    const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    d.Io[i][0] = I[0] + ms * (cc - c[0] * c[0]);
    d.Io[i][1] = I[1] - ms * c[0] * c[1];
    d.Io[i][2] = I[2] - ms * c[0] * c[2];
    d.Io[i][3] = I[4] + ms * (cc - c[1] * c[1]);
    d.Io[i][4] = I[5] - ms * c[1] * c[2];
    d.Io[i][5] = I[8] + ms * (cc - c[2] * c[2]);
  }
  std::memcpy(d.gravity, m.gravity, sizeof(double) * 3);
}

// free-flyer (identity placement) + 4 chains of 3 revolute joints, contact c on the tip joint of leg c
inline bool isQuadruped(const idocp_model_t& m) {
  using DQ = idocp_dev::LeggedDims<4, 3>;
  if (!m.has_floating_base || m.njoints != DQ::NJ || m.nv != DQ::NV || m.nq != DQ::NQ || m.ncontacts != DQ::NC) return false;
  if (m.jtype[0] != IDOCP_JOINT_FREEFLYER || m.parent[0] != -1) return false;
  const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int k = 0; k < 9; ++k) if (std::fabs(m.plc_R[0][k] - I3[k]) > 1e-14) return false;
  for (int k = 0; k < 3; ++k) if (std::fabs(m.plc_p[0][k]) > 1e-14) return false;
  for (int leg = 0; leg < DQ::NL; ++leg)
    for (int j = 0; j < DQ::LJ; ++j) {
      const int ji = 1 + leg * DQ::LJ + j;
      if (m.jtype[ji] != IDOCP_JOINT_REVOLUTE || m.parent[ji] != (j == 0 ? 0 : ji - 1) || m.idx_v[ji] != 6 + leg * DQ::LJ + j) return false;
    }
  for (int c = 0; c < DQ::NC; ++c) if (m.contact_joint[c] != DQ::LJ * (c + 1)) return false;
  return true;
}
constexpr const char* QUADRUPED_SHAPE = "a floating-base quadruped (4 legs x 3 revolute joints, 4 point contacts on the tip joints)";

// The UnOCP kernels are compiled for serial chains of UN_MIN_NV .. UN_MAX_NV revolute joints (unocp_kernels.hip instantiates UnLaunch<NV>
// for each).
constexpr int UN_MIN_NV = 2, UN_MAX_NV = 8;
inline bool isRevoluteChain(const idocp_model_t& m) {
  const int nv = m.nv;
  if (nv < UN_MIN_NV || nv > UN_MAX_NV) return false;
  if (m.njoints != nv || m.nq != nv || m.has_floating_base || m.ncontacts != 0) return false;
  for (int i = 0; i < nv; ++i)
    if (m.parent[i] != i - 1 || m.jtype[i] != IDOCP_JOINT_REVOLUTE || m.idx_v[i] != i) return false;
  return true;
}
constexpr const char* CHAIN_RANGE = "a fixed-base serial chain of 2 .. 8 revolute joints";

}  // namespace idocp_host
#endif  // IDOCP_MODEL_SHAPES_HPP_
