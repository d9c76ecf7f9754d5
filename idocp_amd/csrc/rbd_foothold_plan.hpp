// The schedule of the foothold rollout (idocp_rbd_rollout_footholds; rbd_capi.hip): per step the three contact masks its launches take.  Plain
// C++17 without a HIP call, so that a CPU program can hold the rule to its cases (tests/cpp/rbd_foothold_plan.cpp).
//
//   stage    bit c = contact c is active at step k: the status of the forward launch
//   impulse  the contacts the touchdown impulse in front of step k takes: active at k, not at k - 1; 0 at k = 0 and without touchdown_impulse
//   carry    bit c = stays(k, c) = active[k][c] && (k > 0 ? active[k - 1][c] : !latch_first): slice k of contact_points carries slice k - 1
//            (at k = 0 the caller's value); every other contact's entry is computed from q_traj[k]
#pragma once

namespace idocp_host {

struct FootholdStep { int stage, impulse, carry; };

inline int footholdMask(const int* active, int ncontacts) {
  int mask = 0;
  for (int c = 0; c < ncontacts; ++c) if (active[c]) mask |= 1 << c;
  return mask;
}

// active [steps][ncontacts], 0 <= k < steps
inline FootholdStep footholdStep(const int* active, int ncontacts, int k, bool touchdown_impulse, bool latch_first) {
  FootholdStep s;
  s.stage = footholdMask(active + (long)k * ncontacts, ncontacts);
  const int prev = k > 0 ? footholdMask(active + (long)(k - 1) * ncontacts, ncontacts) : 0;
  s.impulse = (touchdown_impulse && k > 0) ? (s.stage & ~prev) : 0;
  s.carry = k > 0 ? (s.stage & prev) : (latch_first ? 0 : s.stage);
  return s;
}

// whether any step of the schedule has an active contact (the Baumgarte time step is needed then)
inline bool footholdAnyActive(const int* active, int ncontacts, int steps) {
  for (long e = 0; e < (long)steps * ncontacts; ++e) if (active[e]) return true;
  return false;
}

}  // namespace idocp_host
