// The configuration-space reference of a stage time, as the cost components of the solvers define it: one copy for the OCP path (ocp_capi.hip
// fills its q_ref table and the nodes' vref_on with it) and for the objective of the rollout scoring (rbd_objective.hpp).  Host arithmetic only;
// the SE(3) retraction comes from dev_lie.hpp, which a plain C++ program takes without the HIP runtime header under IDOCP_NO_HIP_RUNTIME.
#ifndef IDOCP_COST_REFERENCE_HPP_
#define IDOCP_COST_REFERENCE_HPP_

#include <cmath>

#include "dev_lie.hpp"
#include "idocp_hip.h"

namespace idocp_host {

// (Trotting)ConfigurationSpaceCost reference of stage time t
// (include/idocp/cost/trotting_configuration_space_cost.hpp:126-164)
inline void qRefAt(const idocp_cost_t& c, int nq, double t, double* q_ref) {
  for (int i = 0; i < nq; ++i) q_ref[i] = c.q_ref[i];
  if (c.use_time_varying_ref) {
    // TimeVaryingConfigurationSpaceCost::set_q_ref (time_varying_configuration_space_cost.hpp:98-109):
    // q_begin (+) tau v_ref with tau = t - t_begin clamped to the window (q_end = q_begin (+) (t_end - t_begin) v_ref)
    const double tau = t <= c.tv_t_begin ? 0.0 : ((t < c.tv_t_end ? t : c.tv_t_end) - c.tv_t_begin);
    if (tau > 0.0) {
      double v6[6] = {c.v_ref[0], c.v_ref[1], c.v_ref[2], c.v_ref[3], c.v_ref[4], c.v_ref[5]}, qb[7];
      idocp_dev::lieIntegrateBase(c.q_ref, v6, tau, qb);
      for (int i = 0; i < 7; ++i) q_ref[i] = qb[i];
      for (int i = 7; i < nq; ++i) q_ref[i] = c.q_ref[i] + tau * c.v_ref[i - 1];
    }
    return;
  }
  if (!c.use_trotting_ref || !(t > c.t_start)) return;
  const double tau = t - c.t_start;
  const int steps = (int)std::floor(tau / c.t_period);
  const double rate = (tau - steps * c.t_period) / c.t_period;
  const double sin2 = std::sin(M_PI_2 * rate);
  q_ref[0] += (steps + rate) * c.step_length;
  if (steps % 2 == 0) {
    q_ref[9] -= sin2 * c.front_swing_knee;  q_ref[12] -= sin2 * c.hip_stance_knee;
    q_ref[15] += sin2 * c.front_stance_knee; q_ref[18] += sin2 * c.hip_swing_knee;
  } else {
    q_ref[9] += sin2 * c.front_stance_knee; q_ref[12] += sin2 * c.hip_swing_knee;
    q_ref[15] -= sin2 * c.front_swing_knee; q_ref[18] -= sin2 * c.hip_stance_knee;
  }
}

// TimeVaryingConfigurationSpaceCost::v_ref(t) (time_varying_configuration_space_cost.hpp:111-118): zero outside the window
inline double vRefOnAt(const idocp_cost_t& c, double t) {
  if (!c.use_time_varying_ref) return 1.0;
  return (t > c.tv_t_begin && t < c.tv_t_end) ? 1.0 : 0.0;
}

}  // namespace idocp_host
#endif  // IDOCP_COST_REFERENCE_HPP_
