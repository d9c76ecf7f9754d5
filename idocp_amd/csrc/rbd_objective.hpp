// The objective of the rollout scoring (idocp_rbd_objective_create, idocp_rbd_score_rollout; include/idocp_hip.h), planned on the host: the
// configuration-space reference of every step by the solvers' own rules (cost_reference.hpp), the packed block of weights, bounds and switches the
// kernel reads (rbd_score_kernel.hip), the per-step contact masks of a call, and every refusal.  Plain C++17: this header includes no HIP runtime
// header (a CPU program defines IDOCP_NO_HIP_RUNTIME so that dev_lie.hpp brings none either; tests/cpp/rbd_objective_plan.cpp), rbd_capi.hip
// uploads what it plans.  The same objective serves idocp_rbd_objective_gradients and the LQR weight tables (planGradientCall, lqrWeights, at the
// end; tests/cpp/rbd_gradient_plan.cpp).
#ifndef IDOCP_RBD_OBJECTIVE_HPP_
#define IDOCP_RBD_OBJECTIVE_HPP_

#include <cmath>
#include <string>
#include <vector>

#include "cost_reference.hpp"
#include "idocp_hip.h"

namespace idocp_host {

// What the kernel reads besides the trajectories and the reference tables, as one block of device memory.  Rows r of the tangent space, joints j =
// r - (nv - nu) of the nu actuated ones.
struct RbdScoreBlock {
  double q_weight[IDOCP_MAX_NV], v_weight[IDOCP_MAX_NV], a_weight[IDOCP_MAX_NV], qf_weight[IDOCP_MAX_NV], vf_weight[IDOCP_MAX_NV];
  double u_weight[IDOCP_MAX_NV], u_ref[IDOCP_MAX_NV];
  double f_weight[IDOCP_MAX_CONTACTS][3], f_ref[IDOCP_MAX_CONTACTS][3];
  double q_min[IDOCP_MAX_NV], q_max[IDOCP_MAX_NV], v_max[IDOCP_MAX_NV], u_max[IDOCP_MAX_NV], a_min[IDOCP_MAX_NV], a_max[IDOCP_MAX_NV];
  double mu, dt;
  int position_limits, velocity_limits, torque_limits, acceleration_lower, acceleration_upper;
  int cone;      // 0 none, 1 LinearizedFrictionCone (five rows), 2 FrictionCone (two rows)
};

enum RbdScoreReads { RBD_SCORE_READS_U = 1, RBD_SCORE_READS_A = 2, RBD_SCORE_READS_F = 4 };

// 4 bits per step, 8 steps per word: the contact masks of one call travel as kernel arguments
constexpr int RBD_SCORE_MASK_WORDS = IDOCP_RBD_SCORE_MAX_WINDOW / 8;

struct RbdObjectivePlan {
  int rc = IDOCP_OK;
  std::string error;
  int steps = 0, nq = 0, nv = 0, nu = 0, ncontacts = 0;
  double t0 = 0.0, dt = 0.0;
  std::vector<double> q_ref, v_ref;      // [steps + 1][nq], [steps + 1][nv]: v_ref is vRefOnAt(t_k) times the cost's reference velocity
  RbdScoreBlock block;
  int reads = 0;                         // RbdScoreReads: the optional arrays an enabled weight or row reads
  bool has_constraints = false;          // created with an idocp_constraints_t (constraintRows below)
};

namespace rbd_objective_detail {

inline bool allFinite(const double* x, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false;
  return true;
}
inline bool anyNonZero(const double* x, int n) {
  for (int i = 0; i < n; ++i) if (x[i] != 0.0) return true;
  return false;
}

}  // namespace rbd_objective_detail

// floating: the model is the floating-base quadruped (else a fixed-base chain: nq == nv == nu, no contacts).  constraints may be null (none).
inline RbdObjectivePlan planObjective(const idocp_model_t& model, bool floating, const idocp_cost_t* cost, const idocp_constraints_t* constraints,
                                      double t0, double dt, int steps) {
  using namespace rbd_objective_detail;
  RbdObjectivePlan p;
  const std::string who = "idocp_rbd_objective_create: ";
  auto refuse = [&](int rc, const std::string& what) { p.rc = rc; p.error = who + what; return p; };
  if (!cost) return refuse(IDOCP_E_ARG, "null cost");
  if (steps < 1) return refuse(IDOCP_E_ARG, "steps must be at least 1");
  if (!std::isfinite(t0)) return refuse(IDOCP_E_ARG, "t0 must be finite");
  if (!std::isfinite(dt) || !(dt > 0.0)) return refuse(IDOCP_E_ARG, "dt must be positive and finite");
  const int nq = model.nq, nv = model.nv, nu = model.nu, nc = floating ? model.ncontacts : 0;
  // ---- what is not carried is refused, never dropped
  if (cost->task_dim != 0 || cost->task_extra_count != 0)
    return refuse(IDOCP_E_UNSUPPORTED, "task-space cost components (task_dim != 0) are not scored: a rollout is scored on its configuration-space, torque and contact-force terms");
  if (constraints && constraints->contact_distance) return refuse(IDOCP_E_UNSUPPORTED, "the ContactDistance constraint (contact_distance) is not scored");
  if (constraints && constraints->linearized_friction_cone && constraints->friction_cone)
    return refuse(IDOCP_E_UNSUPPORTED, "LinearizedFrictionCone and FrictionCone together: one cone is scored per contact");
  if (!floating && (cost->use_trotting_ref || cost->use_time_varying_ref))
    return refuse(IDOCP_E_UNSUPPORTED, "the trotting and the time-varying reference are rules of the floating-base quadruped; a chain takes the constant reference");
  // ---- values
  if (cost->use_trotting_ref && !cost->use_time_varying_ref && !(std::isfinite(cost->t_period) && cost->t_period > 0.0 && std::isfinite(cost->t_start)))
    return refuse(IDOCP_E_ARG, "use_trotting_ref needs a finite t_start and a positive finite t_period");
  if (cost->use_time_varying_ref && !(std::isfinite(cost->tv_t_begin) && std::isfinite(cost->tv_t_end)))
    return refuse(IDOCP_E_ARG, "use_time_varying_ref needs finite tv_t_begin and tv_t_end");
  const bool weights_ok = allFinite(cost->q_weight, nv) && allFinite(cost->v_weight, nv) && allFinite(cost->a_weight, nv) && allFinite(cost->qf_weight, nv) &&
                          allFinite(cost->vf_weight, nv) && allFinite(cost->u_weight, nu) && allFinite(&cost->f_weight[0][0], 3 * nc);
  if (!weights_ok) return refuse(IDOCP_E_ARG, "the cost weights must be finite");
  if (!(allFinite(cost->q_ref, nq) && allFinite(cost->v_ref, nv) && allFinite(cost->u_ref, nu) && allFinite(&cost->f_ref[0][0], 3 * nc)))
    return refuse(IDOCP_E_ARG, "the cost references must be finite");
  RbdScoreBlock& b = p.block;
  b = RbdScoreBlock();
  if (constraints) {
    const idocp_constraints_t& c = *constraints;
    p.has_constraints = true;
    b.position_limits = c.joint_position_limits != 0; b.velocity_limits = c.joint_velocity_limits != 0; b.torque_limits = c.joint_torque_limits != 0;
    b.acceleration_lower = c.joint_acceleration_lower_limit != 0; b.acceleration_upper = c.joint_acceleration_upper_limit != 0;
    b.cone = nc == 0 ? 0 : (c.linearized_friction_cone ? 1 : (c.friction_cone ? 2 : 0));
    // (a bound may be infinite -- that row is never active --, not NaN)
    auto noNan = [&](const double* x) { for (int j = 0; j < nu; ++j) if (std::isnan(x[j])) return false; return true; };
    if ((b.position_limits && !(noNan(model.q_min) && noNan(model.q_max))) || (b.velocity_limits && !noNan(model.v_max)) || (b.torque_limits && !noNan(model.u_max)))
      return refuse(IDOCP_E_ARG, "a joint limit of the model is NaN");
    if ((b.acceleration_lower && !noNan(c.a_min)) || (b.acceleration_upper && !noNan(c.a_max))) return refuse(IDOCP_E_ARG, "a joint acceleration bound is NaN");
    if (b.cone && !(std::isfinite(c.mu) && c.mu > 0.0)) return refuse(IDOCP_E_ARG, "a friction cone needs a positive finite mu");
    b.mu = c.mu;
    for (int j = 0; j < nu; ++j) { b.a_min[j] = c.a_min[j]; b.a_max[j] = c.a_max[j]; }
  }
  for (int r = 0; r < nv; ++r) {
    b.q_weight[r] = cost->q_weight[r]; b.v_weight[r] = cost->v_weight[r]; b.a_weight[r] = cost->a_weight[r];
    b.qf_weight[r] = cost->qf_weight[r]; b.vf_weight[r] = cost->vf_weight[r];
  }
  for (int j = 0; j < nu; ++j) {
    b.u_weight[j] = cost->u_weight[j]; b.u_ref[j] = cost->u_ref[j];
    b.q_min[j] = model.q_min[j]; b.q_max[j] = model.q_max[j]; b.v_max[j] = model.v_max[j]; b.u_max[j] = model.u_max[j];
  }
  for (int c = 0; c < nc; ++c) for (int x = 0; x < 3; ++x) { b.f_weight[c][x] = cost->f_weight[c][x]; b.f_ref[c][x] = cost->f_ref[c][x]; }
  b.dt = dt;
  if (anyNonZero(b.u_weight, nu) || b.torque_limits) p.reads |= RBD_SCORE_READS_U;
  if (anyNonZero(b.a_weight, nv) || b.acceleration_lower || b.acceleration_upper) p.reads |= RBD_SCORE_READS_A;
  if (nc && (anyNonZero(&b.f_weight[0][0], 3 * nc) || b.cone)) p.reads |= RBD_SCORE_READS_F;
  // ---- the reference tables
  p.steps = steps; p.nq = nq; p.nv = nv; p.nu = nu; p.ncontacts = nc; p.t0 = t0; p.dt = dt;
  p.q_ref.resize((size_t)(steps + 1) * nq);
  p.v_ref.resize((size_t)(steps + 1) * nv);
  for (int k = 0; k <= steps; ++k) {
    const double t = t0 + k * dt, on = vRefOnAt(*cost, t);
    qRefAt(*cost, nq, t, &p.q_ref[(size_t)k * nq]);
    double* vr = &p.v_ref[(size_t)k * nv];
    for (int r = 0; r < nv; ++r) vr[r] = on * cost->v_ref[r];
    if (cost->use_trotting_ref) vr[0] = on * (cost->step_length / cost->t_period);      // trotting_configuration_space_cost.cpp:81-83
  }
  if (!allFinite(p.q_ref.data(), (int)p.q_ref.size()) || !allFinite(p.v_ref.data(), (int)p.v_ref.size()))
    return refuse(IDOCP_E_ARG, "the reference of a step is not finite");
  return p;
}

// One call of the scoring against a planned objective: everything that can be refused without looking at device memory, and the masks.
struct RbdScoreCall {
  int rc = IDOCP_OK;
  std::string error;
  unsigned masks[RBD_SCORE_MASK_WORDS];
};
// have_*: the caller's pointer is not null
inline RbdScoreCall planScoreCall(const char* who_, const RbdObjectivePlan& o, int n, int first_step, int steps, const int* active, bool have_q, bool have_v,
                                  bool have_u, bool have_a, bool have_f) {
  RbdScoreCall c;
  for (int i = 0; i < RBD_SCORE_MASK_WORDS; ++i) c.masks[i] = 0u;
  const std::string who = std::string(who_) + ": ";
  auto refuse = [&](const std::string& what) { c.rc = IDOCP_E_ARG; c.error = who + what; return c; };
  if (n <= 0) return refuse("n must be positive");
  if (steps < 1) return refuse("steps must be at least 1");
  if (steps > IDOCP_RBD_SCORE_MAX_WINDOW) return refuse("at most IDOCP_RBD_SCORE_MAX_WINDOW = " + std::to_string(IDOCP_RBD_SCORE_MAX_WINDOW) + " steps per call (score window by window with accumulate)");
  if (first_step < 0 || first_step > o.steps - steps) return refuse("first_step + steps must lie within the objective's " + std::to_string(o.steps) + " steps");
  if (!have_q || !have_v) return refuse("q_traj and v_traj are needed");
  if (o.ncontacts == 0 && (active || have_f)) return refuse("a fixed-base chain has no contacts (active and f_traj must be NULL)");
  if (o.ncontacts && !active) return refuse("the contact status `active` is needed");
  if ((o.reads & RBD_SCORE_READS_U) && !have_u) return refuse("u_traj is NULL but a torque weight or the torque limits read it");
  if ((o.reads & RBD_SCORE_READS_A) && !have_a) return refuse("a_traj is NULL but an acceleration weight or the acceleration limits read it");
  if ((o.reads & RBD_SCORE_READS_F) && !have_f) return refuse("f_traj is NULL but a contact-force weight or the friction cone reads it");
  for (int k = 0; k < steps && o.ncontacts; ++k) {
    unsigned m = 0;
    for (int j = 0; j < o.ncontacts; ++j) if (active[(size_t)k * o.ncontacts + j]) m |= 1u << j;
    c.masks[k / 8] |= m << (4 * (k % 8));
  }
  return c;
}

// What idocp_rbd_objective_gradients and the LQR weights cannot carry (include/idocp_hip.h says why): "" when the objective is fine, else the
// text that names the term.
inline std::string gradientUnsupported(const RbdObjectivePlan& o) {
  using namespace rbd_objective_detail;
  if (anyNonZero(o.block.a_weight, o.nv))
    return "a non-zero a_weight: the gradient of the acceleration term needs da/dx, and its Hessian does not fit a diagonal x_weight / u_weight";
  if (o.ncontacts && anyNonZero(&o.block.f_weight[0][0], 3 * IDOCP_MAX_CONTACTS))
    return "a non-zero f_weight: the gradient of the contact-force term needs df/dx, and its Hessian does not fit a diagonal x_weight / u_weight";
  return "";
}

// One call of the gradients against a planned objective: everything that can be refused without looking at device memory.
struct RbdGradientCall {
  int rc = IDOCP_OK;
  std::string error;
};
// have_*: the caller's pointer is not null
inline RbdGradientCall planGradientCall(const char* who_, const RbdObjectivePlan& o, int n, int first_step, int steps, int terminal, bool have_q,
                                        bool have_v, bool have_u, bool have_lx, bool have_lu) {
  using namespace rbd_objective_detail;
  RbdGradientCall c;
  const std::string who = std::string(who_) + ": ";
  auto refuse = [&](int rc, const std::string& what) { c.rc = rc; c.error = who + what; return c; };
  const std::string unsupported = gradientUnsupported(o);
  if (!unsupported.empty()) return refuse(IDOCP_E_UNSUPPORTED, unsupported);
  if (n <= 0) return refuse(IDOCP_E_ARG, "n must be positive");
  if (steps < 1) return refuse(IDOCP_E_ARG, "steps must be at least 1");
  if (first_step < 0 || first_step > o.steps - steps)
    return refuse(IDOCP_E_ARG, "first_step + steps must lie within the objective's " + std::to_string(o.steps) + " steps");
  if (((long long)steps + (terminal ? 1 : 0)) * n > 2147483647LL) return refuse(IDOCP_E_ARG, "(steps + 1) * n must fit an int");
  if (!have_q || !have_v) return refuse(IDOCP_E_ARG, "q_traj and v_traj are needed");
  if (!have_u && anyNonZero(o.block.u_weight, o.nu)) return refuse(IDOCP_E_ARG, "u_traj is NULL but a non-zero u_weight reads it");
  if (!have_lx && !have_lu) return refuse(IDOCP_E_ARG, "no output was asked for (lx_traj, lu_traj)");
  return c;
}

// x_weight [2 nv] = dt [q_weight; v_weight], u_weight [nu] = dt u_weight, xf_weight [2 nv] = [qf_weight; vf_weight]: the diagonal weights
// idocp_rbd_lqr_io_t reads, behind one another in `out` (lqrWeightDoubles of them), each piece at an even number of doubles
inline int lqrWeightOffsetU(const RbdObjectivePlan& o) { return 2 * o.nv; }
inline int lqrWeightOffsetXf(const RbdObjectivePlan& o) { return 2 * o.nv + (o.nu + 1) / 2 * 2; }
inline int lqrWeightDoubles(const RbdObjectivePlan& o) { return lqrWeightOffsetXf(o) + 2 * o.nv; }
inline void lqrWeights(const RbdObjectivePlan& o, double* out) {
  const RbdScoreBlock& b = o.block;
  const int nv = o.nv, nu = o.nu, iu = lqrWeightOffsetU(o), ixf = lqrWeightOffsetXf(o);
  for (int i = 0; i < lqrWeightDoubles(o); ++i) out[i] = 0.0;
  for (int r = 0; r < nv; ++r) { out[r] = b.dt * b.q_weight[r]; out[nv + r] = b.dt * b.v_weight[r]; }
  for (int j = 0; j < nu; ++j) out[iu + j] = b.dt * b.u_weight[j];
  for (int r = 0; r < nv; ++r) { out[ixf + r] = b.qf_weight[r]; out[ixf + nv + r] = b.vf_weight[r]; }
}

// ---- the acceleration and contact-force terms as Gauss-Newton residual rows (idocp_rbd_linearize_rollout_cost; include/idocp_hip.h defines them)
// R = roundup4(nv + 3 ncontacts) rows: the accelerations, the contact forces, padding
inline int residualRows(int nv, int ncontacts) { return (nv + 3 * ncontacts + 3) / 4 * 4; }      // (of every objective of a model with these dimensions)
inline int residualRows(const RbdObjectivePlan& o) { return residualRows(o.nv, o.ncontacts); }
// "" when every a_weight and f_weight entry has a square root, else the text that names the term
inline std::string residualUnsupported(const RbdObjectivePlan& o) {
  for (int r = 0; r < o.nv; ++r) if (o.block.a_weight[r] < 0.0) return "a negative a_weight: a residual row needs its square root";
  for (int c = 0; c < o.ncontacts; ++c)
    for (int x = 0; x < 3; ++x) if (o.block.f_weight[c][x] < 0.0) return "a negative f_weight: a residual row needs its square root";
  return "";
}
// out [2 R]: the scales s_r = sqrt(dt w_r) of the rows, then the references of the rows (f_ref on the force rows, 0 elsewhere)
inline void residualTable(const RbdObjectivePlan& o, double* out) {
  const RbdScoreBlock& b = o.block;
  const int R = residualRows(o);
  for (int i = 0; i < 2 * R; ++i) out[i] = 0.0;
  for (int r = 0; r < o.nv; ++r) out[r] = std::sqrt(b.dt * b.a_weight[r]);
  for (int c = 0; c < o.ncontacts; ++c)
    for (int x = 0; x < 3; ++x) { out[o.nv + 3 * c + x] = std::sqrt(b.dt * b.f_weight[c][x]); out[R + o.nv + 3 * c + x] = b.f_ref[c][x]; }
}

// ---- the constraint rows as a squared-hinge penalty (idocp_rbd_score_penalty, idocp_rbd_linearize_rollout_penalty; include/idocp_hip.h defines them)
inline int coneRows(const RbdObjectivePlan& o) { return o.block.cone == 1 ? 5 : (o.block.cone == 2 ? 2 : 0); }
// Rc = roundup4(nu + ncone ncontacts) dense rows: the acceleration boxes, the cone rows, padding; 0 for an objective without constraints
inline int constraintRows(const RbdObjectivePlan& o) { return o.has_constraints ? (o.nu + coneRows(o) * o.ncontacts + 3) / 4 * 4 : 0; }
// L = 4 nu + ncone ncontacts multiplier rows per (step, sample) (idocp_rbd_objective_multiplier_rows): the q, v, u, a boxes, then the cone rows
inline int multiplierRows(const RbdObjectivePlan& o) { return o.has_constraints ? 4 * o.nu + coneRows(o) * o.ncontacts : 0; }
// "" when every enabled lower / upper pair has lo <= hi (the pair is then ONE signed row), else the text that names the pair
inline std::string penaltyPairRefused(const RbdObjectivePlan& o) {
  const RbdScoreBlock& b = o.block;
  for (int j = 0; j < o.nu; ++j) {
    const std::string at = " of actuated joint " + std::to_string(j) + " has lo > hi";
    if (b.position_limits && b.q_min[j] > b.q_max[j]) return "the pair (q_min, q_max)" + at;
    if (b.velocity_limits && b.v_max[j] < 0.0) return "the pair (-v_max, v_max)" + at;
    if (b.torque_limits && b.u_max[j] < 0.0) return "the pair (-u_max, u_max)" + at;
    if (b.acceleration_lower && b.acceleration_upper && b.a_min[j] > b.a_max[j]) return "the pair (a_min, a_max)" + at;
  }
  return "";
}
// One call of the penalty score: what is refused without looking at device memory, and the masks (those of planScoreCall).  An array is needed
// only where an enabled row reads it.
inline RbdScoreCall planPenaltyCall(const char* who_, const RbdObjectivePlan& o, int n, int first_step, int steps, const int* active, bool have_q,
                                    bool have_v, bool have_u, bool have_a, bool have_f) {
  RbdScoreCall c;
  for (int i = 0; i < RBD_SCORE_MASK_WORDS; ++i) c.masks[i] = 0u;
  const std::string who = std::string(who_) + ": ";
  auto refuse = [&](const std::string& what) { c.rc = IDOCP_E_ARG; c.error = who + what; return c; };
  const RbdScoreBlock& b = o.block;
  if (n <= 0) return refuse("n must be positive");
  if (steps < 1) return refuse("steps must be at least 1");
  if (steps > IDOCP_RBD_SCORE_MAX_WINDOW) return refuse("at most IDOCP_RBD_SCORE_MAX_WINDOW = " + std::to_string(IDOCP_RBD_SCORE_MAX_WINDOW) + " steps per call (score window by window with accumulate)");
  if (first_step < 0 || first_step > o.steps - steps) return refuse("first_step + steps must lie within the objective's " + std::to_string(o.steps) + " steps");
  const std::string pair = penaltyPairRefused(o);
  if (!pair.empty()) return refuse(pair);
  if (o.ncontacts == 0 && (active || have_f)) return refuse("a fixed-base chain has no contacts (active and f_traj must be NULL)");
  if (o.ncontacts && !active) return refuse("the contact status `active` is needed");
  if (b.position_limits && !have_q) return refuse("q_traj is NULL but the position limits read it");
  if (b.velocity_limits && !have_v) return refuse("v_traj is NULL but the velocity limits read it");
  if (b.torque_limits && !have_u) return refuse("u_traj is NULL but the torque limits read it");
  if ((b.acceleration_lower || b.acceleration_upper) && !have_a) return refuse("a_traj is NULL but the acceleration limits read it");
  if (b.cone && !have_f) return refuse("f_traj is NULL but the friction cone reads it");
  for (int k = 0; k < steps && o.ncontacts; ++k) {
    unsigned m = 0;
    for (int j = 0; j < o.ncontacts; ++j) if (active[(size_t)k * o.ncontacts + j]) m |= 1u << j;
    c.masks[k / 8] |= m << (4 * (k % 8));
  }
  return c;
}

}  // namespace idocp_host
#endif  // IDOCP_RBD_OBJECTIVE_HPP_
