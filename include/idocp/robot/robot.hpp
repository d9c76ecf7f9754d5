// idocp::Robot -- facade over the C ABI (include/idocp_hip.h).
// Mirrors the part of the reference class the drivers of the hot path use
// (include/idocp/robot/robot.hpp:26; src/robot/robot.cpp:8-85,113-170).
#ifndef IDOCP_ROBOT_HPP_
#define IDOCP_ROBOT_HPP_

#include <cstdlib>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "idocp/eigen_shim.hpp"
#include "idocp/robot/contact_status.hpp"
#include "idocp/robot/impulse_status.hpp"
#include "idocp/pinocchio_shim.hpp"
#include "idocp_hip.h"

namespace idocp {

class Robot {
 public:
  // Robot(path_to_urdf) / Robot(path_to_urdf, contact_frames): errors follow the
  // reference convention -- message on stderr, std::exit(EXIT_FAILURE).
  explicit Robot(const std::string& path_to_urdf, const std::vector<int>& contact_frames = {}) : path_(path_to_urdf) {
    if (idocp_abi_check(sizeof(idocp_model_t), sizeof(idocp_cost_t), sizeof(idocp_constraints_t)) != IDOCP_OK) {
      std::cerr << idocp_last_error() << '\n';
      std::exit(EXIT_FAILURE);
    }
    const int rc = idocp_model_from_urdf(path_to_urdf.c_str(), contact_frames.empty() ? nullptr : contact_frames.data(),
                                         (int)contact_frames.size(), &model_);
    if (rc != IDOCP_OK) {
      std::cerr << idocp_last_error() << '\n';
      std::exit(EXIT_FAILURE);
    }
  }
  Robot() : model_() {}

  int dimq() const { return model_.nq; }
  int dimv() const { return model_.nv; }
  int dimu() const { return model_.nu; }
  int dim_passive() const { return model_.has_floating_base ? 6 : 0; }
  int max_dimf() const { return 3 * model_.ncontacts; }
  bool hasFloatingBase() const { return model_.has_floating_base != 0; }
  int maxPointContacts() const { return model_.ncontacts; }
  double totalWeight() const { return -model_.total_mass * model_.gravity[2]; }

  Eigen::VectorXd jointEffortLimit() const { return get(model_.u_max); }
  Eigen::VectorXd jointVelocityLimit() const { return get(model_.v_max); }
  Eigen::VectorXd lowerJointPositionLimit() const { return get(model_.q_min); }
  Eigen::VectorXd upperJointPositionLimit() const { return get(model_.q_max); }
  void setJointEffortLimit(const Eigen::VectorXd& v) { set(model_.u_max, v, "invalid size of joint_effort_limit"); }
  void setJointVelocityLimit(const Eigen::VectorXd& v) { set(model_.v_max, v, "invalid size of joint_velocity_limit"); }
  void setLowerJointPositionLimit(const Eigen::VectorXd& v) { set(model_.q_min, v, "invalid size of lower_joint_position_limit"); }
  void setUpperJointPositionLimit(const Eigen::VectorXd& v) { set(model_.q_max, v, "invalid size of upper_joint_position_limit"); }

  // Robot::createContactStatus / updateFrameKinematics / setContactPoints / getContactPoints
  // (include/idocp/robot/robot.hxx:85-91, 262-283, 661-683).  Host arithmetic; see
  // idocp_model_contact_positions in idocp_hip.h.
  ContactStatus createContactStatus() const { return ContactStatus(model_.ncontacts); }
  void updateFrameKinematics(const Eigen::VectorXd& q) {
    if (q.size() != model_.nq) {
      std::cerr << "invalid size: q.size() must be " << model_.nq << "!" << '\n';
      std::exit(EXIT_FAILURE);
    }
    q_kin_.assign(q.data(), q.data() + model_.nq);
    points_.assign(3 * (size_t)model_.ncontacts, 0.0);
    if (model_.ncontacts == 0) return;
    if (idocp_model_contact_positions(&model_, q.data(), points_.data()) != IDOCP_OK) {
      std::cerr << idocp_last_error() << '\n';
      std::exit(EXIT_FAILURE);
    }
  }
  // Robot::updateKinematics(q[, v[, a]]) (robot.hxx:166-203): the facade keeps the state for the frame queries and the contact terms below
  // (computeBaumgarteResidual ..., evaluated on the GPU at this state); a velocity or acceleration that is not given is zero.
  void updateKinematics(const Eigen::VectorXd& q) { updateFrameKinematics(q); v_kin_.assign(model_.nv, 0.0); a_kin_.assign(model_.nv, 0.0); }
  void updateKinematics(const Eigen::VectorXd& q, const Eigen::VectorXd& v) {
    updateFrameKinematics(q); sized(v, model_.nv, "v");
    v_kin_.assign(v.data(), v.data() + model_.nv); a_kin_.assign(model_.nv, 0.0);
  }
  void updateKinematics(const Eigen::VectorXd& q, const Eigen::VectorXd& v, const Eigen::VectorXd& a) {
    updateFrameKinematics(q); sized(v, model_.nv, "v"); sized(a, model_.nv, "a");
    v_kin_.assign(v.data(), v.data() + model_.nv); a_kin_.assign(a.data(), a.data() + model_.nv);
  }

  // ---- Inverse dynamics and contact terms (robot.hxx:237-320, 408-540), each ONE n = 1 call of the batched rigid-body API
  // (idocp_rbd_contact_dynamics_batch, idocp_hip.h) on a handle this Robot creates at the first such call; a copy of the Robot creates its own.
  // The contact outputs are packed like the reference's: three rows per ACTIVE contact, in contact order, from row 0 of the argument.
  // Robot::setContactForces / setImpulseForces (robot.hxx:408-441): f[i] in the local coordinates of contact frame i, ignored where inactive
  void setContactForces(const ContactStatus& contact_status, const std::vector<Eigen::Vector3d>& f) { setForces(contact_status.isContactActive(), f, f_act_, f_); }
  void setImpulseForces(const ImpulseStatus& impulse_status, const std::vector<Eigen::Vector3d>& f) { setForces(impulse_status.isImpulseActive(), f, fi_act_, fi_); }
  void RNEA(const Eigen::VectorXd& q, const Eigen::VectorXd& v, const Eigen::VectorXd& a, Eigen::VectorXd& tau) {
    sized(q, model_.nq, "q"); sized(v, model_.nv, "v"); sized(a, model_.nv, "a"); sized(tau, model_.nv, "tau");
    idocp_rbd_io_t io = dynamicsIO(q.data(), v.data(), a.data(), f_);
    io.tau = tau.data();
    rbdCall(IDOCP_RBD_STAGE, f_act_, 0.0, io);
  }
  void RNEADerivatives(const Eigen::VectorXd& q, const Eigen::VectorXd& v, const Eigen::VectorXd& a, Eigen::MatrixXd& dRNEA_partial_dq,
                       Eigen::MatrixXd& dRNEA_partial_dv, Eigen::MatrixXd& dRNEA_partial_da) {
    sized(q, model_.nq, "q"); sized(v, model_.nv, "v"); sized(a, model_.nv, "a");
    square(dRNEA_partial_dq, "dRNEA_partial_dq"); square(dRNEA_partial_dv, "dRNEA_partial_dv"); square(dRNEA_partial_da, "dRNEA_partial_da");
    idocp_rbd_io_t io = dynamicsIO(q.data(), v.data(), a.data(), f_);
    io.dtau_dq = dRNEA_partial_dq.data(); io.dtau_dv = dRNEA_partial_dv.data(); io.dtau_da = dRNEA_partial_da.data();
    rbdCall(IDOCP_RBD_STAGE, f_act_, 0.0, io);
  }
  void RNEAImpulse(const Eigen::VectorXd& q, const Eigen::VectorXd& dv, Eigen::VectorXd& res) {
    sized(q, model_.nq, "q"); sized(dv, model_.nv, "dv"); sized(res, model_.nv, "res");
    const std::vector<double> zero(model_.nv, 0.0);
    idocp_rbd_io_t io = dynamicsIO(q.data(), zero.data(), dv.data(), fi_);
    io.tau = res.data();
    rbdCall(IDOCP_RBD_IMPULSE, fi_act_, 0.0, io);
  }
  void RNEAImpulseDerivatives(const Eigen::VectorXd& q, const Eigen::VectorXd& dv, Eigen::MatrixXd& dRNEA_partial_dq, Eigen::MatrixXd& dRNEA_partial_ddv) {
    sized(q, model_.nq, "q"); sized(dv, model_.nv, "dv");
    square(dRNEA_partial_dq, "dRNEA_partial_dq"); square(dRNEA_partial_ddv, "dRNEA_partial_ddv");
    const std::vector<double> zero(model_.nv, 0.0);
    idocp_rbd_io_t io = dynamicsIO(q.data(), zero.data(), dv.data(), fi_);
    io.dtau_dq = dRNEA_partial_dq.data(); io.dtau_da = dRNEA_partial_ddv.data();
    rbdCall(IDOCP_RBD_IMPULSE, fi_act_, 0.0, io);
  }
  // at the state of the last updateKinematics(q, v, a)
  void computeBaumgarteResidual(const ContactStatus& contact_status, const double time_step, const std::vector<Eigen::Vector3d>& contact_points,
                                Eigen::VectorXd& baumgarte_residual) const {
    noContacts(); kinematicsKnown();
    if ((int)contact_points.size() != model_.ncontacts) { std::cerr << "invalid size: contact_points.size() must be " << model_.ncontacts << "!" << '\n'; std::exit(EXIT_FAILURE); }
    double pts[3 * IDOCP_MAX_CONTACTS], C[3 * IDOCP_MAX_CONTACTS];
    for (int c = 0; c < model_.ncontacts; ++c) for (int k = 0; k < 3; ++k) pts[3 * c + k] = contact_points[c][k];
    int act[IDOCP_MAX_CONTACTS];
    const int dimf = activeOf(contact_status.isContactActive(), act);
    idocp_rbd_io_t io = dynamicsIO(q_kin_.data(), v_kin_.data(), a_kin_.data(), nullptr);
    io.contact_points = pts; io.C = C;
    rbdCall(IDOCP_RBD_STAGE, act, time_step, io);
    packVector(act, dimf, C, baumgarte_residual, "baumgarte_residual");
  }
  void computeBaumgarteDerivatives(const ContactStatus& contact_status, const double time_step, Eigen::MatrixXd& baumgarte_partial_dq,
                                   Eigen::MatrixXd& baumgarte_partial_dv, Eigen::MatrixXd& baumgarte_partial_da) {
    noContacts(); kinematicsKnown();
    int act[IDOCP_MAX_CONTACTS];
    const int dimf = activeOf(contact_status.isContactActive(), act);
    std::vector<double> d(3 * (size_t)max_dimf() * model_.nv);
    idocp_rbd_io_t io = dynamicsIO(q_kin_.data(), v_kin_.data(), a_kin_.data(), nullptr);
    io.dCdq = d.data(); io.dCdv = d.data() + (size_t)max_dimf() * model_.nv; io.dCda = d.data() + 2 * (size_t)max_dimf() * model_.nv;
    rbdCall(IDOCP_RBD_STAGE, act, time_step, io);
    packMatrix(act, dimf, io.dCdq, baumgarte_partial_dq, "baumgarte_partial_dq");
    packMatrix(act, dimf, io.dCdv, baumgarte_partial_dv, "baumgarte_partial_dv");
    packMatrix(act, dimf, io.dCda, baumgarte_partial_da, "baumgarte_partial_da");
  }
  // the local linear velocity of the active frames at the velocity of the last updateKinematics (the reference's callers pass v + dv there)
  void computeImpulseVelocityResidual(const ImpulseStatus& impulse_status, Eigen::VectorXd& velocity_residual) const {
    noContacts(); kinematicsKnown();
    double C[3 * IDOCP_MAX_CONTACTS];
    int act[IDOCP_MAX_CONTACTS];
    const int dimf = activeOf(impulse_status.isImpulseActive(), act);
    const std::vector<double> zero(model_.nv, 0.0);
    idocp_rbd_io_t io = dynamicsIO(q_kin_.data(), v_kin_.data(), zero.data(), nullptr);
    io.C = C;
    rbdCall(IDOCP_RBD_IMPULSE, act, 0.0, io);
    packVector(act, dimf, C, velocity_residual, "velocity_residual");
  }
  void computeImpulseVelocityDerivatives(const ImpulseStatus& impulse_status, Eigen::MatrixXd& velocity_partial_dq, Eigen::MatrixXd& velocity_partial_dv) {
    noContacts(); kinematicsKnown();
    int act[IDOCP_MAX_CONTACTS];
    const int dimf = activeOf(impulse_status.isImpulseActive(), act);
    const std::vector<double> zero(model_.nv, 0.0);
    std::vector<double> d(2 * (size_t)max_dimf() * model_.nv);
    idocp_rbd_io_t io = dynamicsIO(q_kin_.data(), v_kin_.data(), zero.data(), nullptr);
    io.dCdq = d.data(); io.dCdv = d.data() + (size_t)max_dimf() * model_.nv;
    rbdCall(IDOCP_RBD_IMPULSE, act, 0.0, io);
    packMatrix(act, dimf, io.dCdq, velocity_partial_dq, "velocity_partial_dq");
    packMatrix(act, dimf, io.dCdv, velocity_partial_dv, "velocity_partial_dv");
  }
  // ---- Forward dynamics: ADDITIONS the reference's Robot does not have (it only evaluates the inverse direction).  Each is ONE n = 1 call of
  // idocp_rbd_forward_dynamics_batch (idocp_hip.h) on the same lazily created handle.
  // (a, f) for which RNEA gives [0_6; u] (u on a fixed-base robot) and the Baumgarte residual vanishes on the active contacts; the contact points are
  // those of contact_status; f[i] in the local coordinates of contact frame i, zero where inactive.  u: the nu joint torques.
  void forwardDynamics(const Eigen::VectorXd& q, const Eigen::VectorXd& v, const Eigen::VectorXd& u, const ContactStatus& contact_status,
                       const double time_step, Eigen::VectorXd& a, std::vector<Eigen::Vector3d>& f) {
    sized(q, model_.nq, "q"); sized(v, model_.nv, "v"); sized(u, model_.nu, "u");
    if (a.size() != model_.nv) a.resize(model_.nv);
    double pts[3 * IDOCP_MAX_CONTACTS] = {}, fo[3 * IDOCP_MAX_CONTACTS] = {};
    int act[IDOCP_MAX_CONTACTS] = {};
    idocp_rbd_fd_io_t io = idocp_rbd_fd_io_t();
    io.q = q.data(); io.v = v.data(); io.u = u.data(); io.a = a.data();
    if (model_.ncontacts > 0) {
      activeOf(contact_status.isContactActive(), act);
      for (int c = 0; c < model_.ncontacts; ++c) for (int k = 0; k < 3; ++k) pts[3 * c + k] = contact_status.contactPoints()[c][k];
      io.contact_points = pts; io.f = fo;
    }
    fdCall(IDOCP_RBD_STAGE, act, time_step, 0.0, io);
    f.resize(model_.ncontacts);
    for (int c = 0; c < model_.ncontacts; ++c) for (int k = 0; k < 3; ++k) f[c][k] = fo[3 * c + k];
  }
  // The linearised Euler step, an ADDITION like forwardDynamics: A (2 nv x 2 nv) and B (2 nv x nu), the Jacobians of x_next = (q (+) dt v, v + dt a)
  // with respect to the tangent [dq; dv] and to u at the forward solution (a, f), which is returned as well.  ONE n = 1 call of
  // idocp_rbd_forward_dynamics_derivatives_batch (idocp_hip.h has the definitions).
  void forwardDynamicsDerivatives(const Eigen::VectorXd& q, const Eigen::VectorXd& v, const Eigen::VectorXd& u, const ContactStatus& contact_status,
                                  const double time_step, const double dt, Eigen::VectorXd& a, std::vector<Eigen::Vector3d>& f, Eigen::MatrixXd& A,
                                  Eigen::MatrixXd& B) {
    sized(q, model_.nq, "q"); sized(v, model_.nv, "v"); sized(u, model_.nu, "u");
    if (a.size() != model_.nv) a.resize(model_.nv);
    const size_t nx = 2 * (size_t)model_.nv;
    std::vector<double> Ao(nx * nx), Bo(nx * model_.nu);
    double pts[3 * IDOCP_MAX_CONTACTS] = {}, fo[3 * IDOCP_MAX_CONTACTS] = {};
    int act[IDOCP_MAX_CONTACTS] = {};
    idocp_rbd_fdd_io_t io = idocp_rbd_fdd_io_t();
    io.q = q.data(); io.v = v.data(); io.u = u.data(); io.a = a.data(); io.A = Ao.data(); io.B = Bo.data();
    if (model_.ncontacts > 0) {
      activeOf(contact_status.isContactActive(), act);
      for (int c = 0; c < model_.ncontacts; ++c) for (int k = 0; k < 3; ++k) pts[3 * c + k] = contact_status.contactPoints()[c][k];
      io.contact_points = pts; io.f = fo;
    }
    if (!rbd_.h) ok(idocp_rbd_create(&model_, 0, &rbd_.h));
    ok(idocp_rbd_forward_dynamics_derivatives_batch(rbd_.h, IDOCP_RBD_STAGE, 1, model_.ncontacts > 0 ? act : nullptr, time_step, dt, &io));
    f.resize(model_.ncontacts);
    for (int c = 0; c < model_.ncontacts; ++c) for (int k = 0; k < 3; ++k) f[c][k] = fo[3 * c + k];
    A.resize((int)nx, (int)nx); B.resize((int)nx, model_.nu);
    for (size_t j = 0; j < nx; ++j) for (size_t i = 0; i < nx; ++i) A((int)i, (int)j) = Ao[i + nx * j];
    for (size_t j = 0; j < (size_t)model_.nu; ++j) for (size_t i = 0; i < nx; ++i) B((int)i, (int)j) = Bo[i + nx * j];
  }
  // (dv, lambda) for which RNEAImpulse vanishes and the velocity of the impulse_status's frames is zero at v + dv
  void impulseDynamics(const Eigen::VectorXd& q, const Eigen::VectorXd& v, const ImpulseStatus& impulse_status, Eigen::VectorXd& dv,
                       std::vector<Eigen::Vector3d>& lambda) {
    noContacts(); sized(q, model_.nq, "q"); sized(v, model_.nv, "v");
    if (dv.size() != model_.nv) dv.resize(model_.nv);
    double lo[3 * IDOCP_MAX_CONTACTS] = {};
    int act[IDOCP_MAX_CONTACTS] = {};
    activeOf(impulse_status.isImpulseActive(), act);
    idocp_rbd_fd_io_t io = idocp_rbd_fd_io_t();
    io.q = q.data(); io.v = v.data(); io.a = dv.data(); io.f = lo;
    fdCall(IDOCP_RBD_IMPULSE, act, 0.0, 0.0, io);
    lambda.resize(model_.ncontacts);
    for (int c = 0; c < model_.ncontacts; ++c) for (int k = 0; k < 3; ++k) lambda[c][k] = lo[3 * c + k];
  }
  // the explicit Euler step of the OCP's own discretisation (state_equation.hxx) on the GPU: q_next = q (+) dt v, v_next = v + dt a
  void stepForwardEuler(const Eigen::VectorXd& q, const Eigen::VectorXd& v, const Eigen::VectorXd& u, const ContactStatus& contact_status,
                        const double time_step, const double dt, Eigen::VectorXd& q_next, Eigen::VectorXd& v_next) {
    sized(q, model_.nq, "q"); sized(v, model_.nv, "v"); sized(u, model_.nu, "u");
    Eigen::VectorXd qn(model_.nq), vn(model_.nv);      // (q_next / v_next may be q / v)
    double pts[3 * IDOCP_MAX_CONTACTS] = {};
    int act[IDOCP_MAX_CONTACTS] = {};
    idocp_rbd_fd_io_t io = idocp_rbd_fd_io_t();
    io.q = q.data(); io.v = v.data(); io.u = u.data(); io.q_next = qn.data(); io.v_next = vn.data();
    if (model_.ncontacts > 0) {
      activeOf(contact_status.isContactActive(), act);
      for (int c = 0; c < model_.ncontacts; ++c) for (int k = 0; k < 3; ++k) pts[3 * c + k] = contact_status.contactPoints()[c][k];
      io.contact_points = pts;
    }
    fdCall(IDOCP_RBD_STAGE, act, time_step, dt, io);
    q_next = qn; v_next = vn;
  }
  // The solvers' affine feedback policy at one state, an ADDITION like forwardDynamics: u = u_ff + Kq (q (-) q_ref) + Kv (v - v_ref), q (-) q_ref as
  // subtractConfiguration(q, q_ref) gives it; Kq, Kv: the nu x nv gains of getStateFeedbackGain.  ONE n = 1 call of idocp_rbd_feedback_torques_batch
  // on the same lazily created handle (the batched call and idocp_rbd_rollout_policy take many states, bounds and a whole policy at once).
  void stateFeedbackTorques(const Eigen::VectorXd& q, const Eigen::VectorXd& v, const Eigen::VectorXd& q_ref, const Eigen::VectorXd& v_ref,
                            const Eigen::VectorXd& u_ff, const Eigen::MatrixXd& Kq, const Eigen::MatrixXd& Kv, Eigen::VectorXd& u) {
    sized(q, model_.nq, "q"); sized(v, model_.nv, "v"); sized(q_ref, model_.nq, "q_ref"); sized(v_ref, model_.nv, "v_ref"); sized(u_ff, model_.nu, "u_ff");
    const int nu = model_.nu, nv = model_.nv;
    if (Kq.rows() != nu || Kq.cols() != nv || Kv.rows() != nu || Kv.cols() != nv) {
      std::cerr << "invalid size: Kq and Kv must be " << nu << " x " << nv << "!" << '\n'; std::exit(EXIT_FAILURE);
    }
    std::vector<double> K((size_t)nu * 2 * nv);      // [Kq | Kv], column-major
    for (int c = 0; c < nv; ++c) for (int r = 0; r < nu; ++r) { K[(size_t)c * nu + r] = Kq(r, c); K[(size_t)(nv + c) * nu + r] = Kv(r, c); }
    if (u.size() != nu) u.resize(nu);
    Eigen::VectorXd out(nu);                          // (u may be u_ff)
    idocp_rbd_policy_t pol = idocp_rbd_policy_t();
    pol.u_ff = u_ff.data(); pol.K = K.data(); pol.q_ref = q_ref.data(); pol.v_ref = v_ref.data();
    if (!rbd_.h) ok(idocp_rbd_create(&model_, 0, &rbd_.h));
    ok(idocp_rbd_feedback_torques_batch(rbd_.h, 1, q.data(), v.data(), &pol, out.data()));
    u = out;
  }
  // The solvers' cost and a constraint violation of ONE trajectory, an ADDITION the reference does not have (it evaluates these sums for the
  // solver's own iterate only): q, v of the steps + 1 states, a, u, f of the steps stages (f[k][i] in the local coordinates of contact frame i;
  // only the active ones of contact_status[k] are read; f and contact_status stay empty on a fixed-base robot), against a CostFunction /
  // Constraints pair -- through their native() blocks, the conversion the solver facades use -- on the grid t0 + k dt.  The last state is scored
  // with the terminal weights.  ONE n = 1 call of idocp_rbd_score_rollout on the same lazily created handle (idocp_hip.h defines both sums; the
  // batched call scores many trajectories, windows of them and device arrays).
  template <class CostFunctionT, class ConstraintsT>
  void scoreTrajectory(const CostFunctionT& cost, const ConstraintsT& constraints, const double t0, const double dt,
                       const std::vector<Eigen::VectorXd>& q, const std::vector<Eigen::VectorXd>& v, const std::vector<Eigen::VectorXd>& a,
                       const std::vector<Eigen::VectorXd>& u, const std::vector<std::vector<Eigen::Vector3d>>& f,
                       const std::vector<ContactStatus>& contact_status, double& total_cost, double& violation) {
    const int steps = (int)u.size(), nc = model_.ncontacts;
    if (steps < 1 || (int)q.size() != steps + 1 || (int)v.size() != steps + 1 || (int)a.size() != steps ||
        (nc > 0 && ((int)f.size() != steps || (int)contact_status.size() != steps))) {
      std::cerr << "invalid size: a trajectory of N stages has N + 1 states q, v and N of a, u, f and contact_status!" << '\n'; std::exit(EXIT_FAILURE);
    }
    const FlatTrajectory t = flatten(q, v, &a, u, &f, &contact_status, nullptr);
    const idocp_cost_t c = cost.native();
    const idocp_constraints_t g = constraints.native();
    if (!rbd_.h) ok(idocp_rbd_create(&model_, 0, &rbd_.h));
    idocp_rbd_objective_t* objective = nullptr;
    ok(idocp_rbd_objective_create(rbd_.h, &c, &g, t0, dt, steps, &objective));
    idocp_rbd_score_io_t io = idocp_rbd_score_io_t();
    io.q_traj = t.q.data(); io.v_traj = t.v.data(); io.a_traj = t.a.data(); io.u_traj = t.u.data(); io.f_traj = orNull(t.f);
    io.cost = &total_cost; io.violation = &violation;
    const int rc = idocp_rbd_score_rollout(rbd_.h, objective, 1, 0, steps, orNull(t.active), 1, 0, &io);
    idocp_rbd_objective_destroy(objective);
    ok(rc);
  }
  // Time-varying LQR gains about ONE linearised trajectory, an ADDITION like forwardDynamicsDerivatives, whose A and B it takes per step: the
  // backward pass of idocp_rbd_lqr_backward (idocp_hip.h has the recursion) with the diagonal stage weights x_weight (2 nv, on [dq; dv]),
  // u_weight (nu) and the terminal weight xf_weight (2 nv), already scaled by the caller (dt included), the optional cost gradients lx (N + 1
  // vectors of 2 nv) and lu (N of nu) -- both empty or both given -- and a regularisation of Quu.  K[k] is nu x 2 nv = [Kq | Kv] in the convention
  // of stateFeedbackTorques (u = u_ff + K [q (-) q_ref; v - v_ref]); k[k] is the feed-forward step, zero without gradients.  Returns false, with
  // NaN from the failing step down, where Quu is not positive definite or an input is not finite.  ONE n = 1 call on the same lazily created handle.
  bool lqrGains(const std::vector<Eigen::MatrixXd>& A, const std::vector<Eigen::MatrixXd>& B, const Eigen::VectorXd& x_weight,
                const Eigen::VectorXd& u_weight, const Eigen::VectorXd& xf_weight, const std::vector<Eigen::VectorXd>& lx,
                const std::vector<Eigen::VectorXd>& lu, const double regularization, std::vector<Eigen::MatrixXd>& K, std::vector<Eigen::VectorXd>& k) {
    const int steps = (int)A.size(), nx = 2 * model_.nv, nu = model_.nu;
    const bool grad = !lx.empty() || !lu.empty();
    if (steps < 1 || (int)B.size() != steps || (grad && ((int)lx.size() != steps + 1 || (int)lu.size() != steps))) {
      std::cerr << "invalid size: N steps have N of A, B and, if given, N + 1 of lx and N of lu!" << '\n'; std::exit(EXIT_FAILURE);
    }
    sized(x_weight, nx, "x_weight"); sized(u_weight, nu, "u_weight"); sized(xf_weight, nx, "xf_weight");
    const size_t nxx = (size_t)nx * nx, nxu = (size_t)nx * nu;
    std::vector<double> As(steps * nxx), Bs(steps * nxu), lxs, lus, Ks(steps * nxu), ks;
    for (int s = 0; s < steps; ++s) {
      if (A[s].rows() != nx || A[s].cols() != nx || B[s].rows() != nx || B[s].cols() != nu) {
        std::cerr << "invalid size: A must be " << nx << " x " << nx << " and B " << nx << " x " << nu << "!" << '\n'; std::exit(EXIT_FAILURE);
      }
      for (int c = 0; c < nx; ++c) for (int r = 0; r < nx; ++r) As[s * nxx + (size_t)c * nx + r] = A[s](r, c);
      for (int c = 0; c < nu; ++c) for (int r = 0; r < nx; ++r) Bs[s * nxu + (size_t)c * nx + r] = B[s](r, c);
    }
    if (grad) {
      lxs.resize((size_t)(steps + 1) * nx); lus.resize((size_t)steps * nu); ks.resize((size_t)steps * nu);
      for (int s = 0; s <= steps; ++s) { sized(lx[s], nx, "lx"); for (int j = 0; j < nx; ++j) lxs[(size_t)s * nx + j] = lx[s][j]; }
      for (int s = 0; s < steps; ++s) { sized(lu[s], nu, "lu"); for (int j = 0; j < nu; ++j) lus[(size_t)s * nu + j] = lu[s][j]; }
    }
    int status = -1;
    idocp_rbd_lqr_io_t io = idocp_rbd_lqr_io_t();
    io.A_traj = As.data(); io.B_traj = Bs.data(); io.x_weight = x_weight.data(); io.u_weight = u_weight.data(); io.xf_weight = xf_weight.data();
    io.lx_traj = grad ? lxs.data() : nullptr; io.lu_traj = grad ? lus.data() : nullptr; io.regularization = regularization;
    io.K_traj = Ks.data(); io.k_traj = grad ? ks.data() : nullptr; io.status = &status;
    if (!rbd_.h) ok(idocp_rbd_create(&model_, 0, &rbd_.h));
    ok(idocp_rbd_lqr_backward(rbd_.h, 1, steps, &io));
    K.assign(steps, Eigen::MatrixXd(nu, nx)); k.assign(steps, Eigen::VectorXd::Zero(nu));
    for (int s = 0; s < steps; ++s) {
      for (int c = 0; c < nx; ++c) for (int r = 0; r < nu; ++r) K[s](r, c) = Ks[s * nxu + (size_t)c * nu + r];
      if (grad) for (int j = 0; j < nu; ++j) k[s][j] = ks[(size_t)s * nu + j];
    }
    return status < 0;
  }
  // The gradients lx (N + 1 vectors of 2 nv, the last one of the terminal cost) and lu (N of nu) of the cost scoreTrajectory sums, along ONE stored
  // trajectory, in the tangent [dq; dv] of forwardDynamicsDerivatives: what lqrGains takes as lx and lu.  An ADDITION: ONE n = 1 call of
  // idocp_rbd_objective_gradients (idocp_hip.h has the definition) on the same lazily created handle.  The cost's a_weight and f_weight must be zero
  // (the call says so otherwise); the constraints are not differentiated.
  template <class CostFunctionT>
  void costGradients(const CostFunctionT& cost, const double t0, const double dt, const std::vector<Eigen::VectorXd>& q,
                     const std::vector<Eigen::VectorXd>& v, const std::vector<Eigen::VectorXd>& u, std::vector<Eigen::VectorXd>& lx,
                     std::vector<Eigen::VectorXd>& lu) {
    const int steps = (int)u.size(), nx = 2 * model_.nv;
    if (steps < 1 || (int)q.size() != steps + 1 || (int)v.size() != steps + 1) {
      std::cerr << "invalid size: a trajectory of N stages has N + 1 states q, v and N of u!" << '\n'; std::exit(EXIT_FAILURE);
    }
    const size_t nu = model_.nu;
    const FlatTrajectory t = flatten(q, v, nullptr, u, nullptr, nullptr, nullptr);
    std::vector<double> lxs((size_t)(steps + 1) * nx), lus(steps * nu);
    const idocp_cost_t c = cost.native();
    if (!rbd_.h) ok(idocp_rbd_create(&model_, 0, &rbd_.h));
    idocp_rbd_objective_t* objective = nullptr;
    ok(idocp_rbd_objective_create(rbd_.h, &c, nullptr, t0, dt, steps, &objective));
    idocp_rbd_gradient_io_t io = idocp_rbd_gradient_io_t();
    io.q_traj = t.q.data(); io.v_traj = t.v.data(); io.u_traj = t.u.data(); io.lx_traj = lxs.data(); io.lu_traj = lus.data();
    const int rc = idocp_rbd_objective_gradients(rbd_.h, objective, 1, 0, steps, 1, &io);
    idocp_rbd_objective_destroy(objective);
    ok(rc);
    lx.assign(steps + 1, Eigen::VectorXd(nx)); lu.assign(steps, Eigen::VectorXd(model_.nu));
    for (int k = 0; k <= steps; ++k) for (int j = 0; j < nx; ++j) lx[k][j] = lxs[(size_t)k * nx + j];
    for (int k = 0; k < steps; ++k) for (size_t j = 0; j < nu; ++j) lu[k][j] = lus[k * nu + j];
  }
  // ONE iLQR iteration on ONE stored trajectory, in place, an ADDITION: idocp_rbd_ilqr_iterate with n = 1 (idocp_hip.h has the chain: linearise,
  // gradients, backward pass with the cost's own weights and `regularization`, then up to `trials` closed-loop rollouts with the step alpha halved
  // until the Armijo test with the factor `armijo` passes).  q, v (N + 1) and u (N) are the rollout of u from (q[0], v[0]) under contact_status with
  // the contacts held at contact_points (idocp_rbd_rollout's convention: N entries of ncontacts points; empty on a fixed base), total_cost its score
  // (scoreTrajectory).  Returns the step taken: 0 if none was accepted or the backward pass failed, and the trajectory is then left as it was.
  template <class CostFunctionT>
  double ilqrIterate(const CostFunctionT& cost, const double t0, const double dt, const double time_step, const std::vector<ContactStatus>& contact_status,
                     const std::vector<std::vector<Eigen::Vector3d>>& contact_points, std::vector<Eigen::VectorXd>& q, std::vector<Eigen::VectorXd>& v,
                     std::vector<Eigen::VectorXd>& u, double& total_cost, const double regularization = 1e-6, const double armijo = 1e-4,
                     const int trials = 8) {
    return ilqrIterateForm(IlqrChain::Diagonal, cost, nullptr, t0, dt, time_step, contact_status, contact_points, q, v, u, total_cost, nullptr, nullptr,
                           0.0, regularization, armijo, trials);
  }

 private:
  // ONE trajectory as the step-major arrays the C ABI takes with n = 1: q, v of the N + 1 states, u of the N stages and, where the caller has them,
  // a, f (the active contacts' alone), the contact status and the contact points of the stages.  What is left out (nullptr) stays empty and goes
  // to the C ABI as NULL (orNull).  The entries are checked here, the lengths of the trajectory by the caller, which knows what it takes.
  struct FlatTrajectory {
    std::vector<double> q, v, a, u, f, points;
    std::vector<int> active;
  };
  template <class T> static const T* orNull(const std::vector<T>& x) { return x.empty() ? nullptr : x.data(); }
  FlatTrajectory flatten(const std::vector<Eigen::VectorXd>& q, const std::vector<Eigen::VectorXd>& v, const std::vector<Eigen::VectorXd>* a,
                         const std::vector<Eigen::VectorXd>& u, const std::vector<std::vector<Eigen::Vector3d>>* f,
                         const std::vector<ContactStatus>* contact_status, const std::vector<std::vector<Eigen::Vector3d>>* contact_points) const {
    const int steps = (int)u.size(), nc = contact_status ? model_.ncontacts : 0;
    const size_t nq = model_.nq, nv = model_.nv, nu = model_.nu;
    FlatTrajectory t;
    t.q.resize((steps + 1) * nq); t.v.resize((steps + 1) * nv); t.u.resize(steps * nu); t.active.assign((size_t)steps * nc, 0);
    if (a) t.a.resize(steps * nv);
    if (f) t.f.assign((size_t)steps * 3 * nc, 0.0);
    if (contact_points) t.points.assign((size_t)steps * 3 * nc, 0.0);
    for (int k = 0; k <= steps; ++k) {
      sized(q[k], model_.nq, "q"); sized(v[k], model_.nv, "v");
      for (size_t j = 0; j < nq; ++j) t.q[k * nq + j] = q[k][j];
      for (size_t j = 0; j < nv; ++j) t.v[k * nv + j] = v[k][j];
      if (k == steps) break;
      if (a) { sized((*a)[k], model_.nv, "a"); for (size_t j = 0; j < nv; ++j) t.a[k * nv + j] = (*a)[k][j]; }
      sized(u[k], model_.nu, "u");
      for (size_t j = 0; j < nu; ++j) t.u[k * nu + j] = u[k][j];
      for (int c = 0; c < nc; ++c) {
        const size_t at = (size_t)k * nc + c;
        t.active[at] = (*contact_status)[k].isContactActive(c) ? 1 : 0;
        if (f && t.active[at]) for (int x = 0; x < 3; ++x) t.f[at * 3 + x] = (*f)[k][c][x];
        if (contact_points) for (int x = 0; x < 3; ++x) t.points[at * 3 + x] = (*contact_points)[k][c][x];
      }
    }
    return t;
  }
  void unflatten(const FlatTrajectory& t, std::vector<Eigen::VectorXd>& q, std::vector<Eigen::VectorXd>& v, std::vector<Eigen::VectorXd>& u) const {
    const size_t nq = model_.nq, nv = model_.nv, nu = model_.nu;
    for (size_t k = 0; k < q.size(); ++k) {
      for (size_t j = 0; j < nq; ++j) q[k][j] = t.q[k * nq + j];
      for (size_t j = 0; j < nv; ++j) v[k][j] = t.v[k * nv + j];
      if (k < u.size()) for (size_t j = 0; j < nu; ++j) u[k][j] = t.u[k * nu + j];
    }
  }
  // what the iLQR methods and updateMultipliers take: the rollout of u under contact_status with the contacts held at contact_points
  void rolloutSized(const std::vector<Eigen::VectorXd>& q, const std::vector<Eigen::VectorXd>& v, const std::vector<Eigen::VectorXd>& u,
                    const std::vector<ContactStatus>& contact_status, const std::vector<std::vector<Eigen::Vector3d>>& contact_points) const {
    const int steps = (int)u.size(), nc = model_.ncontacts;
    if (steps < 1 || (int)q.size() != steps + 1 || (int)v.size() != steps + 1 ||
        (nc > 0 && ((int)contact_status.size() != steps || (int)contact_points.size() != steps))) {
      std::cerr << "invalid size: a trajectory of N stages has N + 1 states q, v and N of u, contact_status and contact_points!" << '\n'; std::exit(EXIT_FAILURE);
    }
  }
  // a and f of the stages of a flattened trajectory, which the constraint rows read: from a rollout of its own torques, its q, v, u as given
  int stageAccelerations(const FlatTrajectory& t, const double time_step, const double dt, std::vector<double>& a, std::vector<double>& f) const {
    const int steps = (int)(t.u.size() / model_.nu);
    std::vector<double> tq(t.q), tv(t.v);
    a.resize((size_t)steps * model_.nv); f.resize((size_t)steps * 3 * model_.ncontacts);
    return idocp_rbd_rollout(rbd_.h, 1, steps, orNull(t.active), time_step, dt, t.u.data(), orNull(t.points), tq.data(), tv.data(), a.data(),
                             f.empty() ? nullptr : f.data(), 0);
  }
  // the augmented-Lagrangian forms: multipliers [steps][L], all zeros where the caller's vector has another size
  static void sizeMultipliers(const idocp_rbd_objective_t* objective, const int steps, std::vector<double>& multipliers) {
    const size_t rows = (size_t)steps * idocp_rbd_objective_multiplier_rows(objective);
    if (multipliers.size() != rows) multipliers.assign(rows, 0.0);
  }
  // which chain of include/idocp_hip.h an iteration runs: idocp_rbd_ilqr_iterate, _gn, _penalty or _al
  enum class IlqrChain { Diagonal, GaussNewton, Penalty, AugmentedLagrangian };
  // The body of ilqrIterate, ilqrIterateGaussNewton, ilqrIterateConstrained and ilqrIterateAugmentedLagrangian.  The last two take the constraints,
  // the weight mu, the multipliers (AugmentedLagrangian alone) and *violation_left, which receives the sq_violation (sq_shifted) of the trajectory the
  // call leaves; the trajectory that comes in is scored first: rolled out again for its a and f, then idocp_rbd_score_penalty (idocp_rbd_score_al).
  template <class CostFunctionT>
  double ilqrIterateForm(const IlqrChain chain, const CostFunctionT& cost, const idocp_constraints_t* constraints, const double t0, const double dt,
                         const double time_step, const std::vector<ContactStatus>& contact_status,
                         const std::vector<std::vector<Eigen::Vector3d>>& contact_points, std::vector<Eigen::VectorXd>& q,
                         std::vector<Eigen::VectorXd>& v, std::vector<Eigen::VectorXd>& u, double& total_cost, double* violation_left,
                         std::vector<double>* multipliers, const double mu, const double regularization, const double armijo, const int trials) {
    rolloutSized(q, v, u, contact_status, contact_points);
    const int steps = (int)u.size();
    const bool constrained = chain == IlqrChain::Penalty || chain == IlqrChain::AugmentedLagrangian;
    FlatTrajectory t = flatten(q, v, nullptr, u, nullptr, &contact_status, &contact_points);
    const idocp_cost_t c = cost.native();
    if (!rbd_.h) ok(idocp_rbd_create(&model_, 0, &rbd_.h));
    idocp_rbd_objective_t* objective = nullptr;
    ok(idocp_rbd_objective_create(rbd_.h, &c, constraints, t0, dt, steps, &objective));
    double violation = 0.0, alpha = 0.0, expected[2] = {0.0, 0.0};
    int status = -1;
    idocp_rbd_ilqr_io_t io = idocp_rbd_ilqr_io_t();
    io.q_traj = t.q.data(); io.v_traj = t.v.data(); io.u_traj = t.u.data(); io.cost = &total_cost; io.violation = &violation;
    io.regularization = regularization; io.armijo = armijo; io.shrink = 0.5; io.alpha_min = 0.0; io.penalty = constrained ? mu : 0.0; io.trials = trials;
    io.alpha_accepted = &alpha; io.lqr_status = &status; io.expected = expected;
    const int* const act = orNull(t.active);
    const double* const pts = orNull(t.points);
    int rc = IDOCP_OK;
    if (constrained) {
      std::vector<double> ta, tf;
      rc = stageAccelerations(t, time_step, dt, ta, tf);
      if (chain == IlqrChain::AugmentedLagrangian) {
        sizeMultipliers(objective, steps, *multipliers);
        if (rc == IDOCP_OK)
          rc = idocp_rbd_score_al(rbd_.h, objective, 1, 0, steps, act, 0, t.q.data(), t.v.data(), t.u.data(), ta.data(), orNull(tf), mu, multipliers->data(), &violation);
        if (rc == IDOCP_OK) rc = idocp_rbd_ilqr_iterate_al(rbd_.h, objective, 1, steps, act, time_step, dt, pts, &io, multipliers->data(), 0);
      } else {
        if (rc == IDOCP_OK) rc = idocp_rbd_score_penalty(rbd_.h, objective, 1, 0, steps, act, 0, t.q.data(), t.v.data(), t.u.data(), ta.data(), orNull(tf), &violation);
        if (rc == IDOCP_OK) rc = idocp_rbd_ilqr_iterate_penalty(rbd_.h, objective, 1, steps, act, time_step, dt, pts, &io, 0);
      }
      *violation_left = violation;
    } else {
      rc = (chain == IlqrChain::GaussNewton ? idocp_rbd_ilqr_iterate_gn : idocp_rbd_ilqr_iterate)(rbd_.h, objective, 1, steps, act, time_step, dt, pts, &io, 0);
    }
    idocp_rbd_objective_destroy(objective);
    ok(rc);
    unflatten(t, q, v, u);
    return alpha;
  }

 public:
  // The same iteration under the FULL cost, an ADDITION: idocp_rbd_ilqr_iterate_gn with n = 1 -- the cost's a_weight and f_weight enter as
  // Gauss-Newton residual rows (idocp_hip.h has the definition), so a cost whose u_weight is zero is fine where a_weight is not.
  template <class CostFunctionT>
  double ilqrIterateGaussNewton(const CostFunctionT& cost, const double t0, const double dt, const double time_step,
                                const std::vector<ContactStatus>& contact_status, const std::vector<std::vector<Eigen::Vector3d>>& contact_points,
                                std::vector<Eigen::VectorXd>& q, std::vector<Eigen::VectorXd>& v, std::vector<Eigen::VectorXd>& u, double& total_cost,
                                const double regularization = 1e-6, const double armijo = 1e-4, const int trials = 8) {
    return ilqrIterateForm(IlqrChain::GaussNewton, cost, nullptr, t0, dt, time_step, contact_status, contact_points, q, v, u, total_cost, nullptr, nullptr,
                           0.0, regularization, armijo, trials);
  }
  // The same iteration under the cost AND the constraints, an ADDITION: idocp_rbd_ilqr_iterate_penalty with n = 1 -- the rows the score sums into its
  // violation enter as a squared-hinge penalty with the weight mu (idocp_hip.h has the definition).  total_cost is the cost of the trajectory that
  // comes in and of the one that is left; sq_violation receives that of the one that is left (the incoming trajectory is scored by the call).
  template <class CostFunctionT, class ConstraintsT>
  double ilqrIterateConstrained(const CostFunctionT& cost, const ConstraintsT& constraints, const double t0, const double dt, const double time_step,
                                const std::vector<ContactStatus>& contact_status, const std::vector<std::vector<Eigen::Vector3d>>& contact_points,
                                std::vector<Eigen::VectorXd>& q, std::vector<Eigen::VectorXd>& v, std::vector<Eigen::VectorXd>& u, double& total_cost,
                                double& sq_violation, const double mu, const double regularization = 1e-6, const double armijo = 1e-4,
                                const int trials = 8) {
    const idocp_constraints_t g = constraints.native();
    return ilqrIterateForm(IlqrChain::Penalty, cost, &g, t0, dt, time_step, contact_status, contact_points, q, v, u, total_cost, &sq_violation, nullptr, mu,
                           regularization, armijo, trials);
  }
  // The augmented-Lagrangian iteration, an ADDITION: idocp_rbd_ilqr_iterate_al with n = 1 at the penalty weight mu > 0 under the multipliers
  // [N][L], L = 4 dimu + (cone rows) * contacts (idocp_hip.h has the layout; a vector of another size is replaced by zeros).  sq_shifted receives
  // the shifted squared violation of the trajectory that is left; the multipliers are read, not written.
  template <class CostFunctionT, class ConstraintsT>
  double ilqrIterateAugmentedLagrangian(const CostFunctionT& cost, const ConstraintsT& constraints, const double t0, const double dt, const double time_step,
                                        const std::vector<ContactStatus>& contact_status, const std::vector<std::vector<Eigen::Vector3d>>& contact_points,
                                        std::vector<Eigen::VectorXd>& q, std::vector<Eigen::VectorXd>& v, std::vector<Eigen::VectorXd>& u, double& total_cost,
                                        double& sq_shifted, std::vector<double>& multipliers, const double mu, const double regularization = 1e-6,
                                        const double armijo = 1e-4, const int trials = 8) {
    const idocp_constraints_t g = constraints.native();
    return ilqrIterateForm(IlqrChain::AugmentedLagrangian, cost, &g, t0, dt, time_step, contact_status, contact_points, q, v, u, total_cost, &sq_shifted,
                           &multipliers, mu, regularization, armijo, trials);
  }
  // The outer step, an ADDITION: idocp_rbd_ilqr_al_update with n = 1 -- the multipliers become mu times the shifted rows of the trajectory, in place;
  // sq_shifted receives the shifted squared violation under the new multipliers and mu_next.  Returns the infeasibility (the largest unshifted row);
  // multiplier_change receives the largest change of a multiplier.  The trajectory is left as it is.
  template <class CostFunctionT, class ConstraintsT>
  double updateMultipliers(const CostFunctionT& cost, const ConstraintsT& constraints, const double t0, const double dt, const double time_step,
                           const std::vector<ContactStatus>& contact_status, const std::vector<std::vector<Eigen::Vector3d>>& contact_points,
                           std::vector<Eigen::VectorXd>& q, std::vector<Eigen::VectorXd>& v, std::vector<Eigen::VectorXd>& u,
                           std::vector<double>& multipliers, const double mu, const double mu_next, double& sq_shifted, double& multiplier_change) {
    rolloutSized(q, v, u, contact_status, contact_points);
    const int steps = (int)u.size();
    const FlatTrajectory t = flatten(q, v, nullptr, u, nullptr, &contact_status, &contact_points);
    const idocp_cost_t c = cost.native();
    const idocp_constraints_t g = constraints.native();
    if (!rbd_.h) ok(idocp_rbd_create(&model_, 0, &rbd_.h));
    idocp_rbd_objective_t* objective = nullptr;
    ok(idocp_rbd_objective_create(rbd_.h, &c, &g, t0, dt, steps, &objective));
    std::vector<double> ta, tf;
    double infeasibility = 0.0;
    int rc = stageAccelerations(t, time_step, dt, ta, tf);
    sizeMultipliers(objective, steps, multipliers);
    if (rc == IDOCP_OK)
      rc = idocp_rbd_ilqr_al_update(rbd_.h, objective, 1, steps, orNull(t.active), t.q.data(), t.v.data(), t.u.data(), ta.data(), orNull(tf), mu, mu_next,
                                    multipliers.data(), &sq_shifted, &infeasibility, &multiplier_change);
    idocp_rbd_objective_destroy(objective);
    ok(rc);
    return infeasibility;
  }
  // Robot::framePosition / frameRotation / framePlacement (robot.hxx:206-233): of any frame of the URDF (pinocchio's frame numbering, as the
  // contact frames and the task-space costs use it), at the configuration of the last updateFrameKinematics / updateKinematics
  Eigen::Vector3d framePosition(const int frame_id) const { return framePlacement(frame_id).translation(); }
  Eigen::Matrix3d frameRotation(const int frame_id) const { return framePlacement(frame_id).rotation(); }
  pinocchio::SE3 framePlacement(const int frame_id) const {
    if (q_kin_.empty()) { std::cerr << "invalid function call: call updateFrameKinematics(q) first!" << '\n'; std::exit(EXIT_FAILURE); }
    auto it = frames_.find(frame_id);                      // (where the frame sits is read from the URDF once per frame)
    if (it == frames_.end()) {
      FrameLocation loc;
      ok(idocp_model_frame_placement(path_.c_str(), frame_id, &loc.joint, loc.R, loc.p));
      it = frames_.emplace(frame_id, loc).first;
    }
    double Rw[9], pw[3];
    ok(idocp_model_frame_world_placement(&model_, q_kin_.data(), it->second.joint, it->second.R, it->second.p, Rw, pw));
    Eigen::Matrix3d R;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R(r, c) = Rw[3 * r + c];
    return pinocchio::SE3(R, Eigen::Vector3d(pw[0], pw[1], pw[2]));
  }
  // Robot::generateFeasibleConfiguration (robot.hxx:618-626): uniform between the joint position limits; the base, if any, uniform in [-1, 1]^3 with a
  // uniformly random orientation
  Eigen::VectorXd generateFeasibleConfiguration() const {
    Eigen::VectorXd q(model_.nq);
    auto uni = [](const double lo, const double hi) { return lo + (hi - lo) * (std::rand() / (double)RAND_MAX); };
    const int nb = model_.has_floating_base ? 7 : 0;
    for (int k = 0; k < nb; ++k) q[k] = uni(-1.0, 1.0);
    for (int k = 0; k < model_.nu; ++k) q[nb + k] = uni(model_.q_min[k], model_.q_max[k]);      // (the model's limit arrays run over the actuated joints)
    if (nb) ok(idocp_model_normalize_configuration(&model_, q.data()));
    return q;
  }
  void getContactPoints(std::vector<Eigen::Vector3d>& contact_points) const {
    contact_points.resize(model_.ncontacts);
    for (int c = 0; c < model_.ncontacts; ++c) for (int k = 0; k < 3; ++k) contact_points[c][k] = points_.at(3 * c + k);
  }
  void setContactPoints(ContactStatus& contact_status) const {
    std::vector<Eigen::Vector3d> pts;
    getContactPoints(pts);
    contact_status.setContactPoints(pts);
  }

  // Robot::integrateConfiguration / subtractConfiguration / normalizeConfiguration (robot.hxx:96-147; robot.hpp:105-160): what a driver does
  // between two solver calls (advance the plant, measure a distance on the configuration manifold).  Host arithmetic behind the C ABI
  // (idocp_model_integrate_configuration ...).
  void integrateConfiguration(const Eigen::VectorXd& v, const double integration_length, Eigen::VectorXd& q) const {      // in place (robot.hpp:82-86)
    Eigen::VectorXd out(model_.nq);
    integrateConfiguration(q, v, integration_length, out);
    q = out;
  }
  void integrateConfiguration(const Eigen::VectorXd& q, const Eigen::VectorXd& v, const double integration_length, Eigen::VectorXd& q_integrated) const {
    sized(q, model_.nq, "q"); sized(v, model_.nv, "v");
    if (q_integrated.size() != model_.nq) q_integrated.resize(model_.nq);
    ok(idocp_model_integrate_configuration(&model_, q.data(), v.data(), integration_length, q_integrated.data()));
  }
  void subtractConfiguration(const Eigen::VectorXd& q_plus, const Eigen::VectorXd& q_minus, Eigen::VectorXd& difference) const {
    sized(q_plus, model_.nq, "q_plus"); sized(q_minus, model_.nq, "q_minus");
    if (difference.size() != model_.nv) difference.resize(model_.nv);
    ok(idocp_model_subtract_configuration(&model_, q_plus.data(), q_minus.data(), difference.data()));
  }
  void normalizeConfiguration(Eigen::VectorXd& q) const {
    sized(q, model_.nq, "q");
    ok(idocp_model_normalize_configuration(&model_, q.data()));
  }
  // Robot::setFrictionCoefficient / frictionCoefficient / setRestitutionCoefficient / restitutionCoefficient (robot.hxx:358-406): per-contact properties
  // the reference stores (defaults 0.8 and 0, point_contact.hpp) and nothing on the solver path reads -- the friction cones take their mu as a
  // constructor argument (friction_cone.hpp).  Kept so that a driver that sets them compiles and reads back what it set.
  void setFrictionCoefficient(const std::vector<double>& friction_coefficient) {
    for (int i = 0; i < model_.ncontacts && i < (int)friction_coefficient.size(); ++i) {
      if (friction_coefficient[i] <= 0) { std::cerr << "invalid argument: friction coefficient must be positive" << '\n'; std::exit(EXIT_FAILURE); }
      friction_[i] = friction_coefficient[i];
    }
  }
  double frictionCoefficient(const int contact_index) const { noContacts(); return friction_[contact_index]; }
  void setRestitutionCoefficient(const std::vector<double>& restitution_coefficient) {
    for (int i = 0; i < model_.ncontacts && i < (int)restitution_coefficient.size(); ++i) {
      if (restitution_coefficient[i] < 0 || restitution_coefficient[i] > 1) { std::cerr << "invalid argument: restitution coefficient must be in [0, 1]" << '\n'; std::exit(EXIT_FAILURE); }
      restitution_[i] = restitution_coefficient[i];
    }
  }
  double restitutionCoefficient(const int contact_index) const { noContacts(); return restitution_[contact_index]; }
  // Robot::contactFramesIndices (robot.hxx:655-661)
  std::vector<int> contactFramesIndices() const { return std::vector<int>(model_.contact_frame_id, model_.contact_frame_id + model_.ncontacts); }
  // Robot::createImpulseStatus (robot.hxx:672-675)
  ImpulseStatus createImpulseStatus() const { return ImpulseStatus(model_.ncontacts); }

  const idocp_model_t& model() const { return model_; }
  // the URDF this robot was built from (frame lookups of the task-space costs)
  const std::string& pathToUrdf() const { return path_; }

 private:
  idocp_model_t model_;
  std::string path_;
  std::vector<double> points_;     // contact-frame positions of the last updateFrameKinematics(q)
  std::vector<double> q_kin_;      // that configuration (frame queries)
  std::vector<double> v_kin_, a_kin_;      // velocity and acceleration of the last updateKinematics
  double f_[3 * IDOCP_MAX_CONTACTS] = {}, fi_[3 * IDOCP_MAX_CONTACTS] = {};      // setContactForces / setImpulseForces
  int f_act_[IDOCP_MAX_CONTACTS] = {}, fi_act_[IDOCP_MAX_CONTACTS] = {};
  // the handle of the batched rigid-body API: created at the first call that needs it, never shared (a copied Robot creates its own)
  struct RbdHandle {
    idocp_rbd_t* h = nullptr;
    RbdHandle() {}
    RbdHandle(const RbdHandle&) {}
    RbdHandle& operator=(const RbdHandle&) { reset(); return *this; }      // (the model may have changed with the assignment)
    ~RbdHandle() { reset(); }
    void reset() { if (h) idocp_rbd_destroy(h); h = nullptr; }
  };
  mutable RbdHandle rbd_;
  void rbdCall(int mode, const int* active, double time_step, const idocp_rbd_io_t& io) const {
    if (!rbd_.h) ok(idocp_rbd_create(&model_, 0, &rbd_.h));
    ok(idocp_rbd_contact_dynamics_batch(rbd_.h, mode, 1, model_.ncontacts > 0 ? active : nullptr, time_step, &io));
  }
  void fdCall(int mode, const int* active, double time_step, double dt, const idocp_rbd_fd_io_t& io) const {
    if (!rbd_.h) ok(idocp_rbd_create(&model_, 0, &rbd_.h));
    ok(idocp_rbd_forward_dynamics_batch(rbd_.h, mode, 1, model_.ncontacts > 0 ? active : nullptr, time_step, dt, &io));
  }
  idocp_rbd_io_t dynamicsIO(const double* q, const double* v, const double* a, const double* f) const {
    idocp_rbd_io_t io = idocp_rbd_io_t();
    io.q = q; io.v = v; io.a = a; io.f = model_.ncontacts > 0 ? f : nullptr;
    return io;
  }
  void setForces(const std::vector<bool>& active, const std::vector<Eigen::Vector3d>& f, int* act, double* out) {
    noContacts();
    if ((int)f.size() != model_.ncontacts || (int)active.size() != model_.ncontacts) {
      std::cerr << "invalid size: f.size() must be " << model_.ncontacts << "!" << '\n'; std::exit(EXIT_FAILURE);
    }
    for (int c = 0; c < model_.ncontacts; ++c) {
      act[c] = active[c] ? 1 : 0;
      for (int k = 0; k < 3; ++k) out[3 * c + k] = active[c] ? f[c][k] : 0.0;
    }
  }
  int activeOf(const std::vector<bool>& active, int* act) const {
    int dimf = 0;
    for (int c = 0; c < model_.ncontacts; ++c) { act[c] = (c < (int)active.size() && active[c]) ? 1 : 0; dimf += 3 * act[c]; }
    return dimf;
  }
  void kinematicsKnown() const {
    if (q_kin_.empty() || v_kin_.empty()) { std::cerr << "invalid function call: call updateKinematics(q, v, a) first!" << '\n'; std::exit(EXIT_FAILURE); }
  }
  void square(const Eigen::MatrixXd& m, const char* name) const {
    if (m.rows() != model_.nv || m.cols() != model_.nv) { std::cerr << "invalid size: " << name << " must be " << model_.nv << " x " << model_.nv << "!" << '\n'; std::exit(EXIT_FAILURE); }
  }
  // rows of the active contacts, in contact order, to the top of the argument
  void packVector(const int* act, int dimf, const double* full, Eigen::VectorXd& out, const char* name) const {
    if (out.size() < dimf) { std::cerr << "invalid size: " << name << ".size() must be at least " << dimf << "!" << '\n'; std::exit(EXIT_FAILURE); }
    int row = 0;
    for (int c = 0; c < model_.ncontacts; ++c) if (act[c]) { for (int k = 0; k < 3; ++k) out[row + k] = full[3 * c + k]; row += 3; }
  }
  void packMatrix(const int* act, int dimf, const double* full, Eigen::MatrixXd& out, const char* name) const {
    if (out.rows() < dimf || out.cols() != model_.nv) {
      std::cerr << "invalid size: " << name << " must have at least " << dimf << " rows and " << model_.nv << " columns!" << '\n'; std::exit(EXIT_FAILURE);
    }
    const int nf = max_dimf();
    for (int j = 0; j < model_.nv; ++j) {
      int row = 0;
      for (int c = 0; c < model_.ncontacts; ++c) if (act[c]) { for (int k = 0; k < 3; ++k) out(row + k, j) = full[(size_t)j * nf + 3 * c + k]; row += 3; }
    }
  }
  struct FrameLocation { int joint; double R[9], p[3]; };
  mutable std::map<int, FrameLocation> frames_;
  double friction_[IDOCP_MAX_CONTACTS] = {0.8, 0.8, 0.8, 0.8}, restitution_[IDOCP_MAX_CONTACTS] = {0.0, 0.0, 0.0, 0.0};
  void noContacts() const {
    if (model_.ncontacts == 0) { std::cerr << "invalid function call: robot has no point contacts!" << '\n'; std::exit(EXIT_FAILURE); }
  }
  static void ok(int rc) { if (rc != IDOCP_OK) { std::cerr << idocp_last_error() << '\n'; std::exit(EXIT_FAILURE); } }
  static void sized(const Eigen::VectorXd& x, int n, const char* name) {
    if (x.size() != n) { std::cerr << "invalid size: " << name << ".size() must be " << n << "!" << '\n'; std::exit(EXIT_FAILURE); }
  }
  Eigen::VectorXd get(const double* p) const {
    Eigen::VectorXd v(model_.nu);
    for (int i = 0; i < model_.nu; ++i) v[i] = p[i];
    return v;
  }
  void set(double* p, const Eigen::VectorXd& v, const char* msg) {
    if (v.size() != model_.nu) {   // robot.cpp:113-170: throw -> catch -> exit
      std::cerr << msg << '\n';
      std::exit(EXIT_FAILURE);
    }
    for (int i = 0; i < model_.nu; ++i) p[i] = v[i];
  }
};

}  // namespace idocp
#endif  // IDOCP_ROBOT_HPP_
