// idocp::OCPSolver -- drop-in facade over the HIP contact path.
//
// Same constructor signature and methods as the reference class
// (include/idocp/ocp/ocp_solver.hpp:32-232; src/ocp/ocp_solver.cpp).  Every
// method forwards to the C ABI (include/idocp_hip.h); the arithmetic runs in
// the HIP kernels K5a/K5b/S3/S4/K6/K7/K8.  `nthreads` is accepted for source
// compatibility and ignored (the GPU replaces the OpenMP team).  Argument
// errors: message on stderr + std::exit(EXIT_FAILURE), like the reference.
//
// Contact sequences with discrete events (pushBackContactStatus: lift stages,
// impulse + aux stages, switching constraints) run on the same kernels; the
// event stages are reachable through getSolution("...", "impulse" | "aux" | "lift").
//
// What it shares with ParNMPCSolver (getters, setSolution, the contact-sequence calls, copy and move) is detail::ContactCore.  A FIXED-BASE
// robot without contact frames is bound to the kernels of idocp::UnOCPSolver: why that is the same solver, and what is kept different, is told
// at the head of idocp/detail/solver_core.hpp.
#ifndef IDOCP_OCP_SOLVER_HPP_
#define IDOCP_OCP_SOLVER_HPP_

#include <cstdlib>
#include <iostream>
#include <memory>

#include "idocp/detail/solver_core.hpp"
#include "idocp/unocp/unocp_solver.hpp"

namespace idocp {

class OCPSolver : public detail::ContactCore<UnOCPSolver> {
 public:
  OCPSolver(const Robot& robot, const std::shared_ptr<CostFunction>& cost, const std::shared_ptr<Constraints>& constraints,
            const double T, const int N, const int max_num_impulse = 0, const int nthreads = 1, const int device = 0)
      : detail::ContactCore<UnOCPSolver>(robot, cost, N, N + 1) {
    if (max_num_impulse < 0) {      // ocp_solver.cpp:34-36
      std::cerr << "invalid value: max_num_impulse must be non-negative!" << '\n';
      std::exit(EXIT_FAILURE);
    }
    if (bindFixedBase(robot, cost, constraints, T, N, nthreads, device)) return;
    const idocp_constraints_t k = constraints->native();
    idocp_ocp_t* h = nullptr;
    detail::check(idocp_ocp_create_hybrid(&robot.model(), &cost_.last, &k, T, N, max_num_impulse, 1, device, &h));
    h_ = detail::OcpHandle(h);
  }
  // ocp_solver.hpp:44: an empty solver, to be assigned a constructed one before use.  Copyable and movable like the reference class
  // (ocp_solver.hpp:171-186, `= default`): a copy is a DEEP copy of the solver state on the device (idocp_ocp_clone)
  OCPSolver() = default;

  void updateSolution(const double t, const Eigen::VectorXd& q, const Eigen::VectorXd& v, const bool line_search = false) {
    if (un_) { un_->updateSolution(t, q, v, line_search); return; }
    cost_.sync(h_.get(), idocp_ocp_set_cost);
    syncTaskRefs(t);
    detail::check(idocp_ocp_update_solution(h_.get(), t, q.data(), v.data(), line_search ? 1 : 0));
  }

  // OCPSolver::getStateFeedbackGain (ocp_solver.cpp:103-113): du = Kq dq + Kv dv
  void getStateFeedbackGain(const int time_stage, Eigen::MatrixXd& Kq, Eigen::MatrixXd& Kv) const {
    const int nv = robot_.dimv(), nu = robot_.dimu();
    Kq.resize(nu, nv); Kv.resize(nu, nv);
    if (un_) { detail::check(idocp_unocp_get_torque_feedback_gain(un_->handle(), 0, time_stage, Kq.data(), Kv.data())); return; }
    detail::check(idocp_ocp_get_state_feedback_gain(h_.get(), 0, time_stage, Kq.data(), Kv.data()));
  }

  void computeKKTResidual(const double t, const Eigen::VectorXd& q, const Eigen::VectorXd& v) {
    if (un_) { un_->computeKKTResidual(t, q, v); return; }
    cost_.sync(h_.get(), idocp_ocp_set_cost);
    syncTaskRefs(t);
    detail::check(idocp_ocp_compute_kkt_residual(h_.get(), t, q.data(), v.data()));
  }
  using detail::ContactCore<UnOCPSolver>::handle;
  idocp_ocp_t* handle() const { return h_.get(); }
};

}  // namespace idocp
#endif  // IDOCP_OCP_SOLVER_HPP_
