// idocp::UnOCPSolver -- drop-in facade over the HIP path.
//
// Same constructor signature and methods as the reference class
// (include/idocp/unocp/unocp_solver.hpp:25-188; src/unocp/unocp_solver.cpp).
// Every method forwards to the C ABI (include/idocp_hip.h); the arithmetic runs
// in the HIP kernels.  `nthreads` is accepted for source compatibility and
// ignored (the GPU replaces the OpenMP team).  Argument errors: message on
// stderr + std::exit(EXIT_FAILURE), like the reference.  What it shares with
// UnParNMPCSolver (getters, setSolution, printSolution / saveSolution, copy and
// move) is detail::FixedBaseCore.
#ifndef IDOCP_UNOCP_SOLVER_HPP_
#define IDOCP_UNOCP_SOLVER_HPP_

#include <memory>
#include <vector>

#include "idocp/detail/solver_core.hpp"

namespace idocp {

class UnOCPSolver : public detail::FixedBaseCore {
 public:
  UnOCPSolver(const Robot& robot, const std::shared_ptr<CostFunction>& cost, const std::shared_ptr<Constraints>& constraints,
              const double T, const int N, const int nthreads = 1, const int device = 0)
      : detail::FixedBaseCore(robot, cost, N, N + 1), dt_(T / N) {
    (void)nthreads;
    const idocp_constraints_t k = constraints->native();
    idocp_unocp_t* h = nullptr;
    detail::check(idocp_unocp_create(&robot.model(), &cost_.last, &k, T, N, 1, device, &h));
    h_ = detail::UnocpHandle(h);
  }
  // unocp_solver.hpp:49: an empty solver, to be assigned a constructed one before use.  Copyable and movable like the reference class
  // (unocp_solver.hpp:59-74, `= default`): a copy is a DEEP copy of the solver state on the device (idocp_unocp_clone)
  UnOCPSolver() = default;

  void updateSolution(const double t, const Eigen::VectorXd& q, const Eigen::VectorXd& v, const bool line_search = false) {
    cost_.sync(h_.get(), idocp_unocp_set_cost);
    uploadTaskRefs(t);
    detail::check(idocp_unocp_update_solution(h_.get(), t, q.data(), v.data(), line_search ? 1 : 0));
  }

  // The reference leaves this unimplemented for the Un path (unocp_solver.cpp:144-154);
  // here it returns the acceleration gains Kq, Kv of the LQR policy da = K dx + k.
  void getStateFeedbackGain(const int time_stage, Eigen::MatrixXd& Kq, Eigen::MatrixXd& Kv) const {
    const int nv = robot_.dimv();
    std::vector<double> K((size_t)N_ * nv * 2 * nv);
    detail::check(idocp_unocp_get_riccati(h_.get(), 0, nullptr, nullptr, K.data(), nullptr));
    Kq.resize(nv, nv); Kv.resize(nv, nv);
    const double* Ki = &K[(size_t)time_stage * nv * 2 * nv];
    for (int c = 0; c < nv; ++c) for (int r = 0; r < nv; ++r) { Kq(r, c) = Ki[c * nv + r]; Kv(r, c) = Ki[(nv + c) * nv + r]; }
  }

  void computeKKTResidual(const double t, const Eigen::VectorXd& q, const Eigen::VectorXd& v) {
    cost_.sync(h_.get(), idocp_unocp_set_cost);
    uploadTaskRefs(t);
    detail::check(idocp_unocp_compute_kkt_residual(h_.get(), t, q.data(), v.data()));
  }

 private:
  double dt_ = 0.0;
  std::vector<double> task_refs_;
  // TimeVaryingTaskSpace*Cost: the reference asks the user's ref object at the time of every stage inside linearizeOCP
  // (unocp_solver.cpp:78-94 -> time_varying_task_space_6d_cost.cpp:65-67); here the poses are evaluated up front and uploaded
  void uploadTaskRefs(const double t) {
    if (cost_.cost->taskRefs(t, dt_, N_, task_refs_)) detail::check(idocp_unocp_set_task_refs(h_.get(), task_refs_.data()));
  }
};

}  // namespace idocp
#endif  // IDOCP_UNOCP_SOLVER_HPP_
