// idocp::UnParNMPCSolver -- drop-in facade over the HIP path.
//
// Same constructor signature and methods as the reference class
// (include/idocp/unocp/unparnmpc_solver.hpp:31-189; src/unocp/unparnmpc_solver.cpp).
// Every method forwards to the C ABI (include/idocp_hip.h, idocp_unparnmpc_* and the
// shared idocp_unocp_* accessors); the arithmetic runs in the HIP kernels.  `nthreads`
// is accepted for source compatibility and ignored.  Argument errors: message on
// stderr + std::exit(EXIT_FAILURE), like the reference.  What it shares with UnOCPSolver
// is detail::FixedBaseCore; its stages are the N backward-Euler stages 0 .. N-1 (stage i
// lives at t + (i + 1) dt).
#ifndef IDOCP_UNPARNMPC_SOLVER_HPP_
#define IDOCP_UNPARNMPC_SOLVER_HPP_

#include <memory>

#include "idocp/detail/solver_core.hpp"

namespace idocp {

class UnParNMPCSolver : public detail::FixedBaseCore {
 public:
  UnParNMPCSolver(const Robot& robot, const std::shared_ptr<CostFunction>& cost, const std::shared_ptr<Constraints>& constraints,
                  const double T, const int N, const int nthreads = 1, const int device = 0)
      : detail::FixedBaseCore(robot, cost, N, N) {
    (void)nthreads;
    const idocp_constraints_t k = constraints->native();
    idocp_unocp_t* h = nullptr;
    detail::check(idocp_unparnmpc_create(&robot.model(), &cost_.last, &k, T, N, 1, device, &h));
    h_ = detail::UnocpHandle(h);
  }
  // unparnmpc_solver.hpp:48: an empty solver, to be assigned a constructed one before use.  Copyable and movable like the reference class
  // (`= default` there): a copy is a DEEP copy of the device state (idocp_unocp_clone)
  UnParNMPCSolver() = default;

  void initBackwardCorrection(const double t) {
    cost_.sync(h_.get(), idocp_unocp_set_cost);
    detail::check(idocp_unparnmpc_init_backward_correction(h_.get(), t));
  }
  void updateSolution(const double t, const Eigen::VectorXd& q, const Eigen::VectorXd& v, const bool line_search = false) {
    cost_.sync(h_.get(), idocp_unocp_set_cost);
    detail::check(idocp_unparnmpc_update_solution(h_.get(), t, q.data(), v.data(), line_search ? 1 : 0));
  }

  // left unimplemented by the reference as well (unparnmpc_solver.cpp:107-118)
  void getStateFeedbackGain(const int, Eigen::MatrixXd&, Eigen::MatrixXd&) const {}

  void computeKKTResidual(const double t, const Eigen::VectorXd& q, const Eigen::VectorXd& v) {
    cost_.sync(h_.get(), idocp_unocp_set_cost);
    detail::check(idocp_unparnmpc_compute_kkt_residual(h_.get(), t, q.data(), v.data()));
  }
};

}  // namespace idocp
#endif  // IDOCP_UNPARNMPC_SOLVER_HPP_
