// idocp::ParNMPCSolver -- drop-in facade over the HIP ParNMPC path.
//
// Same constructor signature and methods as the reference class
// (include/idocp/ocp/parnmpc_solver.hpp; src/ocp/parnmpc_solver.cpp).  Every method forwards to
// the C ABI (include/idocp_hip.h: idocp_parnmpc_* and the shared idocp_ocp_* entry points); the
// arithmetic runs in the HIP kernels K5a / K5b<BWD> / K9w / S5 / K10a / S6 / K10b / K6 / K7 and, for
// contact sequences with discrete events (pushBackContactStatus; max_num_impulse > 0), K5s / K9i / K9w's general instantiation
// for the aux and impulse stages of the ParNMPCDiscretizer chain.  Its stages are 0 .. N-1 (stage i lives at t + (i + 1) T / N).
//
// What it shares with OCPSolver is detail::ContactCore.  A FIXED-BASE robot without contact frames is bound to the kernels of
// idocp::UnParNMPCSolver, for the reason given at the head of idocp/detail/solver_core.hpp: one Newton system per stage, condensed in two orders; the
// backward correction only sees its state and costate blocks, which do not depend on the order (tests/test_oracle_fixed_base.py, tests/test_fixed_base_ocp_gpu.py).
#ifndef IDOCP_PARNMPC_SOLVER_HPP_
#define IDOCP_PARNMPC_SOLVER_HPP_

#include <cstdlib>
#include <iostream>
#include <memory>

#include "idocp/detail/solver_core.hpp"
#include "idocp/unocp/unparnmpc_solver.hpp"

namespace idocp {

class ParNMPCSolver : public detail::ContactCore<UnParNMPCSolver> {
 public:
  ParNMPCSolver(const Robot& robot, const std::shared_ptr<CostFunction>& cost, const std::shared_ptr<Constraints>& constraints,
                const double T, const int N, const int max_num_impulse = 0, const int nthreads = 1, const int device = 0)
      : detail::ContactCore<UnParNMPCSolver>(robot, cost, N, N) {
    if (bindFixedBase(robot, cost, constraints, T, N, nthreads, device)) return;
    const idocp_constraints_t k = constraints->native();
    idocp_ocp_t* h = nullptr;
    if (max_num_impulse > 0) detail::check(idocp_parnmpc_create_hybrid(&robot.model(), &cost_.last, &k, T, N, max_num_impulse, 1, device, &h));
    else detail::check(idocp_parnmpc_create(&robot.model(), &cost_.last, &k, T, N, 1, device, &h));
    h_ = detail::OcpHandle(h);
  }
  // Multi-GPU (BASELINE configs[3]): ONE process per GPU, every process constructs the solver with the same arguments plus its
  // communicator (idocp_comm_init_rank over an id made by idocp_comm_get_unique_id on rank 0).  The process then owns the grid
  // stages [rank N / world, (rank + 1) N / world) of the horizon; initBackwardCorrection / updateSolution / KKTError are collective
  // calls (RCCL halo exchange with the two neighbours, idocp_amd/csrc/parnmpc_dist.hip -- the counterpart of the reference's OpenMP
  // loops over one horizon, backward_correction_solver.cpp:255-366).  getSolution returns the local stages.
  ParNMPCSolver(const Robot& robot, const std::shared_ptr<CostFunction>& cost, const std::shared_ptr<Constraints>& constraints,
                const double T, const int N, idocp_comm_t* comm, const int max_num_impulse = 0, const int device = 0)
      : detail::ContactCore<UnParNMPCSolver>(robot, cost, N, N) {
    const idocp_constraints_t k = constraints->native();
    const int rank = idocp_comm_rank(comm), world = idocp_comm_world(comm);
    if (world < 1 || N % world != 0) { std::cerr << "invalid value: N must be divisible by the number of ranks!\n"; std::exit(EXIT_FAILURE); }
    const int Nl = N / world;
    idocp_ocp_t* h = nullptr;
    if (max_num_impulse > 0) detail::check(idocp_parnmpc_create_hybrid_shard(&robot.model(), &cost_.last, &k, T, N, max_num_impulse, rank * Nl, (rank + 1) * Nl, 1, device, &h));
    else detail::check(idocp_parnmpc_create_shard(&robot.model(), &cost_.last, &k, T / world, Nl, rank * Nl, rank == world - 1 ? 1 : 0, rank > 0 ? 1 : 0, 1, device, &h));
    h_ = detail::OcpHandle(h);
    shard_ = detail::CommAttachment(h, comm);
    N_ = nstate_ = Nl;
    cache_.resize(Nl);
  }
  // parnmpc_solver.hpp:47: an empty solver, to be assigned a constructed one before use.  Copyable and movable like the reference class (a copy is
  // a deep copy of the device state; a sharded solver is bound to its communicator and can only be moved: detail::CommAttachment)
  ParNMPCSolver() = default;

  void initBackwardCorrection(const double t) {
    if (un_) { un_->initBackwardCorrection(t); return; }
    syncTaskRefs(t);
    if (shard_.comm()) detail::check(idocp_parnmpc_dist_init_backward_correction(h_.get(), t));
    else detail::check(idocp_parnmpc_init_backward_correction(h_.get(), t));
  }

  void updateSolution(const double t, const Eigen::VectorXd& q, const Eigen::VectorXd& v, const bool line_search = false) {
    if (un_) { un_->updateSolution(t, q, v, line_search); return; }
    cost_.sync(h_.get(), idocp_ocp_set_cost);
    syncTaskRefs(t);
    if (shard_.comm()) {
      if (idocp_comm_rank(shard_.comm()) == 0) detail::check(idocp_parnmpc_dist_set_initial_state(h_.get(), q.data(), v.data(), robot_.dimq(), robot_.dimv()));
      // (line_search: the probes of the filter line search are evaluated collectively, every rank runs the same filter)
      detail::check(line_search ? idocp_parnmpc_dist_update_solution_ls(h_.get(), t) : idocp_parnmpc_dist_update_solution(h_.get(), t));
      detail::check(idocp_ocp_synchronize(h_.get()));
      return;
    }
    detail::check(idocp_parnmpc_update_solution(h_.get(), t, q.data(), v.data(), line_search ? 1 : 0));
  }

  // ParNMPCSolver::getStateFeedbackGain (parnmpc_solver.cpp:116-125): the reference checks its arguments and leaves Kq, Kv as they are
  void getStateFeedbackGain(const int, Eigen::MatrixXd&, Eigen::MatrixXd&) const {}

  // (sharded: the value of the last collective computeKKTResidual)
  double KKTError() { return shard_.comm() ? kkt_error_ : detail::ContactCore<UnParNMPCSolver>::KKTError(); }
  void computeKKTResidual(const double t, const Eigen::VectorXd& q, const Eigen::VectorXd& v) {
    if (un_) { un_->computeKKTResidual(t, q, v); return; }
    cost_.sync(h_.get(), idocp_ocp_set_cost);
    syncTaskRefs(t);
    if (shard_.comm()) {
      if (idocp_comm_rank(shard_.comm()) == 0) detail::check(idocp_parnmpc_dist_set_initial_state(h_.get(), q.data(), v.data(), robot_.dimq(), robot_.dimv()));
      detail::check(idocp_parnmpc_dist_kkt_error(h_.get(), t, &kkt_error_));
      return;
    }
    detail::check(idocp_parnmpc_compute_kkt_residual(h_.get(), t, q.data(), v.data()));
  }

 private:
  detail::CommAttachment shard_;
  double kkt_error_ = 0.0;
};

}  // namespace idocp
#endif  // IDOCP_PARNMPC_SOLVER_HPP_
