// What idocp::OCPSolver, ParNMPCSolver, UnOCPSolver and UnParNMPCSolver share: the owner of a C ABI handle, the cost function shared with the
// driver, the one `check`, a core for the two fixed-base solvers and a core for the two contact solvers.  The four classes derive from a core and
// declare no destructor, copy or move member of their own (`= default` in the reference as well: ocp_solver.hpp:171-186, unocp_solver.hpp:59-74).
//
// A FIXED-BASE robot without contact frames (examples/iiwa14/ocp_benchmark.cpp, parnmpc_benchmark.cpp of the reference) given to a contact solver is
// bound to the kernels of idocp::UnOCPSolver / UnParNMPCSolver (ContactCore::un_): with no contact rows the contact-dynamics formulation (control u,
// the acceleration eliminated through M^-1, contact_dynamics.hxx:105-158) and the unconstrained one (control a, the torque eliminated through
// u = ID(q, v, a), unconstrained_dynamics.hxx:55-106) condense ONE Newton system in two orders -- same direction, step sizes, iterates and KKT error
// (oracle restatement of both: tests/test_oracle_fixed_base.py, 1e-11; GPU against the OCPSolver restatement: tests/test_fixed_base_ocp_gpu.py).
// What differs is kept: setSolution leaves the slack / dual variables alone (idocp_unocp_set_solution_only), initConstraints(t) takes a time,
// OCPSolver::getStateFeedbackGain returns the TORQUE policy.  A fixed-base robot WITH contact frames is refused.
#ifndef IDOCP_DETAIL_SOLVER_CORE_HPP_
#define IDOCP_DETAIL_SOLVER_CORE_HPP_

#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "idocp/constraints/constraints.hpp"
#include "idocp/cost/cost_function.hpp"
#include "idocp/eigen_shim.hpp"
#include "idocp/ocp/split_solution.hpp"
#include "idocp/robot/contact_status.hpp"
#include "idocp/robot/robot.hpp"
#include "idocp_hip.h"

namespace idocp {
namespace detail {

// a C ABI call that failed: its message on stderr + std::exit(EXIT_FAILURE), like the reference's argument errors
inline void check(int rc) {
  if (rc != IDOCP_OK) {
    std::cerr << idocp_last_error() << '\n';
    std::exit(EXIT_FAILURE);
  }
}

// Owner of a handle: a copy is a DEEP copy (Clone), a move steals the pointer and leaves null.  Null is a valid state (no call is made for it).
template <typename T, int (*Clone)(T*, T**), void (*Destroy)(T*)>
class OwnedHandle {
 public:
  OwnedHandle() = default;
  explicit OwnedHandle(T* p) : p_(p) {}
  ~OwnedHandle() { if (p_) Destroy(p_); }
  OwnedHandle(const OwnedHandle& other) : p_(cloneOf(other.p_)) {}
  OwnedHandle& operator=(const OwnedHandle& other) {
    if (this != &other) { T* n = cloneOf(other.p_); if (p_) Destroy(p_); p_ = n; }      // (clone first: a failed clone leaves this one as it was)
    return *this;
  }
  OwnedHandle(OwnedHandle&& other) noexcept : p_(other.p_) { other.p_ = nullptr; }
  OwnedHandle& operator=(OwnedHandle&& other) noexcept {
    if (this != &other) { if (p_) Destroy(p_); p_ = other.p_; other.p_ = nullptr; }
    return *this;
  }
  T* get() const { return p_; }
  T* operator->() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  static T* cloneOf(T* p) { T* n = nullptr; if (p) check(Clone(p, &n)); return n; }
  T* p_ = nullptr;
};
using OcpHandle = OwnedHandle<idocp_ocp_t, idocp_ocp_clone, idocp_ocp_destroy>;
using UnocpHandle = OwnedHandle<idocp_unocp_t, idocp_unocp_clone, idocp_unocp_destroy>;
// (the same owner over a C++ object: the fixed-base solver a contact solver is bound to)
template <typename S> int cloneObject(S* src, S** out) { *out = new S(*src); return IDOCP_OK; }
template <typename S> void destroyObject(S* p) { delete p; }

// The reference's solvers SHARE the cost function with the driver (ocp_solver.hpp:37-39, unocp_solver.hpp: shared_ptr members): a reference or weight
// the driver changes between two calls takes effect at the next one.  The device holds a copy; it is refreshed when the shared object has changed.
struct SharedCost {
  std::shared_ptr<CostFunction> cost;
  idocp_cost_t last{};      // what the device holds
  SharedCost() = default;
  explicit SharedCost(const std::shared_ptr<CostFunction>& c) : cost(c), last(c->native()) {}
  template <typename T>
  void sync(T* h, int (*set_cost)(T*, const idocp_cost_t*)) {
    if (!cost || !h) return;
    const idocp_cost_t c = cost->native();
    if (std::memcmp(&c, &last, sizeof(c)) != 0) { check(set_cost(h, &c)); last = c; }
  }
};

// idocp::UnOCPSolver (nstate = N + 1: a terminal stage) and idocp::UnParNMPCSolver (nstate = N) around an idocp_unocp_t
class FixedBaseCore {
 public:
  void initConstraints() { check(idocp_unocp_init_constraints(h_.get())); }

  // unocp_solver.hpp:96: const reference to the split solution of a time stage -- one device-to-host copy of the stage's record
  const SplitSolution& getSolution(const int stage) const {
    SplitSolution& s = cache_.at(stage);
    const int nv = robot_.dimv();
    std::vector<double> rec((size_t)7 * nv);
    check(idocp_unocp_get_split_solution(h_.get(), 0, stage, rec.data()));
    s.assign(rec.data(), nv, nv, nv, 0, 0);
    return s;
  }
  std::vector<Eigen::VectorXd> getSolution(const std::string& name) const {
    const int dim = robot_.dimv();
    const int n = (name == "a" || name == "u" || name == "beta") ? N_ : nstate_;
    std::vector<double> buf((size_t)(N_ + 1) * dim);
    check(idocp_unocp_get_solution(h_.get(), name.c_str(), 0, buf.data()));
    std::vector<Eigen::VectorXd> out(n, Eigen::VectorXd(dim));
    for (int i = 0; i < n; ++i) for (int j = 0; j < dim; ++j) out[i][j] = buf[(size_t)i * dim + j];
    return out;
  }
  void setSolution(const std::string& name, const Eigen::VectorXd& value) { check(idocp_unocp_set_solution(h_.get(), name.c_str(), value.data())); }
  void clearLineSearchFilter() { check(idocp_unocp_clear_line_search_filter(h_.get())); }

  // UnOCPSolver::isCurrentSolutionFeasible (unocp_solver.cpp:228-237)
  bool isCurrentSolutionFeasible() {
    int ok = 0, where = -1;
    check(idocp_unocp_is_current_solution_feasible(h_.get(), &ok, &where));
    if (!ok) std::cout << "INFEASIBLE at time stage " << where << std::endl;
    return ok != 0;
  }

  // printSolution / saveSolution (unocp_solver.cpp:266-352, unparnmpc_solver.cpp:243-327): the stage-wise solution on stdout / as a text file, one
  // stage per line.  "end-effector" needs frame kinematics of arbitrary frames, which the HIP path does not carry.
  void printSolution(const std::string& name = "all", const std::vector<int> frames = {}) const {
    (void)frames;
    if (name == "end-effector") { std::cerr << "printSolution(\"end-effector\") is not supported by the HIP path" << std::endl; return; }
    const char* fields[4] = {"q", "v", "a", "u"};
    if (name == "all") {
      std::vector<std::vector<Eigen::VectorXd>> all;
      for (const char* f : fields) all.push_back(getSolution(f));
      for (size_t i = 0; i < all[0].size(); ++i)
        for (int f = 0; f < 4; ++f)
          if (i < all[f].size()) std::cout << fields[f] << "[" << i << "] = " << all[f][i] << std::endl;
      return;
    }
    for (const char* f : fields) {
      if (name != f) continue;
      const std::vector<Eigen::VectorXd> sol = getSolution(f);
      for (size_t i = 0; i < sol.size(); ++i) std::cout << f << "[" << i << "] = " << sol[i] << std::endl;
    }
  }
  void saveSolution(const std::string& path_to_file, const std::string& name) const {
    std::ofstream file(path_to_file);
    if (name == "q" || name == "v" || name == "a" || name == "u") {
      const std::vector<Eigen::VectorXd> sol = getSolution(name);
      for (const Eigen::VectorXd& x : sol) {
        for (int j = 0; j < (int)x.size(); ++j) file << x[j] << " ";
        file << "\n";
      }
    }
    file.close();
  }

  double KKTError() {
    double e = 0;
    check(idocp_unocp_kkt_error(h_.get(), &e));
    return e;
  }
  idocp_unocp_t* handle() { return h_.get(); }

 protected:
  FixedBaseCore() = default;      // an empty solver, to be assigned a constructed one before use
  FixedBaseCore(const Robot& robot, const std::shared_ptr<CostFunction>& cost, const int N, const int nstate)
      : robot_(robot), N_(N), nstate_(nstate), cost_(cost), cache_(nstate) {}
  Robot robot_;
  int N_ = 0, nstate_ = 0;
  UnocpHandle h_;
  SharedCost cost_;
  mutable std::vector<SplitSolution> cache_;
};

// idocp::OCPSolver (nstate = N + 1) and idocp::ParNMPCSolver (nstate = N) around an idocp_ocp_t, or bound to the fixed-base solver Un (file head)
template <typename Un>
class ContactCore {
 public:
  void initConstraints(const double t) {
    if (un_) { un_->initConstraints(); return; }      // (the same stage times in both solvers: ocp_linearizer.cpp:50 / unocp_solver.cpp:64, parnmpc_linearizer.cpp:54 / unparnmpc_solver.cpp:59)
    syncTaskRefs(t);
    check(idocp_ocp_init_constraints(h_.get(), t));
  }

  // nstate entries for q, v, lmd, gmm and N otherwise (ParNMPCSolver: stage i lives at t + (i + 1) T / N)
  std::vector<Eigen::VectorXd> getSolution(const std::string& name) const {
    if (un_) {
      if (name == "f" || name == "mu" || name == "nu_passive") return std::vector<Eigen::VectorXd>(N_, Eigen::VectorXd(0));      // (no contact, no passive joint)
      return un_->getSolution(name);
    }
    const int dim = dimOf(name);
    const int n = (name == "q" || name == "v" || name == "lmd" || name == "gmm") ? nstate_ : N_;
    std::vector<double> buf((size_t)nstate_ * dim);
    check(idocp_ocp_get_solution(h_.get(), name.c_str(), 0, buf.data()));
    std::vector<Eigen::VectorXd> out(n, Eigen::VectorXd(dim));
    for (int i = 0; i < n; ++i) for (int j = 0; j < dim; ++j) out[i][j] = buf[(size_t)i * dim + j];
    return out;
  }

  // ocp_solver.hpp:97, parnmpc_solver.hpp:103: const reference to the split solution of a time stage, e.g. getSolution(0).u -- ONE device-to-host
  // copy of the stage's record (idocp_ocp_get_split_solution); the reference stays valid until the next call for the same stage
  const SplitSolution& getSolution(const int stage) const {
    if (un_) return un_->getSolution(stage);
    SplitSolution& s = cache_.at(stage);
    const int nv = robot_.dimv(), nc = robot_.maxPointContacts();
    std::vector<double> rec((size_t)5 * nv + robot_.dimq() + robot_.dimu() + 6 * nc + 6);
    check(idocp_ocp_get_split_solution(h_.get(), 0, stage, rec.data()));
    std::vector<int> active(nc > 0 ? nc : 1, 0);
    if (idocp_ocp_get_stage_contact_status(h_.get(), stage, active.data()) < 0) check(IDOCP_E_ARG);
    s.assign(rec.data(), robot_.dimq(), nv, robot_.dimu(), nc, robot_.dim_passive(), active.data());
    return s;
  }

  void setSolution(const std::string& name, const Eigen::VectorXd& value) {
    if (un_) { check(idocp_unocp_set_solution_only(un_->handle(), name.c_str(), value.data())); return; }      // (no re-initialisation of the constraints: parnmpc_solver.cpp:128-180)
    check(idocp_ocp_set_solution(h_.get(), name.c_str(), value.data()));
  }
  void setSolution(const std::string& name, const Eigen::Vector3d& value) {
    if (un_) {                                        // ocp_solver.cpp:143-153: "f" goes to every contact -- there is none
      if (name != "f") { std::cerr << "invalid arugment: name must be q, v, a, f, or u!" << '\n'; std::exit(EXIT_FAILURE); }
      return;
    }
    check(idocp_ocp_set_solution(h_.get(), name.c_str(), value.data()));
  }

  void setContactStatusUniformly(const ContactStatus& contact_status) {
    std::vector<int> active;
    std::vector<double> pts;
    flatten(contact_status, active, pts);
    if (un_) return;                                  // a status without contacts
    check(idocp_ocp_set_contact_status_uniformly(h_.get(), active.data(), pts.data()));
  }
  // ocp_solver.cpp:174-197, parnmpc_solver.cpp:179-206
  void pushBackContactStatus(const ContactStatus& contact_status, const double switching_time) {
    std::vector<int> active;
    std::vector<double> pts;
    flatten(contact_status, active, pts);
    if (un_) {                                        // a status without contacts after a status without contacts (contact_sequence.hxx:69-72)
      std::cerr << "discrete_event.existDiscreteEvent() must be true!" << '\n';
      std::exit(EXIT_FAILURE);
    }
    check(idocp_ocp_push_back_contact_status(h_.get(), active.data(), pts.data(), switching_time));
  }
  void setContactPoints(const int contact_phase, const std::vector<Eigen::Vector3d>& contact_points) {
    std::vector<double> pts(3 * contact_points.size());
    for (size_t c = 0; c < contact_points.size(); ++c) for (int k = 0; k < 3; ++k) pts[3 * c + k] = contact_points[c][k];
    if (un_) return;
    check(idocp_ocp_set_contact_points(h_.get(), contact_phase, pts.data()));
  }
  void popBackContactStatus() { if (!un_) check(idocp_ocp_pop_back_contact_status(h_.get())); }
  void popFrontContactStatus() { if (!un_) check(idocp_ocp_pop_front_contact_status(h_.get())); }
  void clearLineSearchFilter() { if (un_) un_->clearLineSearchFilter(); else check(idocp_ocp_clear_line_search_filter(h_.get())); }      // ocp_solver.cpp:196-199, parnmpc_solver.cpp:226-228

  // OCPSolver::isCurrentSolutionFeasible (ocp_solver.cpp:216-248), ParNMPCSolver's (parnmpc_solver.cpp:231-273)
  bool isCurrentSolutionFeasible() {
    if (un_) return un_->isCurrentSolutionFeasible();
    int ok = 0, where = -1;
    check(idocp_ocp_is_current_solution_feasible(h_.get(), &ok, &where));
    if (!ok) std::cout << "INFEASIBLE at stage " << where << " of the discretised horizon" << std::endl;
    return ok != 0;
  }

  double KKTError() {
    if (un_) return un_->KKTError();
    double e = 0;
    check(idocp_ocp_kkt_error(h_.get(), &e));
    return e;
  }
  idocp_ocp_t* handle() { return h_.get(); }
  // the solver a fixed-base robot without contacts is bound to (nullptr otherwise); handle() is null then
  Un* unconstrainedSolver() { return un_.get(); }

 protected:
  ContactCore() = default;      // an empty solver, to be assigned a constructed one before use
  ContactCore(const Robot& robot, const std::shared_ptr<CostFunction>& cost, const int N, const int nstate)
      : robot_(robot), N_(N), nstate_(nstate), cost_(cost), cache_(nstate) {}
  // a fixed-base robot without contact frames (no discrete event can ever be pushed): true, and the solver is bound to Un
  bool bindFixedBase(const Robot& robot, const std::shared_ptr<CostFunction>& cost, const std::shared_ptr<Constraints>& constraints,
                     const double T, const int N, const int nthreads, const int device) {
    if (robot.hasFloatingBase() || robot.maxPointContacts() != 0) return false;
    un_ = Bound(new Un(robot, cost, constraints, T, N, nthreads, device));
    return true;
  }
  // TimeVaryingTaskSpace3DCost / 6DCost on the floating base: the reference object is asked for its pose at the time of every stage of the
  // chain (time_varying_task_space_{3d,6d}_cost.cpp) -- up front, in front of every call that takes t
  void syncTaskRefs(const double t) {
    idocp_ocp_t* h = h_.get();
    if (!cost_.cost || !h || !cost_.cost->native().task_time_varying) return;
    if (chain_times_.size() < 4096) chain_times_.resize(4096);
    const int M = idocp_ocp_get_chain_times(h, t, (int)chain_times_.size(), chain_times_.data());
    if (M <= 0) check(M < 0 ? M : IDOCP_E_ARG);
    const std::vector<double> times(chain_times_.begin(), chain_times_.begin() + M);
    if (cost_.cost->taskRefsAt(times, task_refs_)) check(idocp_ocp_set_task_refs(h, t, M, task_refs_.data()));
  }
  int dimOf(const std::string& name) const {
    if (name == "q") return robot_.dimq();
    if (name == "u") return robot_.dimu();
    if (name == "f" || name == "mu") return robot_.max_dimf();
    if (name == "nu_passive") return robot_.dim_passive();
    return robot_.dimv();
  }
  static void flatten(const ContactStatus& cs, std::vector<int>& active, std::vector<double>& pts) {
    const int nc = cs.maxPointContacts();
    active.resize(nc); pts.resize(3 * (size_t)nc);
    for (int c = 0; c < nc; ++c) {
      active[c] = cs.isContactActive(c) ? 1 : 0;
      for (int k = 0; k < 3; ++k) pts[3 * c + k] = cs.contactPoint(c)[k];
    }
  }
  Robot robot_;
  int N_ = 0, nstate_ = 0;
  OcpHandle h_;
  SharedCost cost_;
  mutable std::vector<SplitSolution> cache_;
  std::vector<double> chain_times_, task_refs_;
  using Bound = OwnedHandle<Un, cloneObject<Un>, destroyObject<Un>>;
  Bound un_;
};

// The communicator a sharded ParNMPCSolver's handle is attached to (the communicator itself is not owned).  Declared behind the handle, so
// it detaches before the handle is destroyed.  A sharded solver is bound to its communicator: it can be moved, not copied.
class CommAttachment {
 public:
  CommAttachment() = default;
  CommAttachment(idocp_ocp_t* h, idocp_comm_t* comm) : h_(h), comm_(comm) { check(idocp_parnmpc_dist_attach(h, comm)); }
  ~CommAttachment() { if (comm_) idocp_parnmpc_dist_detach(h_); }
  CommAttachment(const CommAttachment& other) { if (other.comm_) refuse(); }
  CommAttachment& operator=(const CommAttachment& other) {
    if (this != &other && (other.comm_ || comm_)) refuse();
    return *this;
  }
  CommAttachment(CommAttachment&& other) noexcept : h_(other.h_), comm_(other.comm_) { other.h_ = nullptr; other.comm_ = nullptr; }
  CommAttachment& operator=(CommAttachment&& other) noexcept {      // (the handle this one was attached to is gone: its destroy dropped the attachment)
    if (this != &other) { h_ = other.h_; comm_ = other.comm_; other.h_ = nullptr; other.comm_ = nullptr; }
    return *this;
  }
  idocp_comm_t* comm() const { return comm_; }

 private:
  static void refuse() { std::cerr << "a sharded ParNMPCSolver cannot be copied\n"; std::exit(EXIT_FAILURE); }
  idocp_ocp_t* h_ = nullptr;
  idocp_comm_t* comm_ = nullptr;
};

}  // namespace detail
}  // namespace idocp
#endif  // IDOCP_DETAIL_SOLVER_CORE_HPP_
