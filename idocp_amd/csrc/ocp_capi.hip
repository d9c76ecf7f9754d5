// C-ABI implementation of the OCPSolver path (include/idocp_hip.h).
//
// Sequences the contact-path kernels like OCPSolver::updateSolution
// (src/ocp/ocp_solver.cpp:67-92): [host: per-stage reference q_ref(t_i)] ->
// tangent RNEA (K5a) -> condensation (K5b) -> backward / forward Riccati (S3, S4)
// -> expand primal + step sizes (K6) -> expand dual + integrate (K7).
// The contact sequence and the hybrid discretisation (OCPDiscretizer) are host-side
// index logic without a device call: ocp_chain.hpp plans the chain, this file uploads it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cost_reference.hpp"
#include "dev_lie.hpp"
#include "hip_try.hpp"
#include "host_util.hpp"
#include "idocp_hip.h"
#include "line_search_filter.hpp"
#include "model_shapes.hpp"
#include "ocp_forms.hpp"
#include "ocp_launch.hpp"

using namespace idocp_dev;
using idocp_host::set_last_error;
using idocp_host::isQuadruped;

namespace {

using DQ = LeggedDims<4, 3>;
using LQ = OcpLayout<DQ>;
static_assert(DQ::NC == IDOCP_MAX_CONTACTS, "the chain planner (ocp_chain.hpp) counts contacts with IDOCP_MAX_CONTACTS");

}  // namespace

struct idocp_ocp {
  idocp_model_t model;
  idocp_cost_t cost;
  idocp_constraints_t cons;
  int N, E, NS, batch, device;         // N = grid intervals (N_ideal), E = max number of discrete events, NS = slots per instance
  double T;
  hipStream_t stream = nullptr;
  OcpBuffers B{};
  OcpProblem prob;
  std::vector<void*> allocs;
  std::vector<size_t> alloc_bytes;   // parallel to allocs (idocp_ocp_clone copies buffer by buffer)
  double *d_q0 = nullptr, *d_v0 = nullptr, *d_tmp = nullptr, *d_qref = nullptr, *d_taskref = nullptr;
  // filter line search on a shard of a ParNMPC horizon (idocp_parnmpc_set_line_search_hooks, parnmpc_dist.hip): the trial iterate of the
  // state in front of the shard's first stage, and the two collective steps of one probe
  double *d_qtry = nullptr, *d_vtry = nullptr;
  int (*ls_pre)(idocp_ocp_t*) = nullptr;       // after the trial iterate is formed: exchange its boundary state
  int (*ls_post)(idocp_ocp_t*) = nullptr;      // after the shard's sums are formed: all-reduce them
  std::vector<double> task_refs_host;      // idocp_ocp_set_task_refs: [M][12] for the chain discretised at task_refs_t
  double task_refs_t = 0.0;
  bool task_refs_stale = false;            // a lenient discretisation (creation, clone, the chain getters) put the constant pose into the table
  void* d_prob = nullptr;
  OcpNode* d_nodes = nullptr;
  bool parnmpc = false;               // backward-Euler stages + backward correction instead of the Riccati sweep
  int stage_offset = 0;               // ParNMPC horizon sharding: global index of the first stage of this shard
  ContactSequence seq;                // ocp_chain.hpp
  ChainPlan plan;                     // chain of the last discretisation (planChain), as the device holds it
  double disc_time = NAN;
  bool seq_dirty = true;
  int* d_impulse_pos = nullptr;
  int* d_switch_pos = nullptr;
  int* d_general_pos = nullptr;     // ParNMPC: chain positions of the aux (switching rows) / impulse stages
  int* d_cond_pos = nullptr;        // chain positions by stage class of K5b (all feet | half of them | the rest)
  int slice_begin = 0, slice_end = -1;   // ParNMPC with events: this handle keeps the grid stages [slice_begin, slice_end) of the chain (-1: all)
  int M() const { return plan.M(); }
  // hipGraph of one updateSolution (idocp_ocp_update_solution_graph): valid while the discretisation and the input buffers stay
  long disc_epoch = 0, graph_epoch = -1;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  const double *graph_q = nullptr, *graph_v = nullptr;
  bool launched_eagerly = false;
  // filter line search (LineSearchFilter, src/line_search/line_search_filter.cpp): one filter per instance
  std::vector<idocp_host::LineSearchFilter> filters;
  OcpNode* d_nodes_ls = nullptr;
  double* ext_try = nullptr;
  OcpForms forms;                     // which form of a kernel this handle runs (ocp_forms.hpp); idocp_ocp_clone copies the record
  // staging of the per-stage setters (idocp_ocp_set_solution_stages / _chain, the aux-matrix setters): an MPC loop warm-starts every tick, so
  // the device scratch and its pinned host twin are kept (grown on demand) and the setter returns without a stream synchronisation -- the
  // copy and the fill kernel are stream-ordered in front of whatever the caller launches next; fill_done guards the reuse of the host twin
  double *d_fill = nullptr, *h_fill = nullptr;
  size_t fill_cap = 0;
  hipEvent_t fill_done = nullptr;
  // fork / join inside an iteration (round 6): the switching-constraint kernel K5s runs on a stream of its own NEXT TO the nominal sweeps K5n
  // (both read the iterate only and write records of their own); the condensation launches wait for both.  Present where
  // useSideStream(forms, ...) says so (ocp_forms.hpp, idocp_ocp_set_side_stream); every entry point joins an open fork first (enterO).
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool side_pending = false;          // a kernel is in flight on `side` that the next condensation launch has to wait for
};

namespace {

int allocBufO(idocp_ocp* h, double** p, size_t n) {
  HIP_TRY(hipMalloc((void**)p, n * sizeof(double)));
  h->allocs.push_back(*p); h->alloc_bytes.push_back(n * sizeof(double));
  HIP_TRY(hipMemsetAsync(*p, 0, n * sizeof(double), h->stream));
  return IDOCP_OK;
}
int setDev(const idocp_ocp* h) { HIP_TRY(hipSetDevice(h->device)); return IDOCP_OK; }
// a fork opened by launchSwitchO is closed here: the handle's stream waits for what is in flight on the side stream
int joinSideO(idocp_ocp* h) {
  if (h->side_pending) { HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0)); h->side_pending = false; }
  return IDOCP_OK;
}
// The head of every entry point that launches on or reads through h->stream: the handle's device, and no fork left open
// (idocp_ocp_launch_kernel id 0 alone leaves one for ids 7, 8, 1, 2 -- or whatever entry comes next -- to close).
int enterO(idocp_ocp* h) {
  int rc = setDev(h); if (rc) return rc;
  return joinSideO(h);
}
// the measured state of a host-pointer entry point, into the handle's staging buffers (v == nullptr: the configuration alone)
int uploadStateO(idocp_ocp* h, const double* q, const double* v) {
  HIP_TRY(hipMemcpyAsync(h->d_q0, q, sizeof(double) * h->batch * DQ::NQ, hipMemcpyHostToDevice, h->stream));
  if (v) HIP_TRY(hipMemcpyAsync(h->d_v0, v, sizeof(double) * h->batch * DQ::NV, hipMemcpyHostToDevice, h->stream));
  return IDOCP_OK;
}
void dropSideO(idocp_ocp* h) {
  if (h->side) { (void)hipStreamDestroy(h->side); h->side = nullptr; }
  if (h->ev_fork) { (void)hipEventDestroy(h->ev_fork); h->ev_fork = nullptr; }
  if (h->ev_join) { (void)hipEventDestroy(h->ev_join); h->ev_join = nullptr; }
}
// The side stream and its two events exist exactly while the handle's forms ask for them (creation, idocp_ocp_set_side_stream).  Both
// streams are drained first: nothing is in flight on a stream that goes away, and nothing that was forked stays unjoined.
int applySideStreamO(idocp_ocp* h) {
  const bool want = useSideStream(h->forms, h->batch, h->parnmpc);
  if (want == (h->side != nullptr)) return IDOCP_OK;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->side) HIP_TRY(hipStreamSynchronize(h->side));
  h->side_pending = false;
  if (!want) { dropSideO(h); return IDOCP_OK; }
  if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    dropSideO(h);
    set_last_error("side stream: hipStreamCreate / hipEventCreate failed");
    return IDOCP_E_DEVICE;
  }
  return IDOCP_OK;
}

using idocp_host::qRefAt;        // the reference of a stage time: cost_reference.hpp, shared with the rollout scoring
using idocp_host::vRefOnAt;

// reference poses of a TimeVarying task-space cost must exist for the chain (t, M) unless the caller only asks for the chain's shape
// (lenient: creation, clone and the chain getters discretise without poses -- the constant pose goes into the table)
int taskRefsAvailable(idocp_ocp* h, double t, int M, bool lenient) {
  if (h->cost.task_dim == 0 || !h->cost.task_time_varying || lenient) return IDOCP_OK;
  if (h->task_refs_host.size() != (size_t)M * 12 || h->task_refs_t != t) {
    set_last_error("TimeVarying task-space cost: no reference poses for this chain (idocp_ocp_set_task_refs with the same t, M = the chain's length)");
    return IDOCP_E_ARG;
  }
  return IDOCP_OK;
}

// The upload half of a discretisation: the plan the handle holds goes to the device together with everything that depends on the cost --
// vref_on of the nodes, the q_ref table, the reference poses of the task-space cost (the constant pose of the cost, or -- TimeVarying
// variants -- the poses the caller evaluated at the stage times: idocp_ocp_get_chain_times -> idocp_ocp_set_task_refs) -- and the
// problem header.  Uploads the lists this solver kind's kernels read, and only those.
int commitChain(idocp_ocp* h, double t) {
  ChainPlan& plan = h->plan;
  const int M = plan.M();
  std::vector<double> tab((size_t)M * DQ::NQ), poses;
  for (int p = 0; p < M; ++p) {
    qRefAt(h->cost, DQ::NQ, plan.chain_t[p], &tab[(size_t)p * DQ::NQ]);
    plan.nodes[p].vref_on = vRefOnAt(h->cost, plan.chain_t[p]);
    if (!h->parnmpc) plan.nodes_ls[p].vref_on = plan.nodes[p].vref_on;
    else if (parnmpcShape<LQ>(plan.nodes[p]).general) plan.general_pos.push_back(p);
  }
  h->prob.M = M; h->prob.NS = h->NS;
  h->prob.has_terminal = plan.has_terminal ? 1 : 0; h->prob.has_prev = plan.has_prev ? 1 : 0; h->prob.stage_offset = plan.stage_offset;
  h->B.M = M; h->B.NS = h->NS;
  h->B.n_impulse_fe = h->parnmpc ? 0 : plan.n_impulse();
  h->B.n_switch = (int)plan.switch_pos.size();
  auto upload = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess; };
  HIP_TRY(upload(h->d_qref, tab.data(), tab.size() * sizeof(double)));
  if (h->cost.task_dim != 0) {
    const bool have = h->cost.task_time_varying && h->task_refs_host.size() == (size_t)M * 12 && h->task_refs_t == t;
    if (have) poses = h->task_refs_host;
    else { poses.resize((size_t)M * 12); for (int p = 0; p < M; ++p) for (int k = 0; k < 12; ++k) poses[(size_t)p * 12 + k] = h->cost.task_ref[k]; }
    h->task_refs_stale = h->cost.task_time_varying && !have;      // ... to be redone by the next strict discretisation
    HIP_TRY(upload(h->d_taskref, poses.data(), poses.size() * sizeof(double)));
  }
  HIP_TRY(upload(h->d_nodes, plan.nodes.data(), sizeof(OcpNode) * M));
  if (!h->parnmpc) HIP_TRY(upload(h->d_nodes_ls, plan.nodes_ls.data(), sizeof(OcpNode) * M));
  HIP_TRY(upload(h->d_impulse_pos, plan.impulse_pos.data(), sizeof(int) * plan.impulse_pos.size()));
  HIP_TRY(upload(h->d_switch_pos, plan.switch_pos.data(), sizeof(int) * plan.switch_pos.size()));
  HIP_TRY(upload(h->d_general_pos, plan.general_pos.data(), sizeof(int) * plan.general_pos.size()));
  if (!h->parnmpc) HIP_TRY(upload(h->d_cond_pos, plan.cond_pos.data(), sizeof(int) * plan.cond_pos.size()));
  HIP_TRY(hipMemcpyAsync(h->d_prob, &h->prob, sizeof(OcpProblem), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));     // tab and poses are stack temporaries
  h->disc_time = t; h->seq_dirty = false; ++h->disc_epoch;
  return IDOCP_OK;
}

// OCPDiscretizer / ParNMPCDiscretizer::discretizeOCP(contact_sequence, t): planChain (ocp_chain.hpp) builds the chain as a value; the
// handle takes it -- and the device sees it -- only when nothing refuses it, so a refused discretisation leaves the handle describing
// the discretisation its device tables still hold.  Re-run only when the initial time or the contact sequence changes.
int discretize(idocp_ocp* h, double t, bool lenient = false) {
  if (!h->seq_dirty && h->disc_time == t && !(h->task_refs_stale && !lenient)) return IDOCP_OK;
  ChainResult r = planChain(h->seq, t, {h->N, h->E, h->T, h->parnmpc, h->stage_offset, h->slice_begin, h->slice_end, h->plan.has_terminal, h->plan.has_prev});
  if (r.rc) { set_last_error(r.error); return r.rc; }
  if (taskRefsAvailable(h, t, r.plan.M(), lenient)) return IDOCP_E_ARG;
  h->plan = std::move(r.plan);
  return commitChain(h, t);
}
// the chain of the last discretisation, or of t = 0 when there has been none
int ensureDiscretized(idocp_ocp* h) {
  if (!h->seq_dirty && h->disc_time == h->disc_time) return IDOCP_OK;
  return discretize(h, h->disc_time == h->disc_time ? h->disc_time : 0.0);
}

struct Field { int offset, dim, extra; };
bool solFieldO(const std::string& n, Field& f) {
  if (n == "lmd") f = {LQ::S_LMD, DQ::NV, 1};
  else if (n == "gmm") f = {LQ::S_GMM, DQ::NV, 1};
  else if (n == "q") f = {LQ::S_Q, DQ::NQ, 1};
  else if (n == "v") f = {LQ::S_V, DQ::NV, 1};
  else if (n == "a") f = {LQ::S_A, DQ::NV, 0};
  else if (n == "u") f = {LQ::S_U, DQ::NU, 0};
  else if (n == "beta") f = {LQ::S_BETA, DQ::NV, 0};
  else if (n == "f") f = {LQ::S_F, DQ::NF, 0};
  else if (n == "mu") f = {LQ::S_MU, DQ::NF, 0};
  else if (n == "nu_passive") f = {LQ::S_NUP, 6, 0};
  else if (n == "xi") f = {LQ::S_XI, DQ::NF, 0};
  else return false;
  return true;
}
bool dirFieldO(const std::string& n, Field& f) {
  if (n == "dlmd") f = {LQ::D_LMD, DQ::NV, 1};
  else if (n == "dgmm") f = {LQ::D_GMM, DQ::NV, 1};
  else if (n == "dq") f = {LQ::D_Q, DQ::NV, 1};
  else if (n == "dv") f = {LQ::D_V, DQ::NV, 1};
  else if (n == "da") f = {LQ::D_A, DQ::NV, 0};
  else if (n == "du") f = {LQ::D_U, DQ::NU, 0};
  else if (n == "dbeta") f = {LQ::D_BETA, DQ::NV, 0};
  else if (n == "df") f = {LQ::D_F, DQ::NF, 0};
  else if (n == "dmu") f = {LQ::D_MU, DQ::NF, 0};
  else if (n == "dnu_passive") f = {LQ::D_NUP, 6, 0};
  else if (n == "dxi") f = {LQ::D_XI, DQ::NF, 0};
  else return false;
  return true;
}

int copyField(idocp_ocp* h, const double* base, size_t stride, size_t nrec, const Field& f, double* out) {
  HIP_TRY(hipMemcpy2DAsync(out, f.dim * sizeof(double), base + f.offset, stride * sizeof(double), f.dim * sizeof(double), nrec,
                           hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

}  // namespace

extern "C" {

// the cost-dependent fields of the device problem block (idocp_ocp_create*, idocp_ocp_set_cost)
static void fillCostFields(OcpProblem& p, const idocp_cost_t& cost) {
  for (int i = 0; i < DQ::NV; ++i) {
    p.v_ref[i] = cost.v_ref[i]; p.q_weight[i] = cost.q_weight[i]; p.v_weight[i] = cost.v_weight[i]; p.a_weight[i] = cost.a_weight[i];
    p.qf_weight[i] = cost.qf_weight[i]; p.vf_weight[i] = cost.vf_weight[i];
    p.qi_weight[i] = cost.qi_weight[i]; p.vi_weight[i] = cost.vi_weight[i]; p.dvi_weight[i] = cost.dvi_weight[i];
  }
  if (cost.use_trotting_ref) p.v_ref[0] = cost.step_length / cost.t_period;     // trotting_configuration_space_cost.cpp:81-83
  for (int i = 0; i < DQ::NU; ++i) { p.u_ref[i] = cost.u_ref[i]; p.u_weight[i] = cost.u_weight[i]; }
  for (int c = 0; c < DQ::NC; ++c)
    for (int k = 0; k < 3; ++k) {
      p.f_weight[c][k] = cost.f_weight[c][k]; p.f_ref[c][k] = cost.f_ref[c][k];
      p.fi_weight[c][k] = cost.fi_weight[c][k]; p.fi_ref[c][k] = cost.fi_ref[c][k];
    }
  p.task_dim = cost.task_dim; p.task_joint = cost.task_joint;
  for (int k = 0; k < 9; ++k) p.task_R[k] = cost.task_frame_R[k];
  for (int k = 0; k < 3; ++k) p.task_p[k] = cost.task_frame_p[k];
  for (int k = 0; k < 6; ++k) { p.task_weight[k] = cost.task_weight[k]; p.task_weightf[k] = cost.task_weightf[k]; p.task_weighti[k] = cost.task_weighti[k]; }
  for (int k = 0; k < 12; ++k) p.task_ref[k] = cost.task_ref[k];
  const int nextra = cost.task_dim ? cost.task_extra_count : 0;
  p.task_n = cost.task_dim ? 1 + nextra : 0;
  for (int e = 0; e < IDOCP_MAX_EXTRA_TASKS; ++e) {
    OcpProblem::TaskExtra& o = p.task_extra[e];
    std::memset(&o, 0, sizeof(o));
    if (e >= nextra) continue;
    const idocp_task_component_t& t = cost.task_extra[e];
    o.dim = t.dim; o.joint = t.joint;
    for (int k = 0; k < 9; ++k) o.R[k] = t.frame_R[k];
    for (int k = 0; k < 3; ++k) o.p[k] = t.frame_p[k];
    for (int k = 0; k < 6; ++k) { o.weight[k] = t.weight[k]; o.weightf[k] = t.weightf[k]; o.weighti[k] = t.weighti[k]; }
    for (int k = 0; k < 12; ++k) o.ref[k] = t.ref[k];
  }
}
// the task_extra components of a cost block (idocp_cost_t): count, dimensions and frames
static int checkTaskExtras(const idocp_cost_t* cost) {
  if (cost->task_extra_count < 0 || cost->task_extra_count > IDOCP_MAX_EXTRA_TASKS) { set_last_error("invalid value: task_extra_count must be 0 .. " + std::to_string(IDOCP_MAX_EXTRA_TASKS)); return IDOCP_E_ARG; }
  if (cost->task_extra_count > 0 && cost->task_dim == 0) { set_last_error("invalid value: task_extra components need the first task-space component (task_dim != 0)"); return IDOCP_E_ARG; }
  for (int e = 0; e < cost->task_extra_count; ++e) {
    const idocp_task_component_t& t = cost->task_extra[e];
    if (t.dim != 3 && t.dim != 6) { set_last_error("invalid value: task_extra[" + std::to_string(e) + "].dim must be 3 or 6"); return IDOCP_E_ARG; }
    if (t.joint < 0 || t.joint > DQ::NU) { set_last_error("invalid value: the frame of task_extra[" + std::to_string(e) + "] must sit on the floating base or on a leg link"); return IDOCP_E_ARG; }
  }
  return IDOCP_OK;
}

static int createOcpImpl(const idocp_model_t* model, const idocp_cost_t* cost, const idocp_constraints_t* constraints, double T,
                         int N, int max_num_impulse, int batch, int device, bool parnmpc, idocp_ocp_t** out, const OcpForms* forms = nullptr) {
  if (!model || !cost || !constraints || !out) { set_last_error("idocp_ocp_create: null argument"); return IDOCP_E_ARG; }
  if (!(T > 0)) { set_last_error("invalid value: T must be positive!"); return IDOCP_E_ARG; }       // ocp_solver.cpp:27-44
  if (N <= 0) { set_last_error("invalid value: N must be positive!"); return IDOCP_E_ARG; }
  if (max_num_impulse < 0) { set_last_error("invalid value: max_num_impulse must be non-negative!"); return IDOCP_E_ARG; }
  if (batch <= 0) { set_last_error("invalid value: batch must be positive!"); return IDOCP_E_ARG; }
  // ConstraintComponentBase::setBarrier / setFractionToBoundaryRate (constraint_component_base.hxx:10-24) assert these; a
  // non-positive barrier would make the slack initialisation (pdipm.hxx:13-24) loop forever on the device
  if (!(constraints->barrier > 0)) { set_last_error("invalid value: barrier must be positive!"); return IDOCP_E_ARG; }
  // JointAcceleration*Limit bounds: finite, and a_min < a_max where both are in use (an empty interval has no interior point to start the
  // barrier method from)
  for (int r = 0; r < model->nu; ++r) {
    const bool lo = constraints->joint_acceleration_lower_limit != 0, hi = constraints->joint_acceleration_upper_limit != 0;
    if ((lo && !std::isfinite(constraints->a_min[r])) || (hi && !std::isfinite(constraints->a_max[r]))) { set_last_error("invalid value: joint acceleration bounds must be finite!"); return IDOCP_E_ARG; }
    if (lo && hi && !(constraints->a_min[r] < constraints->a_max[r])) { set_last_error("invalid value: a_min must be smaller than a_max!"); return IDOCP_E_ARG; }
  }
  if ((constraints->linearized_friction_cone && constraints->friction_cone) || (constraints->linearized_impulse_friction_cone && constraints->impulse_friction_cone)) {
    set_last_error("unsupported constraints: LinearizedFrictionCone and FrictionCone (or their impulse twins) together; the stage kernels carry one cone per kind of stage");
    return IDOCP_E_UNSUPPORTED;
  }
  if (!(constraints->fraction_to_boundary_rate > 0 && constraints->fraction_to_boundary_rate <= 1)) {
    set_last_error("invalid value: fraction_to_boundary_rate must be in (0, 1]!"); return IDOCP_E_ARG;
  }
  if (cost->task_dim != 0) {
    if (cost->task_dim != 3 && cost->task_dim != 6) { set_last_error("invalid value: task_dim must be 0, 3 or 6"); return IDOCP_E_ARG; }
    if (cost->task_joint < 0 || cost->task_joint > DQ::NU) { set_last_error("invalid value: the task frame must sit on the floating base or on a leg link"); return IDOCP_E_ARG; }
  }
  { const int rc_t = checkTaskExtras(cost); if (rc_t) return rc_t; }
  if (!isQuadruped(*model)) {
    set_last_error("idocp_ocp_create: this build carries OCP kernels for a floating-base quadruped (4 legs x 3 joints, 4 point contacts) only");
    return IDOCP_E_UNSUPPORTED;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: the idocp HIP path has no CPU fallback");
    return IDOCP_E_DEVICE;
  }
  if (device < 0 || device >= ndev) { set_last_error("invalid device ordinal"); return IDOCP_E_ARG; }
  idocp_ocp* h = new idocp_ocp();
  h->model = *model; h->cost = *cost; h->cons = *constraints; h->N = N; h->E = max_num_impulse; h->batch = batch; h->device = device; h->T = T;
  h->NS = N + 1 + 3 * max_num_impulse;
  auto fail = [&](int code) { (void)hipGetLastError(); idocp_ocp_destroy(h); return code; };      // (clears HIP's sticky last error: see HIP_TRY)
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->stream) != hipSuccess) { set_last_error("hipStreamCreate failed"); return fail(IDOCP_E_DEVICE); }
  h->parnmpc = parnmpc;
  if (forms) h->forms = *forms;      // idocp_ocp_clone: the source's record
  else { const idocp_host::EnvSettings env = idocp_host::envSettings(); h->forms.prof_dimf = env.prof_dimf; h->forms.general_axes = env.general_axes ? 1 : 0; }
  { const int rc_s = applySideStreamO(h); if (rc_s) return fail(rc_s); }
  const size_t ns = (size_t)batch * h->NS;
  OcpBuffers& B = h->B;
  int rc;
  double* tmp;
  if ((rc = allocBufO(h, &B.sol, ns * LQ::SOL))) return fail(rc);
  if ((rc = allocBufO(h, &B.dir, ns * LQ::DIR))) return fail(rc);
  if ((rc = allocBufO(h, &B.slack, ns * LQ::CON))) return fail(rc);
  if ((rc = allocBufO(h, &B.dual, ns * LQ::CON))) return fail(rc);
  if ((rc = allocBufO(h, &B.lin, ns * LQ::LIN))) return fail(rc);
  if ((rc = allocBufO(h, &B.lie, ns * LQ::LIE))) return fail(rc);
  if ((rc = allocBufO(h, &B.nom, ns * LQ::NOM))) return fail(rc);
  if ((rc = allocBufO(h, &B.kkt, ns * LQ::KKT))) return fail(rc);
  if ((rc = allocBufO(h, &B.exp, ns * LQ::EXP))) return fail(rc);
  if ((rc = allocBufO(h, &B.ric, ns * LQ::RIC))) return fail(rc);
  if ((rc = allocBufO(h, &B.gain, ns * LQ::GAIN))) return fail(rc);
  if ((rc = allocBufO(h, &B.swc, max_num_impulse > 0 ? ns * LQ::SWC : 16))) return fail(rc);
  if (parnmpc) {
    if ((rc = allocBufO(h, &B.snew, ns * LQ::SNEW))) return fail(rc);
    if ((rc = allocBufO(h, &B.kinv, ns * LQ::KINV))) return fail(rc);
    if ((rc = allocBufO(h, &B.aux, ns * LQ::AUX))) return fail(rc);
    if ((rc = allocBufO(h, &B.xres, ns * LQ::XRES))) return fail(rc);
    if ((rc = allocBufO(h, &B.fwd_prev, (size_t)batch * (DQ::NQ + DQ::NV)))) return fail(rc);
  }
  if ((rc = allocBufO(h, &B.step_stage, ns * 2))) return fail(rc);
  if ((rc = allocBufO(h, &B.step, (size_t)batch * 2))) return fail(rc);
  if ((rc = allocBufO(h, &B.err_stage, ns))) return fail(rc);
  if ((rc = allocBufO(h, &B.err, (size_t)batch))) return fail(rc);
  if ((rc = allocBufO(h, &B.sol_try, ns * LQ::SOL))) return fail(rc);
  B.ext = nullptr; h->ext_try = nullptr;
  if (constraints->contact_distance || cost->task_dim != 0) {      // terms with frame Jacobians of their own (ocp_ext_kernel.hip), of the iterate and of the line search's trial iterate
    if ((rc = allocBufO(h, &B.ext, ns * LQ::EXT))) return fail(rc);
    if ((rc = allocBufO(h, &h->ext_try, ns * LQ::EXT))) return fail(rc);
  }
  if ((rc = allocBufO(h, &B.merit_stage, ns * 4))) return fail(rc);
  if ((rc = allocBufO(h, &B.merit, (size_t)batch * 2))) return fail(rc);
  if ((rc = allocBufO(h, &B.ls_alpha, (size_t)batch))) return fail(rc);
  { double* tmp_ls = nullptr; if ((rc = allocBufO(h, &tmp_ls, ((size_t)h->NS * sizeof(OcpNode) + 7) / 8))) return fail(rc); h->d_nodes_ls = reinterpret_cast<OcpNode*>(tmp_ls); B.nodes_ls = h->d_nodes_ls; }
  h->filters.assign(batch, {});
  if ((rc = allocBufO(h, &h->d_q0, (size_t)batch * DQ::NQ))) return fail(rc);
  if ((rc = allocBufO(h, &h->d_v0, (size_t)batch * DQ::NV))) return fail(rc);
  if (parnmpc) {
    if ((rc = allocBufO(h, &h->d_qtry, (size_t)batch * DQ::NQ))) return fail(rc);
    if ((rc = allocBufO(h, &h->d_vtry, (size_t)batch * DQ::NV))) return fail(rc);
  }
  if ((rc = allocBufO(h, &h->d_tmp, (size_t)batch * IDOCP_MAX_NQ))) return fail(rc);
  if ((rc = allocBufO(h, &h->d_qref, (size_t)h->NS * DQ::NQ))) return fail(rc);
  if ((rc = allocBufO(h, &h->d_taskref, (size_t)h->NS * 12))) return fail(rc);
  if ((rc = allocBufO(h, &tmp, ((size_t)batch * sizeof(int) + 7) / 8))) return fail(rc);
  B.status = reinterpret_cast<int*>(tmp);
  if ((rc = allocBufO(h, &tmp, 64))) return fail(rc);
  B.prof = reinterpret_cast<long long*>(tmp);
  B.prof_dimf = h->forms.prof_dimf;
  if ((rc = allocBufO(h, &tmp, ((size_t)h->NS * sizeof(OcpNode) + 7) / 8))) return fail(rc);
  h->d_nodes = reinterpret_cast<OcpNode*>(tmp);
  B.nodes = h->d_nodes;
  if ((rc = allocBufO(h, &tmp, ((size_t)(max_num_impulse + 1) * sizeof(int) + 7) / 8))) return fail(rc);
  h->d_impulse_pos = reinterpret_cast<int*>(tmp);
  B.impulse_pos = h->d_impulse_pos;
  if ((rc = allocBufO(h, &tmp, ((size_t)(max_num_impulse + 1) * sizeof(int) + 7) / 8))) return fail(rc);
  h->d_switch_pos = reinterpret_cast<int*>(tmp);
  B.switch_pos = h->d_switch_pos;
  B.n_switch = 0;
  if ((rc = allocBufO(h, &tmp, ((size_t)(2 * max_num_impulse + 1) * sizeof(int) + 7) / 8))) return fail(rc);
  h->d_general_pos = reinterpret_cast<int*>(tmp);
  B.general_pos = h->d_general_pos;
  if ((rc = allocBufO(h, &tmp, ((size_t)h->NS * sizeof(int) + 7) / 8))) return fail(rc);
  h->d_cond_pos = reinterpret_cast<int*>(tmp);
  B.cond_pos = h->d_cond_pos;
  B.q_ref = h->d_qref;
  B.task_refs = h->d_taskref;
  B.leg_axes_xyy = 1;
  for (int leg = 0; leg < DQ::NL; ++leg)
    for (int j = 0; j < DQ::LJ; ++j) {
      const int ji = 1 + leg * DQ::LJ + j;
      const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      const double ax[3] = {j == 0 ? 1.0 : 0.0, j == 0 ? 0.0 : 1.0, 0.0};
      for (int k = 0; k < 9; ++k) if (model->plc_R[ji][k] != I3[k]) B.leg_axes_xyy = 0;
      for (int k = 0; k < 3; ++k) if (model->axis[ji][k] != ax[k]) B.leg_axes_xyy = 0;
    }
  for (int c = 0; c < DQ::NC; ++c) {      // ... and contact frames that are not rotated against their joint
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) if (model->contact_R[c][k] != I3[k]) B.leg_axes_xyy = 0;
  }
  if (h->forms.general_axes) B.leg_axes_xyy = 0;      // tests: the general instantiations on a model that qualifies for the special ones
  DevModel dm; idocp_host::toDevModel(*model, dm);
  OcpProblem& p = h->prob;
  std::memset(&p, 0, sizeof(p));
  p.N = N; p.batch = batch; p.T = T; p.dt = T / N; p.NS = h->NS; p.E = max_num_impulse; p.backward_euler = parnmpc ? 1 : 0; p.has_terminal = 1; p.has_prev = 0;
  p.baumgarte_time_step = T / N;                           // hybrid_container.hpp:186-188
  fillCostFields(p, *cost);
  for (int i = 0; i < DQ::NU; ++i) { p.q_min[i] = model->q_min[i]; p.q_max[i] = model->q_max[i]; p.v_max[i] = model->v_max[i]; p.u_max[i] = model->u_max[i]; }
  for (int c = 0; c < DQ::NC; ++c) {
    for (int k = 0; k < 3; ++k) p.contact_p[c][k] = model->contact_p[c][k];
    std::memcpy(p.contact_R[c], model->contact_R[c], sizeof(double) * 9);
  }
  p.use_q_limits = constraints->joint_position_limits; p.use_v_limits = constraints->joint_velocity_limits;
  p.use_u_limits = constraints->joint_torque_limits;
  p.use_a_lower = constraints->joint_acceleration_lower_limit ? 1 : 0;
  p.use_contact_distance = constraints->contact_distance ? 1 : 0;
  p.use_a_upper = constraints->joint_acceleration_upper_limit ? 1 : 0;
  for (int r = 0; r < IDOCP_MAX_NV; ++r) { p.a_min[r] = constraints->a_min[r]; p.a_max[r] = constraints->a_max[r]; }
  p.use_friction_cone = (constraints->linearized_friction_cone || constraints->friction_cone) ? 1 : 0;
  p.use_impulse_friction_cone = (constraints->linearized_impulse_friction_cone || constraints->impulse_friction_cone) ? 1 : 0;
  p.cone_kind = constraints->friction_cone ? 1 : 0; p.impulse_cone_kind = constraints->impulse_friction_cone ? 1 : 0;
  p.mu = constraints->mu; p.barrier = constraints->barrier; p.fraction_rate = constraints->fraction_to_boundary_rate;
  void* d_model = nullptr;
  if (hipMalloc(&d_model, sizeof(DevModel)) != hipSuccess || hipMalloc(&h->d_prob, sizeof(OcpProblem)) != hipSuccess) {
    set_last_error("hipMalloc failed"); return fail(IDOCP_E_DEVICE);
  }
  h->allocs.push_back(d_model); h->alloc_bytes.push_back(sizeof(DevModel));
  h->allocs.push_back(h->d_prob); h->alloc_bytes.push_back(sizeof(OcpProblem));
  if (hipMemcpyAsync(d_model, &dm, sizeof(dm), hipMemcpyHostToDevice, h->stream) != hipSuccess) { set_last_error("hipMemcpy failed"); return fail(IDOCP_E_DEVICE); }
  B.model = static_cast<const DevModel*>(d_model);
  B.prob = static_cast<const OcpProblem*>(h->d_prob);
  if ((rc = discretize(h, 0.0, true))) return fail(rc);
  // identity quaternion in every q so that an unset solution is a valid configuration
  {
    std::vector<double> q(DQ::NQ, 0.0); q[6] = 1.0;
    if (hipMemcpyAsync(h->d_tmp, q.data(), sizeof(double) * DQ::NQ, hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail(IDOCP_E_DEVICE);
    ocpFillField(B.sol, LQ::SOL, LQ::S_Q, DQ::NQ, h->NS, batch, h->d_tmp, 0, 1, h->stream);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(IDOCP_E_DEVICE);
  }
  *out = h;
  return IDOCP_OK;
}

int idocp_ocp_create_hybrid(const idocp_model_t* model, const idocp_cost_t* cost, const idocp_constraints_t* constraints, double T,
                            int N, int max_num_impulse, int batch, int device, idocp_ocp_t** out) {
  return createOcpImpl(model, cost, constraints, T, N, max_num_impulse, batch, device, false, out);
}
int idocp_ocp_create(const idocp_model_t* model, const idocp_cost_t* cost, const idocp_constraints_t* constraints, double T,
                     int N, int batch, int device, idocp_ocp_t** out) {
  return createOcpImpl(model, cost, constraints, T, N, 0, batch, device, false, out);
}

extern "C" void idocp_parnmpc_dist_on_destroy(idocp_ocp_t* h);      // parnmpc_dist.hip: drops the handle's communicator attachment, if any
void idocp_ocp_destroy(idocp_ocp_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  idocp_parnmpc_dist_on_destroy(h);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
  if (h->graph) (void)hipGraphDestroy(h->graph);
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->side) (void)hipStreamSynchronize(h->side);
  dropSideO(h);
  if (h->d_fill) (void)hipFree(h->d_fill);
  if (h->h_fill) (void)hipHostFree(h->h_fill);
  if (h->fill_done) (void)hipEventDestroy(h->fill_done);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// ContactSequence of the handle (ocp_chain.hpp): the outcome of one of its operations goes to idocp_last_error, and the chain is redone
static int sequenceChanged(idocp_ocp_t* h, int rc, const std::string& err) {
  if (rc) set_last_error(err); else h->seq_dirty = true;
  return rc;
}
int idocp_ocp_set_contact_status_uniformly(idocp_ocp_t* h, const int* active, const double* contact_points) {
  if (!h || !active || !contact_points) return IDOCP_E_ARG;
  h->seq.setUniformly(HostStatus::make(active, contact_points));
  return sequenceChanged(h, IDOCP_OK, "");
}
int idocp_ocp_push_back_contact_status(idocp_ocp_t* h, const int* active, const double* contact_points, double switching_time) {
  if (!h || !active || !contact_points) return IDOCP_E_ARG;
  std::string err;
  return sequenceChanged(h, h->seq.pushBack(HostStatus::make(active, contact_points), switching_time, h->N, h->E, err), err);
}
int idocp_ocp_set_contact_points(idocp_ocp_t* h, int contact_phase, const double* contact_points) {
  if (!h || !contact_points) return IDOCP_E_ARG;
  std::string err;
  return sequenceChanged(h, h->seq.setContactPoints(contact_phase, contact_points, err), err);
}
int idocp_ocp_pop_back_contact_status(idocp_ocp_t* h) { return h ? sequenceChanged(h, h->seq.popBack(), "") : IDOCP_E_ARG; }
int idocp_ocp_pop_front_contact_status(idocp_ocp_t* h) { return h ? sequenceChanged(h, h->seq.popFront(), "") : IDOCP_E_ARG; }

int idocp_ocp_get_chain(idocp_ocp_t* h, double t, int capacity, int* kind, int* index, int* slot, double* dt, int* dimf, int* sw_dimi) {
  if (!h) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = discretize(h, t, true))) return rc;
  const int M = h->M();
  if (capacity < M) { set_last_error("idocp_ocp_get_chain: capacity too small"); return IDOCP_E_ARG; }
  for (int p = 0; p < M; ++p) {
    const OcpNode& nd = h->plan.nodes[p];
    if (kind) kind[p] = nd.kind;
    if (index) index[p] = h->plan.chain_index[p];
    if (slot) slot[p] = nd.slot;
    if (dt) dt[p] = nd.dtq;
    if (dimf) dimf[p] = nd.kind == 4 ? 0 : nd.dimf;
    if (sw_dimi) sw_dimi[p] = nd.sw_dimi;
  }
  return M;
}

int idocp_ocp_get_chain_times(idocp_ocp_t* h, double t, int capacity, double* times) {
  if (!h || !times) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  // (the chain's shape and times do not depend on the reference poses: a TimeVarying task cost without poses yet must not stop the
  //  discretisation that tells the caller where to evaluate them)
  if ((rc = discretize(h, t, true))) return rc;
  const int M = h->M();
  if (capacity < M) { set_last_error("idocp_ocp_get_chain_times: capacity too small"); return IDOCP_E_ARG; }
  for (int p = 0; p < M; ++p) times[p] = h->plan.chain_t[p];
  return M;
}
int idocp_ocp_set_task_refs(idocp_ocp_t* h, double t, int M, const double* refs) {
  if (!h || !refs || M <= 0) return IDOCP_E_ARG;
  if (h->cost.task_dim == 0 || !h->cost.task_time_varying) { set_last_error("idocp_ocp_set_task_refs: the solver carries no TimeVarying task-space cost"); return IDOCP_E_ARG; }
  const bool same = h->task_refs_t == t && h->task_refs_host.size() == (size_t)M * 12 &&
                    std::memcmp(h->task_refs_host.data(), refs, sizeof(double) * (size_t)M * 12) == 0;
  if (same && !h->task_refs_stale) return IDOCP_OK;          // the poses the device table already holds
  h->task_refs_host.assign(refs, refs + (size_t)M * 12);
  h->task_refs_t = t;
  if (!h->seq_dirty && h->disc_time == t && M == h->M()) {
    // the chain is the current one (idocp_ocp_get_chain_times has just discretised at t, the facade's order of calls): the table
    // goes straight to the device -- no second discretisation with its host-synchronous uploads in the MPC loop
    int rc = enterO(h); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_taskref, h->task_refs_host.data(), sizeof(double) * (size_t)M * 12, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->task_refs_stale = false;
    return IDOCP_OK;
  }
  h->seq_dirty = true;                       // uploaded with the next discretisation at t
  return IDOCP_OK;
}

static int setSolutionO(idocp_ocp_t* h, const char* name, const double* values, int per_instance) {
  if (!h || !name || !values) return IDOCP_E_ARG;
  const std::string n(name);
  Field f;
  if (!(n == "q" || n == "v" || n == "a" || n == "f" || n == "u") || !solFieldO(n, f)) {
    set_last_error("invalid arugment: name must be q, v, a, f, or u!");
    return IDOCP_E_ARG;
  }
  int rc = enterO(h); if (rc) return rc;
  const int dim = (n == "f") ? 3 : f.dim, repeat = (n == "f") ? DQ::NC : 1;
  const size_t cnt = (size_t)(per_instance ? h->batch : 1) * dim;
  HIP_TRY(hipMemcpyAsync(h->d_tmp, values, cnt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  // every stage incl. the event stages (ocp_solver.cpp:95-165; "a" sets dv on impulse stages)
  ocpFillField(h->B.sol, LQ::SOL, f.offset, dim, h->NS, h->batch, h->d_tmp, per_instance, repeat, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}
int idocp_ocp_set_solution(idocp_ocp_t* h, const char* name, const double* value) { return setSolutionO(h, name, value, 0); }

// Warm start of an MPC loop: a field of every grid stage (slots 0 .. nstages - 1), the same for all instances.
static int fillStagesO(idocp_ocp_t* h, double* rec, int stride, int offset, int dim, int nstages, const double* values, bool chain = false) {
  const size_t bytes = (size_t)nstages * dim * sizeof(double);
  if (h->fill_done) HIP_TRY(hipEventSynchronize(h->fill_done));      // the previous setter's copy has left the host twin (normally long ago)
  else HIP_TRY(hipEventCreateWithFlags(&h->fill_done, hipEventDisableTiming));
  if (bytes > h->fill_cap) {
    if (h->d_fill) { HIP_TRY(hipStreamSynchronize(h->stream)); (void)hipFree(h->d_fill); h->d_fill = nullptr; }
    if (h->h_fill) { (void)hipHostFree(h->h_fill); h->h_fill = nullptr; }
    h->fill_cap = 0;
    const size_t cap = bytes + bytes / 2;
    HIP_TRY(hipMalloc((void**)&h->d_fill, cap));
    HIP_TRY(hipHostMalloc((void**)&h->h_fill, cap, hipHostMallocDefault));
    h->fill_cap = cap;
  }
  std::memcpy(h->h_fill, values, bytes);                              // the caller's buffer is free when the call returns
  HIP_TRY(hipMemcpyAsync(h->d_fill, h->h_fill, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipEventRecord(h->fill_done, h->stream));
  ocpFillStages(rec, stride, offset, dim, h->NS, nstages, h->batch, h->d_fill, h->stream, chain ? h->d_nodes : nullptr);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}
int idocp_ocp_set_solution_stages(idocp_ocp_t* h, const char* name, int nstages, const double* values) {
  if (!h || !name || !values) return IDOCP_E_ARG;
  Field f;
  if (!solFieldO(name, f)) { set_last_error(std::string("unknown field name: ") + name); return IDOCP_E_ARG; }
  const int nmax = h->parnmpc ? h->N : h->N + f.extra;        // grid stages that carry the field (the terminal stage: lmd gmm q v)
  if (nstages <= 0 || nstages > nmax) { set_last_error("idocp_ocp_set_solution_stages: nstages out of range"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  return fillStagesO(h, h->B.sol, LQ::SOL, f.offset, f.dim, nstages, values);
}
int idocp_parnmpc_set_aux_mat(idocp_ocp_t* h, int nstages, const double* values) {
  if (!h || !values || !h->parnmpc) { set_last_error("idocp_parnmpc_set_aux_mat: not a ParNMPC handle"); return IDOCP_E_ARG; }
  if (nstages <= 0 || nstages > h->N) { set_last_error("idocp_parnmpc_set_aux_mat: nstages out of range"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  return fillStagesO(h, h->B.aux, LQ::AUX, 0, DQ::NX * DQ::NX, nstages, values);
}
// warm start along the CHAIN of the current discretisation (event stages included): values[M][dim] in the order of idocp_ocp_get_chain
static int chainLength(idocp_ocp_t* h, int M) {
  if (h->plan.nodes.empty()) { set_last_error("no chain yet: discretise first (initConstraints / initBackwardCorrection / updateSolution)"); return IDOCP_E_ARG; }
  if (M <= 0 || M > h->M()) { set_last_error("chain setter: M out of range"); return IDOCP_E_ARG; }
  return IDOCP_OK;
}
int idocp_ocp_set_solution_chain(idocp_ocp_t* h, const char* name, int M, const double* values) {
  if (!h || !name || !values) return IDOCP_E_ARG;
  Field f;
  if (!solFieldO(name, f)) { set_last_error(std::string("unknown field name: ") + name); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  if ((rc = chainLength(h, M))) return rc;
  return fillStagesO(h, h->B.sol, LQ::SOL, f.offset, f.dim, M, values, true);
}
int idocp_parnmpc_set_aux_mat_chain(idocp_ocp_t* h, int M, const double* values) {
  if (!h || !values || !h->parnmpc) { set_last_error("idocp_parnmpc_set_aux_mat_chain: not a ParNMPC handle"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  if ((rc = chainLength(h, M))) return rc;
  return fillStagesO(h, h->B.aux, LQ::AUX, 0, DQ::NX * DQ::NX, M, values, true);
}
int idocp_ocp_set_solution_batch(idocp_ocp_t* h, const char* name, const double* values) { return setSolutionO(h, name, values, 1); }

int idocp_ocp_init_constraints(idocp_ocp_t* h, double t) {
  if (!h) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = discretize(h, t))) return rc;                 // ocp_solver.cpp:60-64
  OcpLaunch<DQ>::initConstraints(h->B, h->batch, h->NS, h->stream);
  OcpLaunch<DQ>::extInit(h->B, h->batch, h->NS, h->stream);      // ContactDistance rows
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

// K5b: one launch on an event-free chain with all feet in contact, else one launch per stage class
static void launchCondenseO(idocp_ocp_t* h, int M, const double* d_q, int part = 0, hipStream_t st_imp = nullptr) {
  if (h->plan.uniform_dimf == DQ::NF || h->plan.cond_n[0] + h->plan.cond_n[1] + h->plan.cond_n[3] + h->plan.cond_n[4] == 0) OcpLaunch<DQ>::condense(h->B, h->batch, M, h->plan.uniform_dimf, d_q, h->stream, part);
  else OcpLaunch<DQ>::condenseMixed(h->B, h->batch, M, h->plan.cond_n, d_q, h->stream, part, st_imp);
}

// the rules and the measurements behind them: ocp_forms.hpp
static bool fusedForward(const idocp_ocp_t* h) { return useFusedForward(h->forms, h->batch, h->M()); }
static bool wideSweep(const idocp_ocp_t* h) { return useWideSweep(h->forms, h->batch); }
int idocp_ocp_set_riccati_sweep(idocp_ocp_t* h, int mode) {
  if (!h || h->parnmpc || mode < -1 || mode > 1) return IDOCP_E_ARG;
  h->forms.riccati_wide = mode;
  ++h->disc_epoch;                      // a captured hipGraph holds the other kernel
  return IDOCP_OK;
}
int idocp_ocp_riccati_sweep(idocp_ocp_t* h) { return (h && !h->parnmpc && wideSweep(h)) ? 1 : 0; }
// per handle: mode -1 = by batch size (the default), 0 = S4 + K6 + reduction, 1 = the fused forward sweep
int idocp_ocp_set_fused_forward(idocp_ocp_t* h, int mode) {
  if (!h || h->parnmpc || mode < -1 || mode > 1) return IDOCP_E_ARG;
  h->forms.fused_forward = mode;
  ++h->disc_epoch;                      // a captured hipGraph holds the other kernels
  return IDOCP_OK;
}
// 1 when the forward sweep and the primal expansion of this OCPSolver handle run as one kernel, 0 when they are S4, K6 and the reduction
int idocp_ocp_fused_forward(idocp_ocp_t* h) { return (h && !h->parnmpc && fusedForward(h)) ? 1 : 0; }
// per handle: mode -1 = by batch size (the default), 0 = everything on the handle's stream, 1 = K5s and K7b on a stream of their own
int idocp_ocp_set_side_stream(idocp_ocp_t* h, int mode) {
  if (!h || h->parnmpc || mode < -1 || mode > 1) return IDOCP_E_ARG;
  int rc = setDev(h); if (rc) return rc;
  const int before = h->forms.side_stream;
  h->forms.side_stream = mode;
  if ((rc = applySideStreamO(h))) { h->forms.side_stream = before; return rc; }
  ++h->disc_epoch;                      // a captured hipGraph holds the other fork / join structure
  return IDOCP_OK;
}
// 1 when this OCPSolver handle runs K5s (and K7b) on a stream of their own, 0 when everything runs on the handle's stream
int idocp_ocp_side_stream(idocp_ocp_t* h) { return (h && !h->parnmpc && h->side) ? 1 : 0; }
static void launchForwardO(idocp_ocp_t* h, int M, const double* d_q, const double* d_v) {
  if (fusedForward(h)) { OcpLaunch<DQ>::forwardExpand(h->B, h->batch, M, d_q, d_v, h->stream); return; }
  OcpLaunch<DQ>::riccatiForward(h->B, h->batch, M, d_q, d_v, h->stream);
  OcpLaunch<DQ>::expandPrimal(h->B, h->batch, M, h->stream);
}

// one SQP iteration on the handle's stream: K5 (+ K5a on impulse stages, K5s), S3, the forward sweep with the primal expansion (S4 + K6), K7
// K5s (and ParNMPC's impulse kernel K5a) in front of the condensation: on the side stream where the handle has one and the chain carries
// switching constraints (fork here, join in joinSideO before the condensation launches), else on the handle's stream
static int launchSwitchO(idocp_ocp_t* h, int M) {
  OcpLaunch<DQ>::rnea(h->B, h->batch, M, h->plan.n_impulse(), h->stream);
  if (!h->plan.has_switch) return IDOCP_OK;
  if (!h->side) { OcpLaunch<DQ>::switching(h->B, h->batch, M, h->stream); return IDOCP_OK; }
  HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
  HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork, 0));
  OcpLaunch<DQ>::switching(h->B, h->batch, M, h->side);
  HIP_TRY(hipEventRecord(h->ev_join, h->side));        // (recorded again by launchNominalO, behind the impulse stages' nominal launch)
  h->side_pending = true;
  return IDOCP_OK;
}
// the nominal sweeps K5n on the handle's stream; with a fork open (launchSwitchO) the small launch over the impulse stages goes beside them too
static int launchNominalO(idocp_ocp_t* h, int M, const double* d_q) {
  launchCondenseO(h, M, d_q, 1, h->side_pending ? h->side : nullptr);
  if (h->side_pending) HIP_TRY(hipEventRecord(h->ev_join, h->side));
  return IDOCP_OK;
}
// K7 and, independent of it, the base poses K7b: beside each other where the handle has a side stream (joined at once: the next iteration
// reads both)
static int launchIntegrateO(idocp_ocp_t* h, int M) {
  if (!h->side) { OcpLaunch<DQ>::expandDualIntegrate(h->B, h->batch, M, h->stream); return IDOCP_OK; }
  HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
  HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork, 0));
  OcpLaunch<DQ>::expandDualIntegrate(h->B, h->batch, M, h->stream, h->side);
  HIP_TRY(hipEventRecord(h->ev_join, h->side));
  HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
  return IDOCP_OK;
}
// the condensation launches proper, behind K5s and the nominal sweeps (two different instantiations of the 57 kB condensation kernel resident
// together on two streams were measured slower, profiles/experiments/r06_side_stream.md: the classes go one behind the other)
static int launchCondenseClassesO(idocp_ocp_t* h, int M, const double* d_q) {
  int rc;
  if ((rc = joinSideO(h))) return rc;
  launchCondenseO(h, M, d_q, 2);
  return IDOCP_OK;
}
static int launchUpdateO(idocp_ocp_t* h, int M, const double* d_q, const double* d_v) {
  HIP_TRY(hipMemsetAsync(h->B.status, 0, sizeof(int) * h->batch, h->stream));
  int rc;
  if ((rc = launchSwitchO(h, M))) return rc;
  if ((rc = launchNominalO(h, M, d_q))) return rc;        // nominal sweeps (+ Lie tasks, external rows): beside K5s
  if ((rc = launchCondenseClassesO(h, M, d_q))) return rc;
  OcpLaunch<DQ>::riccatiBackward(h->B, h->batch, M, h->plan.has_switch, h->stream, wideSweep(h));
  launchForwardO(h, M, d_q, d_v);
  if ((rc = launchIntegrateO(h, M))) return rc;
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int idocp_ocp_launch_kernel(idocp_ocp_t* h, int kernel_id, const double* d_q, const double* d_v) {
  if (!h || kernel_id < 0 || kernel_id > 8 || !d_q || !d_v) return IDOCP_E_ARG;
  int rc = setDev(h); if (rc) return rc;
  // ids 0, 7 and 1 run beside an open fork (1 closes it between its halves); every other id starts behind it
  if (kernel_id != 0 && kernel_id != 7 && kernel_id != 1 && (rc = joinSideO(h))) return rc;
  if ((rc = ensureDiscretized(h))) return rc;
  const int M = h->M();
  switch (kernel_id) {
    case 0: if ((rc = launchSwitchO(h, M))) return rc; break;      // (with a side stream: K5s starts there and id 8 / 1 waits for it)
    case 1: if ((rc = launchNominalO(h, M, d_q))) return rc; if ((rc = launchCondenseClassesO(h, M, d_q))) return rc; break;
    case 7: if ((rc = launchNominalO(h, M, d_q))) return rc; break;      // the two halves of 1: the nominal rigid-body sweeps (+ external rows) ...
    case 8: if ((rc = launchCondenseClassesO(h, M, d_q))) return rc; break;      // ... and the condensation launches proper
    case 2: OcpLaunch<DQ>::riccatiBackward(h->B, h->batch, M, h->plan.has_switch, h->stream, wideSweep(h)); break;
    // 3: the forward sweep.  Since round 5 it expands as it walks (S4 + K6 + the step-size reduction in one kernel, ocp_forward_expand_kernel);
    // ids 4 and 5 are then empty.  idocp_ocp_set_fused_forward(h, 0) restores the three kernels behind ids 3, 4, 5.
    case 3: if (fusedForward(h)) OcpLaunch<DQ>::forwardExpand(h->B, h->batch, M, d_q, d_v, h->stream); else OcpLaunch<DQ>::riccatiForward(h->B, h->batch, M, d_q, d_v, h->stream); break;
    case 4: case 5: if (!fusedForward(h)) OcpLaunch<DQ>::single(kernel_id, h->B, h->batch, M, h->stream); break;
    case 6: if ((rc = launchIntegrateO(h, M))) return rc; break;
    default: OcpLaunch<DQ>::single(kernel_id, h->B, h->batch, M, h->stream); break;
  }
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int idocp_ocp_update_solution_device(idocp_ocp_t* h, double t, const double* d_q, const double* d_v) {
  if (!h || !d_q || !d_v) return IDOCP_E_ARG;
  if (!h->seq.status_set) { set_last_error("idocp_ocp_update_solution: call setContactStatusUniformly first"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  if ((rc = discretize(h, t))) return rc;                 // ocp_.discretize(contact_sequence_, t) (ocp_solver.cpp:72)
  const int M = h->M();
  if ((rc = launchUpdateO(h, M, d_q, d_v))) return rc;
  h->launched_eagerly = true;
  return IDOCP_OK;
}

// The same iteration replayed from a hipGraph: at small batch sizes the nine launches of an iteration are launch-bound (latency
// mode: one OCP instance, 2 ms per iteration), the graph submits them in one call.  Captured on first use and again whenever the
// discretisation (chain length, stage classes, events) or the input buffers change; the host-side discretiser itself stays outside.
int idocp_ocp_update_solution_graph(idocp_ocp_t* h, double t, const double* d_q, const double* d_v) {
  if (!h || !d_q || !d_v) return IDOCP_E_ARG;
  if (!h->seq.status_set) { set_last_error("idocp_ocp_update_solution: call setContactStatusUniformly first"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  if (!h->launched_eagerly) return idocp_ocp_update_solution_device(h, t, d_q, d_v);      // first call: plain launches (one-time kernel attributes)
  if ((rc = discretize(h, t))) return rc;
  if (!h->graph_exec || h->graph_epoch != h->disc_epoch || h->graph_q != d_q || h->graph_v != d_v) {
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    if (h->graph) { (void)hipGraphDestroy(h->graph); h->graph = nullptr; }
    HIP_TRY(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    rc = launchUpdateO(h, h->M(), d_q, d_v);
    const hipError_t e = hipStreamEndCapture(h->stream, &h->graph);
    if (rc) {      // the capture is over either way; what it recorded -- an open fork included -- is dropped with it
      h->side_pending = false;
      if (h->graph) { (void)hipGraphDestroy(h->graph); h->graph = nullptr; }
      (void)hipGetLastError();
      return rc;
    }
    HIP_TRY(e);
    HIP_TRY(hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
    h->graph_epoch = h->disc_epoch; h->graph_q = d_q; h->graph_v = d_v;
  }
  HIP_TRY(hipGraphLaunch(h->graph_exec, h->stream));
  return IDOCP_OK;
}

int idocp_ocp_synchronize(idocp_ocp_t* h) {
  if (!h) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->side) HIP_TRY(hipStreamSynchronize(h->side));      // (a fork left open by idocp_ocp_launch_kernel id 0 alone)
  return IDOCP_OK;
}
void* idocp_ocp_stream(idocp_ocp_t* h) { return h ? (void*)h->stream : nullptr; }

// LineSearch::computeCostAndViolation (src/line_search/line_search.cpp:63-196) of s (+) alpha[b] d for every instance: trial
// iterate + barrier cost (ocp_trial_kernel), then the rigid-body residual kernels and the MERIT variant of the condensation
// kernel on a copy of the buffers whose `sol` is the trial iterate, then the sums over the chain.  out[2 b] = cost, [2 b + 1] = violation.
// The filter line search of ParNMPCSolver runs on one shard (horizons with discrete events included: every stage of the chain is
// evaluated against the trial iterate of its chain predecessor, src/line_search/line_search.cpp:199-301, line_search.hpp:224-264).
static int parnmpcLineSearchSupported(const idocp_ocp_t* h) {
  if ((h->plan.has_prev || !h->plan.has_terminal) && !(h->ls_pre && h->ls_post)) {
    set_last_error("line_search=true on a shard of a ParNMPC horizon needs the sharded driver (idocp_parnmpc_dist_update_solution_ls)");
    return IDOCP_E_UNSUPPORTED;
  }
  return IDOCP_OK;
}
static int lineSearchEvalO(idocp_ocp_t* h, const std::vector<double>& alpha, const double* d_q, std::vector<double>& out) {
  const int M = h->M();
  { const int rca = uploadTemporary(h->B.ls_alpha, alpha.data(), sizeof(double) * h->batch, h->stream); if (rca) return rca; }
  OcpLaunch<DQ>::trialIterate(h->B, h->batch, M, h->stream);
  OcpBuffers Bt = h->B;
  Bt.sol = h->B.sol_try;
  Bt.ext = h->ext_try;                              // (the trial iterate's heights / rows; the expansion kernels keep reading the linearisation's)
  if (h->parnmpc) {
    // ParNMPC: backward-Euler stages against the trial predecessor (the measured state in front of the first element of the chain;
    // on a shard with a left neighbour: that neighbour's trial iterate of its last stage, fetched by the driver's hook);
    // aux stages add the l1 norm of their switching constraint (K5s on the trial iterate), impulse stages have a kernel of their own
    const double *pq = d_q, *pv = h->d_v0;
    if (h->ls_pre) {
      const int rcp = h->ls_pre(h);
      if (rcp) return rcp;
      if (h->plan.has_prev) { pq = h->d_qtry; pv = h->d_vtry; }
    }
    OcpLaunch<DQ>::rnea(Bt, h->batch, M, h->plan.n_impulse(), h->stream);
    if (h->plan.has_switch) OcpLaunch<DQ>::switching(Bt, h->batch, M, h->stream);
    OcpLaunch<DQ>::meritBackwardEuler(Bt, h->batch, M, pq, pv, h->stream);
    OcpLaunch<DQ>::parnmpcImpulseMerit(Bt, h->batch, h->plan.n_impulse(), pq, pv, h->stream);
  } else {
    Bt.nodes = h->B.nodes_ls;
    OcpLaunch<DQ>::rnea(Bt, h->batch, M, h->plan.n_impulse(), h->stream);
    if (h->plan.has_switch) OcpLaunch<DQ>::switching(Bt, h->batch, M, h->stream);
    OcpLaunch<DQ>::merit(Bt, h->batch, M, d_q, h->stream);
  }
  OcpLaunch<DQ>::meritReduce(h->B, h->batch, h->stream);
  HIP_TRY(hipGetLastError());
  if (h->parnmpc && h->ls_post) { const int rcp = h->ls_post(h); if (rcp) return rcp; }      // sum over the shards
  out.resize((size_t)h->batch * 2);
  HIP_TRY(hipMemcpyAsync(out.data(), h->B.merit, sizeof(double) * out.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}
// LineSearch::computeStepSize (include/idocp/line_search/line_search.hpp:62-92) for every instance of the batch; the filter logic runs on the
// host (line_search_filter.hpp).  On return B.step holds the accepted primal step of every instance.
static int runLineSearchO(idocp_ocp_t* h, const double* d_q) {
  std::vector<double> step((size_t)h->batch * 2);
  HIP_TRY(hipMemcpyAsync(step.data(), h->B.step, sizeof(double) * step.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const int rc = idocp_host::filterLineSearch(h->filters, step.data(), 2, [&](const std::vector<double>& alpha, std::vector<double>& cv) { return lineSearchEvalO(h, alpha, d_q, cv); });
  return rc ? rc : uploadTemporary(h->B.step, step.data(), sizeof(double) * step.size(), h->stream);
}
// kernels 0 .. 5 with the uploaded state, all on the handle's stream (launchUpdateO alone forks K5s onto the side stream)
static int launchDirectionO(idocp_ocp_t* h) {
  const int M = h->M();
  HIP_TRY(hipMemsetAsync(h->B.status, 0, sizeof(int) * h->batch, h->stream));
  OcpLaunch<DQ>::rnea(h->B, h->batch, M, h->plan.n_impulse(), h->stream);
  if (h->plan.has_switch) OcpLaunch<DQ>::switching(h->B, h->batch, M, h->stream);
  launchCondenseO(h, M, h->d_q0);
  OcpLaunch<DQ>::riccatiBackward(h->B, h->batch, M, h->plan.has_switch, h->stream, wideSweep(h));
  launchForwardO(h, M, h->d_q0, h->d_v0);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}
// the status words of the iteration; `what` failed, and the message names the first instance it failed in
static int statusOfO(idocp_ocp_t* h, const char* what) {
  std::vector<int> st(h->batch);
  HIP_TRY(hipMemcpyAsync(st.data(), h->B.status, sizeof(int) * h->batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int b = 0; b < h->batch; ++b)
    if (st[b] != 0) { set_last_error(std::string(what) + ", instance " + std::to_string(b)); return st[b]; }
  return IDOCP_OK;
}

// linearise + Riccati + direction + step sizes WITHOUT integrating (kernels 0 .. 5): the state in which
// idocp_ocp_line_search_eval probes trial steps
int idocp_ocp_compute_direction(idocp_ocp_t* h, double t, const double* q, const double* v) {
  if (!h || !q || !v) return IDOCP_E_ARG;
  if (!h->seq.status_set) { set_last_error("idocp_ocp_update_solution: call setContactStatusUniformly first"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  if ((rc = uploadStateO(h, q, v))) return rc;
  if ((rc = discretize(h, t))) return rc;
  if ((rc = launchDirectionO(h))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}
// (total cost, total constraint violation) of s (+) alpha[b] d for every instance (alpha = 0: the iterate itself, current slacks)
int idocp_ocp_line_search_eval(idocp_ocp_t* h, const double* alpha, double* cost, double* violation) {
  if (!h || !alpha || !cost || !violation) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if (h->parnmpc && (rc = parnmpcLineSearchSupported(h))) return rc;
  std::vector<double> a(alpha, alpha + h->batch), cv;
  if ((rc = lineSearchEvalO(h, a, h->d_q0, cv))) return rc;
  for (int b = 0; b < h->batch; ++b) { cost[b] = cv[2 * b]; violation[b] = cv[2 * b + 1]; }
  return IDOCP_OK;
}
int idocp_ocp_clear_line_search_filter(idocp_ocp_t* h) {
  if (!h) return IDOCP_E_ARG;
  for (auto& f : h->filters) f.clear();
  return IDOCP_OK;
}

int idocp_ocp_update_solution(idocp_ocp_t* h, double t, const double* q, const double* v, int line_search) {
  if (!h || !q || !v) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = uploadStateO(h, q, v))) return rc;      // (in front of the status_set check, which the other branch makes behind it too)
  if (line_search) {
    // OCPSolver::updateSolution(t, q, v, true) (ocp_solver.cpp:67-92): direction, filter line search on the primal step, integration
    if (!h->seq.status_set) { set_last_error("idocp_ocp_update_solution: call setContactStatusUniformly first"); return IDOCP_E_ARG; }
    if ((rc = discretize(h, t))) return rc;
    if ((rc = launchDirectionO(h))) return rc;
    if ((rc = runLineSearchO(h, h->d_q0))) return rc;
    OcpLaunch<DQ>::expandDualIntegrate(h->B, h->batch, h->M(), h->stream);      // (K7 and K7b on the handle's stream: no fork on this path)
    HIP_TRY(hipGetLastError());
  } else
  if ((rc = idocp_ocp_update_solution_device(h, t, h->d_q0, h->d_v0))) return rc;
  return statusOfO(h, "factorisation failed (M, J M^-1 J^T, Quu or the switching-constraint Schur complement not positive definite)");
}

int idocp_ocp_compute_kkt_residual(idocp_ocp_t* h, double t, const double* q, const double* v) {
  if (!h || !q || !v) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = discretize(h, t))) return rc;
  const int M = h->M();
  if ((rc = uploadStateO(h, q, nullptr))) return rc;      // (this residual reads no measured velocity: d_v0 keeps what it held)
  OcpLaunch<DQ>::rnea(h->B, h->batch, M, h->plan.n_impulse(), h->stream);
  if (h->plan.has_switch) OcpLaunch<DQ>::switching(h->B, h->batch, M, h->stream);
  OcpLaunch<DQ>::residual(h->B, h->batch, M, h->d_q0, h->stream);
  ocpKktErrorReduce(h->B, h->batch, h->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}
int idocp_ocp_kkt_error(idocp_ocp_t* h, double* kkt_error) {
  if (!h || !kkt_error) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(kkt_error, h->B.err, sizeof(double) * h->batch, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

// grid stages 0..N live in slots 0..N, so the stage-wise getters are plain strided copies
int idocp_ocp_get_solution(idocp_ocp_t* h, const char* name, int instance, double* out) {
  if (!h || !name || !out || instance < 0 || instance >= h->batch) return IDOCP_E_ARG;
  Field f;
  if (!solFieldO(name, f)) { set_last_error(std::string("unknown field name: ") + name); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  return copyField(h, h->B.sol + (size_t)instance * h->NS * LQ::SOL, LQ::SOL, h->parnmpc ? h->N : h->plan.Ngrid + f.extra, f, out);
}
// OCPSolver::getSolution(stage) (ocp_solver.hpp:97): the whole split solution of ONE grid stage in one device-to-host copy --
// what an MPC loop reads every cycle (getSolution(0).u).  out: lmd gmm q v a u beta f mu nu_passive, the order of the sol record
// (split_solution.hxx:10-31); on the terminal stage only lmd gmm q v are meaningful.
int idocp_ocp_get_split_solution(idocp_ocp_t* h, int instance, int stage, double* out) {
  if (!h || !out || instance < 0 || instance >= h->batch || stage < 0 || stage > (h->parnmpc ? h->N - 1 : h->plan.Ngrid)) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  static_assert(LQ::S_LMD == 0 && LQ::S_NUP > LQ::S_MU, "record order = output order");
  const size_t n = LQ::S_NUP + 6;
  HIP_TRY(hipMemcpyAsync(out, h->B.sol + ((size_t)instance * h->NS + stage) * LQ::SOL, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}
// The contact status the last discretisation linearises grid stage `stage` with (SplitSolution::setContactStatus,
// split_solution.hxx:41-57: isContactActive(i), dimf): active[ncontacts] flags; returns dimf = 3 * (number of active contacts) or a
// negative error code.  What sizes SplitSolution::f_stack() / mu_stack() of getSolution(stage) (split_solution.hpp:93-122).
int idocp_ocp_get_stage_contact_status(idocp_ocp_t* h, int stage, int* active) {
  if (!h || !active || stage < 0 || stage > (h->parnmpc ? h->N - 1 : h->plan.Ngrid)) return IDOCP_E_ARG;
  for (const OcpNode& nd : h->plan.nodes) {
    if ((nd.kind == 0 || nd.kind == 4) && nd.slot == stage) {
      for (int c = 0; c < DQ::NC; ++c) active[c] = nd.kind == 4 ? 0 : nd.active[c];
      return nd.kind == 4 ? 0 : nd.dimf;
    }
  }
  set_last_error("idocp_ocp_get_stage_contact_status: stage " + std::to_string(stage) + " is not a grid stage of the current discretisation");
  return IDOCP_E_ARG;
}
// Direction components that exist only for the ACTIVE contacts of a stage (SplitDirection::df / dmu are daf().tail(dimf) /
// dbetamu().tail(dimf), split_direction.hxx:150-229) or only on a stage that carries a switching constraint (dxi, dimi rows): the record
// keeps whatever an earlier discretisation left in the other slots -- a stage whose contact status has changed since -- and the getters
// report zeros there, like an absent entry (the integration never reads them: K7 steps the active contacts only).
static void maskAbsentDirectionRows(const std::string& name, const OcpNode& nd, double* row) {
  if (name == "df" || name == "dmu") {
    for (int c = 0; c < DQ::NC; ++c) if (!nd.active[c]) for (int k = 0; k < 3; ++k) row[3 * c + k] = 0.0;
  } else if (name == "dxi") {
    for (int k = nd.sw_dimi; k < DQ::NF; ++k) row[k] = 0.0;
  }
}
int idocp_ocp_get_direction(idocp_ocp_t* h, const char* name, int instance, double* out) {
  if (!h || !name || !out || instance < 0 || instance >= h->batch) return IDOCP_E_ARG;
  Field f;
  if (!dirFieldO(name, f)) { set_last_error(std::string("unknown field name: ") + name); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  const size_t nrec = h->parnmpc ? h->N : h->plan.Ngrid + f.extra;
  rc = copyField(h, h->B.dir + (size_t)instance * h->NS * LQ::DIR, LQ::DIR, nrec, f, out);
  if (rc) return rc;
  const std::string n(name);
  if (n == "df" || n == "dmu" || n == "dxi")
    for (const OcpNode& nd : h->plan.nodes)
      if ((nd.kind == 0 || nd.kind == 4) && nd.slot >= 0 && (size_t)nd.slot < nrec) maskAbsentDirectionRows(n, nd, out + (size_t)nd.slot * f.dim);
  return IDOCP_OK;
}

// the same fields for every stage of the chain, in chain order: out[M][dim] (rows of stages that do not carry the
// field, e.g. "u" on an impulse stage, hold whatever the slot holds)
static int getChainField(idocp_ocp_t* h, const double* base, size_t stride, const Field& f, int instance, double* out) {
  int rc = enterO(h); if (rc) return rc;
  const int M = h->M();
  std::vector<double> all((size_t)h->NS * stride);
  HIP_TRY(hipMemcpyAsync(all.data(), base + (size_t)instance * h->NS * stride, all.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int p = 0; p < M; ++p) std::memcpy(out + (size_t)p * f.dim, &all[(size_t)h->plan.nodes[p].slot * stride + f.offset], sizeof(double) * f.dim);
  return IDOCP_OK;
}
// the correction state along the chain: out[M][nx * nx] (column-major per stage), the counterpart of idocp_parnmpc_set_aux_mat_chain --
// together with idocp_ocp_get_solution_chain it is what carries a converged ParNMPC solver over into another handle (another batch
// size, another shard of the horizon)
int idocp_parnmpc_get_aux_mat_chain(idocp_ocp_t* h, int instance, double* out) {
  if (!h || !out || !h->parnmpc || instance < 0 || instance >= h->batch) { set_last_error("idocp_parnmpc_get_aux_mat_chain: not a ParNMPC handle"); return IDOCP_E_ARG; }
  Field f{0, DQ::NX * DQ::NX, 0};
  return getChainField(h, h->B.aux, LQ::AUX, f, instance, out);
}
// the coarse / corrected iterate s_new of the backward correction along the chain (SplitBackwardCorrection's s_new: lmd gmm u q v; "xi": the switching
// multiplier of an aux stage).  On an impulse stage "u" holds the impulse forces f and "xi" the multipliers mu of the velocity constraint, both packed
// (active contacts first).  out[M][dim], dim = nv (lmd gmm v), nq (q), nu (u), 3 nc (xi).
int idocp_parnmpc_get_new_solution_chain(idocp_ocp_t* h, const char* name, int instance, double* out) {
  if (!h || !name || !out || !h->parnmpc || instance < 0 || instance >= h->batch) { set_last_error("idocp_parnmpc_get_new_solution_chain: not a ParNMPC handle, or a null argument"); return IDOCP_E_ARG; }
  const std::string n(name);
  Field f;
  if (n == "lmd") f = {LQ::N_LMD, DQ::NV, 0};
  else if (n == "gmm") f = {LQ::N_GMM, DQ::NV, 0};
  else if (n == "u") f = {LQ::N_U, DQ::NU, 0};
  else if (n == "q") f = {LQ::N_Q, DQ::NQ, 0};
  else if (n == "v") f = {LQ::N_V, DQ::NV, 0};
  else if (n == "xi") f = {LQ::N_XI, DQ::NF, 0};
  else { set_last_error(std::string("unknown field name: ") + name); return IDOCP_E_ARG; }
  return getChainField(h, h->B.snew, LQ::SNEW, f, instance, out);
}
int idocp_ocp_get_solution_chain(idocp_ocp_t* h, const char* name, int instance, double* out) {
  if (!h || !name || !out || instance < 0 || instance >= h->batch) return IDOCP_E_ARG;
  Field f;
  if (!solFieldO(name, f)) { set_last_error(std::string("unknown field name: ") + name); return IDOCP_E_ARG; }
  return getChainField(h, h->B.sol, LQ::SOL, f, instance, out);
}
int idocp_ocp_get_direction_chain(idocp_ocp_t* h, const char* name, int instance, double* out) {
  if (!h || !name || !out || instance < 0 || instance >= h->batch) return IDOCP_E_ARG;
  Field f;
  if (!dirFieldO(name, f)) { set_last_error(std::string("unknown field name: ") + name); return IDOCP_E_ARG; }
  int rc = getChainField(h, h->B.dir, LQ::DIR, f, instance, out);
  if (rc) return rc;
  const std::string n(name);
  if (n == "df" || n == "dmu" || n == "dxi")
    for (int p = 0; p < h->M(); ++p) maskAbsentDirectionRows(n, h->plan.nodes[p], out + (size_t)p * f.dim);
  return IDOCP_OK;
}

int idocp_ocp_get_step_sizes(idocp_ocp_t* h, double* primal, double* dual) {
  if (!h || !primal || !dual) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  std::vector<double> st((size_t)h->batch * 2);
  HIP_TRY(hipMemcpyAsync(st.data(), h->B.step, sizeof(double) * st.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int b = 0; b < h->batch; ++b) { primal[b] = st[2 * b]; dual[b] = st[2 * b + 1]; }
  return IDOCP_OK;
}

// chain != 0: one entry per stage of the chain (P, s: M entries; K, k: M - 1); chain == 0: grid stages 0..N
static int getRiccati(idocp_ocp_t* h, int instance, int chain, double* P, double* s, double* K, double* k) {
  if (!h || instance < 0 || instance >= h->batch) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  const int nv = DQ::NV, nx = DQ::NX, nu = DQ::NU;
  const int n = chain ? h->M() : h->plan.Ngrid + 1;
  std::vector<double> ric((size_t)h->NS * LQ::RIC), gain((size_t)h->NS * LQ::GAIN);
  HIP_TRY(hipMemcpyAsync(ric.data(), h->B.ric + (size_t)instance * h->NS * LQ::RIC, ric.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(gain.data(), h->B.gain + (size_t)instance * h->NS * LQ::GAIN, gain.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; ++i) {
    const int slot = chain ? h->plan.nodes[i].slot : i;
    const double* r = &ric[(size_t)slot * LQ::RIC];
    if (P) {
      double* Pm = P + (size_t)i * nx * nx;
      for (int c = 0; c < nv; ++c) for (int rr = 0; rr < nv; ++rr) {
        Pm[c * nx + rr] = r[LQ::R_PQQ + LQ::psym(rr, c)];          // (packed upper triangle)
        Pm[(nv + c) * nx + rr] = r[LQ::R_PQV + c * nv + rr];
        Pm[c * nx + nv + rr] = r[LQ::R_PQV + rr * nv + c];
        Pm[(nv + c) * nx + nv + rr] = r[LQ::R_PVV + LQ::psym(rr, c)];
      }
    }
    if (s) { std::memcpy(s + (size_t)i * nx, r + LQ::R_SQ, sizeof(double) * nv); std::memcpy(s + (size_t)i * nx + nv, r + LQ::R_SV, sizeof(double) * nv); }
    if (i < n - 1) {
      const double* g = &gain[(size_t)slot * LQ::GAIN];
      if (K) std::memcpy(K + (size_t)i * nu * nx, g + LQ::G_K, sizeof(double) * nu * nx);
      if (k) std::memcpy(k + (size_t)i * nu, g + LQ::G_k, sizeof(double) * nu);
    }
  }
  return IDOCP_OK;
}
int idocp_ocp_get_riccati(idocp_ocp_t* h, int instance, double* P, double* s, double* K, double* k) { return getRiccati(h, instance, 0, P, s, K, k); }
int idocp_ocp_get_riccati_chain(idocp_ocp_t* h, int instance, double* P, double* s, double* K, double* k) { return getRiccati(h, instance, 1, P, s, K, k); }

int idocp_ocp_get_state_feedback_gain(idocp_ocp_t* h, int instance, int stage, double* Kq, double* Kv) {
  if (!h || instance < 0 || instance >= h->batch || stage < 0 || stage >= h->plan.Ngrid || !Kq || !Kv) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  std::vector<double> g(LQ::GAIN);
  HIP_TRY(hipMemcpyAsync(g.data(), h->B.gain + ((size_t)instance * h->NS + stage) * LQ::GAIN, g.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  std::memcpy(Kq, &g[LQ::G_K], sizeof(double) * DQ::NU * DQ::NV);                      // K.leftCols(nv)
  std::memcpy(Kv, &g[LQ::G_K + DQ::NU * DQ::NV], sizeof(double) * DQ::NU * DQ::NV);   // K.rightCols(nv)
  return IDOCP_OK;
}

// OCPSolver::isCurrentSolutionFeasible (ocp_solver.cpp:216-248) / ParNMPCSolver (parnmpc_solver.cpp:231-273): the primal
// iterate against the inequality constraints, stage by stage along the chain.  A host-side check on the downloaded solution
// records (a few kB per instance): joint limits with the time-step gating of constraints_data.hpp:18-42, the linearised
// (impulse) friction cone on the active contacts.  feasible[b] = 1 / 0; where[b] = chain position of the first offending
// stage in the reference's order (stages, impulses, aux, lifts), -1 if none.
int idocp_ocp_is_current_solution_feasible(idocp_ocp_t* h, int* feasible, int* where) {
  if (!h || !feasible) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = ensureDiscretized(h))) return rc;
  const int M = h->M(), nu = DQ::NU;
  const OcpProblem& P = h->prob;
  std::vector<double> sol((size_t)h->batch * h->NS * LQ::SOL);
  HIP_TRY(hipMemcpyAsync(sol.data(), h->B.sol, sol.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  auto stageOk = [&](const OcpNode& nd, const double* s) {
    if (nd.kind == 1) {                                               // linearized_impulse_friction_cone.cpp:82-94
      if (!P.use_impulse_friction_cone) return true;
    } else {
      if (P.use_q_limits && nd.level >= 2)                            // joint_position_{lower,upper}_limit.cpp:38-47
        for (int r = 0; r < nu; ++r) { const double q = s[LQ::S_Q + DQ::NQ - nu + r]; if (q < P.q_min[r] || q > P.q_max[r]) return false; }
      if (P.use_v_limits && nd.level >= 1)
        for (int r = 0; r < nu; ++r) { const double v = s[LQ::S_V + DQ::NV - nu + r]; if (v < -P.v_max[r] || v > P.v_max[r]) return false; }
      if (P.use_u_limits && nd.has_u)
        for (int r = 0; r < nu; ++r) { const double u = s[LQ::S_U + r]; if (u < -P.u_max[r] || u > P.u_max[r]) return false; }
      if (nd.kind != 4)                                               // joint_acceleration_{lower,upper}_limit.cpp:38-47
        for (int r = 0; r < nu; ++r) {
          const double a = s[LQ::S_A + DQ::NV - nu + r];
          if ((P.use_a_lower && a < P.a_min[r]) || (P.use_a_upper && a > P.a_max[r])) return false;
        }
      if (P.use_contact_distance && nd.level >= 2 && nd.kind != 4) {   // contact_distance.cpp:44-55: the frames of the contacts that are not active
        double pts[DQ::NC * 3];
        idocp_model_contact_positions(&h->model, s + LQ::S_Q, pts);
        for (int c = 0; c < DQ::NC; ++c) if (!nd.active[c] && pts[3 * c + 2] <= 0) return false;
      }
      if (!P.use_friction_cone) return true;
    }
    const int ck = nd.kind == 1 ? P.impulse_cone_kind : P.cone_kind;
    for (int c = 0; c < DQ::NC; ++c) {                                // linearized_friction_cone.cpp:87-99, friction_cone.cpp:70-84
      if (!nd.active[c]) continue;
      double J[3];
      for (int r = 0; r < coneRows(ck); ++r) if (coneRow(ck, P.mu, r, s + LQ::S_F + 3 * c, J) > 0) return false;
    }
    return true;
  };
  for (int b = 0; b < h->batch; ++b) {
    int bad = -1;
    for (int kind = 0; kind < 4 && bad < 0; ++kind)
      for (int p = 0; p < M && bad < 0; ++p) {
        const OcpNode& nd = h->plan.nodes[p];
        if (nd.kind != kind) continue;
        if (!stageOk(nd, &sol[((size_t)b * h->NS + nd.slot) * LQ::SOL])) bad = p;
      }
    feasible[b] = bad < 0 ? 1 : 0;
    if (where) where[b] = bad;
  }
  return IDOCP_OK;
}

int idocp_ocp_dimc(const idocp_ocp_t* h) {
  if (!h) return 0;
  const idocp_constraints_t& c = h->cons;
  return 2 * DQ::NU * ((c.joint_position_limits ? 1 : 0) + (c.joint_velocity_limits ? 1 : 0) + (c.joint_torque_limits ? 1 : 0)) +
         (c.linearized_friction_cone ? 5 * DQ::NC : 0) + (c.friction_cone ? 2 * DQ::NC : 0) +
         DQ::NU * ((c.joint_acceleration_lower_limit ? 1 : 0) + (c.joint_acceleration_upper_limit ? 1 : 0)) + (c.contact_distance ? DQ::NC : 0);
}

int idocp_ocp_get_constraint_data(idocp_ocp_t* h, int instance, double* slack, double* dual) {
  if (!h || instance < 0 || instance >= h->batch) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  // (a ParNMPC plan counts its last stage apart: all N stages carry rows, stage i at constraint level i + 1)
  const int N = h->parnmpc ? h->N : h->plan.Ngrid, dimc = idocp_ocp_dimc(h), level0 = h->parnmpc ? 1 + h->stage_offset : 0;
  std::vector<double> sl((size_t)N * LQ::CON), du((size_t)N * LQ::CON);
  HIP_TRY(hipMemcpyAsync(sl.data(), h->B.slack + (size_t)instance * h->NS * LQ::CON, sl.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(du.data(), h->B.dual + (size_t)instance * h->NS * LQ::CON, du.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const idocp_constraints_t& c = h->cons;
  // components in the order 0 .. 5 joint position / velocity / torque (lower, upper), 6 cone, 8 / 9 joint acceleration lower / upper, 10 contact distance
  const int use[11] = {c.joint_position_limits, c.joint_position_limits, c.joint_velocity_limits, c.joint_velocity_limits, c.joint_torque_limits,
                       c.joint_torque_limits, c.linearized_friction_cone || c.friction_cone, 0, c.joint_acceleration_lower_limit, c.joint_acceleration_upper_limit,
                       c.contact_distance};
  const int cr = coneRows(h->prob.cone_kind);        // rows per contact of the cone in use (the records keep five slots per contact)
  for (int i = 0; i < N; ++i) {
    int off = 0;
    for (int comp = 0; comp < 11; ++comp) {
      if (!use[comp]) continue;
      const int n = comp == 10 ? DQ::NC : (comp != 6 ? DQ::NU : cr * DQ::NC);
      const int level = i + level0;
      const bool valid = (comp < 2 || comp == 10) ? level >= 2 : (comp < 4 ? level >= 1 : true);
      for (int r = 0; r < n; ++r) {
        const int src = comp == 10 ? LQ::C_CD + r : (comp != 6 ? ipmCompRow<LQ>(comp) + r : LQ::C_FRIC + 5 * (r / cr) + r % cr);
        if (slack) slack[(size_t)i * dimc + off + r] = valid ? sl[(size_t)i * LQ::CON + src] : 0.0;
        if (dual) dual[(size_t)i * dimc + off + r] = valid ? du[(size_t)i * LQ::CON + src] : 0.0;
      }
      off += n;
    }
  }
  return IDOCP_OK;
}

int idocp_ocp_get_profile(idocp_ocp_t* h, long long* out, int n) {
  if (!h || !out || n <= 0 || n > 64) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  HIP_TRY(hipMemcpy(out, h->B.prof, sizeof(long long) * n, hipMemcpyDeviceToHost));
  return IDOCP_OK;
}

// The inverse of idocp_ocp_get_lqr_stage, for every instance: the condensed LQR stage the backward sweep reads (its kkt record), so that a test can run
// the sweep alone on a problem whose answer it knows (tests/test_golden_riccati.py: the dense KKT solution of a random LQR problem in the reference's
// block structure).  Column-major blocks; terminal != 0: Qxx and lx only.
// The head of the three test-only entries addressed by chain position: the refusals they share, each under the caller's name.
static int chainPositionO(idocp_ocp_t* h, const char* who, int instance, int lowest_instance, int position, bool needs_switch, const OcpNode** nd) {
  const std::string name(who);
  if (!h) { set_last_error(name + ": null handle"); return IDOCP_E_ARG; }
  if (h->parnmpc) { set_last_error(name + ": a ParNMPC handle has no Riccati sweep to inject into"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  if ((rc = ensureDiscretized(h))) return rc;
  if (instance < lowest_instance || instance >= h->batch) { set_last_error(name + ": instance out of range"); return IDOCP_E_ARG; }
  if (position < 0 || position >= h->M()) { set_last_error(name + ": position out of range"); return IDOCP_E_ARG; }
  *nd = &h->plan.nodes[position];
  if (needs_switch && (*nd)->sw_dimi == 0) { set_last_error(name + ": no switching constraint at position " + std::to_string(position)); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

// The inverse of idocp_ocp_get_lqr_stage by chain position: the condensed LQR stage the sweeps read (the kkt record of the node's slot), of one
// instance or of all (instance == -1), so that a test can run a sweep alone on a problem whose answer it knows (tests/riccati_chain_cases.py: the
// dense KKT solution of a random LQ problem along a chain with events).  Column-major blocks.  Terminal node: Qxx and lx only.  Impulse node: no
// control -- the record gets what K5b leaves there (Quu = I, Qxu = 0, Fvu = 0, lu = 0, Fqv6 = 0) and the caller's Qxu, Quu, Fqv6, Fvu, lu are not read.
int idocp_ocp_set_lqr_stage_chain(idocp_ocp_t* h, int instance, int position, const double* Qxx, const double* Qxu, const double* Quu,
                                  const double* Fqq6, const double* Fqv6, const double* Fvq, const double* Fvv, const double* Fvu, const double* lx,
                                  const double* lu, const double* Fx) {
  const char* who = "idocp_ocp_set_lqr_stage_chain";
  const OcpNode* nd = nullptr;
  int rc = chainPositionO(h, who, instance, -1, position, false, &nd); if (rc) return rc;
  const bool terminal = nd->kind == 4, impulse = nd->kind == 1;
  if (!Qxx || !lx || (!terminal && (!Fqq6 || !Fvq || !Fvv || !Fx)) || (!terminal && !impulse && (!Qxu || !Quu || !Fqv6 || !Fvu || !lu))) {
    set_last_error(std::string(who) + ": a block this node kind needs is null");
    return IDOCP_E_ARG;
  }
  const int nv = DQ::NV, nx = DQ::NX, nu = DQ::NU;
  std::vector<double> k(LQ::KKT, 0.0);
  for (int c = 0; c < nx; ++c) for (int r = 0; r <= c; ++r) k[LQ::K_QXX + LQ::xsym(r, c)] = Qxx[c * nx + r];
  std::memcpy(&k[LQ::K_LX], lx, sizeof(double) * nx);
  if (!terminal) {
    std::memcpy(&k[LQ::K_FQQ], Fqq6, sizeof(double) * 36);
    std::memcpy(&k[LQ::K_FVQ], Fvq, sizeof(double) * nv * nv);
    std::memcpy(&k[LQ::K_FVV], Fvv, sizeof(double) * nv * nv);
    std::memcpy(&k[LQ::K_FX], Fx, sizeof(double) * nx);
    if (impulse) {
      for (int j = 0; j < nu; ++j) k[LQ::K_QUU + j + nu * j] = 1.0;
    } else {
      std::memcpy(&k[LQ::K_QXU], Qxu, sizeof(double) * nx * nu);
      std::memcpy(&k[LQ::K_QUU], Quu, sizeof(double) * nu * nu);
      std::memcpy(&k[LQ::K_FQV], Fqv6, sizeof(double) * 36);
      std::memcpy(&k[LQ::K_FVU], Fvu, sizeof(double) * nv * nu);
      std::memcpy(&k[LQ::K_LU], lu, sizeof(double) * nu);
    }
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (long b = instance < 0 ? 0 : instance; b < (instance < 0 ? h->batch : instance + 1); ++b)
    HIP_TRY(hipMemcpy(h->B.kkt + ((size_t)b * h->NS + nd->slot) * LQ::KKT, k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice));
  return IDOCP_OK;
}

// The grid-stage form of the above, for every instance (tests/test_golden_riccati.py): stage = grid index, terminal != 0 for stage N.
int idocp_ocp_set_lqr_stage(idocp_ocp_t* h, int stage, int terminal, const double* Qxx, const double* Qxu, const double* Quu, const double* Fqq6,
                            const double* Fqv6, const double* Fvq, const double* Fvv, const double* Fvu, const double* lx, const double* lu,
                            const double* Fx) {
  if (!h || !Qxx || !lx || stage < 0) return IDOCP_E_ARG;
  if (!terminal && (!Qxu || !Quu || !Fqq6 || !Fqv6 || !Fvq || !Fvv || !Fvu || !lu || !Fx)) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = ensureDiscretized(h))) return rc;
  for (int p = 0; p < h->M(); ++p) {
    const OcpNode& nd = h->plan.nodes[p];
    if (nd.slot != stage || (nd.kind != 0 && nd.kind != 4)) continue;
    if ((nd.kind == 4) != (terminal != 0)) return IDOCP_E_ARG;
    return idocp_ocp_set_lqr_stage_chain(h, -1, p, Qxx, Qxu, Quu, Fqq6, Fqv6, Fvq, Fvv, Fvu, lx, lu, Fx);
  }
  return IDOCP_E_ARG;
}

// The swc record of one chain position as the sweeps read it: P (dimi), Phix (dimi x NX), Phiu (dimi x NU), column-major with leading dimension dimi,
// into the record's leading dimension NF; of one instance or of all (instance == -1).  Rows dimi .. NF - 1 of the record are left as they are, which
// is how ocp_switch_kernel.hip and the condensation leave them: both write rows 0 .. dimi - 1 only, so those rows hold the zeros of the allocation or
// what an earlier, taller constraint wrote there, and the sweep must not read them.  Phia (consumed by the condensation) is not touched.
int idocp_ocp_set_switching_constraint(idocp_ocp_t* h, int instance, int position, int dimi, const double* P, const double* Phix, const double* Phiu) {
  const char* who = "idocp_ocp_set_switching_constraint";
  const OcpNode* nd = nullptr;
  int rc = chainPositionO(h, who, instance, -1, position, true, &nd); if (rc) return rc;
  if (dimi != nd->sw_dimi) {
    set_last_error(std::string(who) + ": dimi " + std::to_string(dimi) + " is not the " + std::to_string(nd->sw_dimi) + " rows of the node");
    return IDOCP_E_ARG;
  }
  if (!P || !Phix || !Phiu) { set_last_error(std::string(who) + ": null block"); return IDOCP_E_ARG; }
  const int nx = DQ::NX, nu = DQ::NU, nf = DQ::NF;
  std::vector<double> w(LQ::SWC);
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (long b = instance < 0 ? 0 : instance; b < (instance < 0 ? h->batch : instance + 1); ++b) {
    double* rec = h->B.swc + ((size_t)b * h->NS + nd->slot) * LQ::SWC;
    HIP_TRY(hipMemcpy(w.data(), rec, w.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int j = 0; j < dimi; ++j) {
      w[LQ::W_P + j] = P[j];
      for (int c = 0; c < nx; ++c) w[LQ::W_PHIX + j + nf * c] = Phix[j + dimi * c];
      for (int c = 0; c < nu; ++c) w[LQ::W_PHIU + j + nf * c] = Phiu[j + dimi * c];
    }
    HIP_TRY(hipMemcpy(rec, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  return IDOCP_OK;
}

// The multiplier policy dxi = M dx + m the backward sweep wrote into the swc record of a chain position: M (dimi x NX, column-major, leading
// dimension dimi) and m (dimi).  Returns dimi, or a negative error code.
int idocp_ocp_get_switching_policy(idocp_ocp_t* h, int instance, int position, double* M, double* m) {
  const char* who = "idocp_ocp_get_switching_policy";
  const OcpNode* nd = nullptr;
  int rc = chainPositionO(h, who, instance, 0, position, true, &nd); if (rc) return rc;
  const int dimi = nd->sw_dimi, nx = DQ::NX, nf = DQ::NF;
  std::vector<double> w(LQ::SWC);
  HIP_TRY(hipMemcpyAsync(w.data(), h->B.swc + ((size_t)instance * h->NS + nd->slot) * LQ::SWC, w.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int j = 0; j < dimi; ++j) {
    if (M) for (int c = 0; c < nx; ++c) M[j + dimi * c] = w[LQ::W_M + j + nf * c];
    if (m) m[j] = w[LQ::W_m + j];
  }
  return dimi;
}

// ContactDynamicsData of a grid stage as the condensation kernel left it (contact_dynamics_data.hxx:8-29: MJtJinv, MJtJinv_dIDCdqv, MJtJinv_IDC), dense and
// column-major with n = nv + dimf rows (the active contacts packed): what the parity tests hold to the INDEPENDENT rigid-body vectors of tests/golden
// (M, J and the derivatives of [ID; C] follow from these three by one inverse).  Returns dimf, or a negative error code.
static int getContactDynamics(idocp_ocp_t* h, int instance, int stage, int dimf, double* MJtJinv, double* MJtJinv_dIDCdqv, double* MJtJinv_IDC);
int idocp_ocp_get_contact_dynamics(idocp_ocp_t* h, int instance, int stage, double* MJtJinv, double* MJtJinv_dIDCdqv, double* MJtJinv_IDC) {
  if (!h || !MJtJinv || !MJtJinv_dIDCdqv || !MJtJinv_IDC || instance < 0 || instance >= h->batch) return IDOCP_E_ARG;
  int dimf = -1;
  for (const OcpNode& nd : h->plan.nodes) if (nd.kind == 0 && nd.slot == stage) dimf = nd.dimf;
  if (dimf < 0) { set_last_error("idocp_ocp_get_contact_dynamics: stage " + std::to_string(stage) + " is not a grid stage of the current discretisation"); return IDOCP_E_ARG; }
  return getContactDynamics(h, instance, stage, dimf, MJtJinv, MJtJinv_dIDCdqv, MJtJinv_IDC);
}
// the same by chain position: any stage that has dynamics -- grid, aux, lift, and IMPULSE stages (ImpulseDynamicsForwardEulerData,
// impulse_dynamics_forward_euler_data.hxx: MJtJinv of the impulse's contacts, the blocks of [ImD; V] in place of [ID; C])
int idocp_ocp_get_contact_dynamics_chain(idocp_ocp_t* h, int instance, int position, double* MJtJinv, double* MJtJinv_dIDCdqv, double* MJtJinv_IDC) {
  if (!h || !MJtJinv || !MJtJinv_dIDCdqv || !MJtJinv_IDC || instance < 0 || instance >= h->batch || position < 0 || position >= h->M()) return IDOCP_E_ARG;
  const OcpNode& nd = h->plan.nodes[position];
  if (nd.kind == 4) { set_last_error("idocp_ocp_get_contact_dynamics_chain: the terminal stage has no dynamics"); return IDOCP_E_ARG; }
  return getContactDynamics(h, instance, nd.slot, nd.dimf, MJtJinv, MJtJinv_dIDCdqv, MJtJinv_IDC);
}
static int getContactDynamics(idocp_ocp_t* h, int instance, int stage, int dimf, double* MJtJinv, double* MJtJinv_dIDCdqv, double* MJtJinv_IDC) {
  int rc = enterO(h); if (rc) return rc;
  std::vector<double> e(LQ::EXP);
  HIP_TRY(hipMemcpyAsync(e.data(), h->B.exp + ((size_t)instance * h->NS + stage) * LQ::EXP, e.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const int n = DQ::NV + dimf;
  for (int c = 0; c < n; ++c) for (int r = 0; r < n; ++r) MJtJinv[r + n * c] = r >= c ? e[LQ::E_MJ + r * (r + 1) / 2 + c] : e[LQ::E_MJ + c * (c + 1) / 2 + r];      // (packed lower triangle)
  for (int c = 0; c < DQ::NX; ++c) for (int r = 0; r < n; ++r) MJtJinv_dIDCdqv[r + n * c] = e[LQ::E_MJD + r + DQ::NVF * c];
  for (int r = 0; r < n; ++r) MJtJinv_IDC[r] = e[LQ::E_MJIDC + r];
  return dimf;
}

// The ext record of one chain position as ocp_ext_kernel left it (OcpLayout::EXT: the ContactDistance rows and the task-space components of a stage
// BEFORE they are added into the kkt record), unpacked into the caller's arrays; every array may be null.  Reaches the node kinds
// idocp_ocp_get_lqr_stage cannot: impulse, aux, lift, terminal, and ParNMPC's last stage.  No arithmetic, no launch: for tests.
int idocp_ocp_get_ext_terms(idocp_ocp_t* h, int instance, int position, double* z, double* Jc, double* w, double* JJ, double* tw, double* lq,
                            double* cost, double* violation, double* kkt_error) {
  if (!h) return IDOCP_E_ARG;
  if (!h->B.ext) { set_last_error("idocp_ocp_get_ext_terms: the handle has no ext record (no ContactDistance constraint, no task-space cost)"); return IDOCP_E_ARG; }
  if (instance < 0 || instance >= h->batch) { set_last_error("idocp_ocp_get_ext_terms: instance out of range"); return IDOCP_E_ARG; }
  if (position < 0 || position >= h->M()) { set_last_error("idocp_ocp_get_ext_terms: position out of range"); return IDOCP_E_ARG; }
  if (h->parnmpc && position == h->M() - 1) { set_last_error("idocp_ocp_get_ext_terms: the placeholder behind ParNMPC's last stage has no terms"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  std::vector<double> x(LQ::EXT);
  HIP_TRY(hipMemcpyAsync(x.data(), h->B.ext + ((size_t)instance * h->NS + h->plan.nodes[position].slot) * LQ::EXT, x.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (z) std::memcpy(z, &x[LQ::X_Z], sizeof(double) * DQ::NC);
  if (Jc) std::memcpy(Jc, &x[LQ::X_CDJ], sizeof(double) * DQ::NC * DQ::NV);
  if (w) std::memcpy(w, &x[LQ::X_W], sizeof(double) * DQ::NC);
  if (JJ) std::memcpy(JJ, &x[LQ::X_TJ], sizeof(double) * LQ::NT * 6 * DQ::NV);
  if (tw) std::memcpy(tw, &x[LQ::X_TW], sizeof(double) * LQ::NT * 6);
  if (lq) std::memcpy(lq, &x[LQ::X_LQ], sizeof(double) * DQ::NV);
  if (cost) *cost = x[LQ::X_COST];
  if (violation) *violation = x[LQ::X_VIOL];
  if (kkt_error) *kkt_error = x[LQ::X_ERR];
  return IDOCP_OK;
}

int idocp_ocp_get_lqr_stage(idocp_ocp_t* h, int instance, int stage, double* Qxx, double* Qxu, double* Quu, double* A, double* Bm,
                            double* lx, double* lu, double* Fx) {
  if (!h || instance < 0 || instance >= h->batch || stage < 0 || stage >= h->plan.Ngrid) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  const int nv = DQ::NV, nx = DQ::NX, nu = DQ::NU;
  std::vector<double> k(LQ::KKT);
  HIP_TRY(hipMemcpyAsync(k.data(), h->B.kkt + ((size_t)instance * h->NS + stage) * LQ::KKT, k.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int c = 0; c < nx; ++c) for (int r = 0; r < nx; ++r) Qxx[c * nx + r] = k[LQ::K_QXX + LQ::xsym(r, c)];      // (the record holds the upper triangle)
  std::memcpy(Qxu, &k[LQ::K_QXU], sizeof(double) * nx * nu);
  std::memcpy(Quu, &k[LQ::K_QUU], sizeof(double) * nu * nu);
  std::memset(A, 0, sizeof(double) * nx * nx);
  std::memset(Bm, 0, sizeof(double) * nx * nu);
  double dt = h->T / h->N;
  for (const OcpNode& nd : h->plan.nodes) if (nd.slot == stage) dt = nd.dtq;
  for (int c = 0; c < nv; ++c) for (int r = 0; r < nv; ++r) {
    double fqq = (r == c) ? 1.0 : 0.0, fqv = (r == c) ? dt : 0.0;
    if (r < 6 && c < 6) { fqq = k[LQ::K_FQQ + r + 6 * c]; fqv = k[LQ::K_FQV + r + 6 * c]; }
    else if (r < 6 || c < 6) { fqq = 0.0; fqv = 0.0; }
    A[r + nx * c] = fqq; A[r + nx * (nv + c)] = fqv;
    A[(nv + r) + nx * c] = k[LQ::K_FVQ + r + nv * c]; A[(nv + r) + nx * (nv + c)] = k[LQ::K_FVV + r + nv * c];
  }
  for (int j = 0; j < nu; ++j) for (int r = 0; r < nv; ++r) Bm[(nv + r) + nx * j] = k[LQ::K_FVU + r + nv * j];
  std::memcpy(lx, &k[LQ::K_LX], sizeof(double) * nx);
  std::memcpy(lu, &k[LQ::K_LU], sizeof(double) * nu);
  std::memcpy(Fx, &k[LQ::K_FX], sizeof(double) * nx);
  return IDOCP_OK;
}

// ---------------------------------------------------------------------------------------------- ParNMPC ----
// idocp::ParNMPCSolver (src/ocp/parnmpc_solver.cpp) for horizons without discrete events.  The handle is an idocp_ocp with
// backward-Euler stages; solution / direction getters, setters and the KKT error go through the idocp_ocp_* entry points
// with stage index 0 .. N-1 (there is no separate terminal stage: stage N-1 carries the terminal cost).
int idocp_parnmpc_create(const idocp_model_t* model, const idocp_cost_t* cost, const idocp_constraints_t* constraints, double T,
                         int N, int batch, int device, idocp_ocp_t** out) {
  return createOcpImpl(model, cost, constraints, T, N, 0, batch, device, true, out);
}

int idocp_parnmpc_create_hybrid(const idocp_model_t* model, const idocp_cost_t* cost, const idocp_constraints_t* constraints, double T,
                                int N, int max_num_impulse, int batch, int device, idocp_ocp_t** out) {
  return createOcpImpl(model, cost, constraints, T, N, max_num_impulse, batch, device, true, out);
}

// ParNMPCSolver::initBackwardCorrection (parnmpc_solver.cpp:66-70)
int idocp_parnmpc_init_backward_correction(idocp_ocp_t* h, double t) {
  if (!h || !h->parnmpc) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = discretize(h, t))) return rc;
  OcpLaunch<DQ>::parnmpcPhase(4, h->B, h->batch, h->M(), h->plan.has_terminal, h->d_q0, h->d_v0, h->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

// phases of ParNMPCSolver::updateSolution (parnmpc_solver.cpp:73-103), separately launchable (bench, tests):
// 0 K5a tangent RNEA, 1 K9a backward-Euler condensation, 2 K9w KKT inverse + coarse update, 3 S5 backward serial,
// 4 K10a backward parallel, 5 S6 forward serial, 6 K10b forward parallel + direction, 7 K6 expansion + step sizes,
// 8 step-size reduction, 9 K7 dual expansion + integration
int idocp_parnmpc_launch_phase(idocp_ocp_t* h, int phase, const double* d_q, const double* d_v) {
  if (!h || !h->parnmpc || phase < 0 || phase > 9 || !d_q || !d_v) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = ensureDiscretized(h))) return rc;
  const int M = h->M();
  switch (phase) {
    case 0: OcpLaunch<DQ>::rnea(h->B, h->batch, M, h->plan.n_impulse(), h->stream); break;
    case 1:
      if (h->plan.has_switch) OcpLaunch<DQ>::switching(h->B, h->batch, M, h->stream);          // P, Pq of the aux stages
      OcpLaunch<DQ>::condenseBackwardEuler(h->B, h->batch, M, d_q, d_v, false, h->stream);
      OcpLaunch<DQ>::parnmpcImpulseCondense(h->B, h->batch, h->plan.n_impulse(), false, d_q, d_v, h->stream);
      break;
    case 2:
      OcpLaunch<DQ>::parnmpcInverse(h->B, h->batch, M, h->stream);
      OcpLaunch<DQ>::parnmpcEventInverse(h->B, h->batch, h->plan.n_general(), h->stream);
      break;
    case 3: case 4: case 5: case 6: OcpLaunch<DQ>::parnmpcPhase(phase - 3, h->B, h->batch, M, h->plan.has_terminal, d_q, d_v, h->stream); break;
    case 7: OcpLaunch<DQ>::single(4, h->B, h->batch, M, h->stream); break;
    case 8: OcpLaunch<DQ>::single(5, h->B, h->batch, M, h->stream); break;
    default: OcpLaunch<DQ>::single(6, h->B, h->batch, M, h->stream); break;
  }
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int idocp_parnmpc_update_solution_device(idocp_ocp_t* h, double t, const double* d_q, const double* d_v) {
  if (!h || !h->parnmpc || !d_q || !d_v) return IDOCP_E_ARG;
  if (!h->seq.status_set) { set_last_error("idocp_parnmpc_update_solution: call setContactStatusUniformly first"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  if ((rc = discretize(h, t))) return rc;
  HIP_TRY(hipMemsetAsync(h->B.status, 0, sizeof(int) * h->batch, h->stream));
  for (int phase = 0; phase <= 9; ++phase) if ((rc = idocp_parnmpc_launch_phase(h, phase, d_q, d_v))) return rc;
  return IDOCP_OK;
}

// coarse update + the four correction sweeps + direction + step sizes WITHOUT integrating (phases 0 .. 8): the state in which
// idocp_ocp_line_search_eval probes trial steps
int idocp_parnmpc_compute_direction(idocp_ocp_t* h, double t, const double* q, const double* v) {
  if (!h || !h->parnmpc || !q || !v) return IDOCP_E_ARG;
  if (!h->seq.status_set) { set_last_error("idocp_parnmpc_update_solution: call setContactStatusUniformly first"); return IDOCP_E_ARG; }
  int rc = enterO(h); if (rc) return rc;
  if ((rc = uploadStateO(h, q, v))) return rc;
  if ((rc = discretize(h, t))) return rc;
  HIP_TRY(hipMemsetAsync(h->B.status, 0, sizeof(int) * h->batch, h->stream));
  for (int phase = 0; phase <= 8; ++phase) if ((rc = idocp_parnmpc_launch_phase(h, phase, h->d_q0, h->d_v0))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

int idocp_parnmpc_update_solution(idocp_ocp_t* h, double t, const double* q, const double* v, int line_search) {
  if (!h || !h->parnmpc || !q || !v) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if (line_search) {
    // ParNMPCSolver::updateSolution(t, q, v, true) (parnmpc_solver.cpp:73-103): direction, filter line search on the primal step, integration
    // (the support check needs the chain of this t; nothing has touched the direction / Riccati records when it refuses)
    if (!h->seq.status_set) { set_last_error("idocp_parnmpc_update_solution: call setContactStatusUniformly first"); return IDOCP_E_ARG; }
    if ((rc = discretize(h, t))) return rc;
    if ((rc = parnmpcLineSearchSupported(h))) return rc;
    if ((rc = idocp_parnmpc_compute_direction(h, t, q, v))) return rc;
    if ((rc = runLineSearchO(h, h->d_q0))) return rc;
    if ((rc = idocp_parnmpc_launch_phase(h, 9, h->d_q0, h->d_v0))) return rc;
  } else {
    if ((rc = uploadStateO(h, q, v))) return rc;
    if ((rc = idocp_parnmpc_update_solution_device(h, t, h->d_q0, h->d_v0))) return rc;
  }
  return statusOfO(h, "factorisation failed (a stage matrix is not positive definite)");
}

// the KKT residual of the chain against the state in d_q0, d_v0; d_err2 (device, [batch]): the squared error goes there too, on the stream
static int launchParnmpcResidualO(idocp_ocp_t* h, double* d_err2 = nullptr) {
  const int M = h->M();
  OcpLaunch<DQ>::rnea(h->B, h->batch, M, h->plan.n_impulse(), h->stream);
  if (h->plan.has_switch) OcpLaunch<DQ>::switching(h->B, h->batch, M, h->stream);
  OcpLaunch<DQ>::condenseBackwardEuler(h->B, h->batch, M, h->d_q0, h->d_v0, true, h->stream);
  OcpLaunch<DQ>::parnmpcImpulseCondense(h->B, h->batch, h->plan.n_impulse(), true, h->d_q0, h->d_v0, h->stream);
  ocpKktErrorReduce(h->B, h->batch, h->stream, d_err2);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}
int idocp_parnmpc_compute_kkt_residual(idocp_ocp_t* h, double t, const double* q, const double* v) {
  if (!h || !h->parnmpc || !q || !v) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = discretize(h, t))) return rc;
  if ((rc = uploadStateO(h, q, v))) return rc;
  if ((rc = launchParnmpcResidualO(h))) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

// ---- horizon sharding (idocp_amd/parnmpc_dist.py; SURVEY.md 8e, BASELINE.json configs[3]) ----
// One handle per shard: the stages [stage_offset, stage_offset + N) of a longer horizon (T = N * dt of the shard).
int idocp_parnmpc_create_shard(const idocp_model_t* model, const idocp_cost_t* cost, const idocp_constraints_t* constraints, double T,
                               int N, int stage_offset, int has_terminal, int has_prev, int batch, int device, idocp_ocp_t** out) {
  if (stage_offset < 0) { set_last_error("invalid value: stage_offset must be non-negative!"); return IDOCP_E_ARG; }
  int rc = createOcpImpl(model, cost, constraints, T, N, 0, batch, device, true, out);
  if (rc) return rc;
  (*out)->stage_offset = stage_offset; (*out)->plan.has_terminal = has_terminal != 0; (*out)->plan.has_prev = has_prev != 0;
  (*out)->seq_dirty = true;
  return IDOCP_OK;
}
// A shard of a horizon WITH discrete events: the handle discretises the whole horizon (T, N, the contact sequence pushed on
// every rank alike) and keeps the grid stages [stage_begin, stage_end) of the chain together with the event stages in front
// of each of them; the halos are those of an event-free shard (they only carry q, v, lmd, gmm and aux_mat).
int idocp_parnmpc_create_hybrid_shard(const idocp_model_t* model, const idocp_cost_t* cost, const idocp_constraints_t* constraints, double T,
                                      int N, int max_num_impulse, int stage_begin, int stage_end, int batch, int device, idocp_ocp_t** out) {
  if (stage_begin < 0 || stage_end <= stage_begin || stage_end > N) { set_last_error("invalid value: 0 <= stage_begin < stage_end <= N must hold!"); return IDOCP_E_ARG; }
  int rc = createOcpImpl(model, cost, constraints, T, N, max_num_impulse, batch, device, true, out);
  if (rc) return rc;
  (*out)->slice_begin = stage_begin; (*out)->slice_end = stage_end;
  (*out)->plan.has_terminal = stage_end == N; (*out)->plan.has_prev = stage_begin > 0;
  (*out)->seq_dirty = true;
  return IDOCP_OK;
}
// doubles per instance of a halo: 0 state_last, 1 costate_first, 2 aux_first, 3 bwd_first, 4 fwd_last, 5 aux_all
int idocp_parnmpc_halo_size(int kind) {
  switch (kind) {
    case 0: case 4: return DQ::NQ + DQ::NV;
    case 1: return 2 * DQ::NV + DQ::NQ;
    case 3: return 2 * DQ::NV;
    case 2: case 5: return DQ::NX * DQ::NX;
    default: return -1;
  }
}
// d_buf[batch][halo_size(kind)] in device memory.  Importing kind 0 sets the state in front of the first stage (what the
// *_device entry points otherwise take as d_q, d_v): use idocp_parnmpc_prev_state to get those pointers.
static int haloImpl(idocp_ocp_t* h, int kind, bool do_import, double* d_buf, bool sync) {
  if (!h || !h->parnmpc || !d_buf || idocp_parnmpc_halo_size(kind) < 0) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = ensureDiscretized(h))) return rc;
  OcpLaunch<DQ>::parnmpcHalo(h->B, h->batch, kind, do_import, d_buf, h->d_q0, h->d_v0, h->stream);
  HIP_TRY(hipGetLastError());
  if (sync) HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}
int idocp_parnmpc_export_halo(idocp_ocp_t* h, int kind, double* d_buf) { return haloImpl(h, kind, false, d_buf, true); }
int idocp_parnmpc_import_halo(idocp_ocp_t* h, int kind, const double* d_buf) { return haloImpl(h, kind, true, const_cast<double*>(d_buf), true); }
// the same pack / unpack kernels ENQUEUED on the handle's stream without waiting for them: what a stream-ordered transport needs
// (idocp_amd/csrc/parnmpc_dist.hip: pack -> ncclSend, ncclRecv -> unpack, all on this stream)
int idocp_parnmpc_export_halo_async(idocp_ocp_t* h, int kind, double* d_buf) { return haloImpl(h, kind, false, d_buf, false); }
int idocp_parnmpc_import_halo_async(idocp_ocp_t* h, int kind, const double* d_buf) { return haloImpl(h, kind, true, const_cast<double*>(d_buf), false); }
// device pointers of the state in front of the first stage, q[batch][nq], v[batch][nv] (rank 0 uploads the measured state
// there; the other shards receive it through import_halo(0))
int idocp_parnmpc_prev_state(idocp_ocp_t* h, double** d_q, double** d_v) {
  if (!h || !h->parnmpc || !d_q || !d_v) return IDOCP_E_ARG;
  *d_q = h->d_q0; *d_v = h->d_v0;
  return IDOCP_OK;
}
// ---- filter line search on a sharded horizon: what the driver (parnmpc_dist.hip) needs from the handle ----
int idocp_parnmpc_set_line_search_hooks(idocp_ocp_t* h, int (*pre)(idocp_ocp_t*), int (*post)(idocp_ocp_t*)) {
  if (!h || !h->parnmpc) return IDOCP_E_ARG;
  h->ls_pre = pre; h->ls_post = post;
  return IDOCP_OK;
}
// the state_last halo of the TRIAL iterate: export (q, v) of the shard's last stage from sol_try; import into the trial state in front of
// the shard's first stage (d_buf[batch][idocp_parnmpc_halo_size(0)], enqueued on the handle's stream)
int idocp_parnmpc_trial_halo_async(idocp_ocp_t* h, int do_import, double* d_buf) {
  if (!h || !h->parnmpc || !d_buf) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  OcpBuffers Bt = h->B;
  if (!do_import) Bt.sol = h->B.sol_try;
  OcpLaunch<DQ>::parnmpcHalo(Bt, h->batch, 0, do_import != 0, d_buf, h->d_qtry, h->d_vtry, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}
// cost and violation sums of the last probe, [batch][2] in device memory (what the driver all-reduces)
int idocp_parnmpc_merit_device(idocp_ocp_t* h, double** d_merit) {
  if (!h || !d_merit) return IDOCP_E_ARG;
  *d_merit = h->B.merit;
  return IDOCP_OK;
}
// LineSearch::computeStepSize on the direction of phases 0 .. 8 (with the hooks above: collectively on every shard); B.step then holds the
// accepted primal steps
int idocp_parnmpc_line_search(idocp_ocp_t* h) {
  if (!h || !h->parnmpc) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = parnmpcLineSearchSupported(h))) return rc;
  return runLineSearchO(h, h->d_q0);
}
// step sizes [batch][2] (primal, dual) in device memory: read after phase 8, overwrite with the global minimum before phase 9
int idocp_parnmpc_step_sizes_device(idocp_ocp_t* h, double** d_steps) {
  if (!h || !d_steps) return IDOCP_E_ARG;
  *d_steps = h->B.step;
  return IDOCP_OK;
}
// discretise at time t (uploads the stage references) without running anything: call before the first phase of an iteration
int idocp_parnmpc_discretize(idocp_ocp_t* h, double t) {
  if (!h || !h->parnmpc) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  HIP_TRY(hipMemsetAsync(h->B.status, 0, sizeof(int) * h->batch, h->stream));
  return discretize(h, t);
}

// KKT residual with the state in front of the first stage already in device memory (sharded horizons); the squared
// error of the shard's stages is then d_err2[batch]
int idocp_parnmpc_kkt_error_squared_device(idocp_ocp_t* h, double t, double* d_err2) {
  if (!h || !h->parnmpc || !d_err2) return IDOCP_E_ARG;
  int rc = enterO(h); if (rc) return rc;
  if ((rc = discretize(h, t))) return rc;
  return launchParnmpcResidualO(h, d_err2);      // stays on the device and on the stream: no synchronisation here
}
int idocp_ocp_batch(idocp_ocp_t* h) { return h ? h->batch : 0; }
// Storage precision of the Riccati factorisation P, s (64 = default; 32 = rounded to single precision after every stage of the
// backward sweep, the device side of BASELINE configs[4]'s tolerance study).  Everything else stays FP64.
int idocp_ocp_set_riccati_storage(idocp_ocp_t* h, int bits) {
  if (!h || (bits != 32 && bits != 64)) return IDOCP_E_ARG;
  if (h->parnmpc) { set_last_error("idocp_ocp_set_riccati_storage: the Riccati sweep belongs to OCPSolver"); return IDOCP_E_UNSUPPORTED; }
  int rc = enterO(h); if (rc) return rc;
  h->prob.ric_fp32 = bits == 32 ? 1 : 0;
  HIP_TRY(hipMemcpyAsync(h->d_prob, &h->prob, sizeof(OcpProblem), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}
int idocp_ocp_state_dims(idocp_ocp_t* h, int* nq, int* nv) {
  if (!h || !nq || !nv) return IDOCP_E_ARG;
  *nq = DQ::NQ; *nv = DQ::NV;
  return IDOCP_OK;
}

// Robot::integrateConfiguration / subtractConfiguration / normalizeConfiguration (include/idocp/robot/robot.hxx:96-147) on the HOST, joint by joint:
// what an MPC loop does between two solver calls -- advance the plant by one sampling period, measure the distance to a goal, keep the base
// quaternion on the unit sphere.  Either side of the hot path, not on it (the kernels carry their own copies: dev_lie.hpp, the same functions).
int idocp_model_integrate_configuration(const idocp_model_t* m, const double* q, const double* v, double length, double* q_out) {
  if (!m || !q || !v || !q_out) { set_last_error("idocp_model_integrate_configuration: null argument"); return IDOCP_E_ARG; }
  for (int i = 0; i < m->njoints; ++i) {
    const int iq = m->idx_q[i], iv = m->idx_v[i];
    if (m->jtype[i] == IDOCP_JOINT_FREEFLYER) idocp_dev::lieIntegrateBase(q + iq, v + iv, length, q_out + iq);      // pinocchio::integrate on SE(3)
    else q_out[iq] = q[iq] + length * v[iv];
  }
  return IDOCP_OK;
}
// diff[nv] = q_plus (-) q_minus: log6(M_minus^-1 M_plus) on the free-flyer (pinocchio::difference(q_minus, q_plus)), q_plus - q_minus on a revolute joint
int idocp_model_subtract_configuration(const idocp_model_t* m, const double* q_plus, const double* q_minus, double* diff) {
  if (!m || !q_plus || !q_minus || !diff) { set_last_error("idocp_model_subtract_configuration: null argument"); return IDOCP_E_ARG; }
  for (int i = 0; i < m->njoints; ++i) {
    const int iq = m->idx_q[i], iv = m->idx_v[i];
    if (m->jtype[i] == IDOCP_JOINT_FREEFLYER) {
      double R[9], p[3];
      idocp_dev::lieRelative(q_minus + iq, q_plus + iq, R, p);
      idocp_dev::lieLog6(R, p, diff + iv);
    } else {
      diff[iv] = q_plus[iq] - q_minus[iq];
    }
  }
  return IDOCP_OK;
}
int idocp_model_normalize_configuration(const idocp_model_t* m, double* q) {
  if (!m || !q) { set_last_error("idocp_model_normalize_configuration: null argument"); return IDOCP_E_ARG; }
  for (int i = 0; i < m->njoints; ++i) {
    if (m->jtype[i] != IDOCP_JOINT_FREEFLYER) continue;
    double* qu = q + m->idx_q[i] + 3;
    const double n = std::sqrt(qu[0] * qu[0] + qu[1] * qu[1] + qu[2] * qu[2] + qu[3] * qu[3]);
    if (!(n > 0)) { set_last_error("idocp_model_normalize_configuration: zero quaternion"); return IDOCP_E_ARG; }
    for (int c = 0; c < 4; ++c) qu[c] /= n;
  }
  return IDOCP_OK;
}

// Deep copy (the reference's solver classes are copyable, `= default`: ocp_solver.hpp:171-186): a new handle of the same
// configuration whose device records, contact sequence and discretisation state equal the source's.
// The reference's solvers hold a shared_ptr to the CostFunction (ocp_solver.hpp:37-39): weights and references a driver changes
// between two updateSolution calls -- an MPC loop moving its goal -- take effect at the next call.  Here the cost was copied at
// creation; this is the way to change it afterwards.  The KIND of cost must stay what it was (a task-space term cannot appear or
// disappear: its record is allocated at creation).
int idocp_ocp_set_cost(idocp_ocp_t* h, const idocp_cost_t* cost) {
  if (!h || !cost) return IDOCP_E_ARG;
  if ((cost->task_dim != 0) != (h->cost.task_dim != 0) || cost->task_time_varying != h->cost.task_time_varying) {
    set_last_error("idocp_ocp_set_cost: a task-space cost cannot be added or removed after creation");
    return IDOCP_E_UNSUPPORTED;
  }
  if (cost->task_dim != 0 && (cost->task_dim != 3 && cost->task_dim != 6)) { set_last_error("invalid value: task_dim must be 0, 3 or 6"); return IDOCP_E_ARG; }
  { const int rc_t = checkTaskExtras(cost); if (rc_t) return rc_t; }
  { const int rc_e = enterO(h); if (rc_e) return rc_e; }
  h->cost = *cost;
  fillCostFields(h->prob, *cost);
  h->seq_dirty = true;              // the problem block and the per-stage reference table are uploaded with the next discretisation
  return IDOCP_OK;
}
int idocp_ocp_clone(idocp_ocp_t* src, idocp_ocp_t** out) {
  if (!src || !out) return IDOCP_E_ARG;
  int rc = enterO(src); if (rc) return rc;      // (the copies below read through the source's stream)
  idocp_ocp_t* h = nullptr;
  if ((rc = createOcpImpl(&src->model, &src->cost, &src->cons, src->T, src->N, src->E, src->batch, src->device, src->parnmpc, &h, &src->forms))) return rc;
  auto fail = [&](int code) { (void)hipGetLastError(); idocp_ocp_destroy(h); return code; };      // (clears HIP's sticky last error: see HIP_TRY)
  if (h->allocs.size() != src->allocs.size()) { set_last_error("idocp_ocp_clone: allocation tables differ"); return fail(IDOCP_E_DEVICE); }
  if (hipStreamSynchronize(src->stream) != hipSuccess) return fail(IDOCP_E_DEVICE);
  for (size_t i = 0; i < h->allocs.size(); ++i) {
    if (h->alloc_bytes[i] != src->alloc_bytes[i]) { set_last_error("idocp_ocp_clone: allocation tables differ"); return fail(IDOCP_E_DEVICE); }
    if (hipMemcpyAsync(h->allocs[i], src->allocs[i], h->alloc_bytes[i], hipMemcpyDeviceToDevice, h->stream) != hipSuccess) return fail(IDOCP_E_DEVICE);
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(IDOCP_E_DEVICE);
  h->task_refs_host = src->task_refs_host; h->task_refs_t = src->task_refs_t;
  h->seq = src->seq; h->stage_offset = src->stage_offset; h->plan.has_terminal = src->plan.has_terminal; h->plan.has_prev = src->plan.has_prev;
  h->slice_begin = src->slice_begin; h->slice_end = src->slice_end;
  h->filters = src->filters;                 // the line-search filter is part of the solver's state (LineSearch is a member of the reference's solvers)
  h->prob = src->prob;
  h->seq_dirty = true;                       // the chain is rebuilt (and uploaded) on first use
  if (src->disc_time == src->disc_time) {
    if ((rc = discretize(h, src->disc_time, true))) return fail(rc);
  }
  *out = h;
  return IDOCP_OK;
}
extern "C" void idocp_set_last_error_string(const char* msg) { set_last_error(msg ? msg : ""); }
int idocp_device_copy(void* d_dst, const void* d_src, unsigned long nbytes) {
  if (!d_dst || !d_src) return IDOCP_E_ARG;
  HIP_TRY(hipMemcpy(d_dst, d_src, nbytes, hipMemcpyDeviceToDevice));
  return IDOCP_OK;
}

}  // extern "C"
