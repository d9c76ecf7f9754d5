// Host-side index logic of the contact path, free of any device call: the contact sequence (ContactSequence,
// include/idocp/hybrid/contact_sequence.hxx:56-333) and the planner that turns it into the CHAIN of stages of one discretisation
// (OCPDiscretizer, ocp_discretizer.hxx:65-374; ParNMPCDiscretizer, parnmpc_discretizer.hxx:65-373).  The planner returns a value;
// ocp_capi.hip commits it to the handle and uploads it only once nothing can refuse it any more.  Knows nothing of cost: vref_on,
// the q_ref table and the task references belong to the upload.
#ifndef IDOCP_OCP_CHAIN_HPP_
#define IDOCP_OCP_CHAIN_HPP_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "idocp_hip.h"

namespace idocp_dev {

// One stage of the CHAIN (time order): stage, [impulse, aux | lift], stage, ..., terminal.  Every stage owns a fixed
// storage SLOT (grid stage i -> i, impulse k -> N+1+k, aux k -> N+1+E+k, lift k -> N+1+2E+k, like the separate arrays
// of the reference's hybrid_container.hpp:60-168); the chain says who the neighbours are.
struct OcpNode {
  int slot, next, prev;     // prev = -1: the predecessor is the initial state
  int kind;                 // 0 stage, 1 impulse, 2 aux, 3 lift, 4 terminal
  int level;                // time step for the constraint gating (constraints_data.hpp:18-42): stage index, 0 aux / lift
  int has_u;                // 0 on impulse stages (no torque variables)
  int dimf, active[IDOCP_MAX_CONTACTS], row_of[IDOCP_MAX_CONTACTS];   // contact (or impulse) status of this stage
  double dt;                // scaling of cost / constraint / dynamics multipliers: the time step, 1 on impulse stages
  double dtq;               // q+ = q (+) dtq v: the time step, 0 on impulse stages
  double vref_on;           // 1, or 0 where a time-varying cost switches its velocity reference off (stage time outside its window)
  double contact_point[IDOCP_MAX_CONTACTS][3];
  int sw_dimi, sw_active[IDOCP_MAX_CONTACTS], sw_row[IDOCP_MAX_CONTACTS];     // switching constraint carried by this stage
  double sw_dt1, sw_dt2, sw_point[IDOCP_MAX_CONTACTS][3];
};
static_assert(sizeof(OcpNode) == 336 && offsetof(OcpNode, dt) == 64 && offsetof(OcpNode, sw_dt1) == 224, "the kernels read this layout");

// idocp::ContactStatus / ImpulseStatus on the host (include/idocp/robot/contact_status.hxx)
struct HostStatus {
  int active[IDOCP_MAX_CONTACTS] = {0, 0, 0, 0};
  double points[IDOCP_MAX_CONTACTS][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  static HostStatus make(const int* active, const double* contact_points) {
    HostStatus st;
    for (int c = 0; c < IDOCP_MAX_CONTACTS; ++c) {
      st.active[c] = active[c] ? 1 : 0;
      for (int k = 0; k < 3; ++k) st.points[c][k] = contact_points[3 * c + k];
    }
    return st;
  }
};

// ContactSequence (contact_sequence.hxx:56-333).  The operations return IDOCP_OK or the error code, with the text in `err`.
struct ContactSequence {
  std::vector<HostStatus> phases = std::vector<HostStatus>(1);      // ContactSequence ctor: default (no contact) status
  std::vector<double> event_time;
  std::vector<char> is_impulse;
  std::vector<HostStatus> impulse_status;          // per event
  bool status_set = false;

  int numEvents() const { return (int)event_time.size(); }
  void setUniformly(const HostStatus& st) {                           // contact_sequence.hxx:47-51
    phases.assign(1, st);
    event_time.clear(); is_impulse.clear(); impulse_status.clear();
    status_set = true;
  }
  // max_events = N: the sequence holds up to N events (ocp_solver.cpp:16: contact_sequence_(robot, N)); the event stages live in
  // max_per_kind = max_num_impulse impulse / aux / lift slots each (hybrid_container.hpp:39-96)
  int pushBack(const HostStatus& post, double switching_time, int max_events, int max_per_kind, std::string& err) {
    if (!status_set) { err = "Call setContactStatusUniformly() before calling push_back()!"; return IDOCP_E_ARG; }
    if (numEvents() + 1 > max_events) {
      err = "Number of discrete events=" + std::to_string(event_time.size() + 1) + " exceeds predefined max_num_events=" + std::to_string(max_events) + "!";
      return IDOCP_E_ARG;
    }
    if (!event_time.empty() && switching_time <= event_time.back()) {
      err = "event_time=" + std::to_string(switching_time) + " must be larger than the last event time=" + std::to_string(event_time.back()) + "!";
      return IDOCP_E_ARG;
    }
    // DiscreteEvent::setDiscreteEvent (discrete_event.hxx:57-84)
    const HostStatus& pre = phases.back();
    HostStatus imp = post;
    bool exist_impulse = false, exist_lift = false;
    for (int c = 0; c < IDOCP_MAX_CONTACTS; ++c) {
      imp.active[c] = 0;
      if (pre.active[c]) { if (!post.active[c]) exist_lift = true; }
      else if (post.active[c]) { imp.active[c] = 1; exist_impulse = true; }
    }
    if (!exist_impulse && !exist_lift) { err = "discrete_event.existDiscreteEvent() must be true!"; return IDOCP_E_ARG; }
    int n_same = 0;
    for (int e : is_impulse) n_same += ((e != 0) == exist_impulse) ? 1 : 0;
    if (n_same + 1 > max_per_kind) {
      err = std::string("Number of ") + (exist_impulse ? "impulse" : "lift") + " events=" + std::to_string(n_same + 1) + " exceeds max_num_impulse=" + std::to_string(max_per_kind) + "!";
      return IDOCP_E_ARG;
    }
    phases.push_back(post);
    event_time.push_back(switching_time);
    is_impulse.push_back(exist_impulse ? 1 : 0);
    impulse_status.push_back(imp);
    return IDOCP_OK;
  }
  int setContactPoints(int contact_phase, const double* contact_points, std::string& err) {
    if (contact_phase < 0 || contact_phase >= (int)phases.size()) {
      err = "contact_phase=" + std::to_string(contact_phase) + " must be smaller than numContactPhases()" + std::to_string(phases.size()) + "!";
      return IDOCP_E_ARG;
    }
    for (int c = 0; c < IDOCP_MAX_CONTACTS; ++c) for (int k = 0; k < 3; ++k) {
      phases[contact_phase].points[c][k] = contact_points[3 * c + k];
      if (contact_phase > 0 && is_impulse[contact_phase - 1]) impulse_status[contact_phase - 1].points[c][k] = contact_points[3 * c + k];
    }
    return IDOCP_OK;
  }
  int popBack() {                                                     // contact_sequence.hxx:105-125
    if (event_time.empty()) { phases.assign(1, HostStatus()); return IDOCP_OK; }
    event_time.pop_back(); is_impulse.pop_back(); impulse_status.pop_back(); phases.pop_back();
    return IDOCP_OK;
  }
  int popFront() {                                                    // contact_sequence.hxx:126-146
    if (event_time.empty()) { phases.assign(1, HostStatus()); return IDOCP_OK; }
    event_time.erase(event_time.begin()); is_impulse.erase(is_impulse.begin());
    impulse_status.erase(impulse_status.begin()); phases.erase(phases.begin());
    return IDOCP_OK;
  }
};

struct ChainParams {
  int N, E;                 // grid intervals (N_ideal), max number of events of a kind
  double T;
  bool parnmpc;             // backward-Euler stages (ParNMPCDiscretizer) instead of forward-Euler ones (OCPDiscretizer)
  int stage_offset;         // event-free ParNMPC shard: global index of its first stage
  int slice_begin, slice_end;   // ParNMPC with events: keep the grid stages [slice_begin, slice_end) of the chain (-1: all)
  bool has_terminal, has_prev;  // event-free ParNMPC shard: what the handle was created with (a chain with events derives them)
};

// One discretisation: everything the handle and its kernels know about the chain.
struct ChainPlan {
  std::vector<OcpNode> nodes;          // prev / next set; vref_on left to the upload
  std::vector<int> chain_index;
  std::vector<double> chain_t;
  std::vector<OcpNode> nodes_ls;       // forward-Euler chain only: the chain as the line search pairs it
  std::vector<int> impulse_pos, switch_pos;      // chain positions: impulse stages | stages with a switching constraint
  std::vector<int> general_pos;        // ParNMPC: stages with a general KKT shape -- left to the upload, which asks parnmpcShape (ocp_device.hpp), the one definition
  std::vector<int> cond_pos;           // forward-Euler chain only: chain positions grouped by stage class of K5b, cond_n of each:
  int cond_n[5] = {0, 0, 0, 0, 0};     // all feet | half of them | the rest | event stages with half of the feet | flight stages
  int Ngrid = 0;                       // grid stages after discretisation
  int uniform_dimf = -1;               // dimf shared by all stages of an event-free forward-Euler chain, else -1
  bool has_switch = false, has_terminal = true, has_prev = false;
  int stage_offset = 0;                // what OcpProblem::stage_offset gets
  int M() const { return (int)nodes.size(); }
  int n_impulse() const { return (int)impulse_pos.size(); }
  int n_general() const { return (int)general_pos.size(); }
};

struct ChainResult {
  int rc = IDOCP_OK;
  std::string error;
  ChainPlan plan;           // empty unless rc == IDOCP_OK
};

namespace chain_detail {

inline ChainResult refuse(int rc, const char* text) { ChainResult r; r.rc = rc; r.error = text; return r; }

inline int slotOf(const ChainParams& P, int kind, int index) {
  switch (kind) {
    case 1: return P.N + 1 + index;
    case 2: return P.N + 1 + P.E + index;
    case 3: return P.N + 1 + 2 * P.E + index;
    default: return index;
  }
}

// room for the longest chain the slots hold (N + 1 grid stages, E impulse, aux and lift stages each): no node moves while the chain grows
inline void reserveChain(ChainPlan& plan, const ChainParams& P) {
  const size_t n = (size_t)P.N + 1 + 3 * (size_t)P.E;
  plan.nodes.reserve(n); plan.chain_index.reserve(n); plan.chain_t.reserve(n);
}

// the one node maker: appends stage `index` of `kind` at time tt to the plan
inline OcpNode& addNode(ChainPlan& plan, const ChainParams& P, int kind, int index, double tt, double dtt, const HostStatus& st, int level) {
  OcpNode nd;
  std::memset(&nd, 0, sizeof(nd));
  nd.kind = kind; nd.slot = slotOf(P, kind, index); nd.level = level;
  nd.has_u = (kind == 1) ? 0 : 1;
  nd.dt = (kind == 1) ? 1.0 : dtt;
  nd.dtq = (kind == 1) ? 0.0 : dtt;
  int row = 0;
  for (int c = 0; c < IDOCP_MAX_CONTACTS; ++c) {
    nd.active[c] = st.active[c] ? 1 : 0;
    nd.row_of[c] = st.active[c] ? row : -1;
    if (st.active[c]) row += 3;
    for (int k = 0; k < 3; ++k) nd.contact_point[c][k] = st.points[c][k];
  }
  nd.dimf = row;
  plan.nodes.push_back(nd); plan.chain_index.push_back(index); plan.chain_t.push_back(tt);
  return plan.nodes.back();
}

// the placeholder behind the last stage of a ParNMPC chain or shard, so that the per-stage kernels see the usual "M - 1 stages + one
// more" chain: a regular step in the storage slot of whatever follows (where a shard's imported halos land)
inline void addPlaceholder(ChainPlan& plan, const ChainParams& P, int slot, int index, double tt, const HostStatus& st, int level) {
  addNode(plan, P, 4, index, tt, P.T / P.N, st, level).slot = slot;
}

// the switching constraint of impulse status `is` on a stage (ocp_linearizer.hxx:152-163, 205-217; switchingconstraint::linearizeSwitchingConstraint)
inline void fillSwitch(OcpNode& nd, const HostStatus& is, double sw_dt1, double sw_dt2) {
  int row = 0;
  for (int c = 0; c < IDOCP_MAX_CONTACTS; ++c) {
    nd.sw_active[c] = is.active[c] ? 1 : 0;
    nd.sw_row[c] = is.active[c] ? row : -1;
    if (is.active[c]) row += 3;
    for (int k = 0; k < 3; ++k) nd.sw_point[c][k] = is.points[c][k];
  }
  nd.sw_dimi = row;
  nd.sw_dt1 = sw_dt1; nd.sw_dt2 = sw_dt2;
}

// the impulses, or the lifts, of a sequence in time order (countDiscreteEvents)
struct EventTrack {
  std::vector<int> event;          // index into the sequence's events
  std::vector<int> stage;          // the time stage before (forward Euler) / after (backward Euler) the event
  std::vector<double> time, dt;    // event time, time step of the event's own stage (aux / lift)
  int cur = 0;
  int n() const { return (int)event.size(); }
  bool at(int i) const { return cur < n() && i == stage[cur]; }
  void reserve(size_t n) { event.reserve(n); stage.reserve(n); time.reserve(n); dt.reserve(n); }
  void add(int e, double te, double t, double dt_ideal) {
    event.push_back(e); time.push_back(te); dt.push_back(0.0); stage.push_back((int)std::floor((te - t) / dt_ideal));
  }
};

struct TimeSteps {
  EventTrack imp, lift;
  std::vector<double> dts, ts;
  int Ng = 0;
  double dt_ideal = 0.0;
  TimeSteps(const ContactSequence& seq, double t, const ChainParams& P) : dts(P.N + 1, P.T / P.N), ts(P.N + 1, 0.0), dt_ideal(P.T / P.N) {
    imp.reserve(seq.event_time.size()); lift.reserve(seq.event_time.size());
    for (int e = 0; e < seq.numEvents(); ++e) (seq.is_impulse[e] ? imp : lift).add(e, seq.event_time[e], t, dt_ideal);
  }
};

// OCPDiscretizer::countTimeSteps (ocp_discretizer.hxx): an event closer than min_dt to the grid point behind it merges with it
inline void forwardEulerSteps(TimeSteps& S, double t, const ChainParams& P) {
  const double min_dt = std::sqrt(std::numeric_limits<double>::epsilon()), dt_ideal = S.dt_ideal, max_dt = dt_ideal - min_dt;      // ocp_discretizer.hpp:108-109
  int on_grid = 0;
  for (int i = 0; i < P.N; ++i) {
    const int stage = i - on_grid;
    EventTrack* ev = S.imp.at(i) ? &S.imp : (S.lift.at(i) ? &S.lift : nullptr);
    if (!ev) { S.dts[stage] = dt_ideal; S.ts[stage] = t + i * dt_ideal; continue; }
    const int k = ev->cur;
    S.dts[stage] = ev->time[k] - i * dt_ideal - t;
    if (S.dts[stage] <= min_dt) { ev->stage[k] = stage - 1; ev->dt[k] = dt_ideal; S.ts[stage] = t + (i - 1) * dt_ideal; ++on_grid; ++ev->cur; }
    else if (S.dts[stage] >= max_dt) { ev->stage[k] = i + 1; S.ts[stage] = t + i * dt_ideal; }
    else { ev->stage[k] = stage; ev->dt[k] = dt_ideal - S.dts[stage]; S.ts[stage] = t + i * dt_ideal; ++ev->cur; }
  }
  S.Ng = P.N - on_grid;
  S.ts[S.Ng] = t + P.T;
}

// ParNMPCDiscretizer::countTimeSteps (parnmpc_discretizer.hxx:265-324): an event closer than min_dt to the grid point in front of it merges with it
inline void backwardEulerSteps(TimeSteps& S, double t, const ChainParams& P) {
  const double min_dt = std::sqrt(std::numeric_limits<double>::epsilon()), dt_ideal = S.dt_ideal, max_dt = dt_ideal - min_dt;
  int on_grid = 0;
  for (int i = 0; i < P.N; ++i) {
    const int stage = i - on_grid;
    EventTrack* ev = S.imp.at(i) ? &S.imp : (S.lift.at(i) ? &S.lift : nullptr);
    if (!ev) { S.dts[stage] = dt_ideal; S.ts[stage] = t + (i + 1) * dt_ideal; continue; }
    const int k = ev->cur;
    S.dts[stage] = (i + 1) * dt_ideal + t - ev->time[k];
    if (S.dts[stage] <= min_dt) { ev->stage[k] = i + 1; S.ts[stage] = t + (i + 1) * dt_ideal; }
    else if (S.dts[stage] >= max_dt) { ev->stage[k] = stage - 1; ev->dt[k] = dt_ideal; S.ts[stage] = t + i * dt_ideal; ++on_grid; ++ev->cur; }
    else { ev->stage[k] = stage; ev->dt[k] = dt_ideal - S.dts[stage]; S.ts[stage] = t + (i + 1) * dt_ideal; ++ev->cur; }
  }
  S.Ng = P.N - on_grid;
  S.ts[S.Ng - 1] = t + P.T;
}

// countTimeStages: which event, if any, each grid stage has next to it
inline void eventsOfStages(TimeSteps& S, int n, std::vector<int>& imp_at, std::vector<int>& lift_at) {
  S.imp.cur = 0; S.lift.cur = 0;
  for (int i = 0; i < n; ++i) {
    if (S.imp.at(i)) imp_at[i] = S.imp.cur++;
    if (S.lift.at(i)) lift_at[i] = S.lift.cur++;
  }
}

// neighbours and position lists of a finished chain
inline void finishChain(ChainPlan& plan) {
  const int M = plan.M();
  for (int p = 0; p < M; ++p) {
    OcpNode& nd = plan.nodes[p];
    nd.prev = p > 0 ? plan.nodes[p - 1].slot : -1;
    nd.next = p + 1 < M ? plan.nodes[p + 1].slot : -1;
    if (nd.kind == 1) plan.impulse_pos.push_back(p);
    if (nd.sw_dimi > 0) plan.has_switch = true;
    if (nd.sw_dimi > 0 && p + 1 < M) plan.switch_pos.push_back(p);
  }
}

inline ChainResult planForwardEuler(const ContactSequence& seq, double t, const ChainParams& P) {
  TimeSteps S(seq, t, P);
  forwardEulerSteps(S, t, P);
  const int Ng = S.Ng;
  std::vector<int> imp_after(Ng + 1, -1), lift_after(Ng + 1, -1), phase(Ng + 1, 0);                                             // countTimeStages / countContactPhase
  eventsOfStages(S, Ng, imp_after, lift_after);
  int num_events = 0;
  for (int i = 0; i < Ng; ++i) {
    phase[i] = num_events;
    if (imp_after[i] >= 0 && lift_after[i] >= 0) return refuse(IDOCP_E_ARG, "OCPDiscretizer: an impulse and a lift fall into the same time stage");
    if (imp_after[i] >= 0 || lift_after[i] >= 0) ++num_events;
  }
  phase[Ng] = num_events;
  if (num_events > (int)seq.phases.size() - 1) return refuse(IDOCP_E_ARG, "OCPDiscretizer: inconsistent contact sequence");
  ChainResult r;
  ChainPlan& plan = r.plan;
  reserveChain(plan, P);
  auto switchAhead = [&](int i) {          // the stage two steps ahead of an impulse carries its switching constraint
    if (i + 1 < Ng && imp_after[i + 1] >= 0) { OcpNode& nd = plan.nodes.back(); fillSwitch(nd, seq.impulse_status[S.imp.event[imp_after[i + 1]]], nd.dtq, S.dts[i + 1]); }
  };
  for (int i = 0; i < Ng; ++i) {
    addNode(plan, P, 0, i, S.ts[i], S.dts[i], seq.phases[phase[i]], i);
    if (imp_after[i] >= 0) {
      const int k = imp_after[i];
      addNode(plan, P, 1, k, S.imp.time[k], 0.0, seq.impulse_status[S.imp.event[k]], -1);
      addNode(plan, P, 2, k, S.imp.time[k], S.imp.dt[k], seq.phases[phase[i + 1]], 0);
    } else if (lift_after[i] >= 0) {
      const int k = lift_after[i];
      addNode(plan, P, 3, k, S.lift.time[k], S.lift.dt[k], seq.phases[phase[i + 1]], 0);
      switchAhead(i);
    } else {
      switchAhead(i);
    }
  }
  addNode(plan, P, 4, Ng, S.ts[Ng], 0.0, seq.phases[phase[Ng]], Ng);
  finishChain(plan);
  const int M = plan.M();
  plan.Ngrid = Ng;
  if (seq.event_time.empty()) plan.uniform_dimf = plan.nodes[0].dimf;
  // The chain as the line search pairs it (line_search.cpp:80-113): the state-equation residual of a grid stage in front of an
  // impulse / lift is evaluated against the NEXT GRID STAGE (the value computed against the event stage is overwritten there).
  plan.nodes_ls = plan.nodes;
  for (int p = 0; p + 1 < M; ++p)
    if (plan.nodes[p].kind == 0 && (plan.nodes[p + 1].kind == 1 || plan.nodes[p + 1].kind == 3)) {
      int pn = p + 2;
      while (pn < M && plan.nodes[pn].kind != 0 && plan.nodes[pn].kind != 4) ++pn;
      if (pn < M) plan.nodes_ls[p].next = plan.nodes[pn].slot;
    }
  // stage classes of K5b (OcpLaunch::condenseMixed)
  const int NF = 3 * IDOCP_MAX_CONTACTS;
  std::vector<int> cls[5];
  for (int p = 0; p < M; ++p) {
    const OcpNode& nd = plan.nodes[p];
    const bool grid = (nd.kind == 0 || nd.kind == 2 || nd.kind == 3), plain = grid && nd.sw_dimi == 0;
    const bool event_half = !plain && (grid || nd.kind == 1) && nd.dimf == NF / 2;      // an impulse / a switching constraint on half of the feet
    const bool flight = plain && nd.dimf == 0;
    cls[plain && nd.dimf == NF ? 0 : (plain && nd.dimf == NF / 2 ? 1 : (event_half ? 3 : (flight ? 4 : 2)))].push_back(p);
  }
  for (int c = 0; c < 5; ++c) { plan.cond_n[c] = (int)cls[c].size(); plan.cond_pos.insert(plan.cond_pos.end(), cls[c].begin(), cls[c].end()); }
  return r;
}

// ParNMPCDiscretizer::discretizeOCP with discrete events (parnmpc_discretizer.hxx:65-72: countDiscreteEvents :246-262,
// countTimeSteps :265-324, countTimeStages :327-361, countContactPhase :364-373).  The event stages sit IN FRONT of the grid
// stage that follows the event:  ..., stage i-1, [aux k, impulse k | lift k], stage i, ...; the aux stage carries the
// switching constraint of its impulse (sw_* fields of the node, with sw_dt1 = sw_dt2 = 0: the constraint acts on the aux
// stage's own configuration).
inline ChainResult planBackwardEulerHybrid(const ContactSequence& seq, double t, const ChainParams& P) {
  if (P.stage_offset != 0) return refuse(IDOCP_E_UNSUPPORTED, "ParNMPC: a horizon with discrete events is sharded by idocp_parnmpc_create_hybrid_shard");
  TimeSteps S(seq, t, P);
  backwardEulerSteps(S, t, P);
  const int Ng = S.Ng;
  std::vector<int> imp_before(Ng, -1), lift_before(Ng, -1), phase(Ng, 0);
  eventsOfStages(S, Ng, imp_before, lift_before);
  int num_events = 0;
  for (int i = 0; i < Ng; ++i) {
    if (imp_before[i] >= 0 && lift_before[i] >= 0) return refuse(IDOCP_E_ARG, "ParNMPCDiscretizer: an impulse and a lift fall into the same time stage");
    if (imp_before[i] >= 0 || lift_before[i] >= 0) ++num_events;
    phase[i] = num_events;
  }
  if (S.imp.cur != S.imp.n() || S.lift.cur != S.lift.n()) return refuse(IDOCP_E_ARG, "ParNMPCDiscretizer: a discrete event lies outside the horizon");
  for (int i = 0; i + 1 < Ng; ++i)
    if (imp_before[i] >= 0 && imp_before[i + 1] >= 0) return refuse(IDOCP_E_ARG, "ParNMPCDiscretizer: impulses in consecutive time stages");
  // a lift or an impulse in front of the first time stage: the event stages are the first elements of the chain and their
  // predecessor is the measured state (backward_correction_solver.cpp:201-217, 232-246).  The aux stage carries the switching
  // constraint like every other aux stage: the reference's call at :203-211 omits the impulse status and then sizes the KKT
  // inverse with it (split_backward_correction.hxx:46-52), which is not defined as written (oracle/ocp.cpp, same place)
  ChainPlan whole;
  reserveChain(whole, P);
  for (int i = 0; i < Ng; ++i) {
    const int phase_before = i > 0 ? phase[i - 1] : 0;
    if (imp_before[i] >= 0) {
      const int k = imp_before[i];
      const HostStatus& is = seq.impulse_status[S.imp.event[k]];
      fillSwitch(addNode(whole, P, 2, k, S.imp.time[k], S.imp.dt[k], seq.phases[phase_before], 0), is, 0.0, 0.0);
      addNode(whole, P, 1, k, S.imp.time[k], 0.0, is, -1);
    } else if (lift_before[i] >= 0) {
      const int k = lift_before[i];
      addNode(whole, P, 3, k, S.lift.time[k], S.lift.dt[k], seq.phases[phase_before], 0);
    }
    addNode(whole, P, 0, i, S.ts[i], S.dts[i], seq.phases[phase[i]], (i == Ng - 1) ? P.N : i + 1);      // parnmpc_linearizer.cpp:43-58
  }
  ChainResult r;
  ChainPlan& plan = r.plan;
  const bool sliced = P.slice_end >= 0;
  const int lo = sliced ? P.slice_begin : 0, hi = sliced ? std::min(P.slice_end, Ng) : Ng;
  if (!sliced) {
    plan = std::move(whole);
  } else {
    // A shard of the chain (idocp_parnmpc_create_hybrid_shard): the grid stages [slice_begin, slice_end) and the event stages in
    // front of each of them; slots and constraint levels stay the global ones.  The placeholder behind the slice is the slot of
    // the right neighbour's first stage, where the imported halos (lmd, gmm, q, aux_mat, corrected lmd, gmm) land.
    int next_slot = -1;
    reserveChain(plan, P);
    for (size_t p = 0; p < whole.nodes.size(); ++p) {
      size_t g = p;
      while (whole.nodes[g].kind != 0) ++g;                            // event stages precede their grid stage
      const int owner = whole.chain_index[g];
      if (owner >= lo && owner < hi) { plan.nodes.push_back(whole.nodes[p]); plan.chain_index.push_back(whole.chain_index[p]); plan.chain_t.push_back(whole.chain_t[p]); }
      else if (owner >= hi && next_slot < 0) next_slot = whole.nodes[p].slot;
    }
    if (plan.nodes.empty()) return refuse(IDOCP_E_ARG, "ParNMPC: empty shard of the chain");
    if (hi < Ng) addPlaceholder(plan, P, next_slot, hi, t + P.T, seq.phases[0], P.N);
  }
  if (hi >= Ng) addPlaceholder(plan, P, P.N, Ng, t + P.T, seq.phases[phase[Ng - 1]], P.N);
  plan.has_terminal = hi >= Ng; plan.has_prev = lo != 0;
  plan.stage_offset = 0;
  plan.Ngrid = Ng - 1;
  finishChain(plan);
  return r;
}

// ParNMPCDiscretizer for a horizon without events (include/idocp/hybrid/parnmpc_discretizer.hxx): N backward-Euler stages,
// stage i at time t + (i + 1) dt with constraint level i + 1 (parnmpc_linearizer.cpp:43-58), followed by the placeholder.
inline ChainResult planBackwardEuler(const ContactSequence& seq, double t, const ChainParams& P) {
  if (!seq.event_time.empty()) return planBackwardEulerHybrid(seq, t, P);
  const int N = P.N;
  const double dt = P.T / N;
  ChainResult r;
  ChainPlan& plan = r.plan;
  reserveChain(plan, P);
  for (int i = 0; i < N; ++i) addNode(plan, P, 0, i, t + (P.stage_offset + i + 1) * dt, dt, seq.phases[0], P.stage_offset + i + 1);
  addPlaceholder(plan, P, N, N, t + (P.stage_offset + N) * dt, seq.phases[0], P.stage_offset + N + 1);
  plan.has_terminal = P.has_terminal; plan.has_prev = P.has_prev;
  plan.stage_offset = P.stage_offset;
  plan.Ngrid = N - 1;                  // getters: stages 0 .. N-1
  finishChain(plan);
  return r;
}

}  // namespace chain_detail

// The chain of the discretisation of `seq` at initial time t, or the refusal (code and text) of a sequence the discretiser does not take.
inline ChainResult planChain(const ContactSequence& seq, double t, const ChainParams& P) {
  return P.parnmpc ? chain_detail::planBackwardEuler(seq, t, P) : chain_detail::planForwardEuler(seq, t, P);
}

}  // namespace idocp_dev
#endif  // IDOCP_OCP_CHAIN_HPP_
