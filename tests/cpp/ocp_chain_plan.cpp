// The contact sequence and the chain planner of the contact path (idocp_amd/csrc/ocp_chain.hpp) as a stand-alone program, driven by a script
// of commands on standard input (tests/test_ocp_chain_host.py):
//   create N T E kind        a new sequence and planner parameters; kind 0 = forward Euler (OCPSolver), 1 = backward Euler (ParNMPCSolver)
//   status a0 a1 a2 a3       setUniformly
//   push a0 a1 a2 a3 time    pushBack
//   pop_front | pop_back
//   chain t                  planChain at initial time t
// Every command answers "rc <code>"; an accepted chain answers "chain M" and M lines "kind index slot dimf sw_dimi dtq level time", a refused
// one "refused <code> <text>".  Every accepted ParNMPC chain with events is also cut at every split point of its grid stages and the two
// shards are held to the whole chain; a violated check ends the program with status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ocp_chain.hpp"

using namespace idocp_dev;

namespace {

long n_sharded = 0, n_splits = 0;

[[noreturn]] void fail(const char* what, double t, int k) {
  std::printf("self-check FAILED: %s (t = %.17g, split %d)\n", what, t, k);
  std::exit(1);
}

// the shards [0, k) and [k, Ng) of a ParNMPC chain with events, for every k
void checkShards(const ContactSequence& seq, double t, const ChainParams& P, const ChainPlan& whole) {
  int Ng = 0;
  for (const OcpNode& nd : whole.nodes) Ng += nd.kind == 0 ? 1 : 0;
  const int Mw = whole.M() - 1;                       // without the placeholder
  ++n_sharded;
  for (int k = 1; k < Ng; ++k, ++n_splits) {
    ChainParams L = P, R = P;
    L.slice_begin = 0; L.slice_end = k; R.slice_begin = k; R.slice_end = Ng;
    const ChainResult l = planChain(seq, t, L), r = planChain(seq, t, R);
    if (l.rc || r.rc) fail("a shard of an accepted chain is refused", t, k);
    const int Ml = l.plan.M() - 1, Mr = r.plan.M() - 1;
    if (Ml + Mr != Mw) fail("the shards do not add up to the chain", t, k);
    if (l.plan.nodes[Ml].kind != 4 || r.plan.nodes[Mr].kind != 4) fail("a shard does not end with a placeholder", t, k);
    for (int p = 0; p < Mw; ++p) {
      const ChainPlan& s = p < Ml ? l.plan : r.plan;
      const int ps = p < Ml ? p : p - Ml;
      OcpNode nd = s.nodes[ps];
      if (p == Ml) nd.prev = whole.nodes[p].prev;     // (the cut: the right shard's first stage has the imported state in front of it, checked below)
      if (std::memcmp(&nd, &whole.nodes[p], sizeof(OcpNode)) != 0) fail("a node of a shard differs from the chain's", t, k);
      if (s.chain_index[ps] != whole.chain_index[p] || s.chain_t[ps] != whole.chain_t[p]) fail("index or time of a shard's node differs", t, k);
    }
    if (r.plan.nodes[0].prev != -1) fail("the right shard's first stage has a predecessor", t, k);
    if (std::memcmp(&r.plan.nodes[Mr], &whole.nodes[Mw], sizeof(OcpNode)) != 0) fail("the right shard's placeholder differs from the chain's", t, k);
    if (l.plan.nodes[Ml].slot != r.plan.nodes[0].slot || l.plan.nodes[Ml - 1].next != r.plan.nodes[0].slot) fail("the left placeholder is not the right shard's first slot", t, k);
    if (l.plan.has_terminal || l.plan.has_prev || !r.plan.has_terminal || !r.plan.has_prev) fail("has_terminal / has_prev do not match the side", t, k);
    if (l.plan.Ngrid != whole.Ngrid || r.plan.Ngrid != whole.Ngrid) fail("Ngrid of a shard", t, k);
  }
  ChainParams X = P;
  X.slice_begin = Ng; X.slice_end = Ng + 1;
  const ChainResult e = planChain(seq, t, X);
  if (e.rc != IDOCP_E_ARG || e.error != "ParNMPC: empty shard of the chain" || e.plan.M() != 0) fail("an empty slice is not refused", t, Ng);
}

}  // namespace

int main() {
  ContactSequence seq;
  ChainParams P{1, 0, 1.0, false, 0, 0, -1, true, false};
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    const std::string c(cmd);
    int a[4];
    const double pts[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::string err;
    if (c == "create") {
      int kind = 0;
      if (std::scanf("%d %lf %d %d", &P.N, &P.T, &P.E, &kind) != 4) return 2;
      P.parnmpc = kind != 0;
      seq = ContactSequence();
      std::printf("rc 0\n");
    } else if (c == "status") {
      if (std::scanf("%d %d %d %d", &a[0], &a[1], &a[2], &a[3]) != 4) return 2;
      seq.setUniformly(HostStatus::make(a, pts));
      std::printf("rc 0\n");
    } else if (c == "push") {
      double time = 0.0;
      if (std::scanf("%d %d %d %d %lf", &a[0], &a[1], &a[2], &a[3], &time) != 5) return 2;
      std::printf("rc %d\n", seq.pushBack(HostStatus::make(a, pts), time, P.N, P.E, err));
    } else if (c == "pop_front") {
      std::printf("rc %d\n", seq.popFront());
    } else if (c == "pop_back") {
      std::printf("rc %d\n", seq.popBack());
    } else if (c == "chain") {
      double t = 0.0;
      if (std::scanf("%lf", &t) != 1) return 2;
      const ChainResult r = planChain(seq, t, P);
      if (r.rc) {
        if (r.plan.M() != 0 || r.error.empty()) fail("a refusal carries a plan or no text", t, 0);
        std::printf("refused %d %s\n", r.rc, r.error.c_str());
        continue;
      }
      const ChainPlan& plan = r.plan;
      std::printf("chain %d\n", plan.M());
      for (int p = 0; p < plan.M(); ++p) {
        const OcpNode& nd = plan.nodes[p];
        std::printf("%d %d %d %d %d %.17g %d %.17g\n", nd.kind, plan.chain_index[p], nd.slot, nd.kind == 4 ? 0 : nd.dimf, nd.sw_dimi, nd.dtq, nd.level, plan.chain_t[p]);
      }
      if (P.parnmpc && !seq.event_time.empty()) checkShards(seq, t, P, plan);
    } else {
      return 2;
    }
  }
  std::printf("ocp chain plan: ok, %ld sharded chains, %ld splits\n", n_sharded, n_splits);
  return 0;
}
