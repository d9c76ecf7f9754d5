// The host-side planning of idocp_rbd_objective_gradients and of the LQR weights of an objective (idocp_amd/csrc/rbd_objective.hpp) as a stand-alone
// program, built with the address and undefined-behaviour sanitizers by tests/test_rbd_gradients_host.py: every refusal with its code and a text
// that names the term, the calls that pass, the weight tables.  No HIP runtime header, no device.
#define IDOCP_NO_HIP_RUNTIME
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rbd_objective.hpp"

using namespace idocp_host;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static idocp_model_t quadruped() {
  idocp_model_t m;
  std::memset(&m, 0, sizeof(m));
  m.nq = 19; m.nv = 18; m.nu = 12; m.ncontacts = 4;
  return m;
}
static idocp_model_t chain(int nv) {
  idocp_model_t m;
  std::memset(&m, 0, sizeof(m));
  m.nq = m.nv = m.nu = nv; m.ncontacts = 0;
  return m;
}
static idocp_cost_t standing() {
  idocp_cost_t c;
  std::memset(&c, 0, sizeof(c));
  c.q_ref[6] = 1.0;
  for (int r = 0; r < 18; ++r) { c.q_weight[r] = 10 + r; c.v_weight[r] = 1 + r; c.qf_weight[r] = 2 + r; c.vf_weight[r] = 3 + r; }
  return c;
}

static bool refused(const RbdGradientCall& r, int rc, const char* text) {
  const bool ok = r.rc == rc && r.error.find("gradients: ") == 0 && r.error.find(text) != std::string::npos;
  if (!ok) std::printf("  got rc %d, \"%s\" for \"%s\"\n", r.rc, r.error.c_str(), text);
  return ok;
}

static void refusals() {
  const idocp_model_t m = quadruped();
  idocp_cost_t c = standing();
  const RbdObjectivePlan p = planObjective(m, true, &c, nullptr, 0, 0.01, 12);
  CHECK(p.rc == IDOCP_OK && gradientUnsupported(p).empty());
  auto call = [&](const RbdObjectivePlan& o, int n, int first, int steps, int terminal, bool q, bool v, bool u, bool lx, bool lu) {
    return planGradientCall("gradients", o, n, first, steps, terminal, q, v, u, lx, lu);
  };
  CHECK(call(p, 3, 0, 12, 1, true, true, true, true, true).rc == IDOCP_OK);
  CHECK(call(p, 3, 0, 12, 1, true, true, false, true, true).rc == IDOCP_OK);      // every u_weight is zero: u_traj may be NULL
  CHECK(call(p, 3, 5, 7, 0, true, true, true, true, false).rc == IDOCP_OK);       // one output is enough
  CHECK(call(p, 3, 5, 7, 0, true, true, true, false, true).rc == IDOCP_OK);
  CHECK(call(p, 1, 11, 1, 1, true, true, true, true, true).rc == IDOCP_OK);       // the last step and the terminal slice
  CHECK(refused(call(p, 0, 0, 2, 1, true, true, true, true, true), IDOCP_E_ARG, "n must be positive"));
  CHECK(refused(call(p, -4, 0, 2, 1, true, true, true, true, true), IDOCP_E_ARG, "n must be positive"));
  CHECK(refused(call(p, 3, 0, 0, 1, true, true, true, true, true), IDOCP_E_ARG, "steps must be at least 1"));
  CHECK(refused(call(p, 3, 0, -1, 1, true, true, true, true, true), IDOCP_E_ARG, "steps must be at least 1"));
  CHECK(refused(call(p, 3, 6, 7, 1, true, true, true, true, true), IDOCP_E_ARG, "first_step + steps must lie within the objective's 12 steps"));
  CHECK(refused(call(p, 3, -1, 2, 1, true, true, true, true, true), IDOCP_E_ARG, "first_step + steps"));
  CHECK(refused(call(p, 3, 0, 13, 0, true, true, true, true, true), IDOCP_E_ARG, "first_step + steps"));
  CHECK(refused(call(p, 3, 0, 2, 1, false, true, true, true, true), IDOCP_E_ARG, "q_traj and v_traj"));
  CHECK(refused(call(p, 3, 0, 2, 1, true, false, true, true, true), IDOCP_E_ARG, "q_traj and v_traj"));
  CHECK(refused(call(p, 3, 0, 2, 1, true, true, true, false, false), IDOCP_E_ARG, "no output was asked for"));
  CHECK(refused(call(p, 2000000000, 0, 2, 1, true, true, true, true, true), IDOCP_E_ARG, "must fit an int"));
  {   // u_traj missing under a non-zero u_weight
    idocp_cost_t x = c; x.u_weight[11] = 1e-3;
    const RbdObjectivePlan o = planObjective(m, true, &x, nullptr, 0, 0.01, 12);
    CHECK(refused(call(o, 3, 0, 2, 1, true, true, false, true, true), IDOCP_E_ARG, "u_traj is NULL but a non-zero u_weight"));
    CHECK(call(o, 3, 0, 2, 1, true, true, true, true, true).rc == IDOCP_OK);
  }
  {   // a_weight: unsupported, named, and in front of every argument error
    idocp_cost_t x = c; x.a_weight[17] = 0.5;
    const RbdObjectivePlan o = planObjective(m, true, &x, nullptr, 0, 0.01, 12);
    CHECK(o.rc == IDOCP_OK);
    CHECK(refused(call(o, 3, 0, 2, 1, true, true, true, true, true), IDOCP_E_UNSUPPORTED, "a_weight"));
    CHECK(refused(call(o, 0, 0, 2, 1, true, true, true, true, true), IDOCP_E_UNSUPPORTED, "a_weight"));
    CHECK(gradientUnsupported(o).find("a_weight") != std::string::npos);
  }
  {   // f_weight of any contact
    idocp_cost_t x = c; x.f_weight[3][2] = 1e-3;
    const RbdObjectivePlan o = planObjective(m, true, &x, nullptr, 0, 0.01, 12);
    CHECK(o.rc == IDOCP_OK);
    CHECK(refused(call(o, 3, 0, 2, 1, true, true, true, true, true), IDOCP_E_UNSUPPORTED, "f_weight"));
    CHECK(gradientUnsupported(o).find("f_weight") != std::string::npos);
  }
  {   // a chain has no contacts: its f_weight entries are not looked at
    const idocp_model_t a = chain(3);
    idocp_cost_t x = c; x.f_weight[0][0] = 1.0;
    const RbdObjectivePlan o = planObjective(a, false, &x, nullptr, 0, 0.01, 4);
    CHECK(o.rc == IDOCP_OK && gradientUnsupported(o).empty());
    CHECK(call(o, 2, 0, 4, 1, true, true, true, true, true).rc == IDOCP_OK);
  }
}

static void weights() {
  const idocp_model_t m = quadruped();
  idocp_cost_t c = standing();
  for (int j = 0; j < 12; ++j) c.u_weight[j] = 0.5 + j;
  const RbdObjectivePlan p = planObjective(m, true, &c, nullptr, 0, 0.25, 3);
  CHECK(lqrWeightOffsetU(p) == 36 && lqrWeightOffsetXf(p) == 48 && lqrWeightDoubles(p) == 84);
  std::vector<double> w((size_t)lqrWeightDoubles(p), -1.0);
  lqrWeights(p, w.data());
  for (int r = 0; r < 18; ++r) {
    CHECK(w[r] == 0.25 * c.q_weight[r] && w[18 + r] == 0.25 * c.v_weight[r]);
    CHECK(w[48 + r] == c.qf_weight[r] && w[48 + 18 + r] == c.vf_weight[r]);
  }
  for (int j = 0; j < 12; ++j) CHECK(w[36 + j] == 0.25 * c.u_weight[j]);
  // an odd nu: the terminal weights start at an even number of doubles, the gap is zero
  const idocp_model_t a = chain(3);
  const RbdObjectivePlan pc = planObjective(a, false, &c, nullptr, 0, 0.5, 2);
  CHECK(lqrWeightOffsetU(pc) == 6 && lqrWeightOffsetXf(pc) == 10 && lqrWeightDoubles(pc) == 16);
  std::vector<double> wc((size_t)lqrWeightDoubles(pc), -1.0);
  lqrWeights(pc, wc.data());
  CHECK(wc[0] == 0.5 * c.q_weight[0] && wc[5] == 0.5 * c.v_weight[2] && wc[6] == 0.5 * c.u_weight[0] && wc[8] == 0.5 * c.u_weight[2] && wc[9] == 0.0);
  CHECK(wc[10] == c.qf_weight[0] && wc[15] == c.vf_weight[2]);
}

int main() {
  refusals();
  weights();
  if (failures) { std::printf("rbd gradient plan: %d FAILED\n", failures); return 1; }
  std::printf("rbd gradient plan: ok\n");
  return 0;
}
