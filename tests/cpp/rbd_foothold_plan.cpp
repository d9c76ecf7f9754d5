// The schedule of the foothold rollout (idocp_amd/csrc/rbd_foothold_plan.hpp) held to its rule on the CPU, as a stand-alone program for the
// address and undefined-behaviour sanitizers (tests/test_rbd_kinematics_host.py builds and runs it).  The rule is restated here contact by
// contact from include/idocp_hip.h, not through the header's mask arithmetic:
//   stays(k, c) = active[k][c] && (k > 0 ? active[k - 1][c] : !latch_first)
//   impulse(k, c) = touchdown_impulse && k > 0 && active[k][c] && !active[k - 1][c]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rbd_foothold_plan.hpp"

using idocp_host::FootholdStep;

namespace {

int failures = 0;

void expect(bool ok, const char* what, int a = -1, int b = -1) {
  if (!ok) { std::printf("FAILED: %s (%d, %d)\n", what, a, b); ++failures; }
}

// every step of a schedule against the rule, for both values of the two switches
void hold(const std::vector<int>& active, int nc, const char* name) {
  const int steps = (int)(active.size() / nc);
  for (int impulse = 0; impulse < 2; ++impulse)
    for (int latch_first = 0; latch_first < 2; ++latch_first)
      for (int k = 0; k < steps; ++k) {
        const FootholdStep s = idocp_host::footholdStep(active.data(), nc, k, impulse != 0, latch_first != 0);
        for (int c = 0; c < nc; ++c) {
          const bool now = active[k * nc + c] != 0, before = k > 0 && active[(k - 1) * nc + c] != 0;
          const bool stays = now && (k > 0 ? before : !latch_first);
          expect(((s.stage >> c) & 1) == (now ? 1 : 0), name, k, c);
          expect(((s.carry >> c) & 1) == (stays ? 1 : 0), name, k, c);
          expect(((s.impulse >> c) & 1) == ((impulse && k > 0 && now && !before) ? 1 : 0), name, k, c);
        }
        expect((s.stage >> nc) == 0 && (s.carry >> nc) == 0 && (s.impulse >> nc) == 0, "no bit beyond the contacts", k);
        expect((s.carry & ~s.stage) == 0 && (s.impulse & ~s.stage) == 0 && (s.carry & s.impulse) == 0, "carry and impulse are disjoint parts of stage", k);
      }
  bool any = false;
  for (int x : active) any = any || x != 0;
  expect(idocp_host::footholdAnyActive(active.data(), nc, steps) == any, "footholdAnyActive");
}

}  // namespace

int main() {
  // lift-off of the diagonal pair, touchdown, and a contact (1) that opens once more and re-closes
  hold({1, 1, 1, 1,  1, 1, 1, 1,  0, 1, 1, 0,  0, 1, 1, 0,  1, 1, 1, 1,  1, 0, 1, 1,  1, 1, 1, 1}, 4, "trot");
  // flight: all-open steps in the middle, at the start and at the end
  hold({1, 1, 1, 1,  0, 0, 0, 0,  0, 0, 0, 0,  1, 1, 1, 1}, 4, "jump");
  hold({0, 0, 0, 0,  1, 0, 0, 1,  0, 0, 0, 0}, 4, "flight at both ends");
  hold({0, 0, 0, 0,  0, 0, 0, 0}, 4, "never closed");
  // steps = 1: the switches alone decide
  hold({1, 1, 1, 1}, 4, "one step, closed");
  hold({1, 0, 1, 0}, 4, "one step, half");
  hold({0, 0, 0, 0}, 4, "one step, open");
  // values other than 1 count as active; fewer contacts than four
  hold({2, 0, -1,  0, 5, 1}, 3, "truthy");
  hold({1,  0,  1,  1}, 1, "one contact");

  // the cases of the rule written out
  {
    const int a[] = {1, 1, 1, 1,  1, 0, 0, 1,  1, 1, 1, 1};
    FootholdStep s = idocp_host::footholdStep(a, 4, 0, true, false);
    expect(s.stage == 15 && s.impulse == 0 && s.carry == 15, "k = 0, latch_first = 0: the caller's points stay");
    s = idocp_host::footholdStep(a, 4, 0, true, true);
    expect(s.stage == 15 && s.impulse == 0 && s.carry == 0, "k = 0, latch_first = 1: every point is latched, no impulse at step 0");
    s = idocp_host::footholdStep(a, 4, 1, true, true);
    expect(s.stage == 9 && s.impulse == 0 && s.carry == 9, "lift-off: the closed contacts carry, the open ones track");
    s = idocp_host::footholdStep(a, 4, 2, true, false);
    expect(s.stage == 15 && s.impulse == 6 && s.carry == 9, "touchdown: impulse and latch on the newly active contacts");
    s = idocp_host::footholdStep(a, 4, 2, false, false);
    expect(s.stage == 15 && s.impulse == 0 && s.carry == 9, "touchdown without the impulse");
  }
  if (failures) { std::printf("rbd foothold plan: %d failures\n", failures); return EXIT_FAILURE; }
  std::printf("rbd foothold plan: ok\n");
  return EXIT_SUCCESS;
}
