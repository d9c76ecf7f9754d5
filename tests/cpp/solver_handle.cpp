// detail::OwnedHandle (include/idocp/detail/solver_core.hpp), the owner behind the copy and move of the four solver facades, on a stub handle
// type: every special member on null and on live owners, with the clone and destroy calls counted.  Needs neither the library nor a device;
// built with the address and undefined-behaviour sanitizers, so a double destroy or a leaked clone ends the program.
//   usage: solver_handle               -> every case; "all checks passed"
//          solver_handle clone_fails   -> a clone that fails: the error text on stderr, EXIT_FAILURE
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>

#include "idocp/detail/solver_core.hpp"

extern "C" const char* idocp_last_error(void) { return "stub: clone refused"; }      // (the one symbol of the library the owner needs)

namespace {
int g_alive = 0;      // stub objects in existence
struct Stub {
  int value;
  explicit Stub(int v) : value(v) { ++g_alive; }
  Stub(const Stub& other) : value(other.value) { ++g_alive; }
  ~Stub() { --g_alive; }
};
int g_made = 0, g_clones = 0, g_destroys = 0;
bool g_clone_fails = false;
std::string g_calls;      // 'c' per clone, 'd' per destroy, in order

Stub* make(int value) { ++g_made; return new Stub(value); }
int stubClone(Stub* src, Stub** out) {
  if (g_clone_fails) return IDOCP_E_ARG;
  *out = new Stub(*src);
  ++g_clones; g_calls += 'c';
  return IDOCP_OK;
}
void stubDestroy(Stub* p) { delete p; ++g_destroys; g_calls += 'd'; }
using Owner = idocp::detail::OwnedHandle<Stub, stubClone, stubDestroy>;

// made + clones - destroys, which must be the number of stubs in existence at every step (-1 otherwise)
int live() { return g_made + g_clones - g_destroys == g_alive ? g_alive : -1; }
}  // namespace

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static int run() {
  {
    Owner a;                                          // default construction: null, no call
    REQUIRE(!a && a.get() == nullptr && live() == 0 && g_calls.empty());
    Owner b(a);                                       // copy of null: null, no call
    REQUIRE(!b && g_calls.empty());
    Owner c(make(7));                                 // construction from a pointer: owns it, no clone
    REQUIRE(c && c->value == 7 && live() == 1 && g_calls.empty());
    Owner d(c);                                       // copy of live: a deep copy
    REQUIRE(d && d.get() != c.get() && d->value == 7 && live() == 2 && g_calls == "c");
    Stub* const was = d.get();
    Owner e(std::move(d));                            // move: steals, leaves null
    REQUIRE(e.get() == was && !d && live() == 2 && g_calls == "c");
    a = c;                                            // copy assignment null <- live
    REQUIRE(a && a.get() != c.get() && a->value == 7 && live() == 3 && g_calls == "cc");
    a = b;                                            // live <- null: destroys, no clone
    REQUIRE(!a && live() == 2 && g_calls == "ccd");
    a = c;
    a->value = 1;
    g_calls.clear();
    a = e;                                            // live <- live: clones FIRST, then destroys its own
    REQUIRE(a->value == 7 && a.get() != e.get() && live() == 3 && g_calls == "cd");
    Stub* const stolen = e.get();
    a = std::move(e);                                 // move assignment onto a live owner: destroys its own, steals
    REQUIRE(a.get() == stolen && !e && live() == 2 && g_calls == "cdd");
    Owner& self = a;
    a = self;                                         // self copy-assignment: nothing happens
    REQUIRE(a.get() == stolen && live() == 2 && g_calls == "cdd");
    a = std::move(self);                              // self move-assignment: nothing happens
    REQUIRE(a.get() == stolen && a->value == 7 && live() == 2 && g_calls == "cdd");
    {
      Owner f(make(3)), g(std::move(f));              // destruction of a moved-from owner: no call
      g_calls.clear();
    }
    REQUIRE(live() == 2 && g_calls == "d");
    e = std::move(a);                                 // a moved-from owner is assigned again and used
    d = e;
    REQUIRE(!a && e.get() == stolen && d->value == 7 && live() == 3);
  }
  REQUIRE(live() == 0 && g_clones + g_made == g_destroys);      // every stub made or cloned was destroyed once
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "clone_fails") == 0) {
    Owner a(make(1));
    g_clone_fails = true;
    Owner b(a);                                       // exits: idocp_last_error() on stderr, EXIT_FAILURE
    std::printf("not reached\n");
    return 0;
  }
  if (run()) return 2;
  std::printf("all checks passed\n");
  return 0;
}
