// The chunk plan of the forward-dynamics derivatives (idocp_amd/csrc/rbd_fdd_plan.hpp) held to its rule on the CPU, as a stand-alone program for
// the address and undefined-behaviour sanitizers (tests/test_rbd_fd_derivatives_host.py builds and runs it, and holds the same plan to its
// Python statement through the numbers printed here).  The rule, restated sample by sample:
//   every sample 0 .. n - 1 lies in exactly one pass, the passes are consecutive and none is empty;
//   no pass has more samples than the scratch has room for, than the caller's limit allows, or than n;
//   the arrays of a pass do not overlap and end at `total`; total <= cap unless one sample alone is larger.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rbd_fdd_plan.hpp"

using idocp_host::FddPlan;

namespace {

int failures = 0;

void expect(bool ok, const char* what, long a = -1, long b = -1) {
  if (!ok) { std::printf("FAILED: %s (%ld, %ld)\n", what, a, b); ++failures; }
}

void hold(int nv, int nf, int n, int limit, size_t cap) {
  const FddPlan p = idocp_host::fddPlan(nv, nf, n, limit, cap);
  const size_t V = (size_t)nv, F = (size_t)nf;
  const size_t per = V + F + (nf ? 0 : V) + 2 * V * V + 2 * F * V + (V + F) * (V + F);
  expect(p.per_sample == per, "per_sample", n, limit);
  expect(p.chunk >= 1 && p.chunk <= n, "1 <= chunk <= n", n, p.chunk);
  expect(limit <= 0 || p.chunk <= limit, "chunk <= limit", limit, p.chunk);
  expect((size_t)p.chunk * per <= cap || p.chunk == 1, "the scratch fits the cap", n, p.chunk);
  // the largest chunk the three bounds allow
  const bool room = (size_t)(p.chunk + 1) * per <= cap;
  expect(p.chunk == n || (limit > 0 && p.chunk == limit) || !room, "chunk is not smaller than it has to be", n, p.chunk);
  // every sample once
  std::vector<int> seen((size_t)n, 0);
  int next = 0;
  for (int i = 0; i < p.nchunks; ++i) {
    expect(p.first(i) == next, "passes are consecutive", i, p.first(i));
    const int cnt = p.count(i, n);
    expect(cnt >= 1 && cnt <= p.chunk, "a pass is neither empty nor too long", i, cnt);
    for (int s = p.first(i); s < p.first(i) + cnt && s < n; ++s) ++seen[(size_t)s];
    next = p.first(i) + cnt;
  }
  expect(next == n, "the passes end at n", next, n);
  for (int s = 0; s < n; ++s) expect(seen[(size_t)s] == 1, "every sample in exactly one pass", s, seen[(size_t)s]);
  // the arrays of a pass, in the order of the header, back to back
  const size_t C = (size_t)p.chunk;
  const size_t off[8] = {p.a, p.f, p.tau, p.dtau_dq, p.dtau_dv, p.dCdq, p.dCdv, p.MJtJinv};
  const size_t size[8] = {C * V, C * F, nf ? 0 : C * V, C * V * V, C * V * V, C * F * V, C * F * V, C * (V + F) * (V + F)};
  size_t at = 0;
  for (int i = 0; i < 8; ++i) { expect(off[i] == at, "arrays lie back to back", i, (long)off[i]); at += size[i]; }
  expect(p.total == at && p.total == C * per, "total", (long)p.total, (long)at);
}

}  // namespace

int main() {
  const size_t cap = idocp_host::FDD_SCRATCH_CAP_DOUBLES;
  expect(cap * sizeof(double) == (size_t(256) << 20), "the cap is 256 MiB");
  const int ns[] = {1, 2, 3, 64, 131, 1024, 16693, 16694, 16695, 122880, 1000000};
  const int limits[] = {0, -1, 1, 2, 50, 64, 130, 131, 132, 100000};
  for (int n : ns)
    for (int limit : limits) {
      hold(18, 12, n, limit, cap);                                    // the quadruped
      for (int nv = 2; nv <= 8; ++nv) hold(nv, 0, n, limit, cap);     // the chains
    }
  // small caps: the cut falls inside a small call; a cap below one sample still makes progress, one sample at a time
  const size_t caps[] = {1, 2009, 2010, 2011, 4019, 4020, 131 * 2010 - 1, 131 * 2010};
  for (size_t c : caps)
    for (int n : {1, 3, 131})
      for (int limit : {0, 50}) hold(18, 12, n, limit, c);
  // the cases written out (the numbers the Python statement of the rule is held to as well)
  {
    FddPlan p = idocp_host::fddPlan(18, 12, 122880, 0);
    expect(p.per_sample == 2010 && p.chunk == 16693 && p.nchunks == 8, "ANYmal, 122 880 samples", p.chunk, p.nchunks);
    std::printf("plan 18 12 122880 0: chunk %d nchunks %d total %zu\n", p.chunk, p.nchunks, p.total);
    p = idocp_host::fddPlan(18, 12, 131, 50);
    expect(p.chunk == 50 && p.nchunks == 3 && p.count(2, 131) == 31, "131 samples cut at 50", p.chunk, p.nchunks);
    std::printf("plan 18 12 131 50: chunk %d nchunks %d total %zu\n", p.chunk, p.nchunks, p.total);
    p = idocp_host::fddPlan(7, 0, 131, 0);
    expect(p.per_sample == 7 + 7 + 3 * 49 && p.chunk == 131 && p.nchunks == 1, "a chain in one pass", p.chunk, p.nchunks);
    std::printf("plan 7 0 131 0: chunk %d nchunks %d total %zu\n", p.chunk, p.nchunks, p.total);
  }
  if (failures) { std::printf("rbd fdd plan: %d failures\n", failures); return EXIT_FAILURE; }
  std::printf("rbd fdd plan: ok\n");
  return EXIT_SUCCESS;
}
