// The scratch of the forward-dynamics derivatives (idocp_rbd_forward_dynamics_derivatives_batch; rbd_capi.hip) and how the sample axis is cut to
// fit it.  Plain C++17 without a HIP call, so that a CPU program can hold the rule to its cases (tests/cpp/rbd_fdd_plan.cpp).
//
// Per sample the composition keeps, between its launches: the forward solution a [nv] and f [nf], and of the inverse call at (q, v, a, f)
// tau [nv] (chains only: their sweep always writes it), dtau_dq, dtau_dv [nv * nv], dCdq, dCdv [nf * nv] and the slot of MJtJinv
// [(nv + nf)^2] (a chain: M = dtau_da [nv * nv]).  The rule:
//   chunk   = min(n, max(1, cap / per_sample), limit > 0 ? limit : n)        samples per pass; `limit` is the caller's own bound (0: none)
//   nchunks = ceil(n / chunk); pass i takes the samples [i chunk, min(n, (i + 1) chunk))
//   the scratch holds chunk * per_sample doubles: never more than the cap (unless ONE sample exceeds it), and it only depends on chunk
// Every array of a pass lies behind the previous one, [chunk][its size].
#pragma once

#include <cstddef>

namespace idocp_host {

constexpr size_t FDD_SCRATCH_CAP_DOUBLES = (size_t(256) << 20) / sizeof(double);      // 256 MiB whatever n is

struct FddPlan {
  int chunk = 0, nchunks = 0;
  size_t per_sample = 0, total = 0;                                     // doubles
  size_t a = 0, f = 0, tau = 0, dtau_dq = 0, dtau_dv = 0, dCdq = 0, dCdv = 0, MJtJinv = 0;      // offsets of the arrays of a pass, doubles
  int first(int i) const { return i * chunk; }                         // first sample of pass i
  int count(int i, int n) const { const int left = n - i * chunk; return left < chunk ? left : chunk; }
};

// nv, nf = 3 ncontacts (0 on a chain), n >= 1 samples, limit: the caller's own bound on the samples of a pass (<= 0: none)
inline FddPlan fddPlan(int nv, int nf, int n, int limit, size_t cap = FDD_SCRATCH_CAP_DOUBLES) {
  FddPlan p;
  const size_t V = (size_t)nv, F = (size_t)nf;
  const size_t sizes[8] = {V, F, nf ? 0 : V, V * V, V * V, F * V, F * V, (V + F) * (V + F)};
  for (size_t s : sizes) p.per_sample += s;
  size_t fit = cap / p.per_sample;
  if (fit < 1) fit = 1;
  size_t chunk = (size_t)n < fit ? (size_t)n : fit;
  if (limit > 0 && (size_t)limit < chunk) chunk = (size_t)limit;
  p.chunk = (int)chunk;
  p.nchunks = (int)(((size_t)n + chunk - 1) / chunk);
  size_t* const offsets[8] = {&p.a, &p.f, &p.tau, &p.dtau_dq, &p.dtau_dv, &p.dCdq, &p.dCdv, &p.MJtJinv};
  size_t at = 0;
  for (int i = 0; i < 8; ++i) { *offsets[i] = at; at += chunk * sizes[i]; }
  p.total = at;
  return p;
}

}  // namespace idocp_host
