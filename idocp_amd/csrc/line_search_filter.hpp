// The filter line search of the four solvers, for a batch of instances: LineSearch::computeStepSize (include/idocp/line_search/line_search.hpp:62-92,
// unline_search.hpp:62-92) over LineSearchFilter (src/line_search/line_search_filter.cpp:33-63).  Host-only and free of HIP, so that a plain C++
// program can include it (tests/cpp/line_search_filter.cpp holds the batch driver to the scalar loop of the reference).
#ifndef IDOCP_LINE_SEARCH_FILTER_HPP_
#define IDOCP_LINE_SEARCH_FILTER_HPP_

#include <algorithm>
#include <utility>
#include <vector>

namespace idocp_host {

constexpr double FilterCostReductionRate = 0.005;          // line_search_filter.hpp:16
constexpr double FilterConstraintsReductionRate = 0.005;   // line_search_filter.hpp:17
constexpr double StepSizeReductionRate = 0.75;             // line_search.hpp:25
constexpr double MinStepSize = 0.05;                       // line_search.hpp:26

// the (cost, constraint violation) pairs that no later iterate may be dominated by
struct LineSearchFilter {
  std::vector<std::pair<double, double>> points;
  bool accepts(double cost, double violation) const {
    for (const auto& p : points) if (cost >= p.first && violation >= p.second) return false;
    return true;
  }
  void augment(double cost, double violation) {
    for (auto it = points.begin(); it != points.end();) { if (cost <= it->first && violation <= it->second) it = points.erase(it); else ++it; }
    points.push_back({cost - FilterCostReductionRate * violation, (1 - FilterConstraintsReductionRate) * violation});
  }
  void clear() { points.clear(); }
  bool empty() const { return points.empty(); }
};

// step[stride * b]: in, the maximum primal step of instance b; out, its accepted step.  eval(alpha, cv) evaluates the trial iterates
// s + alpha[b] d of the WHOLE batch -- cv[2 b] = cost, cv[2 b + 1] = violation -- and returns a status; it alone knows about a device.  Every
// probe is one call: an instance that has finished keeps its last alpha and its result is ignored, so the number of probes is that of the slowest
// instance (+ one at alpha = 0 when some filter is empty: "if filter is empty, augment the current solution to the filter").  A non-zero status
// of eval ends the search and is returned; `step` is then untouched (the filters keep what earlier probes put there).
template <typename Eval>
int filterLineSearch(std::vector<LineSearchFilter>& filters, double* step, int stride, Eval&& eval) {
  const int B = (int)filters.size();
  std::vector<double> alpha(B, 0.0), cv;
  if (std::any_of(filters.begin(), filters.end(), [](const LineSearchFilter& f) { return f.empty(); })) {
    if (const int rc = eval(alpha, cv)) return rc;
    for (int b = 0; b < B; ++b) if (filters[b].empty()) filters[b].augment(cv[2 * b], cv[2 * b + 1]);
  }
  std::vector<char> done(B, 0);
  int open = 0;
  for (int b = 0; b < B; ++b) { alpha[b] = step[stride * b]; if (!(alpha[b] > MinStepSize)) done[b] = 1; else ++open; }      // (a NaN step is finished too)
  while (open > 0) {
    if (const int rc = eval(alpha, cv)) return rc;
    for (int b = 0; b < B; ++b) {
      if (done[b]) continue;
      if (filters[b].accepts(cv[2 * b], cv[2 * b + 1])) { filters[b].augment(cv[2 * b], cv[2 * b + 1]); done[b] = 1; --open; continue; }
      alpha[b] *= StepSizeReductionRate;
      if (!(alpha[b] > MinStepSize)) { done[b] = 1; --open; }
    }
  }
  for (int b = 0; b < B; ++b) step[stride * b] = alpha[b] > MinStepSize ? alpha[b] : MinStepSize;
  return 0;
}

}  // namespace idocp_host
#endif  // IDOCP_LINE_SEARCH_FILTER_HPP_
