// Which form of a kernel an OCPSolver / ParNMPCSolver handle runs: the per-handle record and the rules that resolve it.
// Host-only and free of HIP, so that a plain C++ program can include it (tests/cpp/ocp_forms.cpp holds the rules).
#ifndef IDOCP_OCP_FORMS_HPP_
#define IDOCP_OCP_FORMS_HPP_

namespace idocp_dev {

// longest chain ocp_forward_expand_kernel keeps in LDS (slot, status word, two time steps per node); longer chains run S4 + K6
constexpr int OcpForwardExpandMaxChain = 320;

// Fork / join inside an iteration: the switching-constraint kernel K5s -- one latency-bound wavefront per stage that carries a switching
// constraint, 0.09 ms on configs[2] with most of the chip idle -- runs on a stream of its own next to the nominal sweeps K5n.  A batch of
// instances only: at batch 1 the two event hand-offs cost more than the 9 wavefronts of K5s (1.09 against 1.06 ms per iteration).
constexpr int OcpSideStreamMinBatch = 128;
// The forward sweep that expands as it walks (ocp_forward_expand_kernel) pays when the stage-parallel expansion it absorbs is bandwidth: a
// batch of instances.  A few instances are the opposite case -- K6 spreads their stages over the whole chip while the fused walk strings the
// expansion of all stages of an instance onto one wavefront's chain -- so small batches keep S4 + K6 (latency mode).  Measured on
// configs[2]: S4 + K6 0.315 / 0.405 / 0.587 ms at batch 128 / 256 / 512, the fused walk 0.346 / 0.356 / 0.447.
constexpr int OcpFusedForwardMinBatch = 192;
// The backward sweep of a handful of instances (latency mode: one reference solver object is batch 1) runs eight wavefronts per instance --
// measured on configs[2]: 0.79 / 0.83 against 0.855 / 0.858 ms at batch 1 / 16, 0.88 against 0.86 at 64.
constexpr int OcpWideSweepMaxBatch = 16;

struct OcpForms {
  int side_stream = -1;        // idocp_ocp_set_side_stream: -1 by batch size, 0 everything on the handle's stream, 1 K5s (and K7b) on a stream of their own
  int fused_forward = -1;      // idocp_ocp_set_fused_forward: -1 by batch size, 0 S4 + K6, 1 the fused forward sweep
  int riccati_wide = -1;       // idocp_ocp_set_riccati_sweep: -1 by batch size, 0 one wavefront per instance (register-resident), 1 eight per instance
  int prof_dimf = 12;          // diagnostic: the K5 stage class (contact rows) that writes the clock stamps
  int general_axes = 0;        // tests: the general rigid-body instantiations on a model that qualifies for the special ones
};

inline bool byMode(int mode, bool by_batch) { return mode >= 0 ? mode != 0 : by_batch; }

// ParNMPC has no K5s / K7 fork: never a side stream
inline bool useSideStream(const OcpForms& f, int batch, bool parnmpc) { return !parnmpc && byMode(f.side_stream, batch >= OcpSideStreamMinBatch); }
// M = length of the chain; a chain the walk cannot keep in LDS runs S4 + K6 whatever the mode says
inline bool useFusedForward(const OcpForms& f, int batch, int M) { return M <= OcpForwardExpandMaxChain && byMode(f.fused_forward, batch >= OcpFusedForwardMinBatch); }
inline bool useWideSweep(const OcpForms& f, int batch) { return byMode(f.riccati_wide, batch <= OcpWideSweepMaxBatch); }

}  // namespace idocp_dev
#endif  // IDOCP_OCP_FORMS_HPP_
