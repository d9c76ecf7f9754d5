// Host-visible launch wrapper of the batched rigid-body kernel (defined in rbd_batch_kernel.hip).
#ifndef IDOCP_RBD_LAUNCH_HPP_
#define IDOCP_RBD_LAUNCH_HPP_

#include <hip/hip_runtime.h>

#include "dev_rbd.hpp"
#include "idocp_hip.h"
#include "rbd_objective.hpp"

namespace idocp_dev {

// placement of the contact frames in their tip joints (row-major rotation), behind the model in device memory
struct RbdFrames {
  double R[IDOCP_MAX_CONTACTS][9], p[IDOCP_MAX_CONTACTS][3];
};

// One wavefront per sample, RBD_WAVES samples per workgroup.  io: DEVICE pointers; active_mask: bit c = contact c is active.
constexpr int RBD_WAVES = 2;
void rbdBatchQuadruped(const DevModel* m, const RbdFrames* frames, const idocp_rbd_io_t& io, int n, int mode, int active_mask,
                       double time_step, hipStream_t st);

// Forward dynamics (rbd_forward_kernel.hip), same shape of launch.  io: DEVICE pointers.  STAGE: (a, f) from (q, v, u); IMPULSE: (dv, lambda)
// from (q, v); optionally the explicit Euler step over dt.
void rbdForwardQuadruped(const DevModel* m, const RbdFrames* frames, const idocp_rbd_fd_io_t& io, int n, int mode, int active_mask,
                         double time_step, double dt, hipStream_t st);
// Fixed-base chain of nv = 2 .. 8 joints: a = M^-1 (u - h) from h [n][nv] and the column-major M [n][nv * nv] the chain sweep left at a = 0
// (Cholesky solve, one lane per sample), then the step q + dt v, v + dt a.  Any of a, q_next, v_next may be NULL.
void rbdForwardChainSolve(int nv, int n, const double* h, const double* M, const double* q, const double* v, const double* u, double dt,
                          double* a, double* q_next, double* v_next, hipStream_t st);

// The affine feedback policy (rbd_policy_kernel.hip): u [n][nu] = clamp(u_ff + K [q (-) q_ref ; v - v_ref]).  Every pointer: DEVICE memory.
// k_stride, q_ref_stride, v_ref_stride: doubles between the gains / references of two samples -- nu * 2 nv, nq, nv, or 0 where all samples share
// one.  u_ff NULL = 0; K NULL = no feedback (q, v, q_ref, v_ref are not read); u_min / u_max [nu], either may be NULL.
struct RbdPolicyArgs {
  const double *q, *v, *u_ff, *K, *q_ref, *v_ref, *u_min, *u_max;
  long k_stride, q_ref_stride, v_ref_stride;
  double* u;
};
void rbdPolicy(int nv, bool quadruped, const RbdPolicyArgs& a, int n, hipStream_t st);

// The score of a rollout (rbd_score_kernel.hip).  Every pointer: DEVICE memory, step-major slices of the window: q, v [steps (+ 1 if terminal)][n][..],
// u, a, f [steps][n][..] (any of the three may be NULL: its terms are left out), q_ref / v_ref the objective's tables AT the window's first step,
// block the objective's weights and bounds.  masks: 4 bits per step of the window, bit c = contact c is active.  cost, violation [n] and
// stage_cost [steps (+ 1)][n] may be NULL.
struct RbdScoreArgs {
  const double *q, *v, *u, *a, *f, *q_ref, *v_ref;
  const idocp_host::RbdScoreBlock* block;
  double *cost, *violation, *stage_cost;
  int steps, terminal, accumulate;
  unsigned masks[idocp_host::RBD_SCORE_MASK_WORDS];
};
void rbdScore(int nv, bool quadruped, const RbdScoreArgs& a, int n, hipStream_t st);

// Sampling around a torque sequence (rbd_sample_kernel.hip).  Every pointer: DEVICE memory.  Workgroups of RBD_SAMPLE_THREADS lanes; a chunk is
// IDOCP_RBD_REDUCE_CHUNK consecutive samples, nchunks = ceil(n / chunk).  scratch: RBD_PARTIAL_STRIDE doubles per (row, chunk) -- the column
// partials of the mean with the chunk's weight sum in the last place; the weights call (rows = 1) keeps its five arrays of nchunks doubles there.
constexpr int RBD_SAMPLE_THREADS = 256;
constexpr int RBD_PARTIAL_STRIDE = IDOCP_RBD_MEAN_MAX_COLUMNS + 1;
// u_samples [steps][n][nu] = clamp(u_nominal [steps][nu] + sigma [nu] z); u_min / u_max [nu], either may be NULL.  One launch.
struct RbdPerturbArgs {
  const double *u_nominal, *sigma, *u_min, *u_max;
  double* u_samples;
  unsigned long long seed;
  unsigned draw;
  int n, nu, first_step, steps;
};
void rbdPerturb(const RbdPerturbArgs& a, hipStream_t st);
// weights [n] and stats [IDOCP_RBD_WEIGHT_STATS] from cost [n] and violation [n] (NULL: left out).  Four launches.
struct RbdWeightArgs {
  const double *cost, *violation;
  double penalty, temperature;
  double *weights, *stats, *scratch;
  int n, nchunks;
};
void rbdWeights(const RbdWeightArgs& a, hipStream_t st);
// mean [rows][m] of x [rows][n][m] under weights [n], 1 <= m <= IDOCP_RBD_MEAN_MAX_COLUMNS; rows * nchunks workgroups.  Two launches.
struct RbdMeanArgs {
  const double *weights, *x;
  double *mean, *scratch;
  int n, rows, m, nchunks;
};
void rbdMean(const RbdMeanArgs& a, hipStream_t st);

// Contact-frame kinematics (rbd_kinematics_kernel.hip).  One lane per (sample, leg), RBD_KIN_THREADS / 4 samples per workgroup, any n.
// io: DEVICE pointers; a NULL output is neither computed nor stored.  One launch.
constexpr int RBD_KIN_THREADS = 256;
void rbdKinematicsQuadruped(const DevModel* m, const RbdFrames* frames, const idocp_rbd_kin_io_t& io, int n, hipStream_t st);
// The latch step of the foothold rollout, the same kernel: points [n][nc][3] = carry bit c ? prev[i][c] : p_c(q[i]).  prev NULL: a carried
// entry of `points` is left as it is.  One launch.
void rbdLatchQuadruped(const DevModel* m, const RbdFrames* frames, const double* q, const double* prev, double* points, int carry_mask, int n,
                       hipStream_t st);

// Derivatives of the forward dynamics (rbd_fd_derivatives_kernel.hip): the last launch of the composition.  Every pointer: DEVICE memory.  Reads the
// forward solution a [n][nv], f [n][nf] and the terms of the inverse call at (q, v, a, f) -- dtau_dq, dtau_dv [n][nv * nv], dCdq, dCdv
// [n][nf * nv], the slots of MJtJinv [n][(nv + nf)^2]; on a chain MJtJinv is M = dtau_da [n][nv * nv] and f, dCdq, dCdv are not read -- and v
// and q for the retraction and the correction of dC (the kernel's head has it); writes the outputs that are not NULL.  One launch, one wavefront per sample (chain: one lane per sample), any n.
struct RbdFddArgs {
  const double *q, *v, *a, *f, *dtau_dq, *dtau_dv, *dCdq, *dCdv, *MJtJinv;
  double *a_out, *f_out, *da_dq, *da_dv, *da_du, *df_dq, *df_dv, *df_du, *A, *B;
  double dt;
};
void rbdFddQuadruped(const DevModel* m, const RbdFrames* frames, const RbdFddArgs& a, int n, int mode, int active_mask, hipStream_t st);
void rbdFddChain(int nv, const RbdFddArgs& a, int n, hipStream_t st);
// The impulse product of the rollout linearisation, the same file: A [n][nx * nx] = E A and B [n][nx * nu] = E B in place, E [n][nx * nx], all
// column-major, nx <= 36, nu <= 12; A or B may be NULL.  One wavefront per sample, fixed order of summation.  One launch.
void rbdFddImpulseProduct(int nx, int nu, const double* E, double* A, double* B, int n, hipStream_t st);

// The backward pass of time-varying LQR over a linearised rollout (rbd_lqr_kernel.hip; the arrays of idocp_rbd_lqr_io_t).  Every pointer: DEVICE
// memory.  nx = 2 nv, nu: 36, 12 on the quadruped, at most 16, 8 on a chain.  lx and lu: both or neither; an output that is NULL is not stored.
// One wavefront per sample, RBD_LQR_WAVES samples per workgroup, any n.  One launch.
constexpr int RBD_LQR_WAVES = 1;
struct RbdLqrArgs {
  const double *A, *B, *x_weight, *u_weight, *xf_weight, *lx, *lu;
  double regularization;
  double *K, *k, *P0, *p0, *expected;
  int* status;
  int n, steps, nx, nu;
};
void rbdLqrBackward(bool quadruped, const RbdLqrArgs& a, hipStream_t st);
// The same recursion with G_k^T G_k added to the stage Hessian (idocp_rbd_lqr_backward_gn): G [steps][n][g_rows][nx + nu] row-major, g_rows a
// multiple of 4.  Another template form of the same kernel; the form above keeps its arguments and its code.  One launch.
struct RbdLqrGnArgs : RbdLqrArgs {
  const double* G;
  int g_rows;
};
void rbdLqrBackwardGn(bool quadruped, const RbdLqrGnArgs& a, hipStream_t st);
// The GN form with a per-sample per-stage diagonal (idocp_rbd_lqr_backward_gn_diag): D [steps][n][nx + nu] is added to the diagonal of the stage
// Hessian where wx / wu are.  A third template form (rbd_lqr_gn_diag_kernel.hip); the two forms above keep their code.  One launch.
struct RbdLqrGnDiagArgs : RbdLqrGnArgs {
  const double* D;
};
void rbdLqrBackwardGnDiag(bool quadruped, const RbdLqrGnDiagArgs& a, hipStream_t st);

// The residual rows of the acceleration and contact-force terms (rbd_residual_kernel.hip; idocp_rbd_linearize_rollout_cost).  Every pointer: DEVICE
// memory.  One pass of one step: `count` samples whose forward solution a [count][nv], f [count][nf] and column-major derivative blocks da_dq, da_dv
// [count][nv * nv], da_du [count][nv * nu], df_dq, df_dv [count][nf * nv], df_du [count][nf * nu] lie in scratch (16-byte aligned pieces); table: the
// 2 R doubles of idocp_host::residualTable; mask: bit c = contact c is active at the step.  G [count][R][nz] row-major, rho [count][R], lx
// [count][2 nv] and lu [count][nu] are the slices of the pass; lx and lu HOLD the diagonal part and gain G^T rho.  An output that is NULL is not stored.
// One workgroup per RBD_RESIDUAL_SAMPLES consecutive samples (quadruped) or RBD_RESIDUAL_SAMPLES_CHAIN (chain), any count.  One launch.
// Returns false, having launched nothing, for a chain outside 2 .. 8 joints.
constexpr int RBD_RESIDUAL_THREADS = 256, RBD_RESIDUAL_SAMPLES = 2, RBD_RESIDUAL_SAMPLES_CHAIN = 16;
struct RbdResidualArgs {
  const double *a, *f, *da_dq, *da_dv, *da_du, *df_dq, *df_dv, *df_du, *table;
  double *G, *rho, *lx, *lu;
  int count, mask;
};
bool rbdResidual(int nv, bool quadruped, const RbdResidualArgs& a, hipStream_t st);
// The penalty form (rbd_residual_penalty_kernel.hip; idocp_rbd_linearize_rollout_penalty): the same pass also writes the rc constraint rows behind
// the R cost rows -- G [count][R + rc][nz], rho [count][R + rc] --, D [count][nz] and the diagonal gradient terms.  q [count][nq], v [count][nv],
// u [count][nu] or NULL: the slices of the rollout (read where their limits are switched on); block: the objective's; scale = sqrt(dt mu),
// dtmu = dt mu; rc = idocp_host::constraintRows (0: no constraint rows).  lx, lu as above (either may be NULL).  One launch.
struct RbdResidualPenaltyArgs : RbdResidualArgs {
  const double *q, *v, *u;
  const idocp_host::RbdScoreBlock* block;
  double* D;
  double scale, dtmu;
  int rc;
};
bool rbdResidualPenalty(int nv, bool quadruped, const RbdResidualPenaltyArgs& a, hipStream_t st);

// The squared-hinge penalty of a rollout (rbd_penalty_kernel.hip; idocp_rbd_score_penalty).  Every pointer: DEVICE memory, the slices of the window:
// q, v, u, a, f [steps][n][..], any may be NULL where no enabled row reads it; masks as for the score; sq [n], in / out with accumulate.
// One wavefront per sample.  One launch.  Returns false, having launched nothing, for a chain outside 2 .. 8 joints.
struct RbdPenaltyArgs {
  const double *q, *v, *u, *a, *f;
  const idocp_host::RbdScoreBlock* block;
  double* sq;
  int steps, accumulate;
  unsigned masks[idocp_host::RBD_SCORE_MASK_WORDS];
};
bool rbdPenalty(int nv, bool quadruped, const RbdPenaltyArgs& a, int n, hipStream_t st);

// The augmented-Lagrangian forms (rbd_al_kernel.hip, rbd_residual_al_kernel.hip; idocp_rbd_score_al, idocp_rbd_multiplier_update,
// idocp_rbd_linearize_rollout_al).  lambda: the window's [steps][n][L] multipliers, L = idocp_host::multiplierRows, or NULL (all zeros); mu > 0.
// Score: sq [n] as above, of the shifted rows.  Update: lambda_out [steps][n][L] (may be lambda), infeasibility and change [n] or NULL, running maxima
// with accumulate.  One wavefront per sample.  One launch each.  Both return false, having launched nothing, for a chain outside 2 .. 8 joints.
struct RbdAlArgs : RbdPenaltyArgs {
  const double* lambda;
  double penalty;      // mu (RbdScoreBlock::mu is the friction coefficient)
  double *lambda_out, *infeasibility, *change;
};
bool rbdAlScore(int nv, bool quadruped, const RbdAlArgs& a, int n, hipStream_t st);
bool rbdAlUpdate(int nv, bool quadruped, const RbdAlArgs& a, int n, hipStream_t st);
// The AL form of the residual pass: the penalty form with every constraint row evaluated at its shifted value.  lambda: the pass's slice
// [count][L] or NULL; penalty: mu.
struct RbdResidualAlArgs : RbdResidualPenaltyArgs {
  const double* lambda;
  double penalty;
};
bool rbdResidualAl(int nv, bool quadruped, const RbdResidualAlArgs& a, hipStream_t st);

// Gradients of an objective along a rollout (rbd_gradient_kernel.hip; the arrays of idocp_rbd_gradient_io_t).  Every pointer: DEVICE memory;
// q, v [steps (+ 1 if terminal)][n][..], u [steps][n][nu] or NULL, q_ref / v_ref the objective's tables AT the window's first step, block its
// weights; lx [steps (+ 1)][n][2 nv] and lu [steps][n][nu], either may be NULL.  (steps + 1) * n fits an int.  One wavefront per
// RBD_GRADIENT_ITEMS consecutive (slice, sample) pairs, any n.  One launch.
constexpr int RBD_GRADIENT_ITEMS = 64;
struct RbdGradientArgs {
  const double *q, *v, *u, *q_ref, *v_ref;
  const idocp_host::RbdScoreBlock* block;
  double *lx, *lu;
  int n, steps, terminal;
};
void rbdGradient(int nv, bool quadruped, const RbdGradientArgs& a, hipStream_t st);

// The line-search step of iLQR (rbd_ilqr_kernel.hip).  Every pointer: DEVICE memory.
// out [steps][n][nu] = u + alpha[i] k, alpha [n]; alpha[i] == 0 gives u bit for bit.  One launch.
void rbdIlqrStepTorques(const double* u, const double* k, const double* alpha, double* out, int n, int steps, int nu, hipStream_t st);
// The acceptance test per sample and the copy of the accepted samples' slices (idocp_rbd_ilqr_accept_io_t).  dst / src / width: the current and
// the trial array and the doubles per sample and slice of q, v (steps + 1 slices), u, a, f (steps slices); a pair with a NULL pointer or width 0 is
// left out.  A workgroup owns RBD_ILQR_GROUP consecutive samples.  One launch.
constexpr int RBD_ILQR_GROUP = 32;
struct RbdIlqrAcceptArgs {
  double* dst[5];
  const double* src[5];
  int width[5];
  double *cost, *violation, *alpha, *alpha_accepted;
  const double *trial_cost, *trial_violation, *expected;
  int* done;
  double penalty, armijo, shrink, alpha_min;
  int n, steps;
  int wide;      // set by the launcher: bit c = both pointers of pair c are 16-byte aligned
};
void rbdIlqrAccept(RbdIlqrAcceptArgs a, hipStream_t st);
// alpha [n] = 1, done [n] = 0, alpha_accepted [n] = 0: the start of the rounds of one iteration.  One launch.
void rbdIlqrInit(double* alpha, int* done, double* alpha_accepted, int n, hipStream_t st);

}  // namespace idocp_dev
#endif  // IDOCP_RBD_LAUNCH_HPP_
