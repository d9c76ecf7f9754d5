// C-ABI implementation of the batched rigid-body API (include/idocp_hip.h: idocp_rbd_*).
//
// Host side only: a handle owns the model in device memory, a stream and the staging buffers of the host-pointer form; the terms
// themselves come from rbd_batch_kernel.hip (quadruped) or from the sweep of the fixed-base solvers (UnLaunch<NV>::rneaDerivatives).
// There is NO CPU fallback: without a GPU idocp_rbd_create returns IDOCP_E_DEVICE.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "hip_try.hpp"
#include "host_util.hpp"
#include "idocp_hip.h"
#include "model_shapes.hpp"
#include "rbd_fdd_plan.hpp"
#include "rbd_foothold_plan.hpp"
#include "rbd_launch.hpp"
#include "rbd_stage.hpp"
#include "unocp_launch.hpp"

using namespace idocp_dev;
using idocp_host::set_last_error;
using idocp_host::StagePlan;

// scratch in device memory that only grows: a larger request waits for the stream, frees and allocates anew
struct RbdBuffer {
  double* ptr = nullptr;
  size_t doubles = 0;
  int grow(size_t want, hipStream_t st) {
    if (want <= doubles) return IDOCP_OK;
    if (ptr) { HIP_TRY(hipStreamSynchronize(st)); HIP_TRY(hipFree(ptr)); ptr = nullptr; doubles = 0; }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ptr), sizeof(double) * want));
    doubles = want;
    return IDOCP_OK;
  }
  void release() { if (ptr) (void)hipFree(ptr); }
};

struct idocp_rbd {
  idocp_model_t model;
  int device = 0;
  bool quadruped = false, zaxes = false;
  hipStream_t stream = nullptr;
  void* d_model = nullptr;            // DevModel, then RbdFrames
  const RbdFrames* d_frames = nullptr;
  RbdBuffer stage;                    // host-pointer form: inputs and outputs of one call, laid out by a StagePlan
  RbdBuffer unwanted;                 // chain: where the sweep writes the outputs the caller did not ask for
  RbdBuffer fd_chain;                 // chain, forward dynamics: [a = 0 | h | dtau_dq | dtau_dv | M] of the sweep at a = 0
  RbdBuffer u_buf;                    // closed-loop rollout without u_traj: the torques of the current step, [n][nu]
  RbdBuffer reduce;                   // sampling: the chunk partials of the sums over the sample axis, RBD_PARTIAL_STRIDE per (row, chunk)
  RbdBuffer fdd;                      // forward-dynamics derivatives: what one pass keeps between its launches (rbd_fdd_plan.hpp), at most 256 MiB
  int fdd_limit = 0;                  // idocp_rbd_set_derivatives_chunk (a test hook, not in idocp_hip.h): bound on the samples of a pass (0: none)
  RbdBuffer lin;                      // rollout linearisation at a touchdown: [v_pre [n][nv] | E [n][2 nv * 2 nv]]
  RbdBuffer gn;                       // cost linearisation: a, f and the six derivative blocks of one pass (ResidualPlan), under the cap of `fdd`
};

// the objective of the rollout scoring: the plan of rbd_objective.hpp and its three pieces in ONE block of device memory
struct idocp_rbd_objective {
  idocp_rbd* owner = nullptr;
  idocp_host::RbdObjectivePlan plan;
  double *d_q_ref = nullptr, *d_v_ref = nullptr;      // [steps + 1][nq], [steps + 1][nv]
  idocp_host::RbdScoreBlock* d_block = nullptr;
  std::vector<double> lqr_weights;                    // idocp_host::lqrWeights: [x_weight | u_weight | xf_weight], and the same bits behind the block
  double* d_lqr_weights = nullptr;
  double* d_residual = nullptr;                       // idocp_host::residualTable: [scales | references], 2 R doubles behind the weights
};

namespace {

constexpr size_t MODEL_BYTES = (sizeof(DevModel) + 15) / 16 * 16;

typedef void (*ChainFn)(const DevModel*, int, const double*, const double*, const double*, double*, double*, double*, double*, bool, hipStream_t);
ChainFn chainFn(int nv) {
  switch (nv) {
    case 2: return &UnLaunch<2>::rneaDerivatives;
    case 3: return &UnLaunch<3>::rneaDerivatives;
    case 4: return &UnLaunch<4>::rneaDerivatives;
    case 5: return &UnLaunch<5>::rneaDerivatives;
    case 6: return &UnLaunch<6>::rneaDerivatives;
    case 7: return &UnLaunch<7>::rneaDerivatives;
    case 8: return &UnLaunch<8>::rneaDerivatives;
    default: return nullptr;
  }
}

// ---- the host-pointer form: a StagePlan (rbd_stage.hpp) says what lies where in h->stage and what is copied ----

// room for the plan, its slots bound to it, the inputs on their way up, the zero-filled slots cleared
int stageIn(idocp_rbd* h, const StagePlan& p) {
  int rc = h->stage.grow(p.total(), h->stream); if (rc) return rc;
  double* base = h->stage.ptr;
  p.bind(base);
  for (int i = 0; i < p.n_up; ++i)
    HIP_TRY(hipMemcpyAsync(base + p.up[i].offset, p.up[i].host, sizeof(double) * p.up[i].count, hipMemcpyHostToDevice, h->stream));
  for (int i = 0; i < p.n_zero; ++i) HIP_TRY(hipMemsetAsync(base + p.zero[i].offset, 0, sizeof(double) * p.zero[i].count, h->stream));
  return IDOCP_OK;
}

// the outputs on their way down; returns when they are in place
int stageOut(idocp_rbd* h, const StagePlan& p) {
  for (int i = 0; i < p.n_down; ++i)
    HIP_TRY(hipMemcpyAsync(p.down[i].host, h->stage.ptr + p.down[i].offset, sizeof(double) * p.down[i].count, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

// ---- inverse dynamics ----

const char* const INVERSE = "idocp_rbd_contact_dynamics_batch";      // (both forms report under this name)

int checkCall(const char* who, const idocp_rbd* h, int mode, int n, const int* active, double time_step, const idocp_rbd_io_t* io) {
  const std::string w(who);
  if (!h || !io) { set_last_error(w + ": null handle or io"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (mode != IDOCP_RBD_STAGE && mode != IDOCP_RBD_IMPULSE) { set_last_error(w + ": unknown mode"); return IDOCP_E_ARG; }
  if (!io->q || !io->v || !io->a) { set_last_error(w + ": q, v and a are needed"); return IDOCP_E_ARG; }
  const bool contact_out = io->C || io->dCdq || io->dCdv || io->dCda || io->MJtJinv;
  if (!h->quadruped) {
    if (io->f || io->contact_points || contact_out) {
      set_last_error(w + ": a fixed-base chain has no contacts (f, contact_points and the contact outputs must be NULL)");
      return IDOCP_E_ARG;
    }
    if (mode != IDOCP_RBD_STAGE) { set_last_error(w + ": a fixed-base chain has no impulse mode"); return IDOCP_E_ARG; }
    return IDOCP_OK;
  }
  if (!active) { set_last_error(w + ": the contact status `active` is needed"); return IDOCP_E_ARG; }
  if (mode == IDOCP_RBD_STAGE) {
    if (io->C && !io->contact_points) { set_last_error(w + ": C in STAGE mode needs contact_points"); return IDOCP_E_ARG; }
    if ((io->C || io->dCdq || io->dCdv) && !(time_step > 0.0)) {
      set_last_error(w + ": the Baumgarte terms need a positive time_step"); return IDOCP_E_ARG;
    }
  }
  return IDOCP_OK;
}

int maskOf(const idocp_rbd* h, const int* active) {
  int mask = 0;
  for (int c = 0; c < h->model.ncontacts; ++c) if (active[c]) mask |= 1 << c;
  return mask;
}

// io: device pointers
int launch(idocp_rbd* h, int mode, int n, const int* active, double time_step, const idocp_rbd_io_t& io) {
  HIP_TRY(hipSetDevice(h->device));
  const DevModel* d_m = static_cast<const DevModel*>(h->d_model);
  if (h->quadruped) {
    // (dC/da and MJtJinv do not depend on the Baumgarte time step: any positive number serves where none was given)
    rbdBatchQuadruped(d_m, h->d_frames, io, n, mode, maskOf(h, active), (mode == IDOCP_RBD_STAGE && !(time_step > 0.0)) ? 1.0 : time_step, h->stream);
  } else {
    const size_t nv = h->model.nv, nvec = (size_t)n * nv, nmat = nvec * nv;
    double *tau = io.tau, *dq = io.dtau_dq, *dv = io.dtau_dv, *da = io.dtau_da;
    if (!tau || !dq || !dv || !da) {
      int rc = h->unwanted.grow(nvec + 3 * nmat, h->stream); if (rc) return rc;
      if (!tau) tau = h->unwanted.ptr;
      if (!dq) dq = h->unwanted.ptr + nvec;
      if (!dv) dv = h->unwanted.ptr + nvec + nmat;
      if (!da) da = h->unwanted.ptr + nvec + 2 * nmat;
    }
    chainFn(h->model.nv)(d_m, n, io.q, io.v, io.a, tau, dq, dv, da, h->zaxes, h->stream);
  }
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

// ---- forward dynamics ----

int checkForward(const char* who, const idocp_rbd* h, int mode, int n, const int* active, double dt, const double* q, const double* v, bool contact_args) {
  const std::string w(who);
  if (!h) { set_last_error(w + ": null handle"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (mode != IDOCP_RBD_STAGE && mode != IDOCP_RBD_IMPULSE) { set_last_error(w + ": unknown mode"); return IDOCP_E_ARG; }
  if (!q || !v) { set_last_error(w + ": q and v are needed"); return IDOCP_E_ARG; }
  if (!std::isfinite(dt)) { set_last_error(w + ": dt must be finite"); return IDOCP_E_ARG; }
  if (!h->quadruped) {
    if (contact_args) { set_last_error(w + ": a fixed-base chain has no contacts (f and contact_points must be NULL)"); return IDOCP_E_ARG; }
    if (mode != IDOCP_RBD_STAGE) { set_last_error(w + ": a fixed-base chain has no impulse mode"); return IDOCP_E_ARG; }
    return IDOCP_OK;
  }
  if (!active) { set_last_error(w + ": the contact status `active` is needed"); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

// what a STAGE solve with the given status needs beyond checkForward
int checkStageContacts(const char* who, const idocp_rbd* h, const int* active, double time_step, const double* contact_points) {
  if (!h->quadruped) return IDOCP_OK;
  bool any = false;
  for (int c = 0; c < h->model.ncontacts; ++c) any = any || active[c];
  if (!any) return IDOCP_OK;
  if (!contact_points) { set_last_error(std::string(who) + ": STAGE mode with an active contact needs contact_points"); return IDOCP_E_ARG; }
  if (!(time_step > 0.0) || !std::isfinite(time_step)) {
    set_last_error(std::string(who) + ": STAGE mode with an active contact needs a positive Baumgarte time_step"); return IDOCP_E_ARG;
  }
  return IDOCP_OK;
}

// io: device pointers; quadruped: mask = the contact / impulse status
int launchForward(idocp_rbd* h, int mode, int n, int mask, double time_step, double dt, const idocp_rbd_fd_io_t& io) {
  const DevModel* d_m = static_cast<const DevModel*>(h->d_model);
  if (h->quadruped) {
    rbdForwardQuadruped(d_m, h->d_frames, io, n, mode, mask, time_step, dt, h->stream);
  } else if (io.a || io.q_next || io.v_next) {
    const size_t nv = h->model.nv, nvec = (size_t)n * nv, nmat = nvec * nv;
    int rc = h->fd_chain.grow(2 * nvec + 3 * nmat, h->stream); if (rc) return rc;
    double *zero = h->fd_chain.ptr, *hh = zero + nvec, *dq = hh + nvec, *dv = dq + nmat, *M = dv + nmat;
    if (io.a || io.v_next) {
      HIP_TRY(hipMemsetAsync(zero, 0, sizeof(double) * nvec, h->stream));
      chainFn(h->model.nv)(d_m, n, io.q, io.v, zero, hh, dq, dv, M, h->zaxes, h->stream);
      HIP_TRY(hipGetLastError());
    }
    rbdForwardChainSolve(h->model.nv, n, hh, M, io.q, io.v, io.u, dt, io.a, io.q_next, io.v_next, h->stream);
  }
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int checkForwardCall(idocp_rbd* h, int mode, int n, const int* active, double time_step, double dt, const idocp_rbd_fd_io_t* io) {
  const char* who = "idocp_rbd_forward_dynamics_batch";
  if (!io) { set_last_error(std::string(who) + ": null io"); return IDOCP_E_ARG; }
  int rc = checkForward(who, h, mode, n, active, dt, io->q, io->v, io->f || io->contact_points); if (rc) return rc;
  if (mode == IDOCP_RBD_STAGE) { rc = checkStageContacts(who, h, active, time_step, io->contact_points); if (rc) return rc; }
  return IDOCP_OK;
}

// the schedule of a rollout: per step the stage mask and the mask of the touchdown impulse in front of it (0: none)
int checkRollout(const char* who, idocp_rbd* h, int n, int steps, const int* active, double time_step, double dt, const double* contact_points,
                 const double* q_traj, const double* v_traj, const double* f_traj) {
  if (steps < 1) { set_last_error(std::string(who) + ": steps must be at least 1"); return IDOCP_E_ARG; }
  int rc = checkForward(who, h, IDOCP_RBD_STAGE, n, active, dt, q_traj, v_traj, f_traj || contact_points);
  if (rc) return rc;
  if (h->quadruped)
    for (int k = 0; k < steps; ++k) { rc = checkStageContacts(who, h, active + (size_t)k * h->model.ncontacts, time_step, contact_points); if (rc) return rc; }
  return IDOCP_OK;
}

// ---- the feedback policy ----

// host_bounds: u_min / u_max are host memory and can be looked at
int checkPolicy(const char* who, const idocp_rbd* h, const idocp_rbd_policy_t* pol, bool host_bounds) {
  const std::string w(who);
  if (!pol) { set_last_error(w + ": null policy"); return IDOCP_E_ARG; }
  if (pol->K && (!pol->q_ref || !pol->v_ref)) { set_last_error(w + ": gains K need the references q_ref and v_ref"); return IDOCP_E_ARG; }
  if (host_bounds)
    for (int j = 0; j < h->model.nu; ++j) {
      const bool nan = (pol->u_min && std::isnan(pol->u_min[j])) || (pol->u_max && std::isnan(pol->u_max[j]));
      if (nan || (pol->u_min && pol->u_max && pol->u_min[j] > pol->u_max[j])) {
        set_last_error(w + ": u_min[" + std::to_string(j) + "] <= u_max[" + std::to_string(j) + "] does not hold (or a bound is NaN)"); return IDOCP_E_ARG;
      }
    }
  return IDOCP_OK;
}

// slice k of a policy in device memory, evaluated at (q, v) into u
void launchPolicy(idocp_rbd* h, int n, int k, const idocp_rbd_policy_t& pol, const double* q, const double* v, double* u) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nk = nu * 2 * nv, N = (size_t)n, K = (size_t)k;
  RbdPolicyArgs a;
  a.q = q; a.v = v; a.u = u;
  a.u_ff = pol.u_ff ? pol.u_ff + K * N * nu : nullptr;
  a.k_stride = pol.shared_gains ? 0 : (long)nk;
  a.q_ref_stride = pol.shared_ref ? 0 : (long)nq;
  a.v_ref_stride = pol.shared_ref ? 0 : (long)nv;
  a.K = pol.K ? pol.K + K * (pol.shared_gains ? nk : N * nk) : nullptr;
  a.q_ref = pol.K ? pol.q_ref + K * (pol.shared_ref ? nq : N * nq) : nullptr;
  a.v_ref = pol.K ? pol.v_ref + K * (pol.shared_ref ? nv : N * nv) : nullptr;
  a.u_min = pol.u_min; a.u_max = pol.u_max;
  rbdPolicy(h->model.nv, h->quadruped, a, n, h->stream);
}

int checkTorques(const char* who, const idocp_rbd* h, int n, const double* q, const double* v, const idocp_rbd_policy_t* pol, const double* u,
                 bool host_bounds) {
  const std::string w(who);
  if (!h) { set_last_error(w + ": null handle"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (!q || !v || !u) { set_last_error(w + ": q, v and u are needed"); return IDOCP_E_ARG; }
  return checkPolicy(who, h, pol, host_bounds);
}

// every pointer: device memory.  Open loop (pol == nullptr): the torques u [steps][n][nu].  Closed loop: the torques of step k come from the policy
// at the state of step k and go to slice k of u_traj (or, without u_traj, to the handle's buffer).
int rolloutDevice(idocp_rbd* h, int n, int steps, const int* active, double time_step, double dt, const double* u, const double* contact_points,
                  double* q_traj, double* v_traj, double* a_traj, double* f_traj, int touchdown_impulse, const idocp_rbd_policy_t* pol,
                  double* u_traj, double* latched = nullptr, int latch_first = 0) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n;
  int prev = 0;
  for (int k = 0; k < steps; ++k) {
    int mask = h->quadruped ? maskOf(h, active + (size_t)k * h->model.ncontacts) : 0;
    int touchdown = (touchdown_impulse && k > 0) ? (mask & ~prev) : 0;
    double *qk = q_traj + k * N * nq, *vk = v_traj + k * N * nv;
    if (latched) {
      // the foothold rollout (quadruped): slice k of the contact points before anything of step k reads it (rbd_foothold_plan.hpp)
      const idocp_host::FootholdStep s = idocp_host::footholdStep(active, h->model.ncontacts, k, touchdown_impulse != 0, latch_first != 0);
      mask = s.stage; touchdown = s.impulse;
      rbdLatchQuadruped(static_cast<const DevModel*>(h->d_model), h->d_frames, qk, k > 0 ? latched + (k - 1) * N * nf : nullptr, latched + k * N * nf,
                        s.carry, n, h->stream);
      HIP_TRY(hipGetLastError());
    }
    if (touchdown) {
      idocp_rbd_fd_io_t imp = idocp_rbd_fd_io_t();
      imp.q = qk; imp.v = vk; imp.v_next = vk;            // (in place: slice k becomes the post-impulse velocity)
      int rc = launchForward(h, IDOCP_RBD_IMPULSE, n, touchdown, time_step, dt, imp); if (rc) return rc;
    }
    idocp_rbd_fd_io_t io = idocp_rbd_fd_io_t();
    io.q = qk; io.v = vk;
    if (pol) {
      double* uk = u_traj ? u_traj + k * N * nu : h->u_buf.ptr;
      launchPolicy(h, n, k, *pol, qk, vk, uk);
      HIP_TRY(hipGetLastError());
      io.u = uk;
    } else {
      io.u = u ? u + k * N * nu : nullptr;
    }
    io.contact_points = contact_points ? contact_points + k * N * nf : nullptr;
    io.a = a_traj ? a_traj + k * N * nv : nullptr;
    io.f = f_traj ? f_traj + k * N * nf : nullptr;
    io.q_next = qk + N * nq; io.v_next = vk + N * nv;
    int rc = launchForward(h, IDOCP_RBD_STAGE, n, mask, time_step, dt, io); if (rc) return rc;
    prev = mask;
  }
  return IDOCP_OK;
}

// ---- contact-frame kinematics and the rollout that latches its footholds ----

int checkKinematics(const char* who, const idocp_rbd* h, int n, const idocp_rbd_kin_io_t* io) {
  const std::string w(who);
  if (!h || !io) { set_last_error(w + ": null handle or io"); return IDOCP_E_ARG; }
  if (!h->quadruped) { set_last_error(w + ": a fixed-base chain has no contact frames"); return IDOCP_E_UNSUPPORTED; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (!io->q) { set_last_error(w + ": q is needed"); return IDOCP_E_ARG; }
  if (io->velocity && !io->v) { set_last_error(w + ": velocity needs v"); return IDOCP_E_ARG; }
  if (!io->points && !io->rotation && !io->velocity && !io->jacobian) { set_last_error(w + ": no output was asked for"); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

// host_bounds: the policy's arrays are host memory
int checkFootholds(const char* who, const idocp_rbd* h, int n, int steps, const int* active, double time_step, double dt,
                   const idocp_rbd_foothold_rollout_t* io, bool host_bounds) {
  const std::string w(who);
  if (!h || !io) { set_last_error(w + ": null handle or io"); return IDOCP_E_ARG; }
  if (!h->quadruped) { set_last_error(w + ": a fixed-base chain has no contact frames"); return IDOCP_E_UNSUPPORTED; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (steps < 1) { set_last_error(w + ": steps must be at least 1"); return IDOCP_E_ARG; }
  if (!io->contact_points || !io->q_traj || !io->v_traj || !active) {
    set_last_error(w + ": contact_points, q_traj, v_traj and active are needed"); return IDOCP_E_ARG;
  }
  if (io->u && io->policy) { set_last_error(w + ": u and policy exclude one another"); return IDOCP_E_ARG; }
  if (!std::isfinite(dt)) { set_last_error(w + ": dt must be finite"); return IDOCP_E_ARG; }
  if (io->policy) { int rc = checkPolicy(who, h, io->policy, host_bounds); if (rc) return rc; }
  if (idocp_host::footholdAnyActive(active, h->model.ncontacts, steps) && (!(time_step > 0.0) || !std::isfinite(time_step))) {
    set_last_error(w + ": an active contact needs a positive Baumgarte time_step"); return IDOCP_E_ARG;
  }
  return IDOCP_OK;
}

// The host form of a policy: its six arrays as slots of the plan; *d: the policy with device pointers once the plan is bound.
// N samples, S steps; q_ref and v_ref are not read without K and get no room then.
void policySlots(StagePlan& p, const idocp_rbd* h, const idocp_rbd_policy_t& pol, size_t N, size_t S, idocp_rbd_policy_t* d) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nk = nu * 2 * nv;
  const size_t gains = S * (pol.shared_gains ? 1 : N), refs = S * (pol.shared_ref ? 1 : N);
  *d = pol;
  p.in(pol.u_ff, S * N * nu, &d->u_ff);
  p.in(pol.K, gains * nk, &d->K);
  p.in(pol.K ? pol.q_ref : nullptr, refs * nq, &d->q_ref);
  p.in(pol.K ? pol.v_ref : nullptr, refs * nv, &d->v_ref);
  p.in(pol.u_min, nu, &d->u_min);
  p.in(pol.u_max, nu, &d->u_max);
}

// ---- the score of a rollout ----

// everything that is refused, and the kernel's arguments but for the eight array pointers of io
int checkScore(const char* who, const idocp_rbd* h, const idocp_rbd_objective* o, int n, int first_step, int steps, const int* active, int terminal,
               int accumulate, const idocp_rbd_score_io_t* io, RbdScoreArgs* a) {
  const std::string w(who);
  if (!h || !o || !io) { set_last_error(w + ": null handle, objective or io"); return IDOCP_E_ARG; }
  if (o->owner != h) { set_last_error(w + ": the objective was created on another handle"); return IDOCP_E_ARG; }
  const idocp_host::RbdScoreCall c = idocp_host::planScoreCall(who, o->plan, n, first_step, steps, active, io->q_traj, io->v_traj, io->u_traj, io->a_traj, io->f_traj);
  if (c.rc) { set_last_error(c.error); return c.rc; }
  std::memcpy(a->masks, c.masks, sizeof(c.masks));
  a->q_ref = o->d_q_ref + (size_t)first_step * o->plan.nq;
  a->v_ref = o->d_v_ref + (size_t)first_step * o->plan.nv;
  a->block = o->d_block;
  a->steps = steps; a->terminal = terminal != 0; a->accumulate = accumulate != 0;
  return IDOCP_OK;
}

// ---- sampling around a torque sequence ----

int checkPerturb(const char* who, const idocp_rbd* h, int n, int first_step, int steps, const double* u_nominal, const double* sigma, const double* u_min,
                 const double* u_max, const double* u_samples, bool host) {
  const std::string w(who);
  if (!h) { set_last_error(w + ": null handle"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (steps < 1) { set_last_error(w + ": steps must be at least 1"); return IDOCP_E_ARG; }
  if (first_step < 0 || first_step > INT_MAX - steps) { set_last_error(w + ": first_step must be non-negative, and first_step + steps must fit an int"); return IDOCP_E_ARG; }
  if (!u_nominal || !sigma || !u_samples) { set_last_error(w + ": u_nominal, sigma and u_samples are needed"); return IDOCP_E_ARG; }
  if (!host) return IDOCP_OK;
  for (int j = 0; j < h->model.nu; ++j)
    if (!std::isfinite(sigma[j]) || sigma[j] < 0.0) {
      set_last_error(w + ": sigma[" + std::to_string(j) + "] must be finite and non-negative"); return IDOCP_E_ARG;
    }
  idocp_rbd_policy_t bounds = idocp_rbd_policy_t();
  bounds.u_min = u_min; bounds.u_max = u_max;
  return checkPolicy(who, h, &bounds, true);
}

int launchPerturb(idocp_rbd* h, int n, int first_step, int steps, const double* u_nominal, const double* sigma, const double* u_min, const double* u_max,
                  unsigned long long seed, unsigned draw, double* u_samples) {
  RbdPerturbArgs a;
  a.u_nominal = u_nominal; a.sigma = sigma; a.u_min = u_min; a.u_max = u_max; a.u_samples = u_samples;
  a.seed = seed; a.draw = draw; a.n = n; a.nu = h->model.nu; a.first_step = first_step; a.steps = steps;
  rbdPerturb(a, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int chunksOf(int n) { return (int)(((long long)n + IDOCP_RBD_REDUCE_CHUNK - 1) / IDOCP_RBD_REDUCE_CHUNK); }

// room for the chunk partials of `rows` rows: grows only when rows * ceil(n / chunk) does
int growReduce(idocp_rbd* h, int rows, int n) { return h->reduce.grow((size_t)rows * chunksOf(n) * RBD_PARTIAL_STRIDE, h->stream); }

int checkWeights(const char* who, const idocp_rbd* h, int n, const double* cost, double penalty, double temperature, const double* weights,
                 const double* stats) {
  const std::string w(who);
  if (!h) { set_last_error(w + ": null handle"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (!cost || !weights || !stats) { set_last_error(w + ": cost, weights and stats are needed"); return IDOCP_E_ARG; }
  if (!std::isfinite(temperature) || !(temperature > 0.0)) { set_last_error(w + ": temperature must be finite and positive"); return IDOCP_E_ARG; }
  if (!std::isfinite(penalty) || penalty < 0.0) { set_last_error(w + ": penalty must be finite and non-negative"); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

int launchWeights(idocp_rbd* h, int n, const double* cost, const double* violation, double penalty, double temperature, double* weights, double* stats) {
  int rc = growReduce(h, 1, n); if (rc) return rc;
  RbdWeightArgs a;
  a.cost = cost; a.violation = violation; a.penalty = penalty; a.temperature = temperature;
  a.weights = weights; a.stats = stats; a.scratch = h->reduce.ptr; a.n = n; a.nchunks = chunksOf(n);
  rbdWeights(a, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int checkMean(const char* who, const idocp_rbd* h, int n, int rows, int m, const double* weights, const double* x, const double* mean, bool host) {
  const std::string w(who);
  if (!h) { set_last_error(w + ": null handle"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (rows < 1) { set_last_error(w + ": rows must be at least 1"); return IDOCP_E_ARG; }
  if (m < 1 || m > IDOCP_RBD_MEAN_MAX_COLUMNS) {
    set_last_error(w + ": m must be 1 .. " + std::to_string(IDOCP_RBD_MEAN_MAX_COLUMNS) + " (IDOCP_RBD_MEAN_MAX_COLUMNS)"); return IDOCP_E_ARG;
  }
  if (!weights || !x || !mean) { set_last_error(w + ": weights, x and mean are needed"); return IDOCP_E_ARG; }
  if ((long long)rows * chunksOf(n) > INT_MAX || (long long)rows * m > INT_MAX) {
    set_last_error(w + ": rows * ceil(n / IDOCP_RBD_REDUCE_CHUNK) and rows * m must fit an int (one workgroup per row and chunk)"); return IDOCP_E_UNSUPPORTED;
  }
  if (host)
    for (int i = 0; i < n; ++i)
      if (!std::isfinite(weights[i]) || weights[i] < 0.0) {
        set_last_error(w + ": weights[" + std::to_string(i) + "] must be finite and non-negative"); return IDOCP_E_ARG;
      }
  return IDOCP_OK;
}

int launchMean(idocp_rbd* h, int n, int rows, int m, const double* weights, const double* x, double* mean) {
  int rc = growReduce(h, rows, n); if (rc) return rc;
  RbdMeanArgs a;
  a.weights = weights; a.x = x; a.mean = mean; a.scratch = h->reduce.ptr; a.n = n; a.rows = rows; a.m = m; a.nchunks = chunksOf(n);
  rbdMean(a, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

// ---- derivatives of the forward dynamics ----

int checkDerivatives(const char* who, const idocp_rbd* h, int mode, int n, const int* active, double time_step, double dt, const idocp_rbd_fdd_io_t* io) {
  const std::string w(who);
  if (!h || !io) { set_last_error(w + ": null handle or io"); return IDOCP_E_ARG; }
  if (!h->quadruped && (io->f || io->contact_points || io->df_dq || io->df_dv || io->df_du)) {
    set_last_error(w + ": a fixed-base chain has no contacts (f, contact_points and the contact outputs df_dq, df_dv, df_du must be NULL)");
    return IDOCP_E_ARG;
  }
  int rc = checkForward(who, h, mode, n, active, dt, io->q, io->v, false); if (rc) return rc;
  if (mode == IDOCP_RBD_IMPULSE && (io->u || io->da_du || io->df_du || io->B)) {
    set_last_error(w + ": IMPULSE mode takes no torques (u, da_du, df_du and B must be NULL)"); return IDOCP_E_ARG;
  }
  if (mode == IDOCP_RBD_STAGE) { rc = checkStageContacts(who, h, active, time_step, io->contact_points); if (rc) return rc; }
  return IDOCP_OK;
}

// io: device pointers.  Per pass of the plan: the forward launch, the inverse launch at its solution, the products.
int launchDerivatives(idocp_rbd* h, int mode, int n, int mask, double time_step, double dt, const idocp_rbd_fdd_io_t& io) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = h->quadruped ? 3 * (size_t)h->model.ncontacts : 0, nx = 2 * nv;
  const idocp_host::FddPlan p = idocp_host::fddPlan((int)nv, (int)nf, n, h->fdd_limit);
  int rc = h->fdd.grow(p.total, h->stream); if (rc) return rc;
  double* const S = h->fdd.ptr;
  const DevModel* d_m = static_cast<const DevModel*>(h->d_model);
  auto at = [](double* x, size_t off) { return x ? x + off : nullptr; };
  for (int i = 0; i < p.nchunks; ++i) {
    const size_t F = (size_t)p.first(i);
    const int cnt = p.count(i, n);
    idocp_rbd_fd_io_t fd = idocp_rbd_fd_io_t();
    fd.q = io.q + F * nq; fd.v = io.v + F * nv;
    fd.u = io.u ? io.u + F * nu : nullptr;
    fd.contact_points = io.contact_points ? io.contact_points + F * nf : nullptr;
    fd.a = S + p.a; fd.f = h->quadruped ? S + p.f : nullptr;
    rc = launchForward(h, mode, cnt, mask, time_step, dt, fd); if (rc) return rc;
    RbdFddArgs g;
    g.q = fd.q; g.v = fd.v; g.a = S + p.a; g.f = fd.f; g.dtau_dq = S + p.dtau_dq; g.dtau_dv = S + p.dtau_dv;
    g.dCdq = S + p.dCdq; g.dCdv = S + p.dCdv; g.MJtJinv = S + p.MJtJinv;
    g.a_out = at(io.a, F * nv); g.f_out = at(io.f, F * nf);
    g.da_dq = at(io.da_dq, F * nv * nv); g.da_dv = at(io.da_dv, F * nv * nv); g.da_du = at(io.da_du, F * nv * nu);
    g.df_dq = at(io.df_dq, F * nf * nv); g.df_dv = at(io.df_dv, F * nf * nv); g.df_du = at(io.df_du, F * nf * nu);
    g.A = at(io.A, F * nx * nx); g.B = at(io.B, F * nx * nu);
    g.dt = dt;
    if (h->quadruped) {
      idocp_rbd_io_t b = idocp_rbd_io_t();
      b.q = fd.q; b.v = fd.v; b.a = S + p.a; b.f = S + p.f; b.contact_points = fd.contact_points;
      b.dtau_dq = S + p.dtau_dq; b.dtau_dv = S + p.dtau_dv; b.dCdq = S + p.dCdq; b.dCdv = S + p.dCdv; b.MJtJinv = S + p.MJtJinv;
      rbdBatchQuadruped(d_m, h->d_frames, b, cnt, mode, mask, (mode == IDOCP_RBD_STAGE && !(time_step > 0.0)) ? 1.0 : time_step, h->stream);
      HIP_TRY(hipGetLastError());
      rbdFddQuadruped(d_m, h->d_frames, g, cnt, mode, mask, h->stream);
    } else {
      chainFn(h->model.nv)(d_m, cnt, fd.q, fd.v, S + p.a, S + p.tau, S + p.dtau_dq, S + p.dtau_dv, S + p.MJtJinv, h->zaxes, h->stream);
      HIP_TRY(hipGetLastError());
      rbdFddChain(h->model.nv, g, cnt, h->stream);
    }
    HIP_TRY(hipGetLastError());
  }
  return IDOCP_OK;
}

int checkLinearize(const char* who, idocp_rbd* h, int n, int steps, const int* active, double time_step, double dt, const double* contact_points,
                   const double* q_traj, const double* v_traj) {
  if (steps < 1) { set_last_error(std::string(who) + ": steps must be at least 1"); return IDOCP_E_ARG; }
  int rc = checkForward(who, h, IDOCP_RBD_STAGE, n, active, dt, q_traj, v_traj, contact_points != nullptr); if (rc) return rc;
  if (h->quadruped)
    for (int k = 0; k < steps; ++k) { rc = checkStageContacts(who, h, active + (size_t)k * h->model.ncontacts, time_step, contact_points); if (rc) return rc; }
  return IDOCP_OK;
}

// The scratch of the cost linearisation: a, f and the six derivative blocks of one pass, each piece [chunk][its size] at an even number of doubles.
// The sample axis is cut by the rule of rbd_fdd_plan.hpp under the same cap, with an EVEN chunk (the runs of a workgroup of rbd_residual_kernel.hip
// then start 16-byte aligned).
struct ResidualPlan {
  int chunk = 0;
  size_t a, f, da_dq, da_dv, da_du, df_dq, df_dv, df_du, total;
};
ResidualPlan residualPlan(const idocp_rbd* h, int n) {
  const size_t V = h->model.nv, U = h->model.nu, F = h->quadruped ? 3 * (size_t)h->model.ncontacts : 0;
  const size_t sizes[8] = {V, F, V * V, V * V, V * U, F * V, F * V, F * U};
  size_t per_sample = 0;
  for (size_t s : sizes) per_sample += s;
  size_t fit = idocp_host::FDD_SCRATCH_CAP_DOUBLES / (per_sample + 8) / 2 * 2;      // (+ 8: the rounding of the pieces)
  if (fit < 2) fit = 2;
  ResidualPlan p;
  p.chunk = (size_t)n < fit ? n : (int)fit;
  size_t* const offsets[8] = {&p.a, &p.f, &p.da_dq, &p.da_dv, &p.da_du, &p.df_dq, &p.df_dv, &p.df_du};
  size_t at = 0;
  for (int i = 0; i < 8; ++i) { *offsets[i] = at; at += ((size_t)p.chunk * sizes[i] + 1) / 2 * 2; }
  p.total = at;
  return p;
}

// The form of an iLQR chain and of its pieces (the linearisation with rows, the backward pass, the workspace): built ONCE per call from the entry's
// chain, the handle and the objective; every layer below asks it instead of deriving the rows again.
//   DIAGONAL  idocp_rbd_ilqr_iterate          the plain linearisation, the gradients, the diagonal backward pass
//   GN        idocp_rbd_ilqr_iterate_gn       the cost rows of a_weight and f_weight (every objective whose weights have square roots)
//   PENALTY   idocp_rbd_ilqr_iterate_penalty  the constraint rows behind the cost rows, and the diagonal D
//   AL        idocp_rbd_ilqr_iterate_al       the penalty chain on the rows shifted by the multipliers
struct IlqrForm {
  enum Chain { DIAGONAL, GN, PENALTY, AL };
  Chain chain;
  int cost_rows = 0, constraint_rows = 0, multiplier_rows = 0;      // R, Rc and L of include/idocp_hip.h; 0 where the chain has none
  // o == nullptr (a refusal to come, or idocp_rbd_ilqr_gn_workspace_bytes, which has none): the cost rows of any objective of the handle
  IlqrForm(Chain c, const idocp_rbd* h, const idocp_rbd_objective* o) : chain(c) {
    if (chain == DIAGONAL || (!h && !o)) return;
    cost_rows = o ? idocp_host::residualRows(o->plan) : idocp_host::residualRows(h->model.nv, h->quadruped ? h->model.ncontacts : 0);
    if (o && penalty()) constraint_rows = idocp_host::constraintRows(o->plan);
    if (o && al()) multiplier_rows = idocp_host::multiplierRows(o->plan);
  }
  bool penalty() const { return chain == PENALTY || chain == AL; }      // the workspace and the io have a D_traj
  bool al() const { return chain == AL; }
  int rows() const { return cost_rows + constraint_rows; }              // of G_traj and rho_traj
  bool diagonal() const { return constraint_rows > 0; }                 // D_traj is written and read (without constraint rows it stays out)
  const double* lambdaOf(const double* lambda) const { return multiplier_rows ? lambda : nullptr; }      // NULL (all zeros) where no row reads it
  const char* linearization() const {
    return al() ? "idocp_rbd_linearize_rollout_al" : (penalty() ? "idocp_rbd_linearize_rollout_penalty" : "idocp_rbd_linearize_rollout_cost");
  }
};

// every pointer: device memory.  The touchdown impulse in front of step k + 1, if there is one, folded into A_k and B_k in place.
int touchdownProduct(idocp_rbd* h, int n, int steps, int k, const int* active, double time_step, double dt, const double* u, const double* contact_points,
                     const double* q_traj, const double* v_traj, double* A_traj, double* B_traj) {
  if (!h->quadruped || k + 1 >= steps) return IDOCP_OK;
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, nx = 2 * nv;
  const int mask = maskOf(h, active + (size_t)k * h->model.ncontacts), touchdown = maskOf(h, active + (size_t)(k + 1) * h->model.ncontacts) & ~mask;
  if (!touchdown) return IDOCP_OK;
  const double *qk = q_traj + k * N * nq, *vk = v_traj + k * N * nv;
  int rc = h->lin.grow(N * nv + N * nx * nx, h->stream); if (rc) return rc;
  double *v_pre = h->lin.ptr, *E = v_pre + N * nv;
  idocp_rbd_fd_io_t fd = idocp_rbd_fd_io_t();
  fd.q = qk; fd.v = vk; fd.u = u ? u + k * N * nu : nullptr; fd.contact_points = contact_points ? contact_points + k * N * nf : nullptr;
  fd.v_next = v_pre;      // the pre-impulse velocity v_k + dt a, recomputed
  rc = launchForward(h, IDOCP_RBD_STAGE, n, mask, time_step, dt, fd); if (rc) return rc;
  idocp_rbd_fdd_io_t imp = idocp_rbd_fdd_io_t();
  imp.q = qk + N * nq; imp.v = v_pre; imp.A = E;
  rc = launchDerivatives(h, IDOCP_RBD_IMPULSE, n, touchdown, time_step, dt, imp); if (rc) return rc;
  rbdFddImpulseProduct((int)nx, (int)nu, E, A_traj ? A_traj + k * N * nx * nx : nullptr, B_traj ? B_traj + k * N * nx * nu : nullptr, n, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

// every pointer: device memory.  idocp_rbd_linearize_rollout: per step the derivative composition, then the touchdown in front of the next step.
int linearizeDevice(idocp_rbd* h, int n, int steps, const int* active, double time_step, double dt, const double* u, const double* contact_points,
                    const double* q_traj, const double* v_traj, double* A_traj, double* B_traj, int touchdown_impulse) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, nx = 2 * nv;
  if (!A_traj && !B_traj) return IDOCP_OK;
  for (int k = 0; k < steps; ++k) {
    idocp_rbd_fdd_io_t io = idocp_rbd_fdd_io_t();
    io.q = q_traj + k * N * nq; io.v = v_traj + k * N * nv; io.u = u ? u + k * N * nu : nullptr;
    io.contact_points = contact_points ? contact_points + k * N * nf : nullptr;
    io.A = A_traj ? A_traj + k * N * nx * nx : nullptr;
    io.B = B_traj ? B_traj + k * N * nx * nu : nullptr;
    int rc = launchDerivatives(h, IDOCP_RBD_STAGE, n, h->quadruped ? maskOf(h, active + (size_t)k * h->model.ncontacts) : 0, time_step, dt, io); if (rc) return rc;
    if (touchdown_impulse) { rc = touchdownProduct(h, n, steps, k, active, time_step, dt, u, contact_points, q_traj, v_traj, A_traj, B_traj); if (rc) return rc; }
  }
  return IDOCP_OK;
}

// every pointer: device memory.  The linearisation with the rows of `form` (idocp_rbd_linearize_rollout_cost, _penalty, _al; mu and lambda where the
// form has them).  The diagonal part of the gradients first (rbd_gradient_kernel.hip, first_step 0, the terminal slice included); then step k takes
// the sample axis in the passes of residualPlan: the derivative composition of the pass with a, f and the blocks into h->gn, then ONE launch of the
// form's residual kernel for both kinds of rows, on top of the gradients; A_k, B_k are then in place and the touchdowns follow.
int linearizeRowsDevice(idocp_rbd* h, const idocp_rbd_objective* o, const IlqrForm& form, int n, int steps, const int* active, double time_step, double dt,
                        const double* u, const double* contact_points, const double* q_traj, const double* v_traj,
                        const idocp_rbd_penalty_linearization_io_t& out, double mu, const double* lambda, int touchdown_impulse) {
  // A_traj, B_traj alone: the plain linearisation (the same bits: a sample's do not depend on how the sample axis is cut), no rows formed
  if (!out.G_traj && !out.rho_traj && !out.D_traj && !out.lx_traj && !out.lu_traj)
    return linearizeDevice(h, n, steps, active, time_step, dt, u, contact_points, q_traj, v_traj, out.A_traj, out.B_traj, touchdown_impulse);
  if (out.lx_traj || out.lu_traj) {
    RbdGradientArgs g;
    g.q = q_traj; g.v = v_traj; g.u = u; g.q_ref = o->d_q_ref; g.v_ref = o->d_v_ref; g.block = o->d_block;
    g.lx = out.lx_traj; g.lu = out.lu_traj; g.n = n; g.steps = steps; g.terminal = 1;
    rbdGradient(h->model.nv, h->quadruped, g, h->stream);
    HIP_TRY(hipGetLastError());
  }
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, nx = 2 * nv, nz = nx + nu;
  const size_t R = (size_t)form.rows(), L = (size_t)form.multiplier_rows;
  const ResidualPlan p = residualPlan(h, n);
  int rc = h->gn.grow(p.total, h->stream); if (rc) return rc;
  double* const S = h->gn.ptr;
  lambda = form.lambdaOf(lambda);
  auto at = [](double* x, size_t off) { return x ? x + off : nullptr; };
  for (int k = 0; k < steps; ++k) {
    const int mask = h->quadruped ? maskOf(h, active + (size_t)k * h->model.ncontacts) : 0;
    for (int first = 0; first < n; first += p.chunk) {
      const int cnt = n - first < p.chunk ? n - first : p.chunk;
      const size_t F = (size_t)k * N + first;      // (slice k, sample `first`)
      idocp_rbd_fdd_io_t io = idocp_rbd_fdd_io_t();
      io.q = q_traj + F * nq; io.v = v_traj + F * nv; io.u = u ? u + F * nu : nullptr;
      io.contact_points = contact_points ? contact_points + F * nf : nullptr;
      io.A = at(out.A_traj, F * nx * nx); io.B = at(out.B_traj, F * nx * nu);
      io.a = S + p.a; io.da_dq = S + p.da_dq; io.da_dv = S + p.da_dv; io.da_du = S + p.da_du;
      if (h->quadruped) { io.f = S + p.f; io.df_dq = S + p.df_dq; io.df_dv = S + p.df_dv; io.df_du = S + p.df_du; }
      rc = launchDerivatives(h, IDOCP_RBD_STAGE, cnt, mask, time_step, dt, io); if (rc) return rc;
      RbdResidualAlArgs r;      // (the widest of the three argument structs: each launcher takes the part it knows)
      r.a = io.a; r.f = io.f; r.da_dq = io.da_dq; r.da_dv = io.da_dv; r.da_du = io.da_du; r.df_dq = io.df_dq; r.df_dv = io.df_dv; r.df_du = io.df_du;
      r.table = o->d_residual;
      r.G = at(out.G_traj, F * R * nz); r.rho = at(out.rho_traj, F * R); r.lx = at(out.lx_traj, F * nx); r.lu = at(out.lu_traj, F * nu);
      r.count = cnt; r.mask = mask;
      r.q = io.q; r.v = io.v; r.u = io.u; r.block = o->d_block; r.D = at(out.D_traj, F * nz);
      r.dtmu = dt * mu; r.scale = std::sqrt(r.dtmu); r.rc = form.constraint_rows;
      r.lambda = lambda ? lambda + F * L : nullptr; r.penalty = mu;
      const bool launched = form.al() ? rbdResidualAl(h->model.nv, h->quadruped, r, h->stream)
                                      : (form.penalty() ? rbdResidualPenalty(h->model.nv, h->quadruped, r, h->stream) : rbdResidual(h->model.nv, h->quadruped, r, h->stream));
      if (!launched) { set_last_error(std::string(form.linearization()) + ": no residual kernel for this model"); return IDOCP_E_UNSUPPORTED; }
      HIP_TRY(hipGetLastError());
    }
  }
  if (!touchdown_impulse || (!out.A_traj && !out.B_traj)) return IDOCP_OK;
  for (int k = 0; k < steps; ++k) { rc = touchdownProduct(h, n, steps, k, active, time_step, dt, u, contact_points, q_traj, v_traj, out.A_traj, out.B_traj); if (rc) return rc; }
  return IDOCP_OK;
}

// ---- time-varying LQR gains about a linearised rollout ----

// host: the weight arrays are host memory and can be looked at
int checkLqr(const char* who, const idocp_rbd* h, int n, int steps, const idocp_rbd_lqr_io_t* io, bool host) {
  const std::string w(who);
  if (!h || !io) { set_last_error(w + ": null handle or io"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (steps < 1) { set_last_error(w + ": steps must be at least 1"); return IDOCP_E_ARG; }
  if (!io->A_traj || !io->B_traj) { set_last_error(w + ": A_traj and B_traj are needed"); return IDOCP_E_ARG; }
  if (!io->x_weight || !io->u_weight || !io->xf_weight) { set_last_error(w + ": x_weight, u_weight and xf_weight are needed"); return IDOCP_E_ARG; }
  if ((io->lx_traj != nullptr) != (io->lu_traj != nullptr)) { set_last_error(w + ": lx_traj and lu_traj come together (both or neither)"); return IDOCP_E_ARG; }
  if (!io->lx_traj && (io->k_traj || io->expected)) { set_last_error(w + ": k_traj and expected need the gradients lx_traj and lu_traj"); return IDOCP_E_ARG; }
  if (!io->K_traj && !io->k_traj && !io->P0 && !io->p0 && !io->expected && !io->status) { set_last_error(w + ": no output was asked for"); return IDOCP_E_ARG; }
  if (!std::isfinite(io->regularization) || io->regularization < 0.0) {
    set_last_error(w + ": regularization must be finite and non-negative"); return IDOCP_E_ARG;
  }
  if (!host) return IDOCP_OK;
  const int nx = 2 * h->model.nv, nu = h->model.nu;
  auto weights = [&](const char* name, const double* x, int m) {
    for (int j = 0; j < m; ++j)
      if (!std::isfinite(x[j]) || x[j] < 0.0) { set_last_error(w + ": " + name + "[" + std::to_string(j) + "] must be finite and non-negative"); return false; }
    return true;
  };
  if (!weights("x_weight", io->x_weight, nx) || !weights("u_weight", io->u_weight, nu) || !weights("xf_weight", io->xf_weight, nx)) return IDOCP_E_ARG;
  return IDOCP_OK;
}

int checkLqrGn(const char* who, int g_rows, const double* G_traj, const double* D_traj) {
  const std::string w(who);
  if (G_traj || g_rows != 0) {
    if (!G_traj || g_rows == 0) { set_last_error(w + ": G_traj and g_rows come together (NULL with 0, or both given)"); return IDOCP_E_ARG; }
    if (g_rows < 4 || g_rows > 64 || g_rows % 4 != 0) { set_last_error(w + ": g_rows must be a multiple of 4 within 4 .. 64"); return IDOCP_E_ARG; }
  }
  if (D_traj && !G_traj) { set_last_error(w + ": D_traj needs a G_traj"); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

// io, G, D: device pointers.  The three backward passes: G = nullptr: the plain form; D = nullptr: the GN form; both: the GN form with the diagonal.
// (The widest of the three argument structs is filled; each launcher takes the part it knows.)
int launchLqr(idocp_rbd* h, int n, int steps, const idocp_rbd_lqr_io_t& io, int g_rows, const double* G, const double* D) {
  RbdLqrGnDiagArgs a;
  a.A = io.A_traj; a.B = io.B_traj; a.x_weight = io.x_weight; a.u_weight = io.u_weight; a.xf_weight = io.xf_weight;
  a.lx = io.lx_traj; a.lu = io.lu_traj; a.regularization = io.regularization;
  a.K = io.K_traj; a.k = io.k_traj; a.P0 = io.P0; a.p0 = io.p0; a.expected = io.expected; a.status = io.status;
  a.n = n; a.steps = steps; a.nx = 2 * h->model.nv; a.nu = h->model.nu;
  a.G = G; a.g_rows = g_rows; a.D = D;
  if (!G) rbdLqrBackward(h->quadruped, a, h->stream);
  else if (D) rbdLqrBackwardGnDiag(h->quadruped, a, h->stream);
  else rbdLqrBackwardGn(h->quadruped, a, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

// what the three backward passes refuse, in their order.  host: the weight arrays are host memory
int checkLqrCall(const char* who, const idocp_rbd* h, int n, int steps, const idocp_rbd_lqr_io_t* io, bool host, int g_rows, const double* G_traj,
                 const double* D_traj) {
  int rc = checkLqr(who, h, n, steps, io, host); if (rc) return rc;
  return checkLqrGn(who, g_rows, G_traj, D_traj);
}

// ---- gradients of an objective, the line-search step of iLQR, one iteration ----

// everything that is refused, and the kernel's arguments but for the five array pointers of io
int checkGradients(const char* who, const idocp_rbd* h, const idocp_rbd_objective* o, int n, int first_step, int steps, int terminal,
                   const idocp_rbd_gradient_io_t* io, RbdGradientArgs* a) {
  const std::string w(who);
  if (!h || !o || !io) { set_last_error(w + ": null handle, objective or io"); return IDOCP_E_ARG; }
  if (o->owner != h) { set_last_error(w + ": the objective was created on another handle"); return IDOCP_E_ARG; }
  const idocp_host::RbdGradientCall c = idocp_host::planGradientCall(who, o->plan, n, first_step, steps, terminal, io->q_traj, io->v_traj, io->u_traj,
                                                                     io->lx_traj, io->lu_traj);
  if (c.rc) { set_last_error(c.error); return c.rc; }
  a->q_ref = o->d_q_ref + (size_t)first_step * o->plan.nq;
  a->v_ref = o->d_v_ref + (size_t)first_step * o->plan.nv;
  a->block = o->d_block;
  a->n = n; a->steps = steps; a->terminal = terminal != 0;
  return IDOCP_OK;
}

int checkLqrWeights(const char* who, const idocp_rbd_objective* o) {
  const std::string w(who);
  if (!o) { set_last_error(w + ": null objective"); return IDOCP_E_ARG; }
  const std::string unsupported = idocp_host::gradientUnsupported(o->plan);
  if (!unsupported.empty()) { set_last_error(w + ": " + unsupported); return IDOCP_E_UNSUPPORTED; }
  return IDOCP_OK;
}

// ---- the linearisation with rows and the backward pass with residual rows

int checkMu(const char* who, double mu, const char* name) {
  if (!std::isfinite(mu) || !(mu > 0.0)) { set_last_error(std::string(who) + ": " + name + " must be positive and finite"); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

// what idocp_rbd_linearize_rollout_cost, _penalty and _al refuse, in this order (the cost call's io comes widened: D_traj = NULL, and mu = 0)
int checkLinearizeRows(const char* who, const IlqrForm& form, idocp_rbd* h, const idocp_rbd_objective* o, int n, int steps, const int* active,
                       double time_step, double dt, const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                       const idocp_rbd_penalty_linearization_io_t* io, double mu) {
  const std::string w(who);
  int rc = checkLinearize(who, h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj); if (rc) return rc;
  if (!o || !io) { set_last_error(w + ": null objective or io"); return IDOCP_E_ARG; }
  if (o->owner != h) { set_last_error(w + ": the objective was created on another handle"); return IDOCP_E_ARG; }
  if (steps > o->plan.steps) { set_last_error(w + ": steps must lie within the objective's " + std::to_string(o->plan.steps) + " steps"); return IDOCP_E_ARG; }
  const std::string unsupported = idocp_host::residualUnsupported(o->plan);
  if (!unsupported.empty()) { set_last_error(w + ": " + unsupported); return IDOCP_E_UNSUPPORTED; }
  if (!io->A_traj && !io->B_traj && !io->G_traj && !io->rho_traj && !io->D_traj && !io->lx_traj && !io->lu_traj) {
    set_last_error(w + ": no output was asked for"); return IDOCP_E_ARG;
  }
  if (((long long)steps + 1) * n > 2147483647LL) { set_last_error(w + ": (steps + 1) * n must fit an int"); return IDOCP_E_ARG; }
  if (!u_traj && (io->lx_traj || io->lu_traj) && idocp_host::rbd_objective_detail::anyNonZero(o->plan.block.u_weight, o->plan.nu)) {
    set_last_error(w + ": u_traj is NULL but a non-zero u_weight reads it"); return IDOCP_E_ARG;
  }
  if (form.al()) { rc = checkMu(who, mu, "mu"); if (rc) return rc; }
  if (!form.penalty()) return IDOCP_OK;
  if (!std::isfinite(mu) || mu < 0.0) { set_last_error(w + ": mu must be finite and non-negative"); return IDOCP_E_ARG; }
  const std::string pair = idocp_host::penaltyPairRefused(o->plan);
  if (!pair.empty()) { set_last_error(w + ": " + pair); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

// the device form of the three linearisations with rows
int linearizeRowsEntry(const char* who, IlqrForm::Chain chain, idocp_rbd* h, const idocp_rbd_objective* o, int n, int steps, const int* active,
                       double time_step, double dt, const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                       const idocp_rbd_penalty_linearization_io_t* io, double mu, const double* lambda_traj, int touchdown_impulse) {
  const IlqrForm form(chain, h, o);
  int rc = checkLinearizeRows(who, form, h, o, n, steps, active, time_step, dt, u_traj, contact_points, q_traj, v_traj, io, mu); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return linearizeRowsDevice(h, o, form, n, steps, active, time_step, dt, u_traj, contact_points, q_traj, v_traj, *io, mu, lambda_traj, touchdown_impulse);
}

// the host form of the three: one staging list, D_traj and lambda_traj taking no room where the form has none
int linearizeRowsHost(const char* who, IlqrForm::Chain chain, idocp_rbd* h, const idocp_rbd_objective* o, int n, int steps, const int* active,
                      double time_step, double dt, const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                      const idocp_rbd_penalty_linearization_io_t* io, double mu, const double* lambda_traj, int touchdown_impulse) {
  const IlqrForm form(chain, h, o);
  int rc = checkLinearizeRows(who, form, h, o, n, steps, active, time_step, dt, u_traj, contact_points, q_traj, v_traj, io, mu); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, S = (size_t)steps, nx = 2 * nv;
  const size_t R = (size_t)form.rows();
  StagePlan p;
  const double *d_u, *d_points, *d_q, *d_v, *d_lambda;
  idocp_rbd_penalty_linearization_io_t d;
  p.in(u_traj, S * N * nu, &d_u);
  p.in(contact_points, S * N * nf, &d_points);
  p.in(q_traj, (S + 1) * N * nq, &d_q);
  p.in(v_traj, (S + 1) * N * nv, &d_v);
  p.in(lambda_traj, S * N * (size_t)form.multiplier_rows, &d_lambda);
  p.out(io->A_traj, S * N * nx * nx, &d.A_traj);
  p.out(io->B_traj, S * N * nx * nu, &d.B_traj);
  p.out(io->G_traj, S * N * R * (nx + nu), &d.G_traj);
  p.out(io->rho_traj, S * N * R, &d.rho_traj);
  p.out(io->D_traj, S * N * (nx + nu), &d.D_traj);
  p.out(io->lx_traj, (S + 1) * N * nx, &d.lx_traj);
  p.out(io->lu_traj, S * N * nu, &d.lu_traj);
  rc = stageIn(h, p); if (rc) return rc;
  rc = linearizeRowsDevice(h, o, form, n, steps, active, time_step, dt, d_u, d_points, d_q, d_v, d, mu, d_lambda, touchdown_impulse); if (rc) return rc;
  return stageOut(h, p);
}

// the cost call's io as the penalty call's: D_traj = NULL
const idocp_rbd_penalty_linearization_io_t* widened(const idocp_rbd_cost_linearization_io_t* io, idocp_rbd_penalty_linearization_io_t* wide) {
  if (!io) return nullptr;
  *wide = idocp_rbd_penalty_linearization_io_t();
  wide->A_traj = io->A_traj; wide->B_traj = io->B_traj; wide->G_traj = io->G_traj; wide->rho_traj = io->rho_traj; wide->lx_traj = io->lx_traj; wide->lu_traj = io->lu_traj;
  return wide;
}

// the host form of the three backward passes
int lqrHost(const char* who, idocp_rbd* h, int n, int steps, const idocp_rbd_lqr_io_t* io, int g_rows, const double* G_traj, const double* D_traj) {
  int rc = checkLqrCall(who, h, n, steps, io, true, g_rows, G_traj, D_traj); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nx = 2 * (size_t)h->model.nv, nu = h->model.nu, N = (size_t)n, S = (size_t)steps;
  StagePlan p;
  idocp_rbd_lqr_io_t d = *io;
  double* d_status = nullptr;
  const double *d_G = nullptr, *d_D = nullptr;
  p.in(io->A_traj, S * N * nx * nx, &d.A_traj);
  p.in(io->B_traj, S * N * nx * nu, &d.B_traj);
  p.in(io->x_weight, nx, &d.x_weight);
  p.in(io->u_weight, nu, &d.u_weight);
  p.in(io->xf_weight, nx, &d.xf_weight);
  p.in(io->lx_traj, (S + 1) * N * nx, &d.lx_traj);
  p.in(io->lu_traj, S * N * nu, &d.lu_traj);
  p.out(io->K_traj, S * N * nx * nu, &d.K_traj);
  p.out(io->k_traj, S * N * nu, &d.k_traj);
  p.out(io->P0, N * nx * nx, &d.P0);
  p.out(io->p0, N * nx, &d.p0);
  p.out(io->expected, N * 2, &d.expected);
  if (io->status) p.deviceOnly((N + 1) / 2, &d_status);      // (n ints in a slot of doubles; they come down by a copy of their own, in front of stageOut's wait)
  p.in(G_traj, S * N * (size_t)g_rows * (nx + nu), &d_G);
  p.in(D_traj, S * N * (nx + nu), &d_D);
  rc = stageIn(h, p); if (rc) return rc;
  d.status = reinterpret_cast<int*>(d_status);
  rc = launchLqr(h, n, steps, d, g_rows, d_G, d_D); if (rc) return rc;
  if (io->status) HIP_TRY(hipMemcpyAsync(io->status, d_status, sizeof(int) * N, hipMemcpyDeviceToHost, h->stream));
  return stageOut(h, p);
}

int checkStepTorques(const char* who, const idocp_rbd* h, int n, int steps, const double* u, const double* k, const double* alpha, const double* out) {
  const std::string w(who);
  if (!h) { set_last_error(w + ": null handle"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (steps < 1) { set_last_error(w + ": steps must be at least 1"); return IDOCP_E_ARG; }
  if (!u || !k || !alpha || !out) { set_last_error(w + ": u_traj, k_traj, alpha and u_ff are needed"); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

int checkAccept(const char* who, const idocp_rbd* h, int n, int steps, const idocp_rbd_ilqr_accept_io_t* io) {
  const std::string w(who);
  if (!h || !io) { set_last_error(w + ": null handle or io"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (steps < 1) { set_last_error(w + ": steps must be at least 1"); return IDOCP_E_ARG; }
  if (!io->q_traj || !io->v_traj || !io->u_traj || !io->trial_q || !io->trial_v || !io->trial_u) {
    set_last_error(w + ": q_traj, v_traj, u_traj and their trial arrays are needed"); return IDOCP_E_ARG;
  }
  if (!io->cost || !io->violation || !io->trial_cost || !io->trial_violation) {
    set_last_error(w + ": cost, violation, trial_cost and trial_violation are needed"); return IDOCP_E_ARG;
  }
  if (!io->expected || !io->alpha || !io->done || !io->alpha_accepted) { set_last_error(w + ": expected, alpha, done and alpha_accepted are needed"); return IDOCP_E_ARG; }
  const double values[4] = {io->penalty, io->armijo, io->shrink, io->alpha_min};
  const char* const names[4] = {"penalty", "armijo", "shrink", "alpha_min"};
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(values[i]) || values[i] < 0.0) { set_last_error(w + ": " + names[i] + " must be finite and non-negative"); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

// io: device pointers
int launchAccept(idocp_rbd* h, int n, int steps, const idocp_rbd_ilqr_accept_io_t& io) {
  RbdIlqrAcceptArgs a;
  double* const dst[5] = {io.q_traj, io.v_traj, io.u_traj, io.a_traj, io.f_traj};
  const double* const src[5] = {io.trial_q, io.trial_v, io.trial_u, io.trial_a, io.trial_f};
  const int width[5] = {h->model.nq, h->model.nv, h->model.nu, h->model.nv, 3 * h->model.ncontacts};
  for (int c = 0; c < 5; ++c) { a.dst[c] = dst[c]; a.src[c] = src[c]; a.width[c] = width[c]; }
  a.cost = io.cost; a.violation = io.violation; a.alpha = io.alpha; a.alpha_accepted = io.alpha_accepted;
  a.trial_cost = io.trial_cost; a.trial_violation = io.trial_violation; a.expected = io.expected; a.done = io.done;
  a.penalty = io.penalty; a.armijo = io.armijo; a.shrink = io.shrink; a.alpha_min = io.alpha_min;
  a.n = n; a.steps = steps; a.wide = 0;
  rbdIlqrAccept(a, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

// The workspace of one iteration (include/idocp_hip.h names the order): offsets in doubles, each piece at an even number of doubles.
struct IlqrWorkspace {
  size_t A, B, lx, lu, K, k, u_ff, q, v, u, a, f, cost, violation, alpha, done, G, D, total;
};
// Behind everything else: G_traj with the form's rows (none on the diagonal chain), then D_traj on the penalty and AL chains.
IlqrWorkspace ilqrWorkspace(const idocp_rbd* h, const IlqrForm& form, int n, int steps) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, S = (size_t)steps, nx = 2 * nv;
  IlqrWorkspace w;
  size_t at = 0;
  auto piece = [&](size_t doubles) { const size_t here = at; at += (doubles + 1) / 2 * 2; return here; };
  w.A = piece(S * N * nx * nx); w.B = piece(S * N * nx * nu); w.lx = piece((S + 1) * N * nx); w.lu = piece(S * N * nu);
  w.K = piece(S * N * nx * nu); w.k = piece(S * N * nu); w.u_ff = piece(S * N * nu);
  w.q = piece((S + 1) * N * nq); w.v = piece((S + 1) * N * nv); w.u = piece(S * N * nu); w.a = piece(S * N * nv); w.f = piece(S * N * nf);
  w.cost = piece(N); w.violation = piece(N); w.alpha = piece(N); w.done = piece((N + 1) / 2);
  w.G = piece(S * N * (size_t)form.rows() * (nx + nu));
  w.D = piece(form.penalty() ? S * N * (nx + nu) : 0);
  w.total = at;
  return w;
}

// host: the workspace is the staging buffer's, and io->workspace is not looked at
int checkIterate(const char* who, const IlqrForm& form, const idocp_rbd* h, const idocp_rbd_objective* o, int n, int steps, const idocp_rbd_ilqr_io_t* io,
                 bool host) {
  const std::string w(who);
  if (!h || !o || !io) { set_last_error(w + ": null handle, objective or io"); return IDOCP_E_ARG; }
  if (o->owner != h) { set_last_error(w + ": the objective was created on another handle"); return IDOCP_E_ARG; }
  if (form.chain == IlqrForm::DIAGONAL) { int rc = checkLqrWeights(who, o); if (rc) return rc; }
  else {
    const std::string unsupported = idocp_host::residualUnsupported(o->plan);
    if (!unsupported.empty()) { set_last_error(w + ": " + unsupported); return IDOCP_E_UNSUPPORTED; }
    if (form.penalty()) {
      const std::string pair = idocp_host::penaltyPairRefused(o->plan);
      if (!pair.empty()) { set_last_error(w + ": " + pair); return IDOCP_E_ARG; }
      if (form.rows() > 64) { set_last_error(w + ": more than 64 rows"); return IDOCP_E_UNSUPPORTED; }
    }
  }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (steps < 1) { set_last_error(w + ": steps must be at least 1"); return IDOCP_E_ARG; }
  if (steps > o->plan.steps) { set_last_error(w + ": steps must lie within the objective's " + std::to_string(o->plan.steps) + " steps"); return IDOCP_E_ARG; }
  if (!io->q_traj || !io->v_traj || !io->u_traj) { set_last_error(w + ": q_traj, v_traj and u_traj are needed"); return IDOCP_E_ARG; }
  if (!io->cost || !io->violation) { set_last_error(w + ": cost and violation are needed"); return IDOCP_E_ARG; }
  if (!io->alpha_accepted || !io->lqr_status || !io->expected) { set_last_error(w + ": alpha_accepted, lqr_status and expected are needed"); return IDOCP_E_ARG; }
  if (io->trials < 1) { set_last_error(w + ": trials must be at least 1"); return IDOCP_E_ARG; }
  const double values[5] = {io->regularization, io->armijo, io->shrink, io->alpha_min, io->penalty};
  const char* const names[5] = {"regularization", "armijo", "shrink", "alpha_min", "penalty"};
  for (int i = 0; i < 5; ++i)
    if (!std::isfinite(values[i]) || values[i] < 0.0) { set_last_error(w + ": " + names[i] + " must be finite and non-negative"); return IDOCP_E_ARG; }
  if (form.al() && !(io->penalty > 0.0)) { set_last_error(w + ": penalty (mu) must be positive"); return IDOCP_E_ARG; }
  if (!host && !io->workspace) { set_last_error(w + ": the workspace is needed (idocp_rbd_ilqr_workspace_bytes, idocp_rbd_ilqr_gn_workspace_bytes, idocp_rbd_ilqr_penalty_workspace_bytes)"); return IDOCP_E_ARG; }
  if (!host && (reinterpret_cast<uintptr_t>(io->workspace) & 15u)) { set_last_error(w + ": the workspace must be 16-byte aligned"); return IDOCP_E_ARG; }
  return IDOCP_OK;
}

// the five arrays of a rollout that the score and the row calls read: [steps][n][..] each, those a call can do without may be NULL
struct RolloutArrays { const double *q, *v, *u, *a, *f; };

// A rollout of more than IDOCP_RBD_SCORE_MAX_WINDOW steps is scored window by window (the windows of the header, with accumulate):
// body(first, window, accumulate, the window's contact status, the window's slices) for each, until one refuses.
template <class Body>
int forEachWindow(const idocp_rbd* h, int n, int steps, const int* active, const RolloutArrays& t, Body body) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n;
  auto at = [](const double* x, size_t off) { return x ? x + off : nullptr; };
  for (int first = 0; first < steps; first += IDOCP_RBD_SCORE_MAX_WINDOW) {
    const int window = steps - first < IDOCP_RBD_SCORE_MAX_WINDOW ? steps - first : IDOCP_RBD_SCORE_MAX_WINDOW;
    const RolloutArrays w = {at(t.q, first * N * nq), at(t.v, first * N * nv), at(t.u, first * N * nu), at(t.a, first * N * nv), at(t.f, first * N * nf)};
    const int rc = body(first, window, first > 0, active ? active + (size_t)first * h->model.ncontacts : nullptr, w); if (rc) return rc;
  }
  return IDOCP_OK;
}

// the host form of the calls that take such arrays: their five slots
void stageRollout(StagePlan& p, const idocp_rbd* h, const idocp_rbd_objective* o, int n, int steps, const RolloutArrays& host, RolloutArrays* dev) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)o->plan.ncontacts, N = (size_t)n, S = (size_t)steps;
  p.in(host.q, S * N * nq, &dev->q);      // (the stage slices alone: the terminal slice has no rows)
  p.in(host.v, S * N * nv, &dev->v);
  p.in(host.u, S * N * nu, &dev->u);
  p.in(host.a, S * N * nv, &dev->a);
  p.in(host.f, S * N * nf, &dev->f);
}

// ---- the constraint rows of a window: their square sum plain (idocp_rbd_score_penalty) or shifted (idocp_rbd_score_al), and the multiplier update

enum RowCall { SCORE_PENALTY, SCORE_AL, MULTIPLIER_UPDATE };

// everything the three refuse, and the kernel's arguments but for the array pointers.  mu: not looked at by SCORE_PENALTY; out: sq_violation,
// sq_shifted, or lambda_out, which is needed where the objective has multiplier rows
int checkRowCall(const char* who, RowCall call, const idocp_rbd* h, const idocp_rbd_objective* o, int n, int first_step, int steps, const int* active,
                 int accumulate, const RolloutArrays& t, double mu, const double* out, RbdAlArgs* a) {
  const std::string w(who);
  if (!h || !o) { set_last_error(w + ": null handle or objective"); return IDOCP_E_ARG; }
  if (o->owner != h) { set_last_error(w + ": the objective was created on another handle"); return IDOCP_E_ARG; }
  if (call != SCORE_PENALTY) { int rc = checkMu(who, mu, "mu"); if (rc) return rc; }
  if (call != MULTIPLIER_UPDATE && !out) { set_last_error(w + (call == SCORE_AL ? ": sq_shifted is needed" : ": sq_violation is needed")); return IDOCP_E_ARG; }
  if (call == MULTIPLIER_UPDATE && !out && idocp_host::multiplierRows(o->plan)) { set_last_error(w + ": lambda_out is needed"); return IDOCP_E_ARG; }
  const idocp_host::RbdScoreCall c = idocp_host::planPenaltyCall(who, o->plan, n, first_step, steps, active, t.q, t.v, t.u, t.a, t.f);
  if (c.rc) { set_last_error(c.error); return c.rc; }
  std::memcpy(a->masks, c.masks, sizeof(c.masks));
  a->block = o->d_block; a->steps = steps; a->accumulate = accumulate != 0; a->penalty = mu;
  a->sq = nullptr; a->lambda = nullptr; a->lambda_out = nullptr; a->infeasibility = nullptr; a->change = nullptr;
  return IDOCP_OK;
}

// a: device pointers.  An objective without multiplier rows has nothing to update: the statistics are zero (kept as they are with accumulate)
int launchRowCall(const char* who, RowCall call, idocp_rbd* h, const idocp_rbd_objective* o, const RbdAlArgs& a, int n) {
  bool launched = true;
  if (call == SCORE_PENALTY) launched = rbdPenalty(h->model.nv, h->quadruped, a, n, h->stream);
  else if (call == SCORE_AL) launched = rbdAlScore(h->model.nv, h->quadruped, a, n, h->stream);
  else if (idocp_host::multiplierRows(o->plan)) launched = rbdAlUpdate(h->model.nv, h->quadruped, a, n, h->stream);
  else if (!a.accumulate) {
    if (a.infeasibility) HIP_TRY(hipMemsetAsync(a.infeasibility, 0, sizeof(double) * (size_t)n, h->stream));
    if (a.change) HIP_TRY(hipMemsetAsync(a.change, 0, sizeof(double) * (size_t)n, h->stream));
  }
  if (!launched) { set_last_error(std::string(who) + (call == SCORE_PENALTY ? ": no penalty kernel for this model" : ": no multiplier kernel for this model")); return IDOCP_E_UNSUPPORTED; }
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

// the device form of the three.  out as for checkRowCall; infeasibility and change: of MULTIPLIER_UPDATE
int rowCallDevice(const char* who, RowCall call, idocp_rbd* h, const idocp_rbd_objective* o, int n, int first_step, int steps, const int* active, int accumulate,
                  const RolloutArrays& t, double mu, const double* lambda, double* out, double* infeasibility, double* change) {
  RbdAlArgs a;
  int rc = checkRowCall(who, call, h, o, n, first_step, steps, active, accumulate, t, mu, out, &a); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  a.q = t.q; a.v = t.v; a.u = t.u; a.a = t.a; a.f = t.f;
  a.lambda = idocp_host::multiplierRows(o->plan) ? lambda : nullptr;
  if (call == MULTIPLIER_UPDATE) { a.lambda_out = out; a.infeasibility = infeasibility; a.change = change; }
  else a.sq = out;
  return launchRowCall(who, call, h, o, a, n);
}

// the host form of the three
int rowCallHost(const char* who, RowCall call, idocp_rbd* h, const idocp_rbd_objective* o, int n, int first_step, int steps, const int* active, int accumulate,
                const RolloutArrays& t, double mu, const double* lambda, double* out, double* infeasibility, double* change) {
  RbdAlArgs a;
  int rc = checkRowCall(who, call, h, o, n, first_step, steps, active, accumulate, t, mu, out, &a); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t N = (size_t)n, rows = (size_t)steps * N * (size_t)idocp_host::multiplierRows(o->plan);
  StagePlan p;
  RolloutArrays d;
  stageRollout(p, h, o, n, steps, t, &d);
  p.in(lambda, rows, &a.lambda);
  if (call == MULTIPLIER_UPDATE) {
    // (the staged copies are two slots even where the caller's arrays are one: in place is the caller's business, not the stage's)
    p.out(out, rows, &a.lambda_out);
    if (accumulate) { p.update(infeasibility, N, &a.infeasibility); p.update(change, N, &a.change); }
    else { p.out(infeasibility, N, &a.infeasibility, true); p.out(change, N, &a.change, true); }
  } else if (accumulate) p.update(out, N, &a.sq);
  else p.out(out, N, &a.sq);
  rc = stageIn(h, p); if (rc) return rc;
  a.q = d.q; a.v = d.v; a.u = d.u; a.a = d.a; a.f = d.f;
  rc = launchRowCall(who, call, h, o, a, n); if (rc) return rc;
  return stageOut(h, p);
}

// io: device pointers; ws: the workspace; lambda: the multipliers of the AL chain.  The chain of include/idocp_hip.h for the form: the linearisation
// and the backward pass that belong to it (with rows: the objective's own weight tables, without the refusal of
// idocp_rbd_objective_lqr_weights_device), then the rounds of trials.  Every call on the handle's stream, no synchronisation, no host read; an
// inner call that refuses leaves its own name in idocp_last_error.
int iterateDevice(idocp_rbd* h, const idocp_rbd_objective* o, const IlqrForm& form, int n, int steps, const int* active, double time_step, double dt,
                  const double* contact_points, const idocp_rbd_ilqr_io_t& io, double* ws, const double* lambda, int touchdown_impulse) {
  const size_t nq = h->model.nq, nv = h->model.nv, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n;
  const IlqrWorkspace w = ilqrWorkspace(h, form, n, steps);
  double *A = ws + w.A, *B = ws + w.B, *lx = ws + w.lx, *lu = ws + w.lu, *K = ws + w.K, *kff = ws + w.k, *u_ff = ws + w.u_ff;
  double *qt = ws + w.q, *vt = ws + w.v, *ut = ws + w.u, *at = ws + w.a, *ft = nf ? ws + w.f : nullptr;
  double *cost_t = ws + w.cost, *violation_t = ws + w.violation, *alpha = ws + w.alpha;
  int* done = reinterpret_cast<int*>(ws + w.done);
  int rc = IDOCP_OK;
  idocp_rbd_lqr_io_t lqr = idocp_rbd_lqr_io_t();
  lqr.A_traj = A; lqr.B_traj = B; lqr.lx_traj = lx; lqr.lu_traj = lu; lqr.regularization = io.regularization;
  lqr.K_traj = K; lqr.k_traj = kff; lqr.expected = io.expected; lqr.status = io.lqr_status;
  if (form.chain == IlqrForm::DIAGONAL) {
    rc = idocp_rbd_linearize_rollout_device(h, n, steps, active, time_step, dt, io.u_traj, contact_points, io.q_traj, io.v_traj, A, B, touchdown_impulse);
    if (rc) return rc;
    idocp_rbd_gradient_io_t g = idocp_rbd_gradient_io_t();
    g.q_traj = io.q_traj; g.v_traj = io.v_traj; g.u_traj = io.u_traj; g.lx_traj = lx; g.lu_traj = lu;
    rc = idocp_rbd_objective_gradients_device(h, o, n, 0, steps, 1, &g); if (rc) return rc;
    rc = idocp_rbd_objective_lqr_weights_device(o, &lqr.x_weight, &lqr.u_weight, &lqr.xf_weight); if (rc) return rc;
    rc = idocp_rbd_lqr_backward_device(h, n, steps, &lqr); if (rc) return rc;
  } else {
    // with rows: io.penalty is mu; without constraint rows D stays out and the GN form of the backward pass runs
    idocp_rbd_penalty_linearization_io_t c = idocp_rbd_penalty_linearization_io_t();
    c.A_traj = A; c.B_traj = B; c.G_traj = ws + w.G; c.D_traj = form.diagonal() ? ws + w.D : nullptr; c.lx_traj = lx; c.lu_traj = lu;
    lqr.x_weight = o->d_lqr_weights;
    lqr.u_weight = o->d_lqr_weights + idocp_host::lqrWeightOffsetU(o->plan);
    lqr.xf_weight = o->d_lqr_weights + idocp_host::lqrWeightOffsetXf(o->plan);
    if (form.al())
      rc = idocp_rbd_linearize_rollout_al_device(h, o, n, steps, active, time_step, dt, io.u_traj, contact_points, io.q_traj, io.v_traj, &c, io.penalty, lambda,
                                                 touchdown_impulse);
    else if (form.penalty())
      rc = idocp_rbd_linearize_rollout_penalty_device(h, o, n, steps, active, time_step, dt, io.u_traj, contact_points, io.q_traj, io.v_traj, &c, io.penalty,
                                                      touchdown_impulse);
    else {
      idocp_rbd_cost_linearization_io_t narrow = idocp_rbd_cost_linearization_io_t();
      narrow.A_traj = A; narrow.B_traj = B; narrow.G_traj = c.G_traj; narrow.lx_traj = lx; narrow.lu_traj = lu;
      rc = idocp_rbd_linearize_rollout_cost_device(h, o, n, steps, active, time_step, dt, io.u_traj, contact_points, io.q_traj, io.v_traj, &narrow, touchdown_impulse);
    }
    if (rc) return rc;
    if (form.penalty()) rc = idocp_rbd_lqr_backward_gn_diag_device(h, n, steps, &lqr, form.rows(), c.G_traj, c.D_traj);
    else rc = idocp_rbd_lqr_backward_gn_device(h, n, steps, &lqr, form.rows(), c.G_traj);
    if (rc) return rc;
  }
  rbdIlqrInit(alpha, done, io.alpha_accepted, n, h->stream);
  HIP_TRY(hipGetLastError());
  // every trial starts from the state the rollout started from
  HIP_TRY(hipMemcpyAsync(qt, io.q_traj, sizeof(double) * N * nq, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(vt, io.v_traj, sizeof(double) * N * nv, hipMemcpyDeviceToDevice, h->stream));
  idocp_rbd_policy_t pol = idocp_rbd_policy_t();
  pol.u_ff = u_ff; pol.K = K; pol.q_ref = io.q_traj; pol.v_ref = io.v_traj; pol.u_min = io.u_min; pol.u_max = io.u_max;
  idocp_rbd_ilqr_accept_io_t acc = idocp_rbd_ilqr_accept_io_t();
  acc.q_traj = io.q_traj; acc.v_traj = io.v_traj; acc.u_traj = io.u_traj; acc.a_traj = io.a_traj; acc.f_traj = io.f_traj;
  acc.cost = io.cost; acc.violation = io.violation;
  acc.trial_q = qt; acc.trial_v = vt; acc.trial_u = ut; acc.trial_a = at; acc.trial_f = ft;
  acc.trial_cost = cost_t; acc.trial_violation = violation_t; acc.expected = io.expected; acc.alpha = alpha; acc.done = done;
  acc.alpha_accepted = io.alpha_accepted;
  acc.penalty = io.penalty; acc.armijo = io.armijo; acc.shrink = io.shrink; acc.alpha_min = io.alpha_min;
  const RolloutArrays trial = {qt, vt, ut, at, ft};
  // A sample accepted in an early round is rolled out again in the later rounds, about the trajectory it now holds, and that trial is ignored
  // (done[i] != 0): simpler than compacting the batch, and the stream stays free of host decisions.
  for (int round = 0; round < io.trials; ++round) {
    rc = idocp_rbd_ilqr_step_torques_device(h, n, steps, io.u_traj, kff, alpha, u_ff); if (rc) return rc;
    rc = idocp_rbd_rollout_policy_device(h, n, steps, active, time_step, dt, &pol, contact_points, qt, vt, ut, at, ft, touchdown_impulse); if (rc) return rc;
    rc = forEachWindow(h, n, steps, active, trial, [&](int first, int window, int accumulate, const int* act, const RolloutArrays& t) {
      idocp_rbd_score_io_t sc = idocp_rbd_score_io_t();
      sc.q_traj = t.q; sc.v_traj = t.v; sc.u_traj = t.u; sc.a_traj = t.a; sc.f_traj = t.f;
      sc.cost = cost_t; sc.violation = form.penalty() ? nullptr : violation_t;      // (with constraint rows `violation` is their square sum alone, below)
      const int refused = idocp_rbd_score_rollout_device(h, o, n, first, window, act, first + window == steps, accumulate, &sc);
      if (refused || !form.penalty()) return refused;
      if (form.al())      // the trial sq_shifted under the window's multipliers
        return idocp_rbd_score_al_device(h, o, n, first, window, act, accumulate, t.q, t.v, t.u, t.a, t.f, io.penalty,
                                         lambda ? lambda + (size_t)first * N * (size_t)form.multiplier_rows : nullptr, violation_t);
      // the trial sq_violation over the score's L1 violation, window by window the same way
      return idocp_rbd_score_penalty_device(h, o, n, first, window, act, accumulate, t.q, t.v, t.u, t.a, t.f, violation_t);
    });
    if (rc) return rc;
    rc = launchAccept(h, n, steps, acc); if (rc) return rc;
  }
  return IDOCP_OK;
}

// the two forms of the four iterations.  Device: io holds device pointers and the caller's workspace
int iterateEntry(const char* who, IlqrForm::Chain chain, idocp_rbd* h, const idocp_rbd_objective* o, int n, int steps, const int* active, double time_step,
                 double dt, const double* contact_points, const idocp_rbd_ilqr_io_t* io, const double* lambda, int touchdown_impulse) {
  const IlqrForm form(chain, h, o);
  int rc = checkIterate(who, form, h, o, n, steps, io, false); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return iterateDevice(h, o, form, n, steps, active, time_step, dt, contact_points, *io, static_cast<double*>(io->workspace), lambda, touchdown_impulse);
}

// Host: stages once, owns the workspace in the staging buffer, reads back once
int iterateHost(const char* who, IlqrForm::Chain chain, idocp_rbd* h, const idocp_rbd_objective* o, int n, int steps, const int* active, double time_step,
                double dt, const double* contact_points, const idocp_rbd_ilqr_io_t* io, const double* lambda, int touchdown_impulse) {
  const IlqrForm form(chain, h, o);
  int rc = checkIterate(who, form, h, o, n, steps, io, true); if (rc) return rc;
  {      // (the bounds are host memory here and can be looked at)
    idocp_rbd_policy_t bounds = idocp_rbd_policy_t();
    bounds.u_min = io->u_min; bounds.u_max = io->u_max;
    rc = checkPolicy(who, h, &bounds, true); if (rc) return rc;
  }
  if (h->quadruped && !contact_points) { set_last_error(std::string(who) + ": contact_points are needed"); return IDOCP_E_ARG; }
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, S = (size_t)steps;
  StagePlan p;
  idocp_rbd_ilqr_io_t d = *io;
  const double *d_points, *d_lambda;
  double *d_status = nullptr, *d_ws = nullptr;
  p.update(io->q_traj, (S + 1) * N * nq, &d.q_traj);
  p.update(io->v_traj, (S + 1) * N * nv, &d.v_traj);
  p.update(io->u_traj, S * N * nu, &d.u_traj);
  p.update(io->a_traj, S * N * nv, &d.a_traj);
  p.update(io->f_traj, S * N * nf, &d.f_traj);
  p.update(io->cost, N, &d.cost);
  p.update(io->violation, N, &d.violation);
  p.in(io->u_min, nu, &d.u_min);
  p.in(io->u_max, nu, &d.u_max);
  p.in(contact_points, S * N * nf, &d_points);
  p.out(io->alpha_accepted, N, &d.alpha_accepted);
  p.out(io->expected, 2 * N, &d.expected);
  p.deviceOnly((N + 1) / 2, &d_status);
  p.in(lambda, S * N * (size_t)form.multiplier_rows, &d_lambda);      // (no room but on the AL chain)
  p.deviceOnly(ilqrWorkspace(h, form, n, steps).total, &d_ws);
  rc = stageIn(h, p); if (rc) return rc;
  d.lqr_status = reinterpret_cast<int*>(d_status);
  rc = iterateDevice(h, o, form, n, steps, active, time_step, dt, d_points, d, d_ws, d_lambda, touchdown_impulse); if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(io->lqr_status, d_status, sizeof(int) * N, hipMemcpyDeviceToHost, h->stream));
  return stageOut(h, p);
}

}  // namespace

extern "C" {

int idocp_rbd_create(const idocp_model_t* model, int device, idocp_rbd_t** out) {
  if (!model || !out) { set_last_error("idocp_rbd_create: null argument"); return IDOCP_E_ARG; }
  *out = nullptr;
  const bool quad = idocp_host::isQuadruped(*model), chain = idocp_host::isRevoluteChain(*model);
  if (!quad && !chain) {
    set_last_error(std::string("idocp_rbd_create: the rigid-body kernels take ") + idocp_host::QUADRUPED_SHAPE + " or " + idocp_host::CHAIN_RANGE);
    return IDOCP_E_UNSUPPORTED;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    set_last_error("no HIP device available: the idocp HIP path has no CPU fallback");
    return IDOCP_E_DEVICE;
  }
  if (device < 0 || device >= ndev) { set_last_error("invalid device ordinal"); return IDOCP_E_ARG; }
  idocp_rbd* h = new idocp_rbd();
  h->model = *model; h->device = device; h->quadruped = quad;
  h->zaxes = idocp_host::allAxesZ(*model);      // (the instantiation of the chain sweep the solvers and idocp_rnea_derivatives choose for +z axes)
  auto fail = [&](const char* what) { set_last_error(what); (void)hipGetLastError(); idocp_rbd_destroy(h); return IDOCP_E_DEVICE; };
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->stream) != hipSuccess) return fail("hipStreamCreate failed");
  if (hipMalloc(&h->d_model, MODEL_BYTES + sizeof(RbdFrames)) != hipSuccess) return fail("hipMalloc of the model failed");
  DevModel dm; idocp_host::toDevModel(*model, dm);
  RbdFrames fr; std::memset(&fr, 0, sizeof(fr));
  for (int c = 0; c < model->ncontacts; ++c) {
    std::memcpy(fr.R[c], model->contact_R[c], sizeof(double) * 9);
    std::memcpy(fr.p[c], model->contact_p[c], sizeof(double) * 3);
  }
  h->d_frames = reinterpret_cast<const RbdFrames*>(static_cast<char*>(h->d_model) + MODEL_BYTES);
  if (hipMemcpy(h->d_model, &dm, sizeof(dm), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(static_cast<char*>(h->d_model) + MODEL_BYTES, &fr, sizeof(fr), hipMemcpyHostToDevice) != hipSuccess) return fail("upload of the model failed");
  *out = h;
  return IDOCP_OK;
}

void idocp_rbd_destroy(idocp_rbd_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->d_model) (void)hipFree(h->d_model);
  h->stage.release();
  h->unwanted.release();
  h->fd_chain.release();
  h->u_buf.release();
  h->reduce.release();
  h->fdd.release();
  h->lin.release();
  h->gn.release();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int idocp_rbd_synchronize(idocp_rbd_t* h) {
  if (!h) return IDOCP_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

void* idocp_rbd_stream(idocp_rbd_t* h) { return h ? static_cast<void*>(h->stream) : nullptr; }

int idocp_rbd_contact_dynamics_batch_device(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, const idocp_rbd_io_t* io) {
  int rc = checkCall(INVERSE, h, mode, n, active, time_step, io); if (rc) return rc;
  return launch(h, mode, n, active, time_step, *io);
}

int idocp_rbd_contact_dynamics_batch(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, const idocp_rbd_io_t* io) {
  int rc = checkCall(INVERSE, h, mode, n, active, time_step, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n;
  StagePlan p;
  idocp_rbd_io_t d;
  p.in(io->q, N * nq, &d.q);
  p.in(io->v, N * nv, &d.v);
  p.in(io->a, N * nv, &d.a);
  p.in(io->f, N * nf, &d.f);
  p.in(io->contact_points, N * nf, &d.contact_points);
  p.out(io->tau, N * nv, &d.tau);
  p.out(io->dtau_dq, N * nv * nv, &d.dtau_dq);
  p.out(io->dtau_dv, N * nv * nv, &d.dtau_dv);
  p.out(io->dtau_da, N * nv * nv, &d.dtau_da);
  p.out(io->C, N * nf, &d.C);
  p.out(io->dCdq, N * nf * nv, &d.dCdq);
  p.out(io->dCdv, N * nf * nv, &d.dCdv);
  p.out(io->dCda, N * nf * nv, &d.dCda);
  p.out(io->MJtJinv, N * (nv + nf) * (nv + nf), &d.MJtJinv, true);      // (zero-filled: the part of a slot behind the packed block)
  rc = stageIn(h, p); if (rc) return rc;
  rc = launch(h, mode, n, active, time_step, d); if (rc) return rc;
  return stageOut(h, p);
}

int idocp_rbd_forward_dynamics_batch_device(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt, const idocp_rbd_fd_io_t* io) {
  int rc = checkForwardCall(h, mode, n, active, time_step, dt, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchForward(h, mode, n, h->quadruped ? maskOf(h, active) : 0, time_step, dt, *io);
}

int idocp_rbd_forward_dynamics_batch(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt, const idocp_rbd_fd_io_t* io) {
  int rc = checkForwardCall(h, mode, n, active, time_step, dt, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n;
  StagePlan p;
  idocp_rbd_fd_io_t d;
  p.in(io->q, N * nq, &d.q);
  p.in(io->v, N * nv, &d.v);
  p.in(io->u, N * nu, &d.u);
  p.in(io->contact_points, N * nf, &d.contact_points);
  p.out(io->a, N * nv, &d.a);
  p.out(io->f, N * nf, &d.f);
  p.out(io->q_next, N * nq, &d.q_next);
  p.out(io->v_next, N * nv, &d.v_next);
  rc = stageIn(h, p); if (rc) return rc;
  rc = launchForward(h, mode, n, h->quadruped ? maskOf(h, active) : 0, time_step, dt, d); if (rc) return rc;
  return stageOut(h, p);
}

int idocp_rbd_forward_dynamics_derivatives_batch_device(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt,
                                                        const idocp_rbd_fdd_io_t* io) {
  int rc = checkDerivatives("idocp_rbd_forward_dynamics_derivatives_batch_device", h, mode, n, active, time_step, dt, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchDerivatives(h, mode, n, h->quadruped ? maskOf(h, active) : 0, time_step, dt, *io);
}

int idocp_rbd_forward_dynamics_derivatives_batch(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt,
                                                 const idocp_rbd_fdd_io_t* io) {
  int rc = checkDerivatives("idocp_rbd_forward_dynamics_derivatives_batch", h, mode, n, active, time_step, dt, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, nx = 2 * nv;
  StagePlan p;
  idocp_rbd_fdd_io_t d;
  p.in(io->q, N * nq, &d.q);
  p.in(io->v, N * nv, &d.v);
  p.in(io->u, N * nu, &d.u);
  p.in(io->contact_points, N * nf, &d.contact_points);
  p.out(io->a, N * nv, &d.a);
  p.out(io->f, N * nf, &d.f);
  p.out(io->da_dq, N * nv * nv, &d.da_dq);
  p.out(io->da_dv, N * nv * nv, &d.da_dv);
  p.out(io->da_du, N * nv * nu, &d.da_du);
  p.out(io->df_dq, N * nf * nv, &d.df_dq);
  p.out(io->df_dv, N * nf * nv, &d.df_dv);
  p.out(io->df_du, N * nf * nu, &d.df_du);
  p.out(io->A, N * nx * nx, &d.A);
  p.out(io->B, N * nx * nu, &d.B);
  rc = stageIn(h, p); if (rc) return rc;
  rc = launchDerivatives(h, mode, n, h->quadruped ? maskOf(h, active) : 0, time_step, dt, d); if (rc) return rc;
  return stageOut(h, p);
}

int idocp_rbd_linearize_rollout_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u_traj,
                                       const double* contact_points, const double* q_traj, const double* v_traj, double* A_traj, double* B_traj,
                                       int touchdown_impulse) {
  int rc = checkLinearize("idocp_rbd_linearize_rollout", h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return linearizeDevice(h, n, steps, active, time_step, dt, u_traj, contact_points, q_traj, v_traj, A_traj, B_traj, touchdown_impulse);
}

int idocp_rbd_linearize_rollout(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u_traj,
                                const double* contact_points, const double* q_traj, const double* v_traj, double* A_traj, double* B_traj,
                                int touchdown_impulse) {
  int rc = checkLinearize("idocp_rbd_linearize_rollout", h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, S = (size_t)steps, nx = 2 * nv;
  StagePlan p;
  const double *d_u, *d_points, *d_q, *d_v;
  double *d_A, *d_B;
  p.in(u_traj, S * N * nu, &d_u);
  p.in(contact_points, S * N * nf, &d_points);
  p.in(q_traj, (S + 1) * N * nq, &d_q);
  p.in(v_traj, (S + 1) * N * nv, &d_v);
  p.out(A_traj, S * N * nx * nx, &d_A);
  p.out(B_traj, S * N * nx * nu, &d_B);
  rc = stageIn(h, p); if (rc) return rc;
  rc = linearizeDevice(h, n, steps, active, time_step, dt, d_u, d_points, d_q, d_v, d_A, d_B, touchdown_impulse); if (rc) return rc;
  return stageOut(h, p);
}

// A test hook, deliberately NOT in include/idocp_hip.h: an upper bound on the samples one pass of the derivative call takes (0, the default:
// only the 256 MiB cap bounds a pass), handed to idocp_host::fddPlan as its `limit` argument.  It changes the number of launches, never a bit.
int idocp_rbd_set_derivatives_chunk(idocp_rbd_t* h, int max_samples);
int idocp_rbd_set_derivatives_chunk(idocp_rbd_t* h, int max_samples) {
  if (!h) { set_last_error("idocp_rbd_set_derivatives_chunk: null handle"); return IDOCP_E_ARG; }
  if (max_samples < 0) { set_last_error("idocp_rbd_set_derivatives_chunk: max_samples must not be negative (0: no bound)"); return IDOCP_E_ARG; }
  h->fdd_limit = max_samples;
  return IDOCP_OK;
}

int idocp_rbd_rollout_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u, const double* contact_points,
                             double* q_traj, double* v_traj, double* a_traj, double* f_traj, int touchdown_impulse) {
  int rc = checkRollout("idocp_rbd_rollout", h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj, f_traj); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return rolloutDevice(h, n, steps, active, time_step, dt, u, contact_points, q_traj, v_traj, a_traj, f_traj, touchdown_impulse, nullptr, nullptr);
}

int idocp_rbd_rollout(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u, const double* contact_points,
                      double* q_traj, double* v_traj, double* a_traj, double* f_traj, int touchdown_impulse) {
  int rc = checkRollout("idocp_rbd_rollout", h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj, f_traj); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, S = (size_t)steps;
  StagePlan p;
  const double *d_u, *d_points;
  double *d_q, *d_v, *d_a, *d_f;
  p.inout(q_traj, (S + 1) * N * nq, N * nq, &d_q);      // (slice 0 goes up, slices 1 .. S come back)
  p.inout(v_traj, (S + 1) * N * nv, N * nv, &d_v);
  p.in(u, S * N * nu, &d_u);
  p.in(contact_points, S * N * nf, &d_points);
  p.out(a_traj, S * N * nv, &d_a);
  p.out(f_traj, S * N * nf, &d_f);
  rc = stageIn(h, p); if (rc) return rc;
  rc = rolloutDevice(h, n, steps, active, time_step, dt, d_u, d_points, d_q, d_v, d_a, d_f, touchdown_impulse, nullptr, nullptr); if (rc) return rc;
  return stageOut(h, p);
}

int idocp_rbd_feedback_torques_batch_device(idocp_rbd_t* h, int n, const double* q, const double* v, const idocp_rbd_policy_t* pol, double* u) {
  int rc = checkTorques("idocp_rbd_feedback_torques_batch_device", h, n, q, v, pol, u, false); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  launchPolicy(h, n, 0, *pol, q, v, u);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int idocp_rbd_feedback_torques_batch(idocp_rbd_t* h, int n, const double* q, const double* v, const idocp_rbd_policy_t* pol, double* u) {
  int rc = checkTorques("idocp_rbd_feedback_torques_batch", h, n, q, v, pol, u, true); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t N = (size_t)n;
  StagePlan p;
  idocp_rbd_policy_t d_pol;
  const double *d_q, *d_v;
  double* d_u;
  policySlots(p, h, *pol, N, 1, &d_pol);
  p.in(q, N * h->model.nq, &d_q);
  p.in(v, N * h->model.nv, &d_v);
  p.out(u, N * h->model.nu, &d_u);
  rc = stageIn(h, p); if (rc) return rc;
  launchPolicy(h, n, 0, d_pol, d_q, d_v, d_u);
  HIP_TRY(hipGetLastError());
  return stageOut(h, p);
}

int idocp_rbd_rollout_policy_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const idocp_rbd_policy_t* pol,
                                    const double* contact_points, double* q_traj, double* v_traj, double* u_traj, double* a_traj, double* f_traj,
                                    int touchdown_impulse) {
  const char* who = "idocp_rbd_rollout_policy_device";
  int rc = checkRollout(who, h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj, f_traj); if (rc) return rc;
  rc = checkPolicy(who, h, pol, false); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  if (!u_traj) { rc = h->u_buf.grow((size_t)n * h->model.nu, h->stream); if (rc) return rc; }
  return rolloutDevice(h, n, steps, active, time_step, dt, nullptr, contact_points, q_traj, v_traj, a_traj, f_traj, touchdown_impulse, pol, u_traj);
}

int idocp_rbd_rollout_policy(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const idocp_rbd_policy_t* pol,
                             const double* contact_points, double* q_traj, double* v_traj, double* u_traj, double* a_traj, double* f_traj,
                             int touchdown_impulse) {
  const char* who = "idocp_rbd_rollout_policy";
  int rc = checkRollout(who, h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj, f_traj); if (rc) return rc;
  rc = checkPolicy(who, h, pol, true); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, S = (size_t)steps;
  if (!u_traj) { rc = h->u_buf.grow(N * nu, h->stream); if (rc) return rc; }
  StagePlan p;
  idocp_rbd_policy_t d_pol;
  const double* d_points;
  double *d_q, *d_v, *d_u, *d_a, *d_f;
  policySlots(p, h, *pol, N, S, &d_pol);
  p.inout(q_traj, (S + 1) * N * nq, N * nq, &d_q);      // (slice 0 goes up, slices 1 .. S come back)
  p.inout(v_traj, (S + 1) * N * nv, N * nv, &d_v);
  p.in(contact_points, S * N * nf, &d_points);
  p.out(u_traj, S * N * nu, &d_u);
  p.out(a_traj, S * N * nv, &d_a);
  p.out(f_traj, S * N * nf, &d_f);
  rc = stageIn(h, p); if (rc) return rc;
  rc = rolloutDevice(h, n, steps, active, time_step, dt, nullptr, d_points, d_q, d_v, d_a, d_f, touchdown_impulse, &d_pol, d_u); if (rc) return rc;
  return stageOut(h, p);
}

int idocp_rbd_contact_kinematics_batch_device(idocp_rbd_t* h, int n, const idocp_rbd_kin_io_t* io) {
  int rc = checkKinematics("idocp_rbd_contact_kinematics_batch_device", h, n, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  rbdKinematicsQuadruped(static_cast<const DevModel*>(h->d_model), h->d_frames, *io, n, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int idocp_rbd_contact_kinematics_batch(idocp_rbd_t* h, int n, const idocp_rbd_kin_io_t* io) {
  int rc = checkKinematics("idocp_rbd_contact_kinematics_batch", h, n, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n;
  StagePlan p;
  idocp_rbd_kin_io_t d;
  p.in(io->q, N * nq, &d.q);
  p.in(io->velocity ? io->v : nullptr, N * nv, &d.v);      // (v is read for the velocity alone)
  p.out(io->points, N * nf, &d.points);
  p.out(io->rotation, N * nf * 3, &d.rotation);
  p.out(io->velocity, N * nf, &d.velocity);
  p.out(io->jacobian, N * nf * nv, &d.jacobian);
  rc = stageIn(h, p); if (rc) return rc;
  rbdKinematicsQuadruped(static_cast<const DevModel*>(h->d_model), h->d_frames, d, n, h->stream);
  HIP_TRY(hipGetLastError());
  return stageOut(h, p);
}

int idocp_rbd_rollout_footholds_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt,
                                       const idocp_rbd_foothold_rollout_t* io, int touchdown_impulse, int latch_first) {
  int rc = checkFootholds("idocp_rbd_rollout_footholds_device", h, n, steps, active, time_step, dt, io, false); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  if (io->policy && !io->u_traj) { rc = h->u_buf.grow((size_t)n * h->model.nu, h->stream); if (rc) return rc; }
  return rolloutDevice(h, n, steps, active, time_step, dt, io->u, io->contact_points, io->q_traj, io->v_traj, io->a_traj, io->f_traj, touchdown_impulse,
                       io->policy, io->policy ? io->u_traj : nullptr, io->contact_points, latch_first);
}

int idocp_rbd_rollout_footholds(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt,
                                const idocp_rbd_foothold_rollout_t* io, int touchdown_impulse, int latch_first) {
  int rc = checkFootholds("idocp_rbd_rollout_footholds", h, n, steps, active, time_step, dt, io, true); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, S = (size_t)steps;
  if (io->policy && !io->u_traj) { rc = h->u_buf.grow(N * nu, h->stream); if (rc) return rc; }
  StagePlan p;
  idocp_rbd_policy_t d_pol;
  const double* d_u;
  double *d_points, *d_q, *d_v, *d_ut, *d_a, *d_f;
  if (io->policy) policySlots(p, h, *io->policy, N, S, &d_pol);
  p.inout(io->q_traj, (S + 1) * N * nq, N * nq, &d_q);      // (slice 0 goes up, slices 1 .. S come back)
  p.inout(io->v_traj, (S + 1) * N * nv, N * nv, &d_v);
  p.in(io->u, S * N * nu, &d_u);
  p.inoutAll(io->contact_points, S * N * nf, N * nf, &d_points);      // (slice 0 goes up, every slice comes back)
  p.out(io->policy ? io->u_traj : nullptr, S * N * nu, &d_ut);
  p.out(io->a_traj, S * N * nv, &d_a);
  p.out(io->f_traj, S * N * nf, &d_f);
  rc = stageIn(h, p); if (rc) return rc;
  rc = rolloutDevice(h, n, steps, active, time_step, dt, d_u, d_points, d_q, d_v, d_a, d_f, touchdown_impulse, io->policy ? &d_pol : nullptr, d_ut,
                     d_points, latch_first);
  if (rc) return rc;
  return stageOut(h, p);
}

int idocp_rbd_objective_create(idocp_rbd_t* h, const idocp_cost_t* cost, const idocp_constraints_t* constraints, double t0, double dt, int steps,
                               idocp_rbd_objective_t** out) {
  if (!h || !out) { set_last_error("idocp_rbd_objective_create: null handle or out"); return IDOCP_E_ARG; }
  *out = nullptr;
  idocp_rbd_objective* o = new idocp_rbd_objective();
  o->plan = idocp_host::planObjective(h->model, h->quadruped, cost, constraints, t0, dt, steps);
  if (o->plan.rc) { const int rc = o->plan.rc; set_last_error(o->plan.error); delete o; return rc; }
  o->owner = h;
  const size_t nq_tab = (o->plan.q_ref.size() + 1) / 2 * 2, nv_tab = (o->plan.v_ref.size() + 1) / 2 * 2;      // (16-byte pieces)
  auto fail = [&](const char* what) { set_last_error(what); (void)hipGetLastError(); idocp_rbd_objective_destroy(o); return IDOCP_E_DEVICE; };
  if (hipSetDevice(h->device) != hipSuccess) return fail("idocp_rbd_objective_create: hipSetDevice failed");
  o->lqr_weights.resize((size_t)idocp_host::lqrWeightDoubles(o->plan));
  idocp_host::lqrWeights(o->plan, o->lqr_weights.data());
  const size_t block_bytes = (sizeof(idocp_host::RbdScoreBlock) + 15) / 16 * 16;
  const size_t weights_tab = (o->lqr_weights.size() + 1) / 2 * 2;
  std::vector<double> residual((size_t)2 * idocp_host::residualRows(o->plan));
  idocp_host::residualTable(o->plan, residual.data());      // (a negative weight leaves a NaN here; the calls that read the table refuse it)
  if (hipMalloc(reinterpret_cast<void**>(&o->d_q_ref), sizeof(double) * (nq_tab + nv_tab + weights_tab + residual.size()) + block_bytes) != hipSuccess)
    return fail("idocp_rbd_objective_create: hipMalloc of the objective failed");
  o->d_v_ref = o->d_q_ref + nq_tab;
  o->d_block = reinterpret_cast<idocp_host::RbdScoreBlock*>(o->d_v_ref + nv_tab);
  o->d_lqr_weights = reinterpret_cast<double*>(reinterpret_cast<char*>(o->d_block) + block_bytes);
  o->d_residual = o->d_lqr_weights + weights_tab;
  if (hipMemcpyAsync(o->d_q_ref, o->plan.q_ref.data(), sizeof(double) * o->plan.q_ref.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(o->d_v_ref, o->plan.v_ref.data(), sizeof(double) * o->plan.v_ref.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(o->d_block, &o->plan.block, sizeof(idocp_host::RbdScoreBlock), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(o->d_lqr_weights, o->lqr_weights.data(), sizeof(double) * o->lqr_weights.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(o->d_residual, residual.data(), sizeof(double) * residual.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipStreamSynchronize(h->stream) != hipSuccess) return fail("idocp_rbd_objective_create: upload of the objective failed");
  *out = o;
  return IDOCP_OK;
}

void idocp_rbd_objective_destroy(idocp_rbd_objective_t* o) {
  if (!o) return;
  if (o->d_q_ref) {
    (void)hipSetDevice(o->owner->device);
    (void)hipStreamSynchronize(o->owner->stream);
    (void)hipFree(o->d_q_ref);
  }
  delete o;
}

int idocp_rbd_objective_get_reference(const idocp_rbd_objective_t* o, int k, double* q_ref, double* v_ref) {
  if (!o) { set_last_error("idocp_rbd_objective_get_reference: null objective"); return IDOCP_E_ARG; }
  if (k < 0 || k > o->plan.steps) { set_last_error("idocp_rbd_objective_get_reference: k must be 0 .. steps"); return IDOCP_E_ARG; }
  if (q_ref) std::memcpy(q_ref, &o->plan.q_ref[(size_t)k * o->plan.nq], sizeof(double) * o->plan.nq);
  if (v_ref) std::memcpy(v_ref, &o->plan.v_ref[(size_t)k * o->plan.nv], sizeof(double) * o->plan.nv);
  return IDOCP_OK;
}

int idocp_rbd_objective_reference_device(const idocp_rbd_objective_t* o, const double** d_q_ref, const double** d_v_ref) {
  if (!o) { set_last_error("idocp_rbd_objective_reference_device: null objective"); return IDOCP_E_ARG; }
  if (d_q_ref) *d_q_ref = o->d_q_ref;
  if (d_v_ref) *d_v_ref = o->d_v_ref;
  return IDOCP_OK;
}

int idocp_rbd_score_rollout_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int terminal,
                                   int accumulate, const idocp_rbd_score_io_t* io) {
  RbdScoreArgs a;
  int rc = checkScore("idocp_rbd_score_rollout_device", h, o, n, first_step, steps, active, terminal, accumulate, io, &a); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  a.q = io->q_traj; a.v = io->v_traj; a.u = io->u_traj; a.a = io->a_traj; a.f = io->f_traj;
  a.cost = io->cost; a.violation = io->violation; a.stage_cost = io->stage_cost;
  rbdScore(h->model.nv, h->quadruped, a, n, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int idocp_rbd_score_rollout(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int terminal,
                            int accumulate, const idocp_rbd_score_io_t* io) {
  RbdScoreArgs a;
  int rc = checkScore("idocp_rbd_score_rollout", h, o, n, first_step, steps, active, terminal, accumulate, io, &a); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)o->plan.ncontacts, N = (size_t)n, S = (size_t)steps;
  const size_t slices = S + (terminal ? 1 : 0);
  StagePlan p;
  p.in(io->q_traj, slices * N * nq, &a.q);
  p.in(io->v_traj, slices * N * nv, &a.v);
  p.in(io->u_traj, S * N * nu, &a.u);
  p.in(io->a_traj, S * N * nv, &a.a);
  p.in(io->f_traj, S * N * nf, &a.f);
  if (accumulate) { p.update(io->cost, N, &a.cost); p.update(io->violation, N, &a.violation); }
  else { p.out(io->cost, N, &a.cost); p.out(io->violation, N, &a.violation); }
  p.out(io->stage_cost, slices * N, &a.stage_cost);
  rc = stageIn(h, p); if (rc) return rc;
  rbdScore(h->model.nv, h->quadruped, a, n, h->stream);
  HIP_TRY(hipGetLastError());
  return stageOut(h, p);
}

int idocp_rbd_perturb_torques_device(idocp_rbd_t* h, int n, int first_step, int steps, const double* u_nominal, const double* sigma, const double* u_min,
                                     const double* u_max, unsigned long long seed, unsigned draw, double* u_samples) {
  int rc = checkPerturb("idocp_rbd_perturb_torques_device", h, n, first_step, steps, u_nominal, sigma, u_min, u_max, u_samples, false); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchPerturb(h, n, first_step, steps, u_nominal, sigma, u_min, u_max, seed, draw, u_samples);
}

int idocp_rbd_perturb_torques(idocp_rbd_t* h, int n, int first_step, int steps, const double* u_nominal, const double* sigma, const double* u_min,
                              const double* u_max, unsigned long long seed, unsigned draw, double* u_samples) {
  int rc = checkPerturb("idocp_rbd_perturb_torques", h, n, first_step, steps, u_nominal, sigma, u_min, u_max, u_samples, true); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nu = h->model.nu, N = (size_t)n, S = (size_t)steps;
  StagePlan p;
  const double *d_nominal, *d_sigma, *d_min, *d_max;
  double* d_samples;
  p.in(u_nominal, S * nu, &d_nominal);
  p.in(sigma, nu, &d_sigma);
  p.in(u_min, nu, &d_min);
  p.in(u_max, nu, &d_max);
  p.out(u_samples, S * N * nu, &d_samples);
  rc = stageIn(h, p); if (rc) return rc;
  rc = launchPerturb(h, n, first_step, steps, d_nominal, d_sigma, d_min, d_max, seed, draw, d_samples); if (rc) return rc;
  return stageOut(h, p);
}

int idocp_rbd_importance_weights_device(idocp_rbd_t* h, int n, const double* cost, const double* violation, double penalty, double temperature,
                                        double* weights, double* stats) {
  int rc = checkWeights("idocp_rbd_importance_weights_device", h, n, cost, penalty, temperature, weights, stats); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchWeights(h, n, cost, violation, penalty, temperature, weights, stats);
}

int idocp_rbd_importance_weights(idocp_rbd_t* h, int n, const double* cost, const double* violation, double penalty, double temperature,
                                 double* weights, double* stats) {
  int rc = checkWeights("idocp_rbd_importance_weights", h, n, cost, penalty, temperature, weights, stats); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  StagePlan p;
  const double *d_cost, *d_violation;
  double *d_weights, *d_stats;
  p.in(cost, (size_t)n, &d_cost);
  p.in(violation, (size_t)n, &d_violation);
  p.out(weights, (size_t)n, &d_weights);
  p.out(stats, IDOCP_RBD_WEIGHT_STATS, &d_stats);
  rc = stageIn(h, p); if (rc) return rc;
  rc = launchWeights(h, n, d_cost, d_violation, penalty, temperature, d_weights, d_stats); if (rc) return rc;
  return stageOut(h, p);
}

int idocp_rbd_weighted_mean_device(idocp_rbd_t* h, int n, int rows, int m, const double* weights, const double* x, double* mean) {
  int rc = checkMean("idocp_rbd_weighted_mean_device", h, n, rows, m, weights, x, mean, false); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchMean(h, n, rows, m, weights, x, mean);
}

int idocp_rbd_weighted_mean(idocp_rbd_t* h, int n, int rows, int m, const double* weights, const double* x, double* mean) {
  int rc = checkMean("idocp_rbd_weighted_mean", h, n, rows, m, weights, x, mean, true); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  StagePlan p;
  const double *d_weights, *d_x;
  double* d_mean;
  p.in(weights, (size_t)n, &d_weights);
  p.in(x, (size_t)rows * n * m, &d_x);
  p.out(mean, (size_t)rows * m, &d_mean);
  rc = stageIn(h, p); if (rc) return rc;
  rc = launchMean(h, n, rows, m, d_weights, d_x, d_mean); if (rc) return rc;
  return stageOut(h, p);
}

int idocp_rbd_lqr_backward_device(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io) {
  int rc = checkLqrCall("idocp_rbd_lqr_backward_device", h, n, steps, io, false, 0, nullptr, nullptr); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchLqr(h, n, steps, *io, 0, nullptr, nullptr);
}

int idocp_rbd_lqr_backward(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io) {
  return lqrHost("idocp_rbd_lqr_backward", h, n, steps, io, 0, nullptr, nullptr);
}

int idocp_rbd_lqr_backward_gn_device(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io, int g_rows, const double* G_traj) {
  int rc = checkLqrCall("idocp_rbd_lqr_backward_gn_device", h, n, steps, io, false, g_rows, G_traj, nullptr); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchLqr(h, n, steps, *io, g_rows, G_traj, nullptr);
}

int idocp_rbd_lqr_backward_gn(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io, int g_rows, const double* G_traj) {
  return lqrHost("idocp_rbd_lqr_backward_gn", h, n, steps, io, g_rows, G_traj, nullptr);
}

int idocp_rbd_objective_residual_rows(const idocp_rbd_objective_t* o) { return o ? idocp_host::residualRows(o->plan) : 0; }

int idocp_rbd_linearize_rollout_cost_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step,
                                            double dt, const double* u_traj, const double* contact_points, const double* q_traj,
                                            const double* v_traj, const idocp_rbd_cost_linearization_io_t* io, int touchdown_impulse) {
  idocp_rbd_penalty_linearization_io_t wide;
  return linearizeRowsEntry("idocp_rbd_linearize_rollout_cost_device", IlqrForm::GN, h, o, n, steps, active, time_step, dt, u_traj, contact_points, q_traj, v_traj,
                            widened(io, &wide), 0.0, nullptr, touchdown_impulse);
}

int idocp_rbd_linearize_rollout_cost(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                     const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                                     const idocp_rbd_cost_linearization_io_t* io, int touchdown_impulse) {
  idocp_rbd_penalty_linearization_io_t wide;
  return linearizeRowsHost("idocp_rbd_linearize_rollout_cost", IlqrForm::GN, h, o, n, steps, active, time_step, dt, u_traj, contact_points, q_traj, v_traj,
                           widened(io, &wide), 0.0, nullptr, touchdown_impulse);
}

int idocp_rbd_objective_gradients_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, int terminal,
                                         const idocp_rbd_gradient_io_t* io) {
  RbdGradientArgs a;
  int rc = checkGradients("idocp_rbd_objective_gradients_device", h, o, n, first_step, steps, terminal, io, &a); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  a.q = io->q_traj; a.v = io->v_traj; a.u = io->u_traj; a.lx = io->lx_traj; a.lu = io->lu_traj;
  rbdGradient(h->model.nv, h->quadruped, a, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int idocp_rbd_objective_gradients(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, int terminal,
                                  const idocp_rbd_gradient_io_t* io) {
  RbdGradientArgs a;
  int rc = checkGradients("idocp_rbd_objective_gradients", h, o, n, first_step, steps, terminal, io, &a); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, N = (size_t)n, S = (size_t)steps, slices = S + (terminal ? 1 : 0);
  StagePlan p;
  p.in(io->q_traj, slices * N * nq, &a.q);
  p.in(io->v_traj, slices * N * nv, &a.v);
  p.in(io->u_traj, S * N * nu, &a.u);
  p.out(io->lx_traj, slices * N * 2 * nv, &a.lx);
  p.out(io->lu_traj, S * N * nu, &a.lu);
  rc = stageIn(h, p); if (rc) return rc;
  rbdGradient(h->model.nv, h->quadruped, a, h->stream);
  HIP_TRY(hipGetLastError());
  return stageOut(h, p);
}

int idocp_rbd_objective_lqr_weights_device(const idocp_rbd_objective_t* o, const double** d_x_weight, const double** d_u_weight,
                                           const double** d_xf_weight) {
  int rc = checkLqrWeights("idocp_rbd_objective_lqr_weights_device", o); if (rc) return rc;
  if (d_x_weight) *d_x_weight = o->d_lqr_weights;
  if (d_u_weight) *d_u_weight = o->d_lqr_weights + idocp_host::lqrWeightOffsetU(o->plan);
  if (d_xf_weight) *d_xf_weight = o->d_lqr_weights + idocp_host::lqrWeightOffsetXf(o->plan);
  return IDOCP_OK;
}

int idocp_rbd_objective_get_lqr_weights(const idocp_rbd_objective_t* o, double* x_weight, double* u_weight, double* xf_weight) {
  int rc = checkLqrWeights("idocp_rbd_objective_get_lqr_weights", o); if (rc) return rc;
  const double* w = o->lqr_weights.data();
  if (x_weight) std::memcpy(x_weight, w, sizeof(double) * 2 * o->plan.nv);
  if (u_weight) std::memcpy(u_weight, w + idocp_host::lqrWeightOffsetU(o->plan), sizeof(double) * o->plan.nu);
  if (xf_weight) std::memcpy(xf_weight, w + idocp_host::lqrWeightOffsetXf(o->plan), sizeof(double) * 2 * o->plan.nv);
  return IDOCP_OK;
}

int idocp_rbd_ilqr_step_torques_device(idocp_rbd_t* h, int n, int steps, const double* u_traj, const double* k_traj, const double* alpha,
                                       double* u_ff) {
  int rc = checkStepTorques("idocp_rbd_ilqr_step_torques_device", h, n, steps, u_traj, k_traj, alpha, u_ff); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  rbdIlqrStepTorques(u_traj, k_traj, alpha, u_ff, n, steps, h->model.nu, h->stream);
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

int idocp_rbd_ilqr_step_torques(idocp_rbd_t* h, int n, int steps, const double* u_traj, const double* k_traj, const double* alpha, double* u_ff) {
  int rc = checkStepTorques("idocp_rbd_ilqr_step_torques", h, n, steps, u_traj, k_traj, alpha, u_ff); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t count = (size_t)steps * n * h->model.nu;
  StagePlan p;
  const double *d_u, *d_k, *d_alpha;
  double* d_out;
  p.in(u_traj, count, &d_u);
  p.in(k_traj, count, &d_k);
  p.in(alpha, (size_t)n, &d_alpha);
  p.out(u_ff, count, &d_out);
  rc = stageIn(h, p); if (rc) return rc;
  rbdIlqrStepTorques(d_u, d_k, d_alpha, d_out, n, steps, h->model.nu, h->stream);
  HIP_TRY(hipGetLastError());
  return stageOut(h, p);
}

int idocp_rbd_ilqr_accept_device(idocp_rbd_t* h, int n, int steps, const idocp_rbd_ilqr_accept_io_t* io) {
  int rc = checkAccept("idocp_rbd_ilqr_accept_device", h, n, steps, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchAccept(h, n, steps, *io);
}

int idocp_rbd_ilqr_accept(idocp_rbd_t* h, int n, int steps, const idocp_rbd_ilqr_accept_io_t* io) {
  int rc = checkAccept("idocp_rbd_ilqr_accept", h, n, steps, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, S = (size_t)steps;
  StagePlan p;
  idocp_rbd_ilqr_accept_io_t d = *io;
  double* d_done = nullptr;
  const bool with_a = io->a_traj && io->trial_a, with_f = io->f_traj && io->trial_f;
  p.update(io->q_traj, (S + 1) * N * nq, &d.q_traj);
  p.update(io->v_traj, (S + 1) * N * nv, &d.v_traj);
  p.update(io->u_traj, S * N * nu, &d.u_traj);
  p.update(with_a ? io->a_traj : nullptr, S * N * nv, &d.a_traj);
  p.update(with_f ? io->f_traj : nullptr, S * N * nf, &d.f_traj);
  p.update(io->cost, N, &d.cost);
  p.update(io->violation, N, &d.violation);
  p.in(io->trial_q, (S + 1) * N * nq, &d.trial_q);
  p.in(io->trial_v, (S + 1) * N * nv, &d.trial_v);
  p.in(io->trial_u, S * N * nu, &d.trial_u);
  p.in(with_a ? io->trial_a : nullptr, S * N * nv, &d.trial_a);
  p.in(with_f ? io->trial_f : nullptr, S * N * nf, &d.trial_f);
  p.in(io->trial_cost, N, &d.trial_cost);
  p.in(io->trial_violation, N, &d.trial_violation);
  p.in(io->expected, 2 * N, &d.expected);
  p.update(io->alpha, N, &d.alpha);
  p.update(io->alpha_accepted, N, &d.alpha_accepted);
  p.deviceOnly((N + 1) / 2, &d_done);      // (n ints in a slot of doubles; they travel by copies of their own)
  rc = stageIn(h, p); if (rc) return rc;
  d.done = reinterpret_cast<int*>(d_done);
  HIP_TRY(hipMemcpyAsync(d.done, io->done, sizeof(int) * N, hipMemcpyHostToDevice, h->stream));
  rc = launchAccept(h, n, steps, d); if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(io->done, d.done, sizeof(int) * N, hipMemcpyDeviceToHost, h->stream));
  return stageOut(h, p);
}

unsigned long long idocp_rbd_ilqr_workspace_bytes(const idocp_rbd_t* h, int n, int steps) {
  if (!h || n <= 0 || steps < 1) return 0;
  return sizeof(double) * (unsigned long long)ilqrWorkspace(h, IlqrForm(IlqrForm::DIAGONAL, h, nullptr), n, steps).total;
}

int idocp_rbd_ilqr_iterate_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                  const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse) {
  return iterateEntry("idocp_rbd_ilqr_iterate_device", IlqrForm::DIAGONAL, h, o, n, steps, active, time_step, dt, contact_points, io, nullptr, touchdown_impulse);
}

int idocp_rbd_ilqr_iterate(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                           const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse) {
  return iterateHost("idocp_rbd_ilqr_iterate", IlqrForm::DIAGONAL, h, o, n, steps, active, time_step, dt, contact_points, io, nullptr, touchdown_impulse);
}

unsigned long long idocp_rbd_ilqr_gn_workspace_bytes(const idocp_rbd_t* h, int n, int steps) {
  if (!h || n <= 0 || steps < 1) return 0;
  return sizeof(double) * (unsigned long long)ilqrWorkspace(h, IlqrForm(IlqrForm::GN, h, nullptr), n, steps).total;      // (the cost rows of any objective of the handle)
}

int idocp_rbd_ilqr_iterate_gn_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                     const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse) {
  return iterateEntry("idocp_rbd_ilqr_iterate_gn_device", IlqrForm::GN, h, o, n, steps, active, time_step, dt, contact_points, io, nullptr, touchdown_impulse);
}

int idocp_rbd_ilqr_iterate_gn(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                              const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse) {
  return iterateHost("idocp_rbd_ilqr_iterate_gn", IlqrForm::GN, h, o, n, steps, active, time_step, dt, contact_points, io, nullptr, touchdown_impulse);
}

// ---- the constraint rows as a squared-hinge penalty

int idocp_rbd_objective_constraint_rows(const idocp_rbd_objective_t* o) { return o ? idocp_host::constraintRows(o->plan) : 0; }

int idocp_rbd_score_penalty_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                                   const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj,
                                   double* sq_violation) {
  return rowCallDevice("idocp_rbd_score_penalty_device", SCORE_PENALTY, h, o, n, first_step, steps, active, accumulate, {q_traj, v_traj, u_traj, a_traj, f_traj}, 0.0, nullptr, sq_violation, nullptr, nullptr);
}

int idocp_rbd_score_penalty(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                            const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj,
                            double* sq_violation) {
  return rowCallHost("idocp_rbd_score_penalty", SCORE_PENALTY, h, o, n, first_step, steps, active, accumulate, {q_traj, v_traj, u_traj, a_traj, f_traj}, 0.0, nullptr, sq_violation, nullptr, nullptr);
}

int idocp_rbd_linearize_rollout_penalty_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step,
                                               double dt, const double* u_traj, const double* contact_points, const double* q_traj,
                                               const double* v_traj, const idocp_rbd_penalty_linearization_io_t* io, double mu, int touchdown_impulse) {
  return linearizeRowsEntry("idocp_rbd_linearize_rollout_penalty_device", IlqrForm::PENALTY, h, o, n, steps, active, time_step, dt, u_traj, contact_points, q_traj,
                            v_traj, io, mu, nullptr, touchdown_impulse);
}

int idocp_rbd_linearize_rollout_penalty(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                        const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                                        const idocp_rbd_penalty_linearization_io_t* io, double mu, int touchdown_impulse) {
  return linearizeRowsHost("idocp_rbd_linearize_rollout_penalty", IlqrForm::PENALTY, h, o, n, steps, active, time_step, dt, u_traj, contact_points, q_traj, v_traj,
                           io, mu, nullptr, touchdown_impulse);
}

int idocp_rbd_lqr_backward_gn_diag_device(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io, int g_rows, const double* G_traj,
                                          const double* D_traj) {
  int rc = checkLqrCall("idocp_rbd_lqr_backward_gn_diag_device", h, n, steps, io, false, g_rows, G_traj, D_traj); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchLqr(h, n, steps, *io, g_rows, G_traj, D_traj);
}

int idocp_rbd_lqr_backward_gn_diag(idocp_rbd_t* h, int n, int steps, const idocp_rbd_lqr_io_t* io, int g_rows, const double* G_traj,
                                   const double* D_traj) {
  return lqrHost("idocp_rbd_lqr_backward_gn_diag", h, n, steps, io, g_rows, G_traj, D_traj);
}

unsigned long long idocp_rbd_ilqr_penalty_workspace_bytes(const idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps) {
  if (!h || !o || o->owner != h || n <= 0 || steps < 1) return 0;
  return sizeof(double) * (unsigned long long)ilqrWorkspace(h, IlqrForm(IlqrForm::PENALTY, h, o), n, steps).total;
}

int idocp_rbd_ilqr_iterate_penalty_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step,
                                          double dt, const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse) {
  return iterateEntry("idocp_rbd_ilqr_iterate_penalty_device", IlqrForm::PENALTY, h, o, n, steps, active, time_step, dt, contact_points, io, nullptr, touchdown_impulse);
}

int idocp_rbd_ilqr_iterate_penalty(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                   const double* contact_points, const idocp_rbd_ilqr_io_t* io, int touchdown_impulse) {
  return iterateHost("idocp_rbd_ilqr_iterate_penalty", IlqrForm::PENALTY, h, o, n, steps, active, time_step, dt, contact_points, io, nullptr, touchdown_impulse);
}

// ---- the augmented Lagrangian: multipliers on the constraint rows

int idocp_rbd_objective_multiplier_rows(const idocp_rbd_objective_t* o) { return o ? idocp_host::multiplierRows(o->plan) : 0; }

int idocp_rbd_score_al_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                              const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu,
                              const double* lambda_traj, double* sq_shifted) {
  return rowCallDevice("idocp_rbd_score_al_device", SCORE_AL, h, o, n, first_step, steps, active, accumulate, {q_traj, v_traj, u_traj, a_traj, f_traj}, mu, lambda_traj, sq_shifted, nullptr, nullptr);
}

int idocp_rbd_score_al(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                       const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu,
                       const double* lambda_traj, double* sq_shifted) {
  return rowCallHost("idocp_rbd_score_al", SCORE_AL, h, o, n, first_step, steps, active, accumulate, {q_traj, v_traj, u_traj, a_traj, f_traj}, mu, lambda_traj, sq_shifted, nullptr, nullptr);
}

int idocp_rbd_multiplier_update_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                                       const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj,
                                       double mu, const double* lambda_traj, double* lambda_out, double* infeasibility, double* multiplier_change) {
  return rowCallDevice("idocp_rbd_multiplier_update_device", MULTIPLIER_UPDATE, h, o, n, first_step, steps, active, accumulate, {q_traj, v_traj, u_traj, a_traj, f_traj}, mu, lambda_traj, lambda_out,
                       infeasibility, multiplier_change);
}

int idocp_rbd_multiplier_update(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int first_step, int steps, const int* active, int accumulate,
                                const double* q_traj, const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu,
                                const double* lambda_traj, double* lambda_out, double* infeasibility, double* multiplier_change) {
  return rowCallHost("idocp_rbd_multiplier_update", MULTIPLIER_UPDATE, h, o, n, first_step, steps, active, accumulate, {q_traj, v_traj, u_traj, a_traj, f_traj}, mu, lambda_traj, lambda_out,
                       infeasibility, multiplier_change);
}

int idocp_rbd_linearize_rollout_al_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                          const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                                          const idocp_rbd_penalty_linearization_io_t* io, double mu, const double* lambda_traj, int touchdown_impulse) {
  return linearizeRowsEntry("idocp_rbd_linearize_rollout_al_device", IlqrForm::AL, h, o, n, steps, active, time_step, dt, u_traj, contact_points, q_traj, v_traj,
                            io, mu, lambda_traj, touchdown_impulse);
}

int idocp_rbd_linearize_rollout_al(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                   const double* u_traj, const double* contact_points, const double* q_traj, const double* v_traj,
                                   const idocp_rbd_penalty_linearization_io_t* io, double mu, const double* lambda_traj, int touchdown_impulse) {
  return linearizeRowsHost("idocp_rbd_linearize_rollout_al", IlqrForm::AL, h, o, n, steps, active, time_step, dt, u_traj, contact_points, q_traj, v_traj, io, mu,
                           lambda_traj, touchdown_impulse);
}

int idocp_rbd_ilqr_iterate_al_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                                     const double* contact_points, const idocp_rbd_ilqr_io_t* io, const double* lambda_traj, int touchdown_impulse) {
  return iterateEntry("idocp_rbd_ilqr_iterate_al_device", IlqrForm::AL, h, o, n, steps, active, time_step, dt, contact_points, io, lambda_traj, touchdown_impulse);
}

int idocp_rbd_ilqr_iterate_al(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, double time_step, double dt,
                              const double* contact_points, const idocp_rbd_ilqr_io_t* io, const double* lambda_traj, int touchdown_impulse) {
  return iterateHost("idocp_rbd_ilqr_iterate_al", IlqrForm::AL, h, o, n, steps, active, time_step, dt, contact_points, io, lambda_traj, touchdown_impulse);
}

namespace {
// every pointer: device memory.  The outer step: the multipliers in place under mu, window by window with the running maxima, then `violation`
// = sq_shifted under the new multipliers and mu_next, window by window with accumulate.  A window that refuses leaves the inner call's name in
// idocp_last_error.
int alUpdateDevice(idocp_rbd* h, const idocp_rbd_objective* o, int n, int steps, const int* active, const RolloutArrays& t, double mu, double mu_next,
                   double* lambda, double* violation, double* infeasibility, double* change) {
  const size_t per_step = (size_t)n * (size_t)idocp_host::multiplierRows(o->plan);
  for (int pass = 0; pass < 2; ++pass) {
    const int rc = forEachWindow(h, n, steps, active, t, [&](int first, int window, int accumulate, const int* act, const RolloutArrays& w) {
      double* const lk = lambda ? lambda + first * per_step : nullptr;
      if (pass == 0) return idocp_rbd_multiplier_update_device(h, o, n, first, window, act, accumulate, w.q, w.v, w.u, w.a, w.f, mu, lk, lk, infeasibility, change);
      return idocp_rbd_score_al_device(h, o, n, first, window, act, accumulate, w.q, w.v, w.u, w.a, w.f, mu_next, lk, violation);
    });
    if (rc) return rc;
  }
  return IDOCP_OK;
}

int checkAlUpdate(const char* who, const idocp_rbd* h, const idocp_rbd_objective* o, int n, int steps, const double* q, const double* v, double mu,
                  double mu_next, const double* lambda, const double* violation) {
  const std::string w(who);
  if (!h || !o) { set_last_error(w + ": null handle or objective"); return IDOCP_E_ARG; }
  if (o->owner != h) { set_last_error(w + ": the objective was created on another handle"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error(w + ": n must be positive"); return IDOCP_E_ARG; }
  if (steps < 1 || steps > o->plan.steps) { set_last_error(w + ": steps must lie within 1 .. the objective's " + std::to_string(o->plan.steps) + " steps"); return IDOCP_E_ARG; }
  if (!q || !v) { set_last_error(w + ": q_traj and v_traj are needed"); return IDOCP_E_ARG; }
  if (!violation) { set_last_error(w + ": violation is needed"); return IDOCP_E_ARG; }
  if (!lambda && idocp_host::multiplierRows(o->plan)) { set_last_error(w + ": lambda_traj is needed (the update is in place)"); return IDOCP_E_ARG; }
  int rc = checkMu(who, mu, "mu"); if (rc) return rc;
  return checkMu(who, mu_next, "mu_next");
}
}  // namespace

int idocp_rbd_ilqr_al_update_device(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, const double* q_traj,
                                    const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu, double mu_next,
                                    double* lambda_traj, double* violation, double* infeasibility, double* multiplier_change) {
  int rc = checkAlUpdate("idocp_rbd_ilqr_al_update_device", h, o, n, steps, q_traj, v_traj, mu, mu_next, lambda_traj, violation); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return alUpdateDevice(h, o, n, steps, active, {q_traj, v_traj, u_traj, a_traj, f_traj}, mu, mu_next, lambda_traj, violation, infeasibility, multiplier_change);
}

int idocp_rbd_ilqr_al_update(idocp_rbd_t* h, const idocp_rbd_objective_t* o, int n, int steps, const int* active, const double* q_traj,
                             const double* v_traj, const double* u_traj, const double* a_traj, const double* f_traj, double mu, double mu_next,
                             double* lambda_traj, double* violation, double* infeasibility, double* multiplier_change) {
  int rc = checkAlUpdate("idocp_rbd_ilqr_al_update", h, o, n, steps, q_traj, v_traj, mu, mu_next, lambda_traj, violation); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t N = (size_t)n;
  StagePlan p;
  RolloutArrays d;
  double *d_lambda, *d_violation, *d_inf, *d_change;
  stageRollout(p, h, o, n, steps, {q_traj, v_traj, u_traj, a_traj, f_traj}, &d);
  p.update(lambda_traj, (size_t)steps * N * (size_t)idocp_host::multiplierRows(o->plan), &d_lambda);
  p.out(violation, N, &d_violation);
  p.out(infeasibility, N, &d_inf, true);
  p.out(multiplier_change, N, &d_change, true);
  rc = stageIn(h, p); if (rc) return rc;
  rc = alUpdateDevice(h, o, n, steps, active, d, mu, mu_next, d_lambda, d_violation, d_inf, d_change); if (rc) return rc;
  return stageOut(h, p);
}

}  // extern "C"
