// C-ABI implementation of the batched rigid-body API (include/idocp_hip.h: idocp_rbd_*).
//
// Host side only: a handle owns the model in device memory, a stream and the staging buffers of the host-pointer form; the terms
// themselves come from rbd_batch_kernel.hip (quadruped) or from the sweep of the fixed-base solvers (UnLaunch<NV>::rneaDerivatives).
// There is NO CPU fallback: without a GPU idocp_rbd_create returns IDOCP_E_DEVICE.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "host_util.hpp"
#include "idocp_hip.h"
#include "model_shapes.hpp"
#include "rbd_launch.hpp"
#include "unocp_launch.hpp"

using namespace idocp_dev;
using idocp_host::set_last_error;

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      set_last_error(std::string(#expr) + ": " + hipGetErrorString(e_));                      \
      (void)hipGetLastError(); /* HIP keeps a failed call as the thread's "last error": reported here, it must not fail the next handle's launches */ \
      return IDOCP_E_DEVICE;                                                                  \
    }                                                                                         \
  } while (0)

struct idocp_rbd {
  idocp_model_t model;
  int device = 0;
  bool quadruped = false, zaxes = false;
  hipStream_t stream = nullptr;
  void* d_model = nullptr;            // DevModel, then RbdFrames
  const RbdFrames* d_frames = nullptr;
  double* stage = nullptr;            // host-pointer form: inputs and outputs of one call
  size_t stage_doubles = 0;
  double* unwanted = nullptr;         // chain: where the sweep writes the outputs the caller did not ask for
  size_t unwanted_doubles = 0;
  double* fd_chain = nullptr;         // chain, forward dynamics: [a = 0 | h | dtau_dq | dtau_dv | M] of the sweep at a = 0
  size_t fd_chain_doubles = 0;
  double* u_buf = nullptr;            // closed-loop rollout without u_traj: the torques of the current step, [n][nu]
  size_t u_buf_doubles = 0;
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

int growBuffer(double** buf, size_t* have, size_t want, hipStream_t st) {
  if (want <= *have) return IDOCP_OK;
  if (*buf) { HIP_TRY(hipStreamSynchronize(st)); HIP_TRY(hipFree(*buf)); *buf = nullptr; *have = 0; }
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(buf), sizeof(double) * want));
  *have = want;
  return IDOCP_OK;
}

// doubles per sample of every field of idocp_rbd_io_t, in the order of the struct
struct FieldSizes { size_t in[5], out[9]; };
FieldSizes fieldSizes(const idocp_rbd* h) {
  const size_t nq = h->model.nq, nv = h->model.nv, nf = 3 * (size_t)h->model.ncontacts;
  return {{nq, nv, nv, nf, nf}, {nv, nv * nv, nv * nv, nv * nv, nf, nf * nv, nf * nv, nf * nv, (nv + nf) * (nv + nf)}};
}

int checkCall(const idocp_rbd* h, int mode, int n, const int* active, double time_step, const idocp_rbd_io_t* io) {
  if (!h || !io) { set_last_error("idocp_rbd_contact_dynamics_batch: null handle or io"); return IDOCP_E_ARG; }
  if (n <= 0) { set_last_error("idocp_rbd_contact_dynamics_batch: n must be positive"); return IDOCP_E_ARG; }
  if (mode != IDOCP_RBD_STAGE && mode != IDOCP_RBD_IMPULSE) { set_last_error("idocp_rbd_contact_dynamics_batch: unknown mode"); return IDOCP_E_ARG; }
  if (!io->q || !io->v || !io->a) { set_last_error("idocp_rbd_contact_dynamics_batch: q, v and a are needed"); return IDOCP_E_ARG; }
  const bool contact_out = io->C || io->dCdq || io->dCdv || io->dCda || io->MJtJinv;
  if (!h->quadruped) {
    if (io->f || io->contact_points || contact_out) {
      set_last_error("idocp_rbd_contact_dynamics_batch: a fixed-base chain has no contacts (f, contact_points and the contact outputs must be NULL)");
      return IDOCP_E_ARG;
    }
    if (mode != IDOCP_RBD_STAGE) { set_last_error("idocp_rbd_contact_dynamics_batch: a fixed-base chain has no impulse mode"); return IDOCP_E_ARG; }
    return IDOCP_OK;
  }
  if (!active) { set_last_error("idocp_rbd_contact_dynamics_batch: the contact status `active` is needed"); return IDOCP_E_ARG; }
  if (mode == IDOCP_RBD_STAGE) {
    if (io->C && !io->contact_points) { set_last_error("idocp_rbd_contact_dynamics_batch: C in STAGE mode needs contact_points"); return IDOCP_E_ARG; }
    if ((io->C || io->dCdq || io->dCdv) && !(time_step > 0.0)) {
      set_last_error("idocp_rbd_contact_dynamics_batch: the Baumgarte terms need a positive time_step"); return IDOCP_E_ARG;
    }
  }
  return IDOCP_OK;
}

// io: device pointers
int launch(idocp_rbd* h, int mode, int n, const int* active, double time_step, const idocp_rbd_io_t& io) {
  HIP_TRY(hipSetDevice(h->device));
  const DevModel* d_m = static_cast<const DevModel*>(h->d_model);
  if (h->quadruped) {
    int mask = 0;
    for (int c = 0; c < h->model.ncontacts; ++c) if (active[c]) mask |= 1 << c;
    // (dC/da and MJtJinv do not depend on the Baumgarte time step: any positive number serves where none was given)
    rbdBatchQuadruped(d_m, h->d_frames, io, n, mode, mask, (mode == IDOCP_RBD_STAGE && !(time_step > 0.0)) ? 1.0 : time_step, h->stream);
  } else {
    const size_t nv = h->model.nv, nvec = (size_t)n * nv, nmat = nvec * nv;
    double *tau = io.tau, *dq = io.dtau_dq, *dv = io.dtau_dv, *da = io.dtau_da;
    if (!tau || !dq || !dv || !da) {
      int rc = growBuffer(&h->unwanted, &h->unwanted_doubles, nvec + 3 * nmat, h->stream); if (rc) return rc;
      if (!tau) tau = h->unwanted;
      if (!dq) dq = h->unwanted + nvec;
      if (!dv) dv = h->unwanted + nvec + nmat;
      if (!da) da = h->unwanted + nvec + 2 * nmat;
    }
    chainFn(h->model.nv)(d_m, n, io.q, io.v, io.a, tau, dq, dv, da, h->zaxes, h->stream);
  }
  HIP_TRY(hipGetLastError());
  return IDOCP_OK;
}

// ---- forward dynamics ----

int checkForward(const char* who, const idocp_rbd* h, int mode, int n, const int* active, double time_step, double dt, const double* q, const double* v,
                 const double* contact_points, bool contact_args) {
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
  (void)contact_points; (void)time_step;
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

int maskOf(const idocp_rbd* h, const int* active) {
  int mask = 0;
  for (int c = 0; c < h->model.ncontacts; ++c) if (active[c]) mask |= 1 << c;
  return mask;
}

// io: device pointers; quadruped: mask = the contact / impulse status
int launchForward(idocp_rbd* h, int mode, int n, int mask, double time_step, double dt, const idocp_rbd_fd_io_t& io) {
  const DevModel* d_m = static_cast<const DevModel*>(h->d_model);
  if (h->quadruped) {
    rbdForwardQuadruped(d_m, h->d_frames, io, n, mode, mask, time_step, dt, h->stream);
  } else if (io.a || io.q_next || io.v_next) {
    const size_t nv = h->model.nv, nvec = (size_t)n * nv, nmat = nvec * nv;
    if (2 * nvec + 3 * nmat > h->fd_chain_doubles) {
      int rc = growBuffer(&h->fd_chain, &h->fd_chain_doubles, 2 * nvec + 3 * nmat, h->stream); if (rc) return rc;
    }
    double *zero = h->fd_chain, *hh = zero + nvec, *dq = hh + nvec, *dv = dq + nmat, *M = dv + nmat;
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

// doubles per sample of every field of idocp_rbd_fd_io_t, in the order of the struct
struct FdSizes { size_t in[4], out[4]; };
FdSizes fdSizes(const idocp_rbd* h) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts;
  return {{nq, nv, nu, nf}, {nv, nf, nq, nv}};
}
size_t even(size_t x) { return (x + 1) / 2 * 2; }

int checkForwardCall(idocp_rbd* h, int mode, int n, const int* active, double time_step, double dt, const idocp_rbd_fd_io_t* io) {
  const char* who = "idocp_rbd_forward_dynamics_batch";
  if (!io) { set_last_error(std::string(who) + ": null io"); return IDOCP_E_ARG; }
  int rc = checkForward(who, h, mode, n, active, time_step, dt, io->q, io->v, io->contact_points, io->f || io->contact_points); if (rc) return rc;
  if (mode == IDOCP_RBD_STAGE) { rc = checkStageContacts(who, h, active, time_step, io->contact_points); if (rc) return rc; }
  return IDOCP_OK;
}

// the schedule of a rollout: per step the stage mask and the mask of the touchdown impulse in front of it (0: none)
int checkRollout(const char* who, idocp_rbd* h, int n, int steps, const int* active, double time_step, double dt, const double* contact_points,
                 const double* q_traj, const double* v_traj, const double* f_traj) {
  if (steps < 1) { set_last_error(std::string(who) + ": steps must be at least 1"); return IDOCP_E_ARG; }
  int rc = checkForward(who, h, IDOCP_RBD_STAGE, n, active, time_step, dt, q_traj, v_traj, contact_points, f_traj || contact_points);
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
                  double* q_traj, double* v_traj, double* a_traj, double* f_traj, int touchdown_impulse, const idocp_rbd_policy_t* pol = nullptr,
                  double* u_traj = nullptr) {
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n;
  int prev = 0;
  for (int k = 0; k < steps; ++k) {
    const int mask = h->quadruped ? maskOf(h, active + (size_t)k * h->model.ncontacts) : 0;
    double *qk = q_traj + k * N * nq, *vk = v_traj + k * N * nv;
    if (touchdown_impulse && k > 0 && (mask & ~prev)) {
      idocp_rbd_fd_io_t imp = idocp_rbd_fd_io_t();
      imp.q = qk; imp.v = vk; imp.v_next = vk;            // (in place: slice k becomes the post-impulse velocity)
      int rc = launchForward(h, IDOCP_RBD_IMPULSE, n, mask & ~prev, time_step, dt, imp); if (rc) return rc;
    }
    idocp_rbd_fd_io_t io = idocp_rbd_fd_io_t();
    io.q = qk; io.v = vk;
    if (pol) {
      double* uk = u_traj ? u_traj + k * N * nu : h->u_buf;
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

// The host form of a policy: its arrays behind one another in the staging buffer.  sizes(): doubles of [u_ff | K | q_ref | v_ref | u_min | u_max].
struct PolicyStage {
  size_t sz[6];
  const double* host[6];
  PolicyStage(const idocp_rbd* h, const idocp_rbd_policy_t& p, size_t N, size_t S) {
    const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nk = nu * 2 * nv;
    const size_t full[6] = {S * N * nu, S * (p.shared_gains ? 1 : N) * nk, S * (p.shared_ref ? 1 : N) * nq, S * (p.shared_ref ? 1 : N) * nv, nu, nu};
    const double* ptr[6] = {p.u_ff, p.K, p.K ? p.q_ref : nullptr, p.K ? p.v_ref : nullptr, p.u_min, p.u_max};
    for (int i = 0; i < 6; ++i) { host[i] = ptr[i]; sz[i] = ptr[i] ? full[i] : 0; }
  }
  size_t total() const { size_t t = 0; for (int i = 0; i < 6; ++i) t += even(sz[i]); return t; }
  // uploads on st from `cur` on; d: the policy with device pointers; returns the first double behind it
  int upload(double* cur, hipStream_t st, const idocp_rbd_policy_t& p, idocp_rbd_policy_t* d, double** end) const {
    const double* dev[6];
    for (int i = 0; i < 6; ++i) {
      dev[i] = sz[i] ? cur : nullptr;
      if (sz[i]) HIP_TRY(hipMemcpyAsync(cur, host[i], sizeof(double) * sz[i], hipMemcpyHostToDevice, st));
      cur += even(sz[i]);
    }
    *d = p;
    d->u_ff = dev[0]; d->K = dev[1]; d->q_ref = dev[2]; d->v_ref = dev[3]; d->u_min = dev[4]; d->u_max = dev[5];
    *end = cur;
    return IDOCP_OK;
  }
};

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
  h->zaxes = true;      // (the instantiation of the chain sweep the solvers and idocp_rnea_derivatives choose for +z axes)
  for (int i = 0; i < model->njoints; ++i) if (!(model->axis[i][0] == 0.0 && model->axis[i][1] == 0.0 && model->axis[i][2] == 1.0)) h->zaxes = false;
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
  if (h->stage) (void)hipFree(h->stage);
  if (h->unwanted) (void)hipFree(h->unwanted);
  if (h->fd_chain) (void)hipFree(h->fd_chain);
  if (h->u_buf) (void)hipFree(h->u_buf);
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
  int rc = checkCall(h, mode, n, active, time_step, io); if (rc) return rc;
  return launch(h, mode, n, active, time_step, *io);
}

int idocp_rbd_contact_dynamics_batch(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, const idocp_rbd_io_t* io) {
  int rc = checkCall(h, mode, n, active, time_step, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const FieldSizes fs = fieldSizes(h);
  const double* const host_in[5] = {io->q, io->v, io->a, io->f, io->contact_points};
  double* const host_out[9] = {io->tau, io->dtau_dq, io->dtau_dv, io->dtau_da, io->C, io->dCdq, io->dCdv, io->dCda, io->MJtJinv};
  size_t total = 0;
  for (int i = 0; i < 5; ++i) if (host_in[i]) total += (fs.in[i] * n + 1) / 2 * 2;
  for (int i = 0; i < 9; ++i) if (host_out[i]) total += (fs.out[i] * n + 1) / 2 * 2;
  rc = growBuffer(&h->stage, &h->stage_doubles, total, h->stream); if (rc) return rc;
  const double* dev_in[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  double* dev_out[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double* cur = h->stage;
  for (int i = 0; i < 5; ++i) if (host_in[i]) {
    HIP_TRY(hipMemcpyAsync(cur, host_in[i], sizeof(double) * fs.in[i] * n, hipMemcpyHostToDevice, h->stream));
    dev_in[i] = cur; cur += (fs.in[i] * n + 1) / 2 * 2;
  }
  for (int i = 0; i < 9; ++i) if (host_out[i]) { dev_out[i] = cur; cur += (fs.out[i] * n + 1) / 2 * 2; }
  idocp_rbd_io_t d;
  d.q = dev_in[0]; d.v = dev_in[1]; d.a = dev_in[2]; d.f = dev_in[3]; d.contact_points = dev_in[4];
  d.tau = dev_out[0]; d.dtau_dq = dev_out[1]; d.dtau_dv = dev_out[2]; d.dtau_da = dev_out[3];
  d.C = dev_out[4]; d.dCdq = dev_out[5]; d.dCdv = dev_out[6]; d.dCda = dev_out[7]; d.MJtJinv = dev_out[8];
  if (d.MJtJinv) HIP_TRY(hipMemsetAsync(d.MJtJinv, 0, sizeof(double) * fs.out[8] * n, h->stream));      // (the part of a slot behind the packed block)
  rc = launch(h, mode, n, active, time_step, d); if (rc) return rc;
  for (int i = 0; i < 9; ++i) if (host_out[i])
    HIP_TRY(hipMemcpyAsync(host_out[i], dev_out[i], sizeof(double) * fs.out[i] * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

int idocp_rbd_forward_dynamics_batch_device(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt, const idocp_rbd_fd_io_t* io) {
  int rc = checkForwardCall(h, mode, n, active, time_step, dt, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return launchForward(h, mode, n, h->quadruped ? maskOf(h, active) : 0, time_step, dt, *io);
}

int idocp_rbd_forward_dynamics_batch(idocp_rbd_t* h, int mode, int n, const int* active, double time_step, double dt, const idocp_rbd_fd_io_t* io) {
  int rc = checkForwardCall(h, mode, n, active, time_step, dt, io); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const FdSizes fs = fdSizes(h);
  const double* const host_in[4] = {io->q, io->v, io->u, io->contact_points};
  double* const host_out[4] = {io->a, io->f, io->q_next, io->v_next};
  size_t total = 0;
  for (int i = 0; i < 4; ++i) if (host_in[i]) total += even(fs.in[i] * n);
  for (int i = 0; i < 4; ++i) if (host_out[i]) total += even(fs.out[i] * n);
  rc = growBuffer(&h->stage, &h->stage_doubles, total, h->stream); if (rc) return rc;
  const double* dev_in[4] = {nullptr, nullptr, nullptr, nullptr};
  double* dev_out[4] = {nullptr, nullptr, nullptr, nullptr};
  double* cur = h->stage;
  for (int i = 0; i < 4; ++i) if (host_in[i]) {
    HIP_TRY(hipMemcpyAsync(cur, host_in[i], sizeof(double) * fs.in[i] * n, hipMemcpyHostToDevice, h->stream));
    dev_in[i] = cur; cur += even(fs.in[i] * n);
  }
  for (int i = 0; i < 4; ++i) if (host_out[i]) { dev_out[i] = cur; cur += even(fs.out[i] * n); }
  idocp_rbd_fd_io_t d;
  d.q = dev_in[0]; d.v = dev_in[1]; d.u = dev_in[2]; d.contact_points = dev_in[3];
  d.a = dev_out[0]; d.f = dev_out[1]; d.q_next = dev_out[2]; d.v_next = dev_out[3];
  rc = launchForward(h, mode, n, h->quadruped ? maskOf(h, active) : 0, time_step, dt, d); if (rc) return rc;
  for (int i = 0; i < 4; ++i) if (host_out[i])
    HIP_TRY(hipMemcpyAsync(host_out[i], dev_out[i], sizeof(double) * fs.out[i] * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

int idocp_rbd_rollout_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u, const double* contact_points,
                             double* q_traj, double* v_traj, double* a_traj, double* f_traj, int touchdown_impulse) {
  int rc = checkRollout("idocp_rbd_rollout", h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj, f_traj); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return rolloutDevice(h, n, steps, active, time_step, dt, u, contact_points, q_traj, v_traj, a_traj, f_traj, touchdown_impulse);
}

int idocp_rbd_rollout(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const double* u, const double* contact_points,
                      double* q_traj, double* v_traj, double* a_traj, double* f_traj, int touchdown_impulse) {
  int rc = checkRollout("idocp_rbd_rollout", h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj, f_traj); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, nf = 3 * (size_t)h->model.ncontacts, N = (size_t)n, S = (size_t)steps;
  // [q_traj | v_traj | u | contact_points | a_traj | f_traj]: staged once, read back once
  const size_t sz[6] = {(S + 1) * N * nq, (S + 1) * N * nv, u ? S * N * nu : 0, contact_points ? S * N * nf : 0, a_traj ? S * N * nv : 0, f_traj ? S * N * nf : 0};
  size_t total = 0;
  for (int i = 0; i < 6; ++i) total += even(sz[i]);
  rc = growBuffer(&h->stage, &h->stage_doubles, total, h->stream); if (rc) return rc;
  double* dev[6];
  double* cur = h->stage;
  for (int i = 0; i < 6; ++i) { dev[i] = sz[i] ? cur : nullptr; cur += even(sz[i]); }
  HIP_TRY(hipMemcpyAsync(dev[0], q_traj, sizeof(double) * N * nq, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(dev[1], v_traj, sizeof(double) * N * nv, hipMemcpyHostToDevice, h->stream));
  if (u) HIP_TRY(hipMemcpyAsync(dev[2], u, sizeof(double) * sz[2], hipMemcpyHostToDevice, h->stream));
  if (contact_points) HIP_TRY(hipMemcpyAsync(dev[3], contact_points, sizeof(double) * sz[3], hipMemcpyHostToDevice, h->stream));
  rc = rolloutDevice(h, n, steps, active, time_step, dt, dev[2], dev[3], dev[0], dev[1], dev[4], dev[5], touchdown_impulse); if (rc) return rc;
  // (slice 0 of v_traj comes back too; it is the input)
  HIP_TRY(hipMemcpyAsync(q_traj + N * nq, dev[0] + N * nq, sizeof(double) * S * N * nq, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(v_traj + N * nv, dev[1] + N * nv, sizeof(double) * S * N * nv, hipMemcpyDeviceToHost, h->stream));
  if (a_traj) HIP_TRY(hipMemcpyAsync(a_traj, dev[4], sizeof(double) * sz[4], hipMemcpyDeviceToHost, h->stream));
  if (f_traj) HIP_TRY(hipMemcpyAsync(f_traj, dev[5], sizeof(double) * sz[5], hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
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
  const size_t nq = h->model.nq, nv = h->model.nv, nu = h->model.nu, N = (size_t)n;
  const PolicyStage ps(h, *pol, N, 1);
  rc = growBuffer(&h->stage, &h->stage_doubles, ps.total() + even(N * nq) + even(N * nv) + even(N * nu), h->stream); if (rc) return rc;
  idocp_rbd_policy_t d;
  double* cur = nullptr;
  rc = ps.upload(h->stage, h->stream, *pol, &d, &cur); if (rc) return rc;
  double *dq = cur, *dv = dq + even(N * nq), *du = dv + even(N * nv);
  HIP_TRY(hipMemcpyAsync(dq, q, sizeof(double) * N * nq, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(dv, v, sizeof(double) * N * nv, hipMemcpyHostToDevice, h->stream));
  launchPolicy(h, n, 0, d, dq, dv, du);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(u, du, sizeof(double) * N * nu, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

int idocp_rbd_rollout_policy_device(idocp_rbd_t* h, int n, int steps, const int* active, double time_step, double dt, const idocp_rbd_policy_t* pol,
                                    const double* contact_points, double* q_traj, double* v_traj, double* u_traj, double* a_traj, double* f_traj,
                                    int touchdown_impulse) {
  const char* who = "idocp_rbd_rollout_policy_device";
  int rc = checkRollout(who, h, n, steps, active, time_step, dt, contact_points, q_traj, v_traj, f_traj); if (rc) return rc;
  rc = checkPolicy(who, h, pol, false); if (rc) return rc;
  HIP_TRY(hipSetDevice(h->device));
  if (!u_traj) { rc = growBuffer(&h->u_buf, &h->u_buf_doubles, (size_t)n * h->model.nu, h->stream); if (rc) return rc; }
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
  const PolicyStage ps(h, *pol, N, S);
  // [policy | q_traj | v_traj | contact_points | u_traj | a_traj | f_traj]: staged once, read back once
  const size_t sz[6] = {(S + 1) * N * nq, (S + 1) * N * nv, contact_points ? S * N * nf : 0, u_traj ? S * N * nu : 0, a_traj ? S * N * nv : 0, f_traj ? S * N * nf : 0};
  size_t total = ps.total();
  for (int i = 0; i < 6; ++i) total += even(sz[i]);
  rc = growBuffer(&h->stage, &h->stage_doubles, total, h->stream); if (rc) return rc;
  if (!u_traj) { rc = growBuffer(&h->u_buf, &h->u_buf_doubles, N * nu, h->stream); if (rc) return rc; }
  idocp_rbd_policy_t d;
  double* cur = nullptr;
  rc = ps.upload(h->stage, h->stream, *pol, &d, &cur); if (rc) return rc;
  double* dev[6];
  for (int i = 0; i < 6; ++i) { dev[i] = sz[i] ? cur : nullptr; cur += even(sz[i]); }
  HIP_TRY(hipMemcpyAsync(dev[0], q_traj, sizeof(double) * N * nq, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(dev[1], v_traj, sizeof(double) * N * nv, hipMemcpyHostToDevice, h->stream));
  if (contact_points) HIP_TRY(hipMemcpyAsync(dev[2], contact_points, sizeof(double) * sz[2], hipMemcpyHostToDevice, h->stream));
  rc = rolloutDevice(h, n, steps, active, time_step, dt, nullptr, dev[2], dev[0], dev[1], dev[4], dev[5], touchdown_impulse, &d, dev[3]); if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(q_traj + N * nq, dev[0] + N * nq, sizeof(double) * S * N * nq, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(v_traj + N * nv, dev[1] + N * nv, sizeof(double) * S * N * nv, hipMemcpyDeviceToHost, h->stream));
  if (u_traj) HIP_TRY(hipMemcpyAsync(u_traj, dev[3], sizeof(double) * sz[3], hipMemcpyDeviceToHost, h->stream));
  if (a_traj) HIP_TRY(hipMemcpyAsync(a_traj, dev[4], sizeof(double) * sz[4], hipMemcpyDeviceToHost, h->stream));
  if (f_traj) HIP_TRY(hipMemcpyAsync(f_traj, dev[5], sizeof(double) * sz[5], hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return IDOCP_OK;
}

}  // extern "C"
