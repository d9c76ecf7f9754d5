// Host-visible launch wrapper of the batched rigid-body kernel (defined in rbd_batch_kernel.hip).
#ifndef IDOCP_RBD_LAUNCH_HPP_
#define IDOCP_RBD_LAUNCH_HPP_

#include <hip/hip_runtime.h>

#include "dev_rbd.hpp"
#include "idocp_hip.h"

namespace idocp_dev {

// placement of the contact frames in their tip joints (row-major rotation), behind the model in device memory
struct RbdFrames {
  double R[IDOCP_MAX_CONTACTS][9], p[IDOCP_MAX_CONTACTS][3];
};

// One wavefront per sample, RBD_WAVES samples per workgroup.  io: DEVICE pointers; active_mask: bit c = contact c is active.
constexpr int RBD_WAVES = 2;
void rbdBatchQuadruped(const DevModel* m, const RbdFrames* frames, const idocp_rbd_io_t& io, int n, int mode, int active_mask,
                       double time_step, hipStream_t st);

}  // namespace idocp_dev
#endif  // IDOCP_RBD_LAUNCH_HPP_
