// HIP_TRY: a HIP call of a C-ABI function; a failure becomes idocp_last_error() and IDOCP_E_DEVICE.  For the .hip units only (host_util.hpp is
// also included by .cpp units that are built without HIP).
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "host_util.hpp"
#include "idocp_hip.h"

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      idocp_host::set_last_error(std::string(#expr) + ": " + hipGetErrorString(e_));          \
      (void)hipGetLastError(); /* HIP keeps a failed call as the thread's "last error": reported here, it must not fail the next handle's launches */ \
      return IDOCP_E_DEVICE;                                                                  \
    }                                                                                         \
  } while (0)

// A host temporary (a stack object, a local vector) to the device, complete on return: the stream is synchronised even when the copy call itself
// reports an error, so no way out of the caller leaves a copy in flight from a frame that is gone.
inline int uploadTemporary(void* d_dst, const void* h_src, size_t bytes, hipStream_t stream) {
  const hipError_t copied = hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, stream);
  const hipError_t waited = hipStreamSynchronize(stream);
  HIP_TRY(copied);
  HIP_TRY(waited);
  return IDOCP_OK;
}
