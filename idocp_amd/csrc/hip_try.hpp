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
