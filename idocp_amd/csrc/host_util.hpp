// Small host-side helpers shared by the C-ABI translation units.
#ifndef IDOCP_HOST_UTIL_HPP_
#define IDOCP_HOST_UTIL_HPP_

#include <cstdlib>
#include <string>

#include "idocp_hip.h"

namespace idocp_host {

// Thread-local message returned by idocp_last_error().
void set_last_error(const std::string& msg);
const char* last_error();

// What the library takes from the process environment, read here and nowhere else.  Everything else that selects a kernel form is a
// per-handle setting (ocp_forms.hpp).
//   IDOCP_GENERAL_AXES  (set: tests) the general rigid-body instantiations on a model that qualifies for the special ones
//   IDOCP_PROF_DIMF     (diagnostic) the K5 stage class, by its contact rows, that writes the clock stamps of idocp_ocp_get_profile
struct EnvSettings { bool general_axes; int prof_dimf; };
inline EnvSettings envSettings() {
  const char* dimf = std::getenv("IDOCP_PROF_DIMF");
  return {std::getenv("IDOCP_GENERAL_AXES") != nullptr, dimf ? std::atoi(dimf) : 12};
}
// every joint axis is +z: the chain sweeps have an instantiation for it
inline bool allAxesZ(const idocp_model_t& m) {
  for (int i = 0; i < m.njoints; ++i) if (!(m.axis[i][0] == 0.0 && m.axis[i][1] == 0.0 && m.axis[i][2] == 1.0)) return false;
  return true;
}

}  // namespace idocp_host

#endif  // IDOCP_HOST_UTIL_HPP_
