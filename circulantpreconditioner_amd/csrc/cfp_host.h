// cfp_host.h -- host-side helpers shared by the plan, the real plan, the slab-distributed plan and
// the PETSc-interface layer: the error plumbing, the device guard, the twiddles and the natural
// pass geometry.  The symbols' arithmetic and the z route are cfp_symbol.h's, included here.
#pragma once
#include <hip/hip_runtime.h>

#include <complex>
#include <cstdarg>
#include <vector>

#include "cfp_internal.h"
#include "cfp_symbol.h"

namespace cfp {
int set_error(int code, const char* fmt, ...);
int hip_error(hipError_t e, const char* what);
std::vector<cd> host_twiddles(int n, int sign);
int ilog2_exact(i64 v);
Side natural_side(int axis, const i64 n[3]);
void natural_cols(int axis, const i64 n[3], i64* ncols, i64* inner_n);

// makes `dev` the current device for a scope
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    hipGetDevice(&prev);
    if (prev != dev) hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur;
    hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) hipSetDevice(prev);
  }
};
}  // namespace cfp

// internal plan option used by the real (r2c) plan, cfp_plan.hip
extern "C" int cfp_plan_set_external_x(struct cfp_plan_s* plan, int on);
