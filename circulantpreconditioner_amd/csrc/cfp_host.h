// cfp_host.h -- host-side helpers shared by the plan, the real plan, the two wave plans, the
// slab-distributed plan and the PETSc-interface layer: the error plumbing (HIPCHK / CFPCHK), the
// device guard and check, the twiddle cache, the natural pass geometry, the wave field's pass
// descriptor and the per-pass timer (all defined in cfp_plan.hip).  The symbols' arithmetic and
// the z route are cfp_symbol.h's, included here; the wave family's are cfp_wave_host.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <complex>
#include <cstdarg>
#include <functional>
#include <map>
#include <vector>

#include "cfp_internal.h"
#include "cfp_symbol.h"

#define HIPCHK(expr)                                        \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) return cfp::hip_error(_e, #expr); \
  } while (0)
#define CFPCHK(expr)                  \
  do {                                \
    int _r = (expr);                  \
    if (_r != CFP_SUCCESS) return _r; \
  } while (0)

namespace cfp {
int set_error(int code, const char* fmt, ...);
int hip_error(hipError_t e, const char* what);
int check_device(int device);  // CFP_ERR_ARG_OUTOFRANGE unless 0 <= device < the device count
std::vector<cd> host_twiddles(int n, int sign);
int ilog2_exact(i64 v);
Side natural_side(int axis, const i64 n[3]);
void natural_cols(int axis, const i64 n[3], i64* ncols, i64* inner_n);

// Device forward twiddles W_n per length n, uploaded on first use.  The owner calls clear() under
// its DeviceGuard before it goes away.
struct TwiddleCache {
  std::map<int, cd*> tab;
  int get(int n, cd** out);
  cd* at(int n) const { return tab.at(n); }
  void clear();
};

// The y / z / fused pass (axis 1 or 2) over an interleaved wave field of ncomp components on the
// grid g0 x n1 x n2: the scalar pass of a grid whose x extent is ncomp g0 (the components ride
// along x as extra columns), with the per-axis (p, q) tables, c0 and the fused axis of the solve.
// (Axis 0: the same descriptor with that grid's natural x geometry, which the complex wave plan
// replaces by its strided columns.)
PassDesc wave_field_pass(int ncomp, i64 g0, i64 n1, i64 n2, const double2* const tab[3], double c0, int fused,
                         int axis, int mode, double scale);

// Mean milliseconds per pass over `iters` runs of `run`, which records into the events it is
// given: one per pass boundary (np + 1 events), or, `paired`, a start and a stop per pass (2 np).
int time_passes(size_t np, bool paired, int iters, const std::function<int(std::vector<hipEvent_t>*)>& run,
                double* ms_out);

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
