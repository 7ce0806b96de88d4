// cfp_host.h -- host-side helpers shared by the plan, the slab-distributed plan and the
// PETSc-interface layer.
#pragma once
#include <hip/hip_runtime.h>

#include <complex>
#include <cstdarg>
#include <vector>

#include "cfp_internal.h"

namespace cfp {
int set_error(int code, const char* fmt, ...);
int hip_error(hipError_t e, const char* what);
std::vector<cd> host_twiddles(int n, int sign);
std::vector<cd> host_transport_symbol(i64 n);
// the advection-diffusion symbol's 1-D parts and the factors of its two-sided z recurrence
// (cfp_plan.hip; the real plan builds its half-spectrum tables from the same functions)
std::vector<cd> host_advdiff_symbol(i64 n, std::complex<double> lam, std::complex<double> mu);
std::complex<double> advdiff_z_beta(cd x, cd y, std::complex<double> p, std::complex<double> q);
void advdiff_z_ratio(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz,
                     std::complex<double> mz, double ratios[2]);
std::vector<cd> advdiff_z_table(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz,
                                std::complex<double> mz, int nxt);
// two scans, eps / ((1 - |a|) (1 - |b|)): this cap keeps 8 eps / (1 - r)^2 at 2.9e-11
constexpr double kZrec2MaxRatio = 1.0 - 1.0 / 128.0;
int ilog2_exact(i64 v);
Side natural_side(int axis, const i64 n[3]);
void natural_cols(int axis, const i64 n[3], i64* ncols, i64* inner_n);
}  // namespace cfp

// internal plan option used by the real (r2c) plan, cfp_plan.hip
extern "C" int cfp_plan_set_external_x(struct cfp_plan_s* plan, int on);
