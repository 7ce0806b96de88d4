// cfp_symbol.h -- host arithmetic of the closed-form symbols (transport, advection-diffusion,
// upwind) and of the 256^3 z route: the per-axis tables, their column sums, the z ratios, the
// two-sided recurrence's column table and the rule "which middle kernel does this symbol get".
// Plain functions on host vectors (cfp_symbol.cpp): no HIP runtime calls, no error state.  The
// complex plan, the real plan and the z-slab plan all decide here.
#pragma once
#include <array>
#include <complex>
#include <vector>

#include "../../include/circulant_fft.h"
#include "cfp_internal.h"

namespace cfp {

typedef std::array<std::vector<cd>, 3> AxisTables;

std::vector<cd> host_transport_symbol(i64 n);
// hat[k] * lam: one axis' part of a separable symbol (the transport setters' tables)
std::vector<cd> transport_product(const std::vector<cd>& hat, std::complex<double> lam);
std::vector<cd> host_advdiff_symbol(i64 n, std::complex<double> lam, std::complex<double> mu);
// host_advdiff_symbol of the three axes, lam6 and mu6 as (re, im) per axis
AxisTables axis_symbols(const i64 n[3], const double lam6[6], const double mu6[6]);
// col[kx + stride ky] = sx[kx0 + kx] + sy[ky0 + ky], kx < nkx, ky < nky (stride * nky values)
std::vector<cd> column_sums(const std::vector<cd>& sx, i64 kx0, i64 nkx, const std::vector<cd>& sy, i64 ky0, i64 nky,
                            i64 stride);
// cfp_upwind_to_advdiff on nc components per axis: 2 (re, im) or 1 (real numbers)
void upwind_to_advdiff(int nc, const double* lam, const double* mu, double* lam_out, double* mu_out);

double transport_z_ratio(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz);
std::complex<double> advdiff_z_beta(cd x, cd y, std::complex<double> p, std::complex<double> q);
void advdiff_z_ratio(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz,
                     std::complex<double> mz, double ratios[2]);
std::vector<cd> advdiff_z_table(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz,
                                std::complex<double> mz, int nxt, int nk1 = 32, int k1_off = 0);

// the recurrence's rounding grows like eps / (1 - |a|): this cap keeps it near 1e-12
constexpr double kZrecMaxRatio = 1.0 - 1.0 / 8192.0;
// two scans, eps / ((1 - |a|) (1 - |b|)): this cap keeps 8 eps / (1 - r)^2 at 2.9e-11
constexpr double kZrec2MaxRatio = 1.0 - 1.0 / 128.0;

// The middle kernel a symbol's z part admits at 256^3 (the grid test is the caller's):
//   Z_REC       mz == 0 and the transport ratio <= kZrecMaxRatio (k_tp_mid_rec, lamz = lz)
//   Z_REC2      mz != 0 and both advdiff ratios <= kZrec2MaxRatio (k_tp_mid_rec2, advdiff_z_table)
//   Z_REC_BACK  back_allowed and max |b| of the pair (lz, -lz) <= kZrecMaxRatio (k_tp_mid_recb,
//               lamz = -lz); over that cap Z_FFT, never Z_REC2
//   Z_FFT       everything else
enum ZRoute { Z_FFT = CFP_MID_KERNEL_FFT, Z_REC = CFP_MID_KERNEL_ZREC, Z_REC2 = CFP_MID_KERNEL_ZREC2,
              Z_REC_BACK = CFP_MID_KERNEL_ZREC_BACK };
struct ZDecision {
  ZRoute route;
  std::complex<double> lamz;  // what Z_REC / Z_REC_BACK pass to the kernel
  double ratios[2];           // what the route was decided on ({transport ratio, 0} for mz == 0)
};
// pure upwind transport against z, first order towards z + 1: an upwind setter's own z numbers
inline bool upwind_back(std::complex<double> lz, std::complex<double> mz) { return lz.real() < 0.0 && mz == 0.0; }
// sx, sy: the x and y tables the symbol was built with; lz, mz: its z numbers (an upwind symbol's
// mapped pair); back_allowed: it came through an upwind setter whose numbers were upwind_back()
ZDecision decide_z_route(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz,
                         std::complex<double> mz, bool back_allowed);

}  // namespace cfp
