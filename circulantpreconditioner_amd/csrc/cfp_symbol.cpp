// cfp_symbol.cpp -- host arithmetic of the closed-form symbols and the z route (cfp_symbol.h).
#include "cfp_symbol.h"

#include <cmath>

namespace cfp {

// 1 - e^{-2 pi i k / n}: the 1-D DFT of the transport column (1, -1, 0, ...)
std::vector<cd> host_transport_symbol(i64 n) {
  std::vector<cd> s((size_t)n, make_cd(0.0, 0.0));
  if (n <= 1) return s;
  for (i64 k = 0; k < n; ++k) {
    long double a = 2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
    s[k] = make_cd((double)(1.0L - cosl(a)), (double)sinl(a));
  }
  return s;
}

std::vector<cd> transport_product(const std::vector<cd>& hat, std::complex<double> lam) {
  std::vector<cd> s(hat.size());
  for (size_t k = 0; k < hat.size(); ++k) {
    // c * lambda as in vec_kronecker_product_identity_* (src/FftLinearSolver_3D.c:100,122)
    const double re = hat[k].x * lam.real() - hat[k].y * lam.imag();
    const double im = hat[k].x * lam.imag() + hat[k].y * lam.real();
    s[k] = make_cd(re, im);
  }
  return s;
}

// max over (kx, ky) of |lamz / (1 + sx[kx] + sy[ky] + lamz)|, s_d = lambda_d (1 - e^{-2 pi i k / n_d}):
// the ratio a of the z recurrence u_z = a u_{z-1} + w_z that the transport symbol's z part is
// (cfp_tp_rec.hip k_tp_mid_rec).  A zero denominator gives infinity.
double transport_z_ratio(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz) {
  double amax = 0.0;
  const double lzn = std::abs(lz);
  for (const cd& y : sy)
    for (const cd& x : sx) {
      const std::complex<double> den(x.x + y.x + 1.0 + lz.real(), x.y + y.y + lz.imag());
      const double d = std::abs(den);
      const double r = d > 0.0 ? lzn / d : (lzn > 0.0 ? INFINITY : 0.0);
      if (!(r <= amax)) amax = r;
    }
  return amax;
}

// lambda (1 - w) + mu (2 - w - conj(w)), w = e^{-2 pi i k / n}: one axis' part of the
// advection-diffusion symbol (0 for n == 1)
std::vector<cd> host_advdiff_symbol(i64 n, std::complex<double> lam, std::complex<double> mu) {
  std::vector<cd> s((size_t)n, make_cd(0.0, 0.0));
  if (n <= 1) return s;
  const std::vector<cd> hat = host_transport_symbol(n);
  for (i64 k = 0; k < n; ++k) {
    // the advection part exactly as the transport setter forms it (set_separable), so that mu = 0
    // gives its tables bit for bit; 2 - w - conj(w) = 2 Re(1 - w)
    const double re = hat[k].x * lam.real() - hat[k].y * lam.imag();
    const double im = hat[k].x * lam.imag() + hat[k].y * lam.real();
    const double c2 = 2.0 * hat[k].x;
    s[k] = make_cd(re + mu.real() * c2, im + mu.imag() * c2);
  }
  return s;
}

AxisTables axis_symbols(const i64 n[3], const double lam6[6], const double mu6[6]) {
  AxisTables s;
  for (int a = 0; a < 3; ++a)
    s[a] = host_advdiff_symbol(n[a], {lam6[2 * a], lam6[2 * a + 1]}, {mu6[2 * a], mu6[2 * a + 1]});
  return s;
}

std::vector<cd> column_sums(const std::vector<cd>& sx, i64 kx0, i64 nkx, const std::vector<cd>& sy, i64 ky0, i64 nky,
                            i64 stride) {
  std::vector<cd> col((size_t)(stride * nky));
  for (i64 ky = 0; ky < nky; ++ky)
    for (i64 kx = 0; kx < nkx; ++kx) {
      const cd x = sx[(size_t)(kx0 + kx)], y = sy[(size_t)(ky0 + ky)];
      col[(size_t)(kx + stride * ky)] = make_cd(x.x + y.x, x.y + y.y);
    }
  return col;
}

void upwind_to_advdiff(int nc, const double* lam, const double* mu, double* lam_out, double* mu_out) {
  // |lam| (1 - conj w) + mu (2 - w - conj w) = lam (1 - w) + (mu - lam) (2 - w - conj w) for lam < 0
  for (int a = 0; a < 3; ++a) {
    const bool neg = lam[nc * a] < 0.0;
    for (int c = 0; c < nc; ++c) {
      const double l = lam[nc * a + c], m = mu[nc * a + c];
      lam_out[nc * a + c] = l;
      mu_out[nc * a + c] = neg ? m - l : m;
    }
  }
}

// Along z the advection-diffusion symbol of a column, d - p e^{-i theta} - q e^{i theta} with
// p = lamz + muz, q = muz, d = 1 + sx[kx] + sy[ky] + p + q, factors as
// beta (1 - a e^{-i theta}) (1 - b e^{i theta}), beta the root of beta^2 - d beta + p q = 0 of
// larger modulus, a = p / beta, b = q / beta (cfp_tp_rec.hip k_tp_mid_rec2).  ratios = max |a|,
// max |b| over the columns; beta = 0 gives infinity.
std::complex<double> advdiff_z_beta(cd x, cd y, std::complex<double> p, std::complex<double> q) {
  const std::complex<double> d = std::complex<double>(x.x + y.x + 1.0, x.y + y.y) + p + q;
  if (q == 0.0) return d;  // first order: the roots are d and 0 (a is the transport ratio exactly)
  std::complex<double> sq = std::sqrt(d * d - 4.0 * p * q);
  if (d.real() * sq.real() + d.imag() * sq.imag() < 0.0) sq = -sq;  // the root on d's side is the larger
  return 0.5 * (d + sq);
}
void advdiff_z_ratio(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz,
                     std::complex<double> mz, double ratios[2]) {
  const std::complex<double> p = lz + mz, q = mz;
  const double pn = std::abs(p), qn = std::abs(q);
  ratios[0] = ratios[1] = 0.0;
  for (const cd& y : sy)
    for (const cd& x : sx) {
      const double bn = std::abs(advdiff_z_beta(x, y, p, q));
      const double ra = bn > 0.0 ? pn / bn : (pn > 0.0 ? INFINITY : 0.0);
      const double rb = bn > 0.0 ? qn / bn : (qn > 0.0 ? INFINITY : 0.0);
      if (!(ra <= ratios[0])) ratios[0] = ra;
      if (!(rb <= ratios[1])) ratios[1] = rb;
    }
}
// k_tp_mid_rec2's column table at 256^3 (cfp_three_pass.h): [unit u][a, r = 256 / beta, b][lane],
// lane = x + 8 y2 holding column kx = 8 (u % nxt) + x, ky = k1_off + u / nxt + 32 brev3(y2); nxt x
// tiles per row: 32 on the complex grid (1024 units), 16 on the real plan's half spectrum (512
// units); nk1 rows u / nxt from k1_off on: all 32 on one GPU, rank r's 32 / P from r 32 / P on in
// a z-slab plan of P ranks (its z-pencil block [256 z][256 / P][256 x])
std::vector<cd> advdiff_z_table(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz,
                                std::complex<double> mz, int nxt, int nk1, int k1_off) {
  const std::complex<double> p = lz + mz, q = mz;
  const int units = nk1 * nxt;
  std::vector<cd> t((size_t)units * 3 * 64);
  for (int u = 0; u < units; ++u)
    for (int lane = 0; lane < 64; ++lane) {
      const int x = lane & 7, y2 = lane >> 3;
      const int k2 = ((y2 & 1) << 2) | (y2 & 2) | (y2 >> 2);
      const std::complex<double> be =
          advdiff_z_beta(sx[(size_t)(8 * (u % nxt) + x)], sy[(size_t)(k1_off + u / nxt + 32 * k2)], p, q);
      const std::complex<double> a = p / be, b = q / be, r = 256.0 / be;
      t[(size_t)((3 * u) * 64 + lane)] = make_cd(a.real(), a.imag());
      t[(size_t)((3 * u + 1) * 64 + lane)] = make_cd(r.real(), r.imag());
      t[(size_t)((3 * u + 2) * 64 + lane)] = make_cd(b.real(), b.imag());
    }
  return t;
}

ZDecision decide_z_route(const std::vector<cd>& sx, const std::vector<cd>& sy, std::complex<double> lz,
                         std::complex<double> mz, bool back_allowed) {
  ZDecision d{Z_FFT, lz, {0.0, 0.0}};
  if (back_allowed) {
    // the mapped pair has p = 0 and q = -lamz, so its ratios are a = 0 and b = q / (c + q): the
    // backward recurrence under k_tp_mid_rec's cap, else the FFT kernel (never the two-sided one)
    advdiff_z_ratio(sx, sy, lz, -lz, d.ratios);
    d.lamz = -lz;
    if (d.ratios[1] <= kZrecMaxRatio) d.route = Z_REC_BACK;
  } else if (mz == 0.0) {
    // first order along z: k_tp_mid_rec, which reads c from the column table
    d.ratios[0] = transport_z_ratio(sx, sy, lz);
    if (d.ratios[0] <= kZrecMaxRatio) d.route = Z_REC;
  } else {
    advdiff_z_ratio(sx, sy, lz, mz, d.ratios);
    if (d.ratios[0] <= kZrec2MaxRatio && d.ratios[1] <= kZrec2MaxRatio) d.route = Z_REC2;
  }
  return d;
}

}  // namespace cfp
