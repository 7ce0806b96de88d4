// cfp_wave_host.h -- the host arithmetic of the wave family: the symbol's validation and per-axis
// tables shared by the complex wave plan (cfp_wave.hip), its slab-backed PCSHELL (wave_system.cpp)
// and the real-data wave plan (cfp_wave_real.hip), and which grids the real-data plan serves and
// its schedule.  Plain C++ without a HIP include, so a stand-alone program can run it under a
// host sanitizer (tools/wave_real_host_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace cfp {
namespace wave {

// NULL when (kappa, c0) is a wave symbol, else why not
inline const char* symbol_refusal(const double kappa[3], double c0) {
  if (!(c0 > 0.0)) return "c0 must be > 0";
  for (int a = 0; a < 3; ++a)
    if (!(kappa[a] >= 0.0)) return "kappa must be >= 0";
  return nullptr;
}

// (p, q)[k] = (kappa c0 (1 - cos theta), kappa sin theta), theta = 2 pi k / n, interleaved, for
// k < count.  exact_self_mirror: q = 0 exactly at the self-mirrored frequencies k = 0 and 2 k = n,
// where sin theta is 0 but (double)sinl(pi) is not.  The real-data plan sets it: its Nyquist field
// (kx = nx / 2) is a real-data field of its own only with q = 0 there.  The complex plan and the
// slab PCSHELL leave it off and keep (double)sinl(theta) everywhere, the tables their recorded
// results were measured with.
inline std::vector<double> axis_table(int64_t n, int64_t count, double kappa, double c0, bool exact_self_mirror) {
  std::vector<double> t((size_t)(2 * count));
  for (int64_t k = 0; k < count; ++k) {
    const long double th = 2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
    t[(size_t)(2 * k)] = (double)((long double)kappa * c0 * (1.0L - cosl(th)));
    const bool self_mirrored = k == 0 || 2 * k == n;
    t[(size_t)(2 * k + 1)] = exact_self_mirror && self_mirrored ? 0.0 : (double)((long double)kappa * sinl(th));
  }
  return t;
}

}  // namespace wave
namespace wave_real {

constexpr int64_t kMaxAxis = 4096;   // y / z passes: the mixed-radix pass's longest axis
constexpr int64_t kMaxFused = 1024;  // the fused wave pass keeps a cell's columns in LDS (complex plan's limit)

// the last axis with n > 1 among y, z: the fused pass; 0 when there is none
inline int fused_axis(int64_t ny, int64_t nz) { return nz > 1 ? 2 : (ny > 1 ? 1 : 0); }

// NULL when the grid is served, else why not (a printf format taking nx, ny, nz as long long and dim)
inline const char* refusal(int64_t nx, int64_t ny, int64_t nz, int dim) {
  if (nx < 1 || ny < 1 || nz < 1) return "real wave plan: grid sizes must be >= 1 (%lld x %lld x %lld, dim %d)";
  if (dim != 2 && dim != 3) return "real wave plan: dim must be 2 or 3 (grid %lld x %lld x %lld, dim = %d)";
  if (dim == 2 && nz != 1) return "real wave plan: a 2-D wave system has nz = 1 (grid %lld x %lld x %lld, dim %d)";
  const int64_t M = nx / 2;
  if (nx % 2 || M < 16 || M > 512 || (M & (M - 1)))
    return "real wave plan: nx/2 must be a power of two in [16, 512] (grid %lld x %lld x %lld, dim %d)";
  if (ny > kMaxAxis || nz > kMaxAxis) return "real wave plan: ny, nz above 4096 are not supported (grid %lld x %lld x %lld, dim %d)";
  if (ny * nz < 2) return "real wave plan: needs ny > 1 or nz > 1 (grid %lld x %lld x %lld, dim %d)";
  if ((fused_axis(ny, nz) == 2 ? nz : ny) > kMaxFused)
    return "real wave plan: the last axis (the fused pass) is at most 1024 long (grid %lld x %lld x %lld, dim %d)";
  return nullptr;
}

// one launch of the schedule
enum Kind : int { R2C = 0, AXIS = 1, C2R = 2 };
struct Step {
  int kind;
  int axis;   // AXIS: 1 or 2
  int mode;   // AXIS: PassMode (0 forward, 1 inverse, 4 fused wave)
  int field;  // AXIS: 0 = H (half spectrum), 1 = Q (Nyquist)
};
// r2c rows | y of H, Q | fused of H, Q | inverse y of H, Q | c2r rows (the y passes: ny, nz > 1 only)
inline std::vector<Step> schedule(int64_t ny, int64_t nz) {
  std::vector<Step> st;
  const int f = fused_axis(ny, nz);
  const bool ypass = f == 2 && ny > 1;
  st.push_back({R2C, 0, 0, 0});
  if (ypass)
    for (int q = 0; q < 2; ++q) st.push_back({AXIS, 1, 0, q});
  for (int q = 0; q < 2; ++q) st.push_back({AXIS, f, 4, q});
  if (ypass)
    for (int q = 0; q < 2; ++q) st.push_back({AXIS, 1, 1, q});
  st.push_back({C2R, 0, 0, 0});
  return st;
}

// the x table of the half spectrum and the Nyquist column: k = 0 .. nx/2, nx/2 + 1 entries (the
// plan's tables have the self-mirrored q exactly 0)
inline std::vector<double> x_table(int64_t nx, double kappa, double c0) {
  return wave::axis_table(nx, nx / 2 + 1, kappa, c0, true);
}

}  // namespace wave_real
}  // namespace cfp
