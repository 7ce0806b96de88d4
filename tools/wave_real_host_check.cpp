// wave_real_host_check.cpp -- the host arithmetic of the wave family
// (circulantpreconditioner_amd/csrc/cfp_wave_host.h) in a stand-alone program, meant to be
// built with a host sanitizer and run on the CPU:
//
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I circulantpreconditioner_amd/csrc tools/wave_real_host_check.cpp -o wave_real_host_check
//   ./wave_real_host_check
//
// It checks the supported-grid predicate on a sweep, the schedule of every kind of grid and the
// symbol tables (sizes, end values, the exact zeros the Nyquist field relies on, and that the
// shared table's two rules differ in nothing else).  Exit 0 = ok.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "cfp_wave_host.h"

using namespace cfp::wave_real;

static int fails = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                      \
    }                                                               \
  } while (0)

// the rule of include/wave_system_real.h, restated
static bool rule(int64_t nx, int64_t ny, int64_t nz, int dim) {
  if (nx < 1 || ny < 1 || nz < 1) return false;
  if (!(dim == 3 || (dim == 2 && nz == 1))) return false;
  bool okx = false;
  for (int64_t M = 16; M <= 512; M *= 2) okx = okx || nx == 2 * M;
  if (!okx) return false;
  if (ny > 4096 || nz > 4096 || (ny == 1 && nz == 1)) return false;
  return (nz > 1 ? nz : ny) <= 1024;
}

int main() {
  const int64_t nxs[] = {0, 1, 16, 31, 32, 33, 48, 64, 100, 128, 256, 512, 1000, 1024, 1025, 2048};
  const int64_t nys[] = {0, 1, 2, 7, 24, 1024, 1025, 4096, 4097};
  int accepted = 0;
  for (int64_t nx : nxs)
    for (int64_t ny : nys)
      for (int64_t nz : nys)
        for (int dim = 0; dim <= 4; ++dim) {
          const char* why = refusal(nx, ny, nz, dim);
          CHECK((why == nullptr) == rule(nx, ny, nz, dim));
          if (why) {
            char buf[512];
            const int len = std::snprintf(buf, sizeof buf, why, (long long)nx, (long long)ny, (long long)nz, dim);
            CHECK(len > 0 && len < (int)sizeof buf);
          } else {
            ++accepted;
          }
        }
  CHECK(accepted > 0);

  // schedules: 3-D with both axes, 3-D with one axis, 2-D
  CHECK(schedule(6, 5).size() == 8 && schedule(1, 5).size() == 4 && schedule(24, 1).size() == 4);
  for (auto g : {std::pair<int64_t, int64_t>{6, 5}, {1, 5}, {24, 1}, {5, 1}}) {
    const std::vector<Step> st = schedule(g.first, g.second);
    CHECK(st.front().kind == R2C && st.back().kind == C2R);
    int fusedH = 0, fusedQ = 0;
    for (const Step& s : st)
      if (s.kind == AXIS) {
        CHECK(s.axis == 1 || s.axis == 2);
        CHECK((s.axis == 1 ? g.first : g.second) > 1);
        if (s.mode == 4) {
          CHECK(s.axis == fused_axis(g.first, g.second));
          ++(s.field ? fusedQ : fusedH);
        }
      }
    CHECK(fusedH == 1 && fusedQ == 1);
  }

  // tables
  const double kappa = 0.37, c0 = 700.0;
  for (int64_t nx : {32, 64, 1024}) {
    const std::vector<double> t = x_table(nx, kappa, c0);
    const int64_t M = nx / 2;
    CHECK((int64_t)t.size() == 2 * (M + 1));
    CHECK(t[0] == 0.0 && t[1] == 0.0);
    CHECK(t[(size_t)(2 * M + 1)] == 0.0);                                     // q(kx = M) = 0 exactly
    CHECK(std::fabs(t[(size_t)(2 * M)] - 2.0 * kappa * c0) <= 1e-15 * 2.0 * kappa * c0);  // p(kx = M) = 2 kappa c0
    for (int64_t k = 0; k <= M; ++k) {
      const double th = 2.0 * M_PI * (double)k / (double)nx;
      CHECK(std::fabs(t[(size_t)(2 * k)] - kappa * c0 * (1.0 - std::cos(th))) <= 1e-12 * kappa * c0);
      CHECK(std::fabs(t[(size_t)(2 * k + 1)] - kappa * std::sin(th)) <= 1e-15);
    }
  }
  for (int64_t n : {1, 3, 5, 12, 20}) {
    const std::vector<double> t = cfp::wave::axis_table(n, n, kappa, c0, true);
    CHECK((int64_t)t.size() == 2 * n && t[0] == 0.0 && t[1] == 0.0);
    for (int64_t k = 1; k < n; ++k)  // q(-k) = -q(k), p(-k) = p(k): the symbol is Hermitian
      CHECK(std::fabs(t[(size_t)(2 * k + 1)] + t[(size_t)(2 * (n - k) + 1)]) <= 1e-15 &&
            std::fabs(t[(size_t)(2 * k)] - t[(size_t)(2 * (n - k))]) <= 1e-12 * kappa * c0);
  }
  // the shared table: the complex plan's rule (flag off) and the real-data plan's (flag on) agree
  // bit for bit except q at the self-mirrored k = 0 and 2 k = n, which the flag makes exactly 0
  for (int64_t n : {1, 2, 5, 32, 50, 1024}) {
    const std::vector<double> off = cfp::wave::axis_table(n, n, kappa, c0, false),
                              on = cfp::wave::axis_table(n, n, kappa, c0, true);
    CHECK(off.size() == on.size() && (int64_t)on.size() == 2 * n);
    for (int64_t k = 0; k < n; ++k) {
      CHECK(off[(size_t)(2 * k)] == on[(size_t)(2 * k)]);  // p never differs
      if (k == 0 || 2 * k == n) CHECK(on[(size_t)(2 * k + 1)] == 0.0);
      else CHECK(off[(size_t)(2 * k + 1)] == on[(size_t)(2 * k + 1)]);
    }
  }
  const double bad[3] = {0.1, -1.0, 0.0}, good[3] = {0.1, 0.0, 0.2};
  CHECK(cfp::wave::symbol_refusal(good, c0) == nullptr && cfp::wave::symbol_refusal(good, 0.0) != nullptr &&
        cfp::wave::symbol_refusal(bad, c0) != nullptr);
  std::printf(fails ? "wave_real_host_check: %d check(s) failed\n" : "wave_real_host_check: ok (%d grids accepted)\n",
              fails ? fails : accepted);
  return fails ? 1 : 0;
}
