// cfp_tp_dispatch.hip -- the dispatch of the 3-sweep apply (the schedule: cfp_three_pass.hip): the
// public launch_three_pass* functions of cfp_three_pass.h choose a kernel family's entry by stage
// and grid.  This unit launches no kernel.  The families, each with the launchers that
// instantiate its kernels: cfp_three_pass.hip (P1 / P3 rows), cfp_tp_mid.hip (P2 by FFT),
// cfp_tp_rec.hip (P2 with z by recurrence), cfp_tp_rows_r2c.hip (the real plan's P1 / P3).
#include "cfp_tp_launch.h"

namespace cfp {

bool three_pass_supported(const i64 n[3]) {
  return n[0] == n[1] && n[1] == n[2] && (n[0] == 128 || n[0] == 256 || n[0] == 512);
}

bool three_pass_slab_supported(const i64 n[3], int P) {
  // N1 = 32 rows per P1 unit, k1 split over the ranks (P | 32); P3 reads chunk rows N2 apart
  // per thread and N2 TY = 2 N2 apart per slot (nyl >= 2 N2: 256^3 N2 = 8, 512^3 N2 = 16)
  const bool cube = n[0] == n[1] && n[1] == n[2] && (n[0] == 256 || n[0] == 512);
  return cube && P >= 1 && P <= 16 && (32 % P) == 0;
}

int three_pass_slab_n2(i64 n) { return n == 512 ? 16 : 8; }

bool three_pass_fused_supported(int n, TPShape shape) { return n == 256 && shape.n1 == 0 && shape.mid == TP_MID_DEFAULT; }

bool three_pass_zrec_shape(int n, TPShape shape) {
  return n == 256 && shape.mid == TP_MID_DEFAULT && (shape.n1 == 0 || shape.n1 == 32);
}

bool three_pass_shape_valid(int n1, int mid, i64 n) {
  if (mid == TP_MID_ROWSALT) return n1 == 0;
  if (n1 == 16) return n == 128 && mid >= TP_MID_DEFAULT && mid <= TP_MID_SWAP64;
  return (n1 == 0 || n1 == 32 || n1 == 64) && (mid >= 0 && mid <= TP_MID_SWAP32X) &&
         !(mid >= TP_MID_BLOCKED && n1 == 64);
}

hipError_t launch_three_pass(int stage, int n, const cd* in, cd* out, const TPArgs& a, TPShape shape,
                             hipStream_t s) {
  // TP_MID_ROWSALT: the default shape with the other phase-C exchanges in P1 / P3 (A/B)
  const bool ra = shape.mid == TP_MID_ROWSALT;
  if (ra) shape.mid = TP_MID_DEFAULT;
  if (n == 100) return launch_three_pass_sq(stage, n, in, out, a, shape, s);
  if (stage != 1) return tp_rows(stage, n, in, out, a, shape, ra, s);
  // an eligible transport symbol under the default 256^3 shape: z by recurrence (k_tp_mid_rec);
  // swap64_pf stays the FFT kernel for a same-process A/B
  if (a.zrec && three_pass_zrec_shape(n, shape)) return tp_mid_rec(out, a, s);
  return tp_mid(n, out, a, shape, s);
}

hipError_t launch_three_pass_slab(int stage, int n, const cd* in, cd* out, const TPArgs& a, int nzl, hipStream_t s) {
  return stage == 1 ? tp_mid_slab(n, out, a, s) : tp_rows_slab(stage, n, in, out, a, nzl, s);
}

// The default 256^3 row sweeps with the stand-in GMRES's Krylov work fused in (TPArgs pre_* /
// post_*): P1 on A b, P3 with the dots.  Same grids and unit order as the plain default sweeps.
hipError_t launch_three_pass_fused(int stage, int n, const cd* in, cd* out, const TPArgs& a, hipStream_t s,
                                   unsigned* grid_out) {
  if (n != 256 || (stage != 0 && stage != 2)) return hipErrorNotSupported;
  if (stage == 0 && (!a.pre_cls || in == out || a.pre_ncls < 1 || a.pre_ncls > TP_PRE_MAX_CLS || a.pre_nd < 1 ||
                     a.pre_nd > 3))
    return hipErrorInvalidValue;
  if (stage == 2 && (a.post_nv < 1 || a.post_nv > TP_POST_MAX || !a.post_partial)) return hipErrorInvalidValue;
  constexpr int units = 256 * 8;
  const unsigned gx = kRowsXCD ? grid_xcd(units, 2) : 0;
  const unsigned g = gx ? gx : grid_of(units, 2);
  if (grid_out) *grid_out = g;
  return tp_rows_fused(stage, in, out, a, s, g, gx != 0);
}

hipError_t launch_three_pass_real(int stage, int n, const double* b, cd* H, cd* Q, double* x, const TPArgs& a,
                                  hipStream_t s, bool alt_rows) {
  if (stage == 1 || stage == 3) return tp_mid_real(stage, n, H, Q, a, s);
  return tp_rows_real(stage, n, b, H, Q, x, a, s, alt_rows);
}

}  // namespace cfp
