// cfp_tp_launch.h -- host side of the 3-sweep units: the stamping launch, persistent grids, the
// measured launch policies with their A/B macros, and the kernel families' entry points, which
// the dispatch (cfp_tp_dispatch.hip) chooses among.  Internal: the public interface is
// cfp_three_pass.h.
#pragma once
#include "cfp_fft_device.h"  // the cache-policy flags F_*
#include "cfp_three_pass.h"

#include <hip/hip_ext.h>

#include <type_traits>

// a launch that stamps its own dispatch while per-launch profiling is on (cfp_internal.h)
#define TP_LAUNCH(K, G, B, S, ...)                                                                    \
  do {                                                                                                \
    if (g_stamp.start || g_stamp.stop)                                                                \
      hipExtLaunchKernelGGL(K, G, B, 0, S, g_stamp.start, g_stamp.stop, 0, __VA_ARGS__);              \
    else                                                                                              \
      hipLaunchKernelGGL(K, G, B, 0, S, __VA_ARGS__);                                                 \
  } while (0)

namespace cfp {

inline int cu_count() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
      cus = 256;
  }
  return cus;
}

// persistent grid: per_cu workgroups per CU, at most one per unit
inline unsigned grid_of(int units, int per_cu) {
  const int g = per_cu * cu_count();
  return (unsigned)(units < g ? units : g);
}
// the same for the XCD-ordered kernels (xcd_unit), whose rounds must be whole and a multiple of
// 8 workgroups: the largest power of two <= grid_of (units is a power of two), 0 if below 8
inline unsigned grid_xcd(int units, int per_cu) {
  unsigned g = grid_of(units, per_cu), p = 1;
  while (2 * p <= g) p *= 2;
  return p >= 8 && units % p == 0 ? p : 0;
}

// P1 load policy (r03, profiles/r03f_p1_inplace_ab.jsonl, r03g_p1_out_of_place_ab.jsonl):
// out of place, non-temporal loads (plain loads leave P2 at 153-160 us); in place (the direct
// solver's Un, Un), plain loads -- with NT loads of the lines it then overwrites, P1's output
// drops out of the Infinity Cache and P2 takes 143-145 us instead of 128.
constexpr int kP1Flags = F_NT_LD, kP1InPlaceFlags = 0;
// P3 store policy: non-temporal.  r03v A/B of all 24 P1 / P2 / P3 cache policies in the apply
// chain (tools/kexp/tp_chain.hip, profiles/r03v_tp_chain.txt): plain P3 stores 310 us against
// 314 us there, but +0.3-0.8 % in bench.py and -2 % inside GMRES (0.387 vs 0.379 ms per PCApply),
// so the measured policy stays.
constexpr int kP3Flags = F_NT_ST;
// 256^3, N1 = 32 (r03z, tools/kexp/run_tp_lp.py, profiles/r03z_tp_lp.txt, 3-sweep chain):
// P1 / P3 with the lane-pair phase A (no LDS exchange there): 310.8 -> 303.0 us.  Every executor
// (one GPU, slabs, pieces) runs it.  (Moving the four-step twiddle W_256^{y2 k1} from P2 into
// P1 / P3 lost: 313.1 us, P1 +9 us for its table loads, P2 -1 us; DESIGN.md.)
constexpr bool kRowsLP = true;
// P2 load policy (r03z, profiles/r03z_tp_p2nt.txt): non-temporal loads and LDS-DMA of its input,
// which nothing reads after it: chain 304.4 -> 300.7 us
constexpr int kP2LoadFlags = F_NT_LD;
// P1 / P3 phase C (the row FFT) with wave-local exchanges (r04ab): shape TP_MID_ROWSALT runs the
// other setting for A/B
constexpr bool kRowsWave = true;
// P1 / P3 units in XCD order at 256^3 and 512^3 (r05j, tools/kexp/run_rows_512.py,
// profiles/r05j_rows_probes.txt): each XCD walks whole z-planes of b / x, so an XCD's units read
// and write one contiguous region; 256^3 P1 93.8 -> 90.8 us, P3 90.4 -> 86.6 us; 512^3 P1 911 ->
// 884 us, P3 915 -> 866 us (the units of one plane in blockIdx order spread over all eight
// XCDs).  Whole apply (r05k, against a -DCFP_ROWS_XCD=0 build, alternating processes): 256^3
// 3,361-3,388 against 3,288-3,316 PCApply/s, 512^3 282.3-282.5 against 274.6-275.4.
constexpr bool kRowsXCD = CFP_ROWS_XCD != 0;
// The one-GPU 256^3 row sweeps with the LDS-DMA prefetch of kRowsNPF of the next unit's 16 slots
// (k_tp_rows<.., NPF>); -DCFP_ROWS_PF=0 builds the sweeps without it for A/B.
#ifndef CFP_ROWS_PF
#define CFP_ROWS_PF 8
#endif
constexpr int kRowsNPF = CFP_ROWS_PF;
static_assert(kRowsNPF == 0 || (kRowsNPF >= 4 && kRowsNPF <= 8), "CFP_ROWS_PF: 0 (off) or 4 to 8 slots");

// The real plan's 256^3 FFT stage 1 with units in XCD order (whole rounds: 512 units, 256
// workgroups; r05q, profiles/r05q_mid_xcd_ab.txt: 5,713-5,736 against 5,639-5,681 real
// PCApply/s); -DCFP_REAL_MID_XCD=0: A/B
#ifndef CFP_REAL_MID_XCD
#define CFP_REAL_MID_XCD 1
#endif
// The same stage by the two-sided recurrence: linear unit order or the XCD order of that stage's
// FFT kernel, by measurement (profiles/r12_real_zrec2_ab.txt); -DCFP_REAL_REC2_XCD=0/1 builds
// the other for A/B.
#ifndef CFP_REAL_REC2_XCD
#define CFP_REAL_REC2_XCD 1
#endif

// f(P, Q) with the two run-time choices p and q as std::bool_constant arguments: a launcher's
// two-by-two ladder of instantiations (in-solver TAG x alignment, sweep x unit order) written once
template <class F>
void by2(bool p, bool q, F f) {
  if (p) {
    if (q) f(std::true_type{}, std::true_type{});
    else f(std::true_type{}, std::false_type{});
  } else {
    if (q) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
  }
}

// The kernel families' entry points.  stage 0: P1, 1: P2, 2: P3 (3: the real plan's Nyquist
// column); each launches on s and returns hipGetLastError(), or the error that kept it from
// launching.  The arguments are those of the public function of cfp_three_pass.h that calls it.
// cfp_three_pass.hip (k_tp_rows): stage 0 / 2 of one GPU (alt: shape ROWSALT), of a z-slab rank, and
// of the fused Krylov step on the grid g the dispatch chose (xcd: g walks whole XCD rounds)
hipError_t tp_rows(int stage, int n, const cd* in, cd* out, const TPArgs& a, TPShape shape, bool alt, hipStream_t s);
hipError_t tp_rows_slab(int stage, int n, const cd* in, cd* out, const TPArgs& a, int nzl, hipStream_t s);
hipError_t tp_rows_fused(int stage, const cd* in, cd* out, const TPArgs& a, hipStream_t s, unsigned g, bool xcd);
// cfp_tp_mid.hip (k_tp_mid, k_tp_mid_sw): the FFT stage 1 of one GPU and of a z-slab rank, the
// real plan's stage 1 (H) and 3 (Q)
hipError_t tp_mid(int n, cd* data, const TPArgs& a, TPShape shape, hipStream_t s);
hipError_t tp_mid_slab(int n, cd* data, const TPArgs& a, hipStream_t s);
hipError_t tp_mid_real(int stage, int n, cd* H, cd* Q, const TPArgs& a, hipStream_t s);
// cfp_tp_rec.hip (k_tp_mid_rec): stage 1 at 256^3 for an eligible transport symbol (a.zrec); the
// other recurrence launchers are public (launch_three_pass_rec2, _recb, _slab_rec2, _real_rec2)
hipError_t tp_mid_rec(cd* data, const TPArgs& a, hipStream_t s);
// cfp_tp_rows_r2c.hip (k_tp_rows_r2c): the real plan's stage 0 / 2
hipError_t tp_rows_real(int stage, int n, const double* b, cd* H, cd* Q, double* x, const TPArgs& a, hipStream_t s,
                        bool alt_rows);

}  // namespace cfp
