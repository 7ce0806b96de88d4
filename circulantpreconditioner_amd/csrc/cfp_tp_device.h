// cfp_tp_device.h -- device helpers shared by the 3-sweep kernel units (cfp_three_pass.hip, which
// describes the schedule, cfp_tp_mid.hip, cfp_tp_rec.hip, cfp_tp_rows_r2c.hip): lane
// butterflies, unit order, the timing probes' bits.  Everything here is inlined into the kernels.
#pragma once
#include "cfp_fft_device.h"
#include "cfp_lane.h"
#include "cfp_three_pass.h"

namespace cfp {

// Radix-2 butterflies across lanes.  The DIF forms take points in natural lane order and
// leave the frequencies bit-reversed; the DIT forms are the forward transform from that order
// back to natural order (used inside the conjugate trick for the inverse).
// 4 points over an aligned quad: lane q holds point q -> frequency brev2(q)
__device__ __forceinline__ cd dft4_dif(cd v, int q) {
  const cd p = dpp_c<DPP_XOR2>(v);
  cd t = (q & 2) ? csub(p, v) : cadd(v, p);
  if (q == 3) t = mul_mi(t);
  const cd r = dpp_c<DPP_XOR1>(t);
  return (q & 1) ? csub(r, t) : cadd(t, r);
}
// lane q holds frequency brev2(q) -> point q
__device__ __forceinline__ cd dft4_dit(cd v, int q) {
  const cd r = dpp_c<DPP_XOR1>(v);
  cd u = (q & 1) ? csub(r, v) : cadd(v, r);
  if (q == 3) u = mul_mi(u);
  const cd p = dpp_c<DPP_XOR2>(u);
  return (q & 2) ? csub(p, u) : cadd(u, p);
}
// The 8-point DFT over 8 aligned lanes (N2 = 8) is a lane-xor-4 radix-2 stage (twiddle
// W_8^(j & 3) on the upper half) followed by dft4_dif, and dft4_dit followed by the mirrored
// stage for the inverse; k_tp_mid runs each stage as its own sweep over the 16 slots, which
// keeps the kernel out of scratch.  Lane j ends up holding frequency brev3(j).
template <int N2>
__device__ __forceinline__ int brev(int j) {
  if constexpr (N2 == 16) return ((j & 1) << 3) | ((j & 2) << 1) | ((j & 4) >> 1) | (j >> 3);
  return N2 == 4 ? ((j & 1) << 1) | (j >> 1) : ((j & 1) << 2) | (j & 2) | (j >> 2);
}
// XCD-aware unit order of a persistent grid of G workgroups (G % 8 == 0, whole rounds): the
// workgroups of one XCD (blockIdx % 8, round-robin dispatch) take G / 8 consecutive units of a
// round, so units that share 128-byte lines run under one L2
__device__ __forceinline__ int xcd_unit(int it, int G) {
  const int b = it % G;
  return it - b + (b & 7) * (G >> 3) + (b >> 3);
}

// Opaque copy of a thread or lane index: what is derived from it is recomputed at its use
// instead of living in a register across an FFT or a unit (every 3-sweep kernel holds its
// points plus one stage's temporaries in 128 VGPRs, and an address or index kept live spills)
__device__ __forceinline__ int idx(int i) {
  asm volatile("" : "+v"(i));
  return i;
}

// a byte load with the sweep's load policy (the fused stencil's row classes)
template <int FLAGS>
__device__ __forceinline__ unsigned char gload_u8(const unsigned char* p) {
  if constexpr ((FLAGS & F_NT_LD) != 0) return __builtin_nontemporal_load(p);
  return *p;
}

// first radix of an n-point FFT done as r0 x PTS x ... x PTS (n = r0 PTS^k, r0 <= PTS)
constexpr int r0_of(int n, int pts) { return n > pts ? r0_of(n / pts, pts) : n; }

// The radix-2 stage over lane bit 3 of k_tp_mid_sw's and the recurrence kernels' y2 DFT.
// partner across lane bit 3 (row_ror:8 inside each 16-lane row)
__device__ __forceinline__ double ror8_d(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)(b & 0xffffffffll), 0x128, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), 0x128, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// radix-2 over lane bit 3 without twiddle: bit clear -> own + partner, set -> partner - own
__device__ __forceinline__ cd bfly_l3(cd v, double sgn) {
  return make_cd(fma(sgn, v.x, ror8_d(v.x)), fma(sgn, v.y, ror8_d(v.y)));
}

// P3's reads of the Krylov basis vectors for the fused dots (FUSE > 0): non-temporal, so the
// 256 MiB vectors do not push the next P1 output out of the Infinity Cache before P2 reads it;
// -DCFP_POST_NT=0: plain loads, A/B (here, not with the launch policies of cfp_tp_launch.h: the
// kernel itself reads it)
#ifndef CFP_POST_NT
#define CFP_POST_NT 1
#endif
constexpr int kPostLoadFlags = CFP_POST_NT ? F_NT_LD : 0;

// PROBE != 0 only in tools/kexp (tp_probe.hip, p2_512.hip, rows_512.hip, built with CFP_KEXP):
// timing probes that drop a part of the work (output invalid).  The product library
// instantiates PROBE = 0 only.
enum { PR_NO_Y2 = 1, PR_NO_ZMATH = 2, PR_NO_XCHG = 4, PR_NO_LOAD = 8, PR_NO_STORE = 16,
       PR_PRIO = 32 /* experiment, full work: s_setprio 1 for the second half of the waves */,
       PR_ZMAJOR = 64 /* experiment, full work (k_tp_rows): units in z-major order (the units of one
                         round share y2 and differ in z) */ };

// the address spaces of the LDS-DMA builtin's operands (global_load_lds_dwordx4)
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glb_void_t;

}  // namespace cfp
