// cfp_tp_rec.hip -- the middle sweep P2 of the 256^3 3-sweep apply with z solved by recurrence
// instead of transformed (the schedule: cfp_three_pass.hip): k_tp_mid_rec (transport symbol),
// k_tp_mid_recb (upwind, lambda_z < 0), k_tp_mid_rec2 (advection-diffusion) and
// k_tp_mid_rec2_half (the same on the real plan's half spectrum), with their launchers.
#include "cfp_tp_device.h"
#include "cfp_tp_launch.h"

namespace cfp {

// ---------------------------------------------------------------------------------------------
// P2 for the transport symbol with z solved by recurrence (k_tp_mid_rec; 256^3, N2 = 8).  The
// symbol of column (kx, ky) is c + lamz (1 - e^{-2 pi i kz / nz}), c = 1 + colsym: with
// a = lamz / (c + lamz), "z DFT, divide, inverse z DFT" of v is the cyclic first-order system
//   u_z = a u_{z-1} + w_z,  w = v nz / (c + lamz)   (nz: the factor the unnormalised pair leaves),
// solved as u_z = t_z + a^{z+1} t_{nz-1} / (1 - a^nz), t the same recurrence started from zero.
// The host enables it only where max |a| <= 1 - 2^-13 (cfp_plan.hip); k_tp_mid_sw's output is the
// same array, so P1 and P3 do not change.
//
// The tile is k_tp_mid_sw's (8 x times 8 y2 times 256 z, 128-byte runs, in place), and so is the
// access: lane = x + 8 y2, so one wave-wide load or store is the 8 rows times 128 bytes of one
// z-plane (4 KiB apart).  A wave holds 16 consecutive z (z = 16 wave + m, slot m), a thread the
// 16 z of one (x, y2).  The y2 DFT runs across lane bits 5, 4, 3 on all 16 slots: radix-2 DIF,
// natural order in, bit-reversed out.  Bits 5 and 4: a permlane32 / permlane16 swap of a slot
// pair gives each lane of a lane pair one slot's two inputs, the lane runs that butterfly whole,
// and a second swap returns the results to their owners; bit 3: DPP row_ror:8 and one fma with a
// per-lane sign; stage twiddles are per-lane constants.  Lane (x, y2) then owns column
// (x, k2 = brev3(y2)) and the scan is a register loop: t_m = a t_{m-1} + r v_m over the 16
// slots.  Wave level: every wave writes its 64 columns' block-end values E_w = t_15 (16 KiB),
// one workgroup barrier, then each lane forms the carry into its wave for its own column,
//   U_{16 w - 1} = sum_k a^{16 k} E_{(w - 1 - k) mod 16} / (1 - a^256)   (Horner in a^16),
// and adds a^{m+1} U to slot m (a running product).  That barrier is the only one of a unit; the
// block-end buffer alternates between two units, so a wave that runs ahead writes the next
// unit's values while others still read this one's.  The inverse y2 DFT is the forward DIT on the
// conjugate, from the bit-reversed order back to natural over lane bits 3, 4, 5.
//
// The columns' a and r = 256 / (c + lamz) come from a table that wave 0 fills one unit ahead
// (lane (x, y2) fills column (x, brev3(y2)), the column that lane scans).
//
// PF: slots 0..6 of the next unit come by LDS-DMA into this wave's own 7 KiB, issued between
// the unit's last arithmetic and its stores (measured best there, see the unit's end); a buffer
// that is only 8-byte aligned runs without it (global_load_lds_dwordx4 takes 16-byte addresses).
//
// The body is a function of __restrict__ pointers to the kernel's LDS arrays: inlined, its LDS
// reads carry the information that they do not alias the prefetch buffer, without which the
// compiler waits for every LDS-DMA in flight (vmcnt(0)) before the first LDS read that follows.
constexpr int kRecNPF = 7;  // slots that come from the LDS prefetch (154 of 160 KiB LDS)

// What the recurrence bodies (tp_mid_rec_body, tp_mid_rec2_body) share: each helper is defined
// here once and compiles to the instructions the bodies held as lambdas of their own (compare
// with tools/isa_same.py).  They take and return values or single points, never the 16-slot
// array: with the y2 loops moved whole into functions of cd (&v)[16], k_tp_mid_rec went from 118
// VGPRs without scratch to 128 with 68 spilled (180 B of scratch), k_tp_mid_rec2 to 26-30 spilled.
namespace rec {
__device__ __forceinline__ cd* at(cd* base, unsigned off) {
  return reinterpret_cast<cd*>(reinterpret_cast<char*>(base) + off);
}
// Radix-2 stage over lane bit B (5 or 4) on the slot pair (p, q): the swap gives the lower lane
// both lanes' p and the upper lane both lanes' q, each lane runs one whole butterfly (no
// duplicated value, no half thrown away), and the second swap hands every lane its own results
// back: sums to the lower lane, differences to the upper.  DIF: a + b, (a - b) w.
template <int B>
__device__ __forceinline__ void dif2(cd& p, cd& q, cd w) {
  swap_c<B>(p, q);
  const cd s = cadd(p, q), d = cmul(csub(p, q), w);
  p = s;
  q = d;
  swap_c<B>(p, q);
}
// DIT: a + b w, a - b w
template <int B>
__device__ __forceinline__ void dit2(cd& p, cd& q, cd w) {
  swap_c<B>(p, q);
  const cd t = cmul(q, w);
  q = csub(p, t);
  p = cadd(p, t);
  swap_c<B>(p, q);
}
// pin(): the values are formed where the source forms them.  Sunk towards their uses, a DFT's
// or a column's last operations keep their inputs live as well and the kernel goes to scratch.
__device__ __forceinline__ void pin(cd& w) { asm volatile("" : "+v"(w.x), "+v"(w.y)); }
// p q + c in 4 fused operations
__device__ __forceinline__ cd cfma(cd p, cd q, cd c) {
  return make_cd(fma(p.x, q.x, fma(-p.y, q.y, c.x)), fma(p.x, q.y, fma(p.y, q.x, c.y)));
}
// One slot pair of the y2 DFT across lane bits 5, 4, 3 (DIF): lane (x, y2) ends as frequency
// k2 = brev3(y2).  The per-lane constants: the stage twiddles w8 = W_8^{y2 & 3} (lane bit 5) and
// w4 = W_4^{y2 & 1} (lane bit 4), which the two lanes of a pair share, and the sign s3 of the DPP
// stage (+1 where lane bit 3 is clear, -1 where set).
__device__ __forceinline__ void y2_fwd_pair(cd& p, cd& q, cd w8, cd w4, double s3) {
  dif2<5>(p, q, w8);
  dif2<4>(p, q, w4);
  p = bfly_l3(p, s3);
  q = bfly_l3(q, s3);
  pin(p);
  pin(q);
}
// One slot pair of the inverse y2 DFT on the conjugate (DIT over lane bits 3, 4, 5: bit-reversed
// in, natural out), then the conjugate twiddle w = W_256^{y2 k1}
template <int PROBE>
__device__ __forceinline__ void y2_inv_pair(cd& vp, cd& vq, cd w, cd w8, cd w4, double s3) {
  cd p = cconj(vp), q = cconj(vq);
  if constexpr (!(PROBE & PR_NO_Y2)) {
    p = bfly_l3(p, s3);
    q = bfly_l3(q, s3);
    dit2<4>(p, q, w4);
    dit2<5>(p, q, w8);
  }
  vp = cconj(cmul(p, w));
  vq = cconj(cmul(q, w));
  pin(vp);
  pin(vq);
}
// A unit's memory access.  A point's address = a wave-uniform base (unit u = (x tile, local k1):
// row 8 k1; slot m: z = 16 wv + m) + this lane's 32-bit byte offset loff (x, row y2): a scalar
// base plus one offset register for all 16 slots, instead of 16 address pairs.  The callers pass
// opaque copies of u and loff, so that the addresses are formed again at each phase.
// NX: the row length in points (256; the real plan's half spectrum: 128, with loff on rows of NX).
// ZREV: the planes in reverse order, slot m of wave wv is z = 255 - (16 wv + m) (k_tp_mid_recb):
// the same 256 planes of the tile, so the same addresses, bounds and 16-byte alignment.
template <int NX, bool ZREV = false>
struct TileT {
  static constexpr int TN = 256, N2 = 8, XT = 8, NXT = NX / XT;
  cd* data;
  i64 zs;
  int wv;
  double* pf_l;
  __device__ __forceinline__ cd* slot_ptr(int u, int m) const {
    if constexpr (ZREV) return data + ((u % NXT) * XT + (i64)NX * N2 * (u / NXT) + zs * (TN - 1 - (16 * wv + m)));
    else return data + ((u % NXT) * XT + (i64)NX * N2 * (u / NXT) + zs * (16 * wv + m));
  }
  // this wave's slots 0 .. NPF-1 of unit u -> LDS, lane-linear
  template <int NPF, int LD>
  __device__ __forceinline__ void prefetch(int u, unsigned loff) const {
    asm volatile("" : "+s"(u), "+v"(loff));
#pragma unroll
    for (int m = 0; m < NPF; ++m)
      __builtin_amdgcn_global_load_lds((glb_void_t*)at(slot_ptr(u, m), loff), (lds_void_t*)(pf_l + (wv * NPF + m) * 128),
                                       16, 0, (LD & F_NT_LD) ? 2 : 0);
  }
  // slot m < NPF, which the prefetch brought
  template <int NPF>
  __device__ __forceinline__ cd prefetched(int m, int lane) const {
    return fromv(*reinterpret_cast<const dv2*>(pf_l + (wv * NPF + m) * 128 + 2 * lane));
  }
  template <int LD>
  __device__ __forceinline__ cd load(int u, int m, unsigned loff) const {
    return gload<LD>(at(slot_ptr(u, m), loff));
  }
  __device__ __forceinline__ void store(int u, int m, unsigned loff, cd v) const { gstore<0>(at(slot_ptr(u, m), loff), v); }
};
using Tile = TileT<256>;
}  // namespace rec

template <int PROBE, bool PF, int LD, bool ZREV = false>
__device__ __forceinline__ void tp_mid_rec_body(cd* __restrict__ data, const TPArgs& a, int nunits,
                                                double* __restrict__ pf_l, cd* __restrict__ carr,
                                                cd* __restrict__ ctab, cd* __restrict__ tw_l) {
  constexpr int TN = 256, N2 = 8, N1 = TN / N2, XT = 8, NXT = TN / XT, NW = 16;
  constexpr int NPF = PF ? kRecNPF : 0;
  const int tid = threadIdx.x;
  const int lane = tid & 63, x = lane & 7, y2 = lane >> 3;
  const int wv = __builtin_amdgcn_readfirstlane(tid / 64);
  const i64 zs = (i64)TN << (a.lnyl ? a.lnyl : ilog2(TN));
  const cd lz = a.lamz;
  using rec::pin, rec::cfma;
  // Column table of unit u: lane c = x + 8 y2 of wave 0 loads the symbol of column (x, brev3(y2)),
  // the column every wave's lane c scans after the y2 DFT, and
  // writes a = lamz / (c + lamz) and r = 256 / (c + lamz), one unit ahead (the unit's barrier
  // publishes it; three buffers: waves behind that barrier still read the previous unit's).
  // One division per column and unit instead of one per thread, and no global load inside the
  // unit, whose wait would also wait for the prefetch in flight.
  const auto colsym_of = [&](int u) {
    return a.colsym[(u % NXT) * XT + x + (i64)TN * (a.k1_off + u / NXT + N1 * brev<N2>(y2))];
  };
  const auto ctab_put = [&](int buf, cd cs) {
    const cd den = make_cd(cs.x + 1.0 + lz.x, cs.y + lz.y);
    const double id = 1.0 / fma(den.x, den.x, den.y * den.y);
    const cd ri = make_cd(den.x * id, -den.y * id);  // 1 / (c + lamz)
    ctab[(2 * buf) * 64 + idx(lane)] = cmul(lz, ri);
    ctab[(2 * buf + 1) * 64 + idx(lane)] = make_cd(ri.x * (double)TN, ri.y * (double)TN);
  };
  if (tid < TN) tw_l[tid] = a.tw[tid];
  if (wv == 0 && (int)blockIdx.x < nunits) ctab_put(0, colsym_of((int)blockIdx.x));
  __syncthreads();
  const unsigned loff = 16u * ((unsigned)x + (unsigned)TN * (unsigned)y2);  // this lane's (x, row y2)
  const rec::TileT<256, ZREV> tile{data, zs, wv, pf_l};
  if constexpr (PF) {
    if ((int)blockIdx.x < nunits) tile.template prefetch<NPF, LD>((int)blockIdx.x, loff);
  }
  const cd zero = make_cd(0.0, 0.0);
  // the y2 DFT's per-lane constants (rec::y2_fwd_pair)
  const double s3 = (y2 & 1) ? -1.0 : 1.0;
  const cd w8 = a.tw[(TN / 8) * (y2 & 3)], w4 = a.tw[(TN / 4) * (y2 & 1)];

  // One unit.  MORE: another unit follows (its prefetch and column table are issued here); the
  // last unit is its own instantiation, so that every wait inside a unit knows what is in flight.
  int par = 0, buf = 0;
  const auto unit = [&](const int it, auto more_c) {
    constexpr bool more = decltype(more_c)::value;
    const int u = it;
    const int k1 = a.k1_off + u / NXT;  // global k1
    // (buf, then par, read here first: with par first read at its use below, the compiler orders
    // the two loop counters the other way round and the kernel's scalar registers are renumbered)
    const int nbuf = buf == 2 ? 0 : buf + 1;
    const int npar = par ^ 1;
    cd v[16], csn = zero;
    // (the slot loops of the load and the store phase stay here and in tp_mid_rec2_body, one
    // rec::Tile access per slot: moved whole into helpers that take v they spill, see rec)
    if constexpr (PROBE & PR_NO_LOAD) {
#pragma unroll
      for (int m = 0; m < 16; ++m) v[m] = make_cd(lane + m, wv + u);
    } else {
      if constexpr (PF) {
        // this wave's DMA landed (and its stores of the previous unit: leaving those in flight
        // behind a vmcnt(16) measured 0.7 % slower, profiles/r07_zrec_ab.txt)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int m = 0; m < NPF; ++m) v[m] = tile.template prefetched<NPF>(m, idx(lane));
      }
      if constexpr (more) csn = colsym_of(it + (int)gridDim.x);  // every wave loads (no wait at a join), wave 0 uses it
      {
        int ul = u;
        unsigned lo1 = loff;
        asm volatile("" : "+s"(ul), "+v"(lo1));  // scalar base + this register, formed here
#pragma unroll
        for (int m = NPF; m < 16; ++m) v[m] = tile.template load<LD>(ul, m, lo1);
      }
    }
    if (more && wv == 0) ctab_put(nbuf, csn);
    // twiddle W_256^{y2 k1}: one per thread (k1 uniform over the workgroup, y2 the lane's)
    {
      const cd w = tw_l[((idx(lane) >> 3) * k1) & (TN - 1)];
#pragma unroll
      for (int m = 0; m < 16; ++m) v[m] = cmul(v[m], w);
    }
    // (the scheduling barriers keep a few slots' temporaries live at a time)
    __builtin_amdgcn_sched_barrier(0);
    // y2 DFT across lane bits 5, 4, 3 (DIF): lane (x, y2) ends as frequency k2 = brev3(y2)
    if constexpr (!(PROBE & PR_NO_Y2)) {
#pragma unroll
      for (int m = 0; m < 16; m += 2) {
        rec::y2_fwd_pair(v[m], v[m + 1], w8, w4, s3);
        if ((m & 2) == 2) __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (!(PROBE & PR_NO_ZMATH)) {
      const int ln = idx(lane);
      const cd aa = ctab[(2 * buf) * 64 + ln];  // this lane's column (x, k2)
      // the wave-local solution (zero carry into the wave) without its factor r:
      // s_m = a s_{m-1} + v_m, t_m = r s_m (r joins in the fix-up's multiply-add below)
#pragma unroll
      for (int m = 1; m < 16; ++m) v[m] = cfma(aa, v[m - 1], v[m]);
      const cd E = cmul(ctab[(2 * buf + 1) * 64 + ln], v[15]);
      carr[(par * NW + wv) * 64 + ln] = E;  // the wave's block-end value t_15 of this column
#pragma unroll
      for (int m = 0; m < 16; ++m) pin(v[m]);
      lds_barrier();  // the unit's only barrier: every wave's block-end values are in carr[par]
      cd cin;  // the carry into this wave for this lane's column
      {
        const cd am2 = cmul(aa, aa), am4 = cmul(am2, am2), am8 = cmul(am4, am4);
        const cd A = cmul(am8, am8);  // a^16
        cd acc = E;                   // E_wv
#pragma unroll
        for (int k = 14; k >= 0; --k) {
          acc = cfma(acc, A, carr[(par * NW + ((wv - 1 - k) & 15)) * 64 + ln]);
          if ((k & 3) == 0) __builtin_amdgcn_sched_barrier(0);  // 4 reads in flight, not 16 (64 VGPRs)
        }
        const cd A2 = cmul(A, A), A4 = cmul(A2, A2), A8 = cmul(A4, A4), A16 = cmul(A8, A8);
        const cd d = make_cd(1.0 - A16.x, -A16.y);
        const double id = 1.0 / fma(d.x, d.x, d.y * d.y);
        cin = make_cd(fma(acc.x, d.x, acc.y * d.y) * id, fma(acc.y, d.x, -acc.x * d.y) * id);
      }
      // u_m = r s_m + a^{m+1} cin
      const cd r = ctab[(2 * buf + 1) * 64 + ln];
      cd g = cmul(aa, cin);
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        v[m] = cfma(r, v[m], g);
        if (m < 15) g = cmul(aa, g);
      }
    }
    // inverse y2 DFT on the conjugate (DIT over lane bits 3, 4, 5: bit-reversed in, natural
    // out), conjugate twiddle, then the next unit's prefetch and this unit's stores
    {
      // opaque copies: the twiddle is read again and the addresses formed again, instead of
      // living in registers since the loads
      int k1s = k1, us = u;
      unsigned lo2 = loff;
      asm volatile("" : "+s"(k1s), "+s"(us), "+v"(lo2));
      const cd w = tw_l[((idx(lane) >> 3) * k1s) & (TN - 1)];
#pragma unroll
      for (int m = 0; m < 16; m += 2) {
        rec::y2_inv_pair<PROBE>(v[m], v[m + 1], w, w8, w4, s3);
        if ((m & 2) == 2) __builtin_amdgcn_sched_barrier(0);
      }
      // The next unit's prefetch goes out here, behind all of this unit's arithmetic and in
      // front of its stores, which then leave in one burst.  Issued right after the loads (where
      // it flies longest) and with the stores spread over the inverse DFT the same kernel takes
      // 90.0 us instead of 86.0 (profiles/r08_zrows_probe.txt).  No global load follows it inside
      // the unit, so no wait drains it early.
      if constexpr (PF && more && !(PROBE & PR_NO_LOAD)) {
        tile.template prefetch<NPF, LD>(it + (int)gridDim.x, loff);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (!(PROBE & PR_NO_STORE)) {
#pragma unroll
        for (int m = 0; m < 16; ++m) tile.store(us, m, lo2, v[m]);
      }
      if constexpr (PROBE & PR_NO_STORE) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < 16; ++m) acc += v[m].x + v[m].y;
        if (acc == 1.2345e300) tile.store(us, 0, lo2, make_cd(acc, 0.0));  // keeps the work live, never true
      }
    }
    par = npar;
    buf = nbuf;
  };
  int it = blockIdx.x;
  for (; it + (int)gridDim.x < nunits; it += gridDim.x) unit(it, std::true_type{});
  if (it < nunits) unit(it, std::false_type{});
}

template <int PROBE = 0, bool PF = false, int LD = 0, int TAG = 0>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4)))
k_tp_mid_rec(cd* data, TPArgs a, int nunits) {
#ifndef CFP_KEXP
  static_assert(PROBE == 0, "timing probes are built in tools/kexp only");
#endif
  __shared__ __attribute__((aligned(16))) double pf_l[PF ? 16 * kRecNPF * 128 : 2];
  __shared__ __attribute__((aligned(16))) cd carr[2 * 16 * 64];  // block-end values [unit parity][wave][column]
  __shared__ __attribute__((aligned(16))) cd ctab[3 * 2 * 64];   // the columns' a and r [unit mod 3][a, r][column]
  __shared__ cd tw_l[256];  // the twiddles: a global load after the kernel's own stores is a vector load
  tp_mid_rec_body<PROBE, PF, LD>(data, a, nunits, pf_l, carr, ctab, tw_l);
}

// ---------------------------------------------------------------------------------------------
// P2 for the upwind transport symbol with lambda_z < 0 (k_tp_mid_recb; 256^3, default shape).  The
// column's symbol is c + q (1 - e^{+2 pi i kz / nz}), q = -lambda_z: with a = q / (c + q) the z
// solve is the backward cyclic system u_z = a u_{z+1} + w_z, w = v nz / (c + q), which z -> 255 - z
// turns into k_tp_mid_rec's forward one.  So the kernel is tp_mid_rec_body on the planes in reverse
// order (rec::TileT<256, true>: slot m of wave wv is plane 255 - (16 wv + m); wave 15 slot 15 is
// plane 0, wave 0 slot 0 plane 255, the tile's own 256 planes) with a.lamz = q: the twiddle
// W^{y2 k1}, the y2 DFT, the column table and the scans do not depend on z.
template <int PROBE = 0, bool PF = false, int LD = 0, int TAG = 0>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4)))
k_tp_mid_recb(cd* data, TPArgs a, int nunits) {
#ifndef CFP_KEXP
  static_assert(PROBE == 0, "timing probes are built in tools/kexp only");
#endif
  __shared__ __attribute__((aligned(16))) double pf_l[PF ? 16 * kRecNPF * 128 : 2];
  __shared__ __attribute__((aligned(16))) cd carr[2 * 16 * 64];
  __shared__ __attribute__((aligned(16))) cd ctab[3 * 2 * 64];
  __shared__ cd tw_l[256];
  tp_mid_rec_body<PROBE, PF, LD, true>(data, a, nunits, pf_l, carr, ctab, tw_l);
}

// ---------------------------------------------------------------------------------------------
// P2 for the advection-diffusion symbol with z solved by a two-sided recurrence (k_tp_mid_rec2;
// 256^3, N2 = 8): tp_mid_rec_body's tile, access, y2 DFT and forward scan, then the same scan
// backwards.  A function of its own, so that the transport kernel's code stays what it was.
// With p = lamz + muz, q = muz and d = c + p + q the column's symbol is
//   d - p e^{-i theta} - q e^{i theta} = beta (1 - a e^{-i theta}) (1 - b e^{i theta}),
// beta the root of beta^2 - d beta + p q = 0 of larger modulus, a = p / beta, b = q / beta: the
// forward system t_z = a t_{z-1} + w_z, w = v nz / beta, as in tp_mid_rec_body, then the backward
// system u_z = b u_{z+1} + t_z the same way downwards: a register scan from slot 15 to 0, the
// waves' block-start values F_w = s'_0 into the second carry array, a second workgroup barrier,
// the carry
//   U_{16 (w + 1)} = sum_k b^{16 k} F_{(w + 1 + k) mod 16} / (1 - b^256)   (Horner in b^16)
// from the later waves, and b^{16-m} U added to slot m.  With two barriers per unit the carry
// arrays need no unit parity (a wave that runs ahead into the next unit's forward write has passed
// this unit's second barrier, behind every read of the forward array; the backward array likewise
// behind the next unit's first), so the forward and the backward array share the 32 KiB and the
// seven prefetched slots stay: 157 of 160 KiB with the table's third entry (b).
//
// The columns' a, r = 256 / beta and b (one complex square root each) come from the host, which
// computes them when the symbol is set (cfp_plan.hip, [unit][a, r, b][lane], 3 MiB): wave 0
// brings 3 KiB per unit by LDS-DMA straight into the table, two units ahead and issued with the
// prefetch at the unit's end (a DMA pending across the next unit's loads would turn their counted
// waits into vmcnt(0)); the next unit's first barrier publishes it.  Three buffers: the one
// written at a unit's end was last read two units earlier.  The host enables the kernel where
// max(|a|, |b|) <= 1 - 2^-7 on every column.
//
// NX = 128 (k_tp_mid_rec2_half): the same unit on the real plan's half spectrum H (128 x, 256 y,
// 256 z: rows of NX points, 16 x tiles per row, 512 units, tab2 with 512 units); XCD: units in
// xcd_unit order (the host launches whole rounds), as the FFT kernel of that stage runs.
template <int PROBE, bool PF, int LD, int NX = 256, bool XCD = false>
__device__ __forceinline__ void tp_mid_rec2_body(cd* __restrict__ data, const TPArgs& a, int nunits,
                                                 double* __restrict__ pf_l, cd* __restrict__ carr,
                                                 cd* __restrict__ ctab, cd* __restrict__ tw_l,
                                                 const cd* __restrict__ tab2) {
  constexpr int TN = 256, NXT = rec::TileT<NX>::NXT, NW = 16;
  constexpr int NPF = PF ? kRecNPF : 0;
  const int tid = threadIdx.x;
  const int lane = tid & 63, x = lane & 7, y2 = lane >> 3;
  const int wv = __builtin_amdgcn_readfirstlane(tid / 64);
  const i64 zs = (i64)NX << (a.lnyl ? a.lnyl : ilog2(TN));
  using rec::at, rec::pin, rec::cfma;
  // the unit of persistent-grid iteration `it`
  const auto unit_of = [](int it) {
    if constexpr (XCD) return xcd_unit(it, (int)gridDim.x);
    else return it;
  };
  // unit u's a, r, b of the host's table -> ctab[buf] by LDS-DMA, lane-linear (wave 0)
  const auto tab_fetch = [&](int u, int buf) {
    unsigned lo = 16u * (unsigned)lane;
    asm volatile("" : "+s"(u), "+v"(lo));
#pragma unroll
    for (int e = 0; e < 3; ++e)
      __builtin_amdgcn_global_load_lds((glb_void_t*)at(const_cast<cd*>(tab2) + (i64)(3 * u + e) * 64, lo),
                                       (lds_void_t*)(ctab + (3 * buf + e) * 64), 16, 0, 0);
  };
  if (tid < TN) tw_l[tid] = a.tw[tid];
  if (wv == 0 && (int)blockIdx.x < nunits) {  // the first two units' tables
    tab_fetch(unit_of((int)blockIdx.x), 0);
    if ((int)(blockIdx.x + gridDim.x) < nunits) tab_fetch(unit_of((int)(blockIdx.x + gridDim.x)), 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  const unsigned loff = 16u * ((unsigned)x + (unsigned)NX * (unsigned)y2);  // this lane's (x, row y2)
  const rec::TileT<NX> tile{data, zs, wv, pf_l};
  if constexpr (PF) {
    if ((int)blockIdx.x < nunits) tile.template prefetch<NPF, LD>(unit_of((int)blockIdx.x), loff);
  }
  // the y2 DFT's per-lane constants (rec::y2_fwd_pair)
  const double s3 = (y2 & 1) ? -1.0 : 1.0;
  const cd w8 = a.tw[(TN / 8) * (y2 & 3)], w4 = a.tw[(TN / 4) * (y2 & 1)];
  // the cyclic closure of a Horner sum: acc / (1 - P16^16), P16 the ratio's 16th power
  const auto close = [](cd acc, cd P16) {
    const cd P2 = cmul(P16, P16), P4 = cmul(P2, P2), P8 = cmul(P4, P4), P = cmul(P8, P8);
    const cd d = make_cd(1.0 - P.x, -P.y);
    const double id = 1.0 / fma(d.x, d.x, d.y * d.y);
    return make_cd(fma(acc.x, d.x, acc.y * d.y) * id, fma(acc.y, d.x, -acc.x * d.y) * id);
  };
  const auto pow16 = [](cd t) {
    const cd t2 = cmul(t, t), t4 = cmul(t2, t2), t8 = cmul(t4, t4);
    return cmul(t8, t8);
  };

  // One unit.  MORE: another unit follows; the last unit is its own instantiation.
  int buf = 0;
  const auto unit = [&](const int it, auto more_c) {
    constexpr bool more = decltype(more_c)::value;
    const int u = unit_of(it);
    const int k1 = a.k1_off + u / NXT;  // global k1
    const int nbuf = buf == 2 ? 0 : buf + 1;
    cd v[16];
    if constexpr (PROBE & PR_NO_LOAD) {
#pragma unroll
      for (int m = 0; m < 16; ++m) v[m] = make_cd(lane + m, wv + u);
    } else {
      if constexpr (PF) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA landed
#pragma unroll
        for (int m = 0; m < NPF; ++m) v[m] = tile.template prefetched<NPF>(m, idx(lane));
      }
      {
        int ul = u;
        unsigned lo1 = loff;
        asm volatile("" : "+s"(ul), "+v"(lo1));  // scalar base + this register, formed here
#pragma unroll
        for (int m = NPF; m < 16; ++m) v[m] = tile.template load<LD>(ul, m, lo1);
      }
    }
    // twiddle W_256^{y2 k1}
    {
      const cd w = tw_l[((idx(lane) >> 3) * k1) & (TN - 1)];
#pragma unroll
      for (int m = 0; m < 16; ++m) v[m] = cmul(v[m], w);
    }
    __builtin_amdgcn_sched_barrier(0);
    // y2 DFT across lane bits 5, 4, 3 (DIF): lane (x, y2) ends as frequency k2 = brev3(y2)
    if constexpr (!(PROBE & PR_NO_Y2)) {
#pragma unroll
      for (int m = 0; m < 16; m += 2) {
        rec::y2_fwd_pair(v[m], v[m + 1], w8, w4, s3);
        if ((m & 2) == 2) __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (!(PROBE & PR_NO_ZMATH)) {
      const int ln = idx(lane);
      // forward: s_m = a s_{m-1} + v_m, t_m = r s_m + a^{m+1} (carry into the wave)
      const cd aa = ctab[(3 * buf) * 64 + ln];  // this lane's column (x, k2)
#pragma unroll
      for (int m = 1; m < 16; ++m) v[m] = cfma(aa, v[m - 1], v[m]);
      const cd E = cmul(ctab[(3 * buf + 1) * 64 + ln], v[15]);
      carr[wv * 64 + ln] = E;  // the wave's block-end value t_15 of this column
#pragma unroll
      for (int m = 0; m < 16; ++m) pin(v[m]);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // wave 0: the table DMA of the previous unit's end has landed
      lds_barrier();  // every wave's block-end values are in carr[0]
      {
        const cd A = pow16(aa);
        cd acc = E;  // E_wv
#pragma unroll
        for (int k = 14; k >= 0; --k) {
          acc = cfma(acc, A, carr[((wv - 1 - k) & 15) * 64 + ln]);
          if ((k & 3) == 0) __builtin_amdgcn_sched_barrier(0);  // 4 reads in flight, not 16
        }
        const cd r = ctab[(3 * buf + 1) * 64 + ln];
        cd g = cmul(aa, close(acc, A));
#pragma unroll
        for (int m = 0; m < 16; ++m) {
          v[m] = cfma(r, v[m], g);
          if (m < 15) g = cmul(aa, g);
        }
      }
      // backward: s'_m = b s'_{m+1} + t_m, u_m = s'_m + b^{16-m} (carry from the later waves)
      const cd bb = ctab[(3 * buf + 2) * 64 + ln];
#pragma unroll
      for (int m = 14; m >= 0; --m) v[m] = cfma(bb, v[m + 1], v[m]);
      carr[(NW + wv) * 64 + ln] = v[0];  // the wave's block-start value of this column
#pragma unroll
      for (int m = 0; m < 16; ++m) pin(v[m]);
      lds_barrier();  // every wave's block-start values are in carr[1]
      {
        const cd B = pow16(bb);
        cd acc = v[0];  // F_wv
#pragma unroll
        for (int k = 14; k >= 0; --k) {
          acc = cfma(acc, B, carr[(NW + ((wv + 1 + k) & 15)) * 64 + ln]);
          if ((k & 3) == 0) __builtin_amdgcn_sched_barrier(0);
        }
        cd g = cmul(bb, close(acc, B));
#pragma unroll
        for (int m = 15; m >= 0; --m) {
          v[m] = cadd(v[m], g);
          if (m > 0) g = cmul(bb, g);
        }
      }
    }
    // inverse y2 DFT on the conjugate, conjugate twiddle, then the DMAs and this unit's stores
    {
      int k1s = k1, us = u;
      unsigned lo2 = loff;
      asm volatile("" : "+s"(k1s), "+s"(us), "+v"(lo2));
      const cd w = tw_l[((idx(lane) >> 3) * k1s) & (TN - 1)];
#pragma unroll
      for (int m = 0; m < 16; m += 2) {
        rec::y2_inv_pair<PROBE>(v[m], v[m + 1], w, w8, w4, s3);
        if ((m & 2) == 2) __builtin_amdgcn_sched_barrier(0);
      }
      // behind all of this unit's arithmetic and in front of its stores: the next unit's prefetch
      // and the table of the unit after it (nobody reads that buffer any more: its last readers
      // passed this unit's second barrier)
      if constexpr (more) {
        if constexpr (PF && !(PROBE & PR_NO_LOAD)) tile.template prefetch<NPF, LD>(unit_of(it + (int)gridDim.x), loff);
        if (wv == 0 && it + 2 * (int)gridDim.x < nunits)
          tab_fetch(unit_of(it + 2 * (int)gridDim.x), nbuf == 2 ? 0 : nbuf + 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (!(PROBE & PR_NO_STORE)) {
#pragma unroll
        for (int m = 0; m < 16; ++m) tile.store(us, m, lo2, v[m]);
      }
      if constexpr (PROBE & PR_NO_STORE) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < 16; ++m) acc += v[m].x + v[m].y;
        if (acc == 1.2345e300) tile.store(us, 0, lo2, make_cd(acc, 0.0));  // keeps the work live, never true
      }
    }
    buf = nbuf;
  };
  int it = blockIdx.x;
  for (; it + (int)gridDim.x < nunits; it += gridDim.x) unit(it, std::true_type{});
  if (it < nunits) unit(it, std::false_type{});
}

// the kernel of tp_mid_rec2_body: tab2 the columns' a, r, b (cfp_three_pass.h)
template <int PROBE = 0, bool PF = false, int LD = 0, int TAG = 0>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4)))
k_tp_mid_rec2(cd* data, TPArgs a, int nunits, const cd* tab2) {
#ifndef CFP_KEXP
  static_assert(PROBE == 0, "timing probes are built in tools/kexp only");
#endif
  __shared__ __attribute__((aligned(16))) double pf_l[PF ? 16 * kRecNPF * 128 : 2];
  __shared__ __attribute__((aligned(16))) cd carr[2 * 16 * 64];  // [forward block ends, backward block starts][wave][column]
  __shared__ __attribute__((aligned(16))) cd ctab[3 * 3 * 64];   // the columns' a, r and b [unit mod 3][a, r, b][column]
  __shared__ cd tw_l[256];
  tp_mid_rec2_body<PROBE, PF, LD>(data, a, nunits, pf_l, carr, ctab, tw_l, tab2);
}

// the same on the real plan's half spectrum H (rows of 128 points, 512 units; cfp_three_pass.h
// launch_three_pass_real_rec2).  H is plan-owned and 16-byte aligned: the prefetching body only.
template <bool XCD, int LD = 0>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4)))
k_tp_mid_rec2_half(cd* data, TPArgs a, int nunits, const cd* tab2) {
  __shared__ __attribute__((aligned(16))) double pf_l[16 * kRecNPF * 128];
  __shared__ __attribute__((aligned(16))) cd carr[2 * 16 * 64];
  __shared__ __attribute__((aligned(16))) cd ctab[3 * 3 * 64];
  __shared__ cd tw_l[256];
  tp_mid_rec2_body<0, true, LD, 128, XCD>(data, a, nunits, pf_l, carr, ctab, tw_l, tab2);
}

// The launchers.  Each one-GPU kernel has four instantiations, chosen by by2(pf, krylov): PF, the
// body with the LDS-DMA prefetch, which takes 16-byte addresses (a buffer that is only 8-byte
// aligned runs the body without it), and TAG 1 inside the stand-in KSP (TPArgs::krylov, as
// launch_mid_sw of cfp_tp_mid.hip).
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
constexpr int kRecUnits = (256 / 8) * (256 / 8);  // x tiles x k1 of the 256^3 grid

// k_tp_mid_rec: 256^3, default shape, an eligible transport symbol (a.zrec)
hipError_t tp_mid_rec(cd* data, const TPArgs& a, hipStream_t s) {
  const dim3 g(grid_of(kRecUnits, 1)), b(1024);
  by2(aligned16(data), a.krylov != 0, [&](auto pf, auto kr) {
    TP_LAUNCH((k_tp_mid_rec<0, decltype(pf)::value, kP2LoadFlags, decltype(kr)::value>), g, b, s, data, a, kRecUnits);
  });
  return hipGetLastError();
}

// a.lamz = -lambda_z (the caller has checked the ratio's cap)
hipError_t launch_three_pass_recb(cd* data, const TPArgs& a, hipStream_t s) {
  if (a.lnyl != 0 || a.k1_off != 0) return hipErrorInvalidValue;  // one GPU's natural layout only
  const dim3 g(grid_of(kRecUnits, 1)), b(1024);
  by2(aligned16(data), a.krylov != 0, [&](auto pf, auto kr) {
    TP_LAUNCH((k_tp_mid_recb<0, decltype(pf)::value, kP2LoadFlags, decltype(kr)::value>), g, b, s, data, a, kRecUnits);
  });
  return hipGetLastError();
}

hipError_t launch_three_pass_rec2(cd* data, const TPArgs& a, const cd* tab2, hipStream_t s) {
  const dim3 g(grid_of(kRecUnits, 1)), b(1024);
  by2(aligned16(data), a.krylov != 0, [&](auto pf, auto kr) {
    TP_LAUNCH((k_tp_mid_rec2<0, decltype(pf)::value, kP2LoadFlags, decltype(kr)::value>), g, b, s, data, a, kRecUnits,
              tab2);
  });
  return hipGetLastError();
}

// Stage 1 of a z-slab rank at 256^3 by the two-sided recurrence: launch_three_pass_rec2's kernels
// (no instantiation of its own, never TAG 1, not stamped) on the rank's [256 z][nyl][256 x] block.
// Units: 32 x tiles times the nyl / 8 local k1 rows, so with 8 or 16 ranks (128 or 64 units) every
// workgroup has one unit and runs the body's last-unit instantiation alone: one table fetch, no
// prefetch of a next unit.
hipError_t launch_three_pass_slab_rec2(cd* data, const TPArgs& a, const cd* tab2, hipStream_t s) {
  const int nk1 = a.lnyl ? (1 << a.lnyl) / 8 : 32;  // local k1 values: nyl / N2
  const int units = 32 * nk1;
  if (nk1 < 1 || nk1 > 32 || a.k1_off < 0 || a.k1_off + nk1 > 32) return hipErrorInvalidValue;
  const dim3 g(grid_of(units, 1)), b(1024);
  if (aligned16(data))
    hipLaunchKernelGGL((k_tp_mid_rec2<0, true, kP2LoadFlags>), g, b, 0, s, data, a, units, tab2);
  else
    hipLaunchKernelGGL((k_tp_mid_rec2<0, false, kP2LoadFlags>), g, b, 0, s, data, a, units, tab2);
  return hipGetLastError();
}

// The half-spectrum stage 1 of the real plan at 256^3 by the two-sided recurrence, in the unit
// order CFP_REAL_REC2_XCD chooses (cfp_tp_launch.h)
hipError_t launch_three_pass_real_rec2(cd* H, const TPArgs& a, const cd* tab2, hipStream_t s) {
  constexpr int units = (128 / 8) * 32;  // x tiles of the half spectrum x k1
  static_assert(units * 3 * 64 == kRealRec2TabLen, "the table of launch_three_pass_real_rec2");
  const unsigned gx = CFP_REAL_REC2_XCD ? grid_xcd(units, 1) : 0;
  if (gx) TP_LAUNCH((k_tp_mid_rec2_half<true, kP2LoadFlags>), dim3(gx), dim3(1024), s, H, a, units, tab2);
  else TP_LAUNCH((k_tp_mid_rec2_half<false, kP2LoadFlags>), dim3(grid_of(units, 1)), dim3(1024), s, H, a, units, tab2);
  return hipGetLastError();
}

}  // namespace cfp
