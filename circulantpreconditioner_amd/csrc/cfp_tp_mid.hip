// cfp_tp_mid.hip -- the middle sweep P2 of the 3-sweep apply by FFT (k_tp_mid: the y2 DFT on DPP
// lane permutations; k_tp_mid_sw: on permlane register transposes; the schedule:
// cfp_three_pass.hip) and every launcher that instantiates them: one GPU, z-slab ranks, the real
// plan's half spectrum and Nyquist column.
#include "cfp_tp_device.h"
#include "cfp_tp_launch.h"

namespace cfp {

// Persistent over units u = (x-tile, k1); T columns per unit = T/N2 x values times N2 y2.
// Barriers wait for LDS only, so one unit's stores drain while the next unit loads.
// N2 = 16 (512^3, r04): one more radix-2 lane stage (lane ^ 8, twiddle W_16^(y2 & 7)) in front of
// the 8-point one.  XCD: units in xcd_unit order (the host launches whole rounds).
// BLK: the blocked layout of k_tp_rows<.., BLK> (BLK = XT: one run of T values per z; 512^3 with
// BLK = 8: the unit's 16 32-byte pieces of a z lie in one contiguous 2 KiB block, shared by the
// four x tiles of the block, which run under one L2 in XCD order).
template <int FLAGS, int T, int N2, int TN, int PTS = 16, bool XS = true, int NX = TN, bool XCD = false,
          int BLK = 0, int PROBE = 0>
__global__ void __launch_bounds__(T * (TN / PTS)) __attribute__((amdgpu_waves_per_eu(4)))
k_tp_mid(cd* data, TPArgs a, int nunits) {
#ifndef CFP_KEXP
  static_assert(PROBE == 0, "timing probes are built in tools/kexp only");
#endif
  constexpr int N1 = TN / N2, TZ = TN / PTS, NT = T * TZ, XT = T / N2, NXT = NX / XT;
  constexpr int F = FLAGS | (XS ? F_SPLIT_LDS : 0) | F_LDS_SYNC;
  static_assert(N2 == 4 || N2 == 8 || N2 == 16, "the y2 DFT runs across 4, 8 or 16 lanes");
  static_assert(BLK == 0 || (BLK % XT == 0 && NX % BLK == 0), "blocks of whole x tiles");
  __shared__ __attribute__((aligned(16))) double lds[T * TN * (XS ? 1 : 2)];
  __shared__ cd tw_l[TN];
  const int tid = threadIdx.x;
  for (int i = tid; i < TN; i += NT) tw_l[i] = a.tw[i];
  const int c0 = tid & (T - 1), tz0 = tid / T;
  // NX: row length (TN; the real plan's half spectrum: TN / 2).  Slab plans (a.lnyl): this rank's
  // z-pencil block [TN z][nyl][NX] with the global k1 range [k1_off, k1_off + nyl / N2)
  const i64 zs = (i64)NX << (a.lnyl ? a.lnyl : ilog2(TN));
  // Everything but the 16 points is rebuilt from laundered copies of the thread indices where
  // it is used: 128 VGPRs hold the points plus one radix-16 stage's twiddles, and an address,
  // twiddle or index kept live across the FFTs (or hoisted out of the unit loop) spills.
  struct Col {
    cd* col;  // this thread's first point; slot m adds the uniform zs * TZ m
    int y2, xk;
    cd w, w8, w16;  // W_TN^{y2 k1}; W_8^(y2 & 3) (N2 >= 8); W_16^(y2 & 7) (N2 = 16)
  };
  const auto column = [&](int u) {
    int c = c0, tz = tz0;
    asm volatile("" : "+v"(c), "+v"(tz));
    Col q;
    const int xt = u % NXT, k1 = u / NXT;
    q.y2 = c & (N2 - 1);
    q.xk = xt * XT + c / N2;
    q.col = BLK ? data + (i64)NX * N2 * k1 + (q.xk / BLK) * (N2 * BLK) + q.y2 * BLK + q.xk % BLK + zs * tz
                : data + q.xk + (i64)NX * (q.y2 + N2 * k1) + zs * tz;
    q.w = a.tw[(q.y2 * (a.k1_off + k1)) & (TN - 1)];  // global k1
    q.w8 = a.tw[(TN / 8) * (q.y2 & 3)];
    if constexpr (N2 == 16) q.w16 = a.tw[(TN / 16) * (q.y2 & 7)];
    return q;
  };
  for (int it = blockIdx.x; it < nunits; it += gridDim.x) {
    const int u = XCD ? xcd_unit(it, gridDim.x) : it;
    cd v[PTS];
    {
      const Col q = column(u);
#pragma unroll
      for (int m = 0; m < PTS; ++m) {
        if constexpr (PROBE & PR_NO_LOAD) v[m] = make_cd(c0 + m, tz0 + u);
        else v[m] = gload<FLAGS>(q.col + zs * TZ * m);
      }
#pragma unroll
      for (int m = 0; m < PTS; ++m) {  // the lane DFT in two sweeps over the slots: fewer live temporaries
        v[m] = cmul(v[m], q.w);
        if constexpr ((PROBE & PR_NO_Y2) != 0) continue;
        if constexpr (N2 == 16) {  // dft16_dif's first stage
          const cd p = lane_xor8(v[m]);
          v[m] = (q.y2 & 8) ? cmul(csub(p, v[m]), q.w16) : cadd(v[m], p);
        }
        if constexpr (N2 >= 8) {  // dft8_dif's first stage
          const cd p = lane_xor4(v[m]);
          v[m] = (q.y2 & 4) ? cmul(csub(p, v[m]), q.w8) : cadd(v[m], p);
        }
      }
#pragma unroll
      for (int m = 0; m < PTS; ++m)
        if constexpr (!(PROBE & PR_NO_Y2)) v[m] = dft4_dif(v[m], q.y2 & 3);  // the lane now holds k2
    }
    {
      int c = c0, tz = tz0;
      asm volatile("" : "+v"(c), "+v"(tz));
      if constexpr (!(PROBE & PR_NO_ZMATH))
        fft_stages<TN, PTS, r0_of(TN, PTS), false, T, F>(v, lds, tw_l, c, tz, true);  // kz = tz + TZ m
    }
    {
      int c = c0, tz = tz0;
      asm volatile("" : "+v"(c), "+v"(tz));
      const int k1 = a.k1_off + u / NXT, y2 = c & (N2 - 1);  // global k1
      const cd cs = a.colsym[(u % NXT) * XT + c / N2 + (i64)NX * (k1 + N1 * brev<N2>(y2))];
#pragma unroll
      for (int m = 0; m < PTS; ++m) {
        const cd d = cadd(cadd(cs, a.axsym[tz + TZ * m]), make_cd(1.0, 0.0));
        v[m] = (PROBE & PR_NO_ZMATH) ? cconj(v[m]) : cconj(cdiv_sym(v[m], d));
      }
      if constexpr (!(PROBE & PR_NO_ZMATH)) fft_stages<TN, PTS, r0_of(TN, PTS), false, T, F>(v, lds, tw_l, c, tz, false);
    }
    {
      const Col q = column(u);
#pragma unroll
      for (int m = 0; m < PTS; ++m)
        if constexpr (!(PROBE & PR_NO_Y2)) v[m] = dft4_dit(v[m], q.y2 & 3);
#pragma unroll
      for (int m = 0; m < PTS; ++m) {
        if constexpr ((PROBE & PR_NO_Y2) != 0) {
          v[m] = cmul(v[m], q.w);
          continue;
        }
        if constexpr (N2 >= 8) {  // dft8_dit's last stage
          const cd u = (q.y2 & 4) ? cmul(v[m], q.w8) : v[m];
          const cd p = lane_xor4(u);
          v[m] = (q.y2 & 4) ? csub(p, u) : cadd(u, p);
        }
        if constexpr (N2 == 16) {  // dft16_dit's last stage
          const cd u = (q.y2 & 8) ? cmul(v[m], q.w16) : v[m];
          const cd p = lane_xor8(u);
          v[m] = (q.y2 & 8) ? csub(p, u) : cadd(u, p);
        }
        v[m] = cmul(v[m], q.w);
      }
      if constexpr (PROBE & PR_NO_STORE) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < PTS; ++m) acc += v[m].x + v[m].y;
        if (acc == 1.2345e300) q.col[0] = make_cd(acc, 0.0);  // keeps the work live, never true
      } else {
#pragma unroll
        for (int m = 0; m < PTS; ++m) gstore<FLAGS>(q.col + zs * TZ * m, cconj(v[m]));
      }
    }
    lds_barrier();  // the next unit's first exchange overwrites LDS
  }
}

// ---------------------------------------------------------------------------------------------
// P2 with the y2 DFT on register transposes (k_tp_mid_sw).  A wave is one z-group tz and all
// 64 columns c = x + XT * y2 of the tile (XT = 64 / N2), so the y2 bits are the top lane bits:
// N2 = 8: y2 = lane bits 3..5; N2 = 4: lane bits 4..5.  A radix-2 stage over lane bit 5 / 4
// transposes a register pair with v_permlane32_swap / v_permlane16_swap (lane bit <-> register
// bit, 2 swaps per double) and then runs a plain butterfly on the pair: no per-lane selects, no
// duplicated butterfly halves.  Lane bit 3 (N2 = 8 only) has no swap instruction: DPP row_ror:8
// brings the partner's value, and one fma with a per-lane sign forms sum or difference.
//
// The y2 DFT commutes with the z DFT, so it runs between the z transform's first radix-16 stage
// (per lane, over the 16 slots) and the LDS exchange; the exchange writes each value from its
// transposed register straight to its (column, z) place, so the transposes are never undone.
// Register r at lane L then holds slot s = (r & 12) | L5 | 2 L4 and y2 position
// p = 4 r0 + 2 r1 + L3 (N2 = 8) or p = 2 r0 + r1 (N2 = 4).  Forward: DIF, natural order in,
// bit-reversed frequencies out (the symbol index follows, as in k_tp_mid).  Inverse: DIT from
// the bit-reversed order back to natural, same register map, so the second exchange lands in
// the load layout.
// DIF stage over register pairs (k, k + D) after a swap on lane bit B: a + b, (a - b) w
// (TW = false: no twiddle)
template <int B, int D, bool TW = true, int NR = 16>
__device__ __forceinline__ void dif_pairs(cd* v, cd w) {
#pragma unroll
  for (int k = 0; k < NR; ++k)
    if ((k & D) == 0) swap_c<B>(v[k], v[k + D]);
#pragma unroll
  for (int k = 0; k < NR; ++k)
    if ((k & D) == 0) {
      const cd a = v[k], b = v[k + D];
      v[k] = cadd(a, b);
      v[k + D] = TW ? cmul(csub(a, b), w) : csub(a, b);
    }
}

//
// PF (prefetch): the exchange buffer is idle from the second exchange's last read to the next
// unit's first exchange, which is exactly where the next unit's data is needed.  Right after
// the second exchange each wave DMAs slots 0..7 of its columns of unit u + gridDim.x into that
// buffer (global_load_lds_dwordx4: 1 KiB per wave-instruction, lane-linear), so those loads
// fly during stage B', the twiddle and the stores; the next unit then loads only slots 8..15
// from HBM and reads 0..7 back from LDS.  Barriers stay LDS-only (no vmcnt), so the DMA is not
// drained early.
// NX: x extent (row length in points) of the grid P2 runs on: TN for the complex apply, TN / 2
// for the real-data plan's half spectrum (cfp_real.hip); y and z are TN long.
// BL: the blocked intermediate layout of k_tp_rows<.., BLK = XT>: a unit's T columns c = x + XT y2
// are the run at block column xt of row block k1, for every z (T 16 bytes).
//
// T = 32 (r04): 512 threads, two workgroups per CU that run their barrier phases independently.
// A wave then holds two z groups of the 32 columns: lane = x (bits 0-1) + tz parity (bit 2) +
// y2 (bits 3-5), so y2 keeps lane bits 3-5 and every y2 stage below (permlane swaps on bits 5 and
// 4, DPP on bit 3) is the T = 64 code; c (the column x + 4 y2) and tz index memory and LDS,
// `lane` the lane bits.
// XCD (r04): units in xcd_unit order (whole rounds), so x tiles that share 128-byte lines run
// under one L2 (T = 32 natural layout: 64-byte tiles).
template <int T, int N2, int TN, int PROBE = 0, bool PF = false, int NX = TN, int ST = 0, int LD = 0, bool BL = false,
          bool XCD = false, int TAG = 0>
__global__ void __launch_bounds__(T * (TN / 16)) __attribute__((amdgpu_waves_per_eu(4)))
k_tp_mid_sw(cd* data, TPArgs a, int nunits) {
#ifndef CFP_KEXP
  static_assert(PROBE == 0, "timing probes are built in tools/kexp only");
#endif
  static_assert(T == 64 || (T == 32 && N2 == 8), "a wave = the 64 columns of one z group, or 32 columns of two");
  static_assert(N2 == 4 || N2 == 8, "y2 = the top 2 or 3 lane bits");
  static_assert(TN == 256, "z = 16 x 16: radix-16 stage A in registers, one exchange, radix-16 stage B");
  constexpr int N1 = TN / N2, TZ = TN / 16, NT = T * TZ, XT = T / N2, NXT = NX / XT;
  constexpr int XB = ilog2(XT);  // lane bits of x
  static_assert(NX % XT == 0, "whole x tiles");
  static_assert(!BL || (NX == TN && N2 == 8), "blocked layout: complex grid, 8 x times 8 y2");
  __shared__ __attribute__((aligned(16))) double lds[T * TN];  // split exchange
  __shared__ cd tw_l[TN];
  const int tid = threadIdx.x;
  for (int i = tid; i < TN; i += NT) tw_l[i] = a.tw[i];
  __syncthreads();  // the y2 stages read tw_l before the first exchange barrier
  const int lane0 = tid & 63;
  const int c0 = T == 64 ? lane0 : (lane0 & 3) | ((lane0 >> 3) << 2);
  const int tz0 = T == 64 ? tid / 64 : 2 * (tid >> 6) + ((lane0 >> 2) & 1);
  // rows of this rank's block [TN z][nyl][NX] (one GPU: nyl = TN); unit u = (x tile, local k1)
  const i64 zs = (i64)NX << (a.lnyl ? a.lnyl : ilog2(TN));
  // this lane's first point and the twiddle W_TN^{y2 k1} (natural layout: x = c % XT, y2 = c / XT)
  const auto col_ptr = [&](int u, int c, int tz) {
    const int xt = u % NXT, k1 = u / NXT;
    if constexpr (BL) return data + (i64)NX * N2 * k1 + xt * T + c + zs * tz;
    return data + xt * XT + (c & (XT - 1)) + (i64)NX * ((c >> XB) + N2 * k1) + zs * tz;
  };
  const auto tw_y = [&](int u, int c) { return tw_l[((c >> XB) * (a.k1_off + u / NXT)) & (TN - 1)]; };
  constexpr int NPF = PF ? 8 : 0;  // slots 0 .. NPF-1 come from the LDS prefetch (exchange buffer)
  const int wv = __builtin_amdgcn_readfirstlane(tid / 64);
  if constexpr ((PROBE & PR_PRIO) != 0) {
    if (wv >= NT / 128) __builtin_amdgcn_s_setprio(1);
  }
  const auto prefetch = [&](int u) {  // this wave's slots 0 .. NPF-1 of unit u -> LDS
    const int c = idx(c0), tz = idx(tz0);
    const cd* src = col_ptr(u, c, tz);
#pragma unroll
    for (int m = 0; m < NPF; ++m)
      __builtin_amdgcn_global_load_lds((glb_void_t*)(src + zs * TZ * m), (lds_void_t*)(lds + (wv * NPF + m) * 128),
                                       16, 0, (LD & F_NT_LD) ? 2 : 0);
  };
  static_assert(!PF || (NT / 64) * NPF * 128 <= T * TN, "the prefetch fits the exchange buffer");
  if constexpr (PF) {
    if ((int)blockIdx.x < nunits) prefetch(XCD ? xcd_unit(blockIdx.x, gridDim.x) : (int)blockIdx.x);
  }
  // split exchange from the transposed registers (first radix-16 stage done) to the column
  // layout: v[t] = point tz + 16 t of column c
  const auto exchange_t = [&](cd* v, bool first) {
    if constexpr (PROBE & PR_NO_XCHG) return;
    const int c = idx(c0), tz = idx(tz0), lane = idx(lane0);
    const int l3 = N2 == 8 ? ((lane >> 3) & 1) : 0, l4 = (lane >> 4) & 1, l5 = (lane >> 5) & 1;
    const int wbase = (tz * 16 + l5 + 2 * l4) * T + (c & (XT - 1)) + XT * l3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (!(first && h == 0)) lds_barrier();
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = N2 == 8 ? 4 * (r & 1) + 2 * ((r >> 1) & 1) : 2 * (r & 1) + ((r >> 1) & 1);
        const int off = (r & 12) * T + XT * (N2 == 8 ? p & 6 : p);
        lds[wbase + off] = h ? v[r].y : v[r].x;
      }
      lds_barrier();
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const double d = lds[(tz + TZ * t) * T + c];
        if (h) v[t].y = d; else v[t].x = d;
      }
    }
  };
  // second radix-16 stage (Ns = 16): twiddles W_TN^{tz t}, then the in-register DFT
  const auto stage_b = [&](cd* v) {
    if constexpr (PROBE & PR_NO_ZMATH) return;
    const int tz = idx(tz0);
#pragma unroll
    for (int t = 1; t < 16; ++t) v[t] = cmul(v[t], tw_l[tz * t]);
    dft_reg<16>(v);
  };
  const auto lane_sign = [&]() {  // +1 where lane bit 3 is clear, -1 where set
    const int lane = idx(lane0);
    return (lane & 8) ? -1.0 : 1.0;
  };

  for (int it = blockIdx.x; it < nunits; it += gridDim.x) {
    const int u = XCD ? xcd_unit(it, gridDim.x) : it;
    cd v[16];
    if constexpr (PROBE & PR_NO_LOAD) {
      const int c = idx(c0), tz = idx(tz0);
#pragma unroll
      for (int m = 0; m < 16; ++m) v[m] = make_cd(c + m, tz + u);
    } else {
      const int c = idx(c0), tz = idx(tz0);
      const cd* src = col_ptr(u, c, tz);
#pragma unroll
      for (int m = NPF; m < 16; ++m) v[m] = gload<LD>(src + zs * TZ * m);  // LD: load policy
      if constexpr (PF) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA (and loads) landed
#pragma unroll
        for (int m = 0; m < NPF; ++m) {  // the DMA is lane-linear
          const int lane = idx(lane0);
          v[m] = fromv(*reinterpret_cast<const dv2*>(lds + (wv * NPF + m) * 128 + 2 * lane));
        }
      }
    }
    {
      const int c = idx(c0);
      const cd w = tw_y(u, c);
#pragma unroll
      for (int m = 0; m < 16; ++m) v[m] = cmul(v[m], w);
    }
    if constexpr (!(PROBE & PR_NO_ZMATH)) dft_reg<16>(v);  // z stage A (Ns = 1: no twiddles), per lane
    // y2 DFT, DIF: natural positions in, bit-reversed frequencies out
    if constexpr (PROBE & PR_NO_Y2) {
    } else if constexpr (N2 == 8) {
      {
        const int lane = idx(lane0);
        dif_pairs<5, 1>(v, tw_l[(TN / 8) * ((lane >> 3) & 3)]);  // W_8^{y2 & 3}
      }
      {
        const int lane = idx(lane0);
        dif_pairs<4, 2>(v, tw_l[(TN / 4) * ((lane >> 3) & 1)]);  // W_4^{y2 & 1}
      }
      const double s = lane_sign();
#pragma unroll
      for (int r = 0; r < 16; ++r) v[r] = bfly_l3(v[r], s);
    } else {
      {
        const int lane = idx(lane0);
        dif_pairs<5, 1>(v, tw_l[(TN / 4) * ((lane >> 4) & 1)]);  // W_4^{y2 & 1}
      }
      dif_pairs<4, 2, false>(v, make_cd(1.0, 0.0));
    }
    exchange_t(v, !PF);  // PF: other waves may still be reading their prefetched slots
    stage_b(v);  // v[m]: kz = tz + 16 m; column c = x + XT p
    {
      const int c = idx(c0), tz = idx(tz0);
      const int k1 = a.k1_off + u / NXT, p = c >> XB;  // global k1
      const cd cs = a.colsym[(u % NXT) * XT + (c & (XT - 1)) + (i64)NX * (k1 + N1 * brev<N2>(p))];
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        const cd d = cadd(cadd(cs, a.axsym[tz + TZ * m]), make_cd(1.0, 0.0));
        v[m] = (PROBE & PR_NO_ZMATH) ? cconj(v[m]) : cconj(cdiv_sym(v[m], d));
      }
    }
    if constexpr (!(PROBE & PR_NO_ZMATH)) dft_reg<16>(v);  // inverse (on the conjugate): z stage A
    // y2 DFT, DIT: bit-reversed positions in, natural out
    if constexpr (PROBE & PR_NO_Y2) {
    } else if constexpr (N2 == 8) {
      {
        const double s = lane_sign();
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = bfly_l3(v[r], s);
      }
      {
        const int lane = idx(lane0);
        const cd w = tw_l[(TN / 4) * ((lane >> 3) & 1)];  // W_4^{p & 1}, p bit 0 = lane bit 3
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if ((k & 2) == 0) swap_c<4>(v[k], v[k + 2]);
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if ((k & 2) == 0) {
            const cd x = v[k], y = cmul(v[k + 2], w);
            v[k] = cadd(x, y);
            v[k + 2] = csub(x, y);
          }
      }
      {
        // W_8^{p & 3}: p bit 0 = lane bit 3, p bit 1 = register bit 1 -> W_8^{l3} (x -i if r1)
        const int lane = idx(lane0);
        const cd w = tw_l[(TN / 8) * ((lane >> 3) & 1)];
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if ((k & 1) == 0) swap_c<5>(v[k], v[k + 1]);
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if ((k & 1) == 0) {
            cd y = cmul(v[k + 1], w);
            if (k & 2) y = mul_mi(y);
            const cd x = v[k];
            v[k] = cadd(x, y);
            v[k + 1] = csub(x, y);
          }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if ((k & 2) == 0) swap_c<4>(v[k], v[k + 2]);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if ((k & 2) == 0) {
          const cd x = v[k], y = v[k + 2];
          v[k] = cadd(x, y);
          v[k + 2] = csub(x, y);
        }
      // W_4^{p & 1}, p bit 0 = register bit 1
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if ((k & 1) == 0) swap_c<5>(v[k], v[k + 1]);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if ((k & 1) == 0) {
          const cd y = (k & 2) ? mul_mi(v[k + 1]) : v[k + 1];
          const cd x = v[k];
          v[k] = cadd(x, y);
          v[k + 1] = csub(x, y);
        }
    }
    exchange_t(v, false);
    if constexpr (PF) {
      lds_barrier();  // every wave has read the exchange buffer
      if (it + (int)gridDim.x < nunits) prefetch(XCD ? xcd_unit(it + gridDim.x, gridDim.x) : it + (int)gridDim.x);
    }
    stage_b(v);  // natural layout again: column c = x + XT y2, slot m = z
    {
      const int c = idx(c0), tz = idx(tz0);
      const cd w = tw_y(u, c);
      cd* dst = col_ptr(u, c, tz);
      if constexpr (PROBE & PR_NO_STORE) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < 16; ++m) acc += v[m].x * w.x + v[m].y;
        if (acc == 1.2345e300) dst[0] = make_cd(acc, 0.0);  // keeps the work live, never true
      } else {
#pragma unroll
        for (int m = 0; m < 16; ++m) gstore<ST>(dst + zs * TZ * m, cconj(cmul(v[m], w)));  // ST: store policy
      }
    }
    if constexpr (!PF) lds_barrier();  // the next unit's first exchange overwrites LDS
  }
}

template <int T, int N2, int TN, int PER_CU, int PTS = 16, bool XS = true>
static void launch_mid(cd* data, const TPArgs& a, hipStream_t s) {
  constexpr int units = (TN / (T / N2)) * (TN / N2);  // x-tiles x k1
  TP_LAUNCH((k_tp_mid<0, T, N2, TN, PTS, XS>), dim3(grid_of(units, PER_CU)), dim3(T * (TN / PTS)), s, data, a, units);
}

template <int N2, int TN, bool PF, bool BL, int T>
static void launch_mid_sw_pf(cd* data, const TPArgs& a, hipStream_t s) {
  constexpr int units = (TN / (T / N2)) * (TN / N2);
  if constexpr (T == 64 && N2 == 8 && TN == 256 && PF && !BL) {
    if (a.krylov) {  // the default 256^3 P2 inside the stand-in KSP: same kernel, TAG 1 (TPArgs::krylov)
      TP_LAUNCH((k_tp_mid_sw<T, N2, TN, 0, PF, TN, 0, kP2LoadFlags, BL, false, 1>), dim3(grid_of(units, 64 / T)),
                dim3(T * (TN / 16)), s, data, a, units);
      return;
    }
  }
  TP_LAUNCH((k_tp_mid_sw<T, N2, TN, 0, PF, TN, 0, kP2LoadFlags, BL>), dim3(grid_of(units, 64 / T)),
            dim3(T * (TN / 16)), s, data, a, units);
}

// pf: with the LDS-DMA prefetch (global_load_lds_dwordx4), which takes 16-byte aligned addresses:
// a buffer that is only 8-byte aligned runs the same kernel without it
template <int N2, int TN, bool BL = false, int T = 64>
static void launch_mid_sw(bool pf, cd* data, const TPArgs& a, hipStream_t s) {
  if (pf) launch_mid_sw_pf<N2, TN, true, BL, T>(data, a, s);
  else launch_mid_sw_pf<N2, TN, false, BL, T>(data, a, s);
}

// The FFT stage 1 of one GPU (cfp_tp_launch.h); the rows of each shape: tp_rows, cfp_three_pass.hip
hipError_t tp_mid(int n, cd* data, const TPArgs& a, TPShape shape, hipStream_t s) {
  if (n == 512) {
    // 512^3 (r04): N1 = 32 x N2 = 16.  The z FFT of 512 bounds the tile to 32 columns (128 KiB
    // split exchange) = 2 x times 16 y2, 32-byte runs; units in XCD order so the 4 tiles of a
    // 128-byte line share an L2.  96 N bytes per apply against 160 N.
    // shape.mid = blocked: blocks of 2 x (P2 reads one 512-byte run per z); blocked32: blocks of
    // 8 x (P2's 32-byte pieces of a z lie in one 2 KiB block).
    constexpr int units = (512 / 2) * 32;
    const unsigned g = grid_xcd(units, 1);  // whole rounds of a power of two >= 8
    if (g == 0) return hipErrorNotSupported;
    if (shape.mid == TP_MID_BLOCKED)
      TP_LAUNCH((k_tp_mid<0, 32, 16, 512, 16, true, 512, true, 2>), dim3(g), dim3(1024), s, data, a, units);
    else if (shape.mid == TP_MID_BLOCKED32)
      TP_LAUNCH((k_tp_mid<0, 32, 16, 512, 16, true, 512, true, 8>), dim3(g), dim3(1024), s, data, a, units);
    else  // NT loads: 204 against 262 /s (r04y)
      TP_LAUNCH((k_tp_mid<0, 32, 16, 512, 16, true, 512, true>), dim3(g), dim3(1024), s, data, a, units);
    return hipGetLastError();
  }
  if (n == 128) {
    // 128^3, n1 = 32 (N1 = 32 x N2 = 4; AUTO from r03m to r04): 32 columns = 8 x times 4 y2
    // (128-byte runs), 8 points per thread and whole-complex LDS exchanges (one barrier pair per
    // exchange instead of two), 512 threads, 64 KiB (2 per CU).  shape.mid = lane64 keeps the
    // round-2 kernels (16 points per thread, split exchanges, 64 columns) for A/B: 15.9k against
    // 18.4k applies/s, the 5-pass schedule 17.3k (profiles/r03m_128_three_sweep.md).
    // Default since r04: y split 16 x 8, 21,475 against 18,520 applies/s for the r03 split 32 x 4
    // (n1 = 32) in the same process (profiles/r04_schedule_ab.jsonl).
    const int n1 = shape.n1 ? shape.n1 : (shape.mid == TP_MID_LANE64 || shape.mid == TP_MID_SWAP64 ? 32 : 16);
    if (n1 != 16) {
      if (shape.mid == TP_MID_LANE64) launch_mid<64, 4, 128, 2>(data, a, s);
      else launch_mid<32, 4, 128, 2, 8, false>(data, a, s);
    }
    // P2 default (r04z): 32 columns = 4 x times 8 y2 (64-byte tiles, 512 units, two 512-thread
    // workgroups per CU, 8 points, whole-complex) in XCD order, so the two tiles of a 128-byte
    // line meet in one L2: 21,475 /s; in blockIdx order 19,130.  A/B: lane32 = 64 columns,
    // 8 points, whole-complex (1,024 threads; 21,070-21,150 /s); lane64 = 64 columns, 16
    // points, split (20,530 /s); swap64 = 64 columns, 16 points, whole-complex (20,750 /s)
    else if (shape.mid == TP_MID_LANE32) launch_mid<64, 8, 128, 1, 8, false>(data, a, s);
    else if (shape.mid == TP_MID_LANE64) launch_mid<64, 8, 128, 1>(data, a, s);
    else if (shape.mid == TP_MID_SWAP64) launch_mid<64, 8, 128, 1, 16, false>(data, a, s);
    else {
      constexpr int units = (128 / 4) * 16;
      const unsigned g = grid_xcd(units, 2);
      if (g) TP_LAUNCH((k_tp_mid<0, 32, 8, 128, 8, false, 128, true>), dim3(g), dim3(512), s, data, a, units);
      else launch_mid<32, 8, 128, 2, 8, false>(data, a, s);
    }
    return hipGetLastError();
  }
  // 256^3.  Default shape = the measured best: N1 = 32, P2 tiles of 64 columns (8 x times 8 y2,
  // 128-byte runs) with the y2 DFT on permlane transposes and the LDS-DMA prefetch of half the
  // next unit (k_tp_mid_sw<.., PF>; r02 A/B in the apply chain, profiles/r02e_p2_ab.txt: 138 us
  // without the prefetch, 144 us for the DPP lane kernel, 128 us with it), persistent grids.  The
  // other shapes are selected per plan (cfp_plan_set_three_pass_shape) for tests and measurements.
  const bool n64 = shape.n1 == 64;
  const bool pf_ok = ((uintptr_t)data & 15) == 0;
  switch (shape.mid) {
    case TP_MID_BLOCKED:  // N1 = 32, blocked intermediate layout (k_tp_rows<.., 8>)
      launch_mid_sw<8, 256, true>(pf_ok, data, a, s);
      break;
    case TP_MID_SWAP32X: {  // natural layout; 32 columns in XCD order, two per CU
      constexpr int units = (256 / 4) * 32;
      const dim3 g(grid_xcd(units, 2)), blk(512);
      if (g.x == 0) return hipErrorNotSupported;
      if (pf_ok) TP_LAUNCH((k_tp_mid_sw<32, 8, 256, 0, true, 256, 0, kP2LoadFlags, false, true>), g, blk, s, data, a, units);
      else TP_LAUNCH((k_tp_mid_sw<32, 8, 256, 0, false, 256, 0, kP2LoadFlags, false, true>), g, blk, s, data, a, units);
      break;
    }
    case TP_MID_BLOCKED32:  // blocks of 4 x; 32 columns, two workgroups per CU
      launch_mid_sw<8, 256, true, 32>(pf_ok, data, a, s);
      break;
    case TP_MID_DEFAULT:
    case TP_MID_SWAP64_PF:
    case TP_MID_SWAP64:  // never the prefetch
      if (n64) launch_mid_sw<4, 256>(pf_ok && shape.mid != TP_MID_SWAP64, data, a, s);
      else launch_mid_sw<8, 256>(pf_ok && shape.mid != TP_MID_SWAP64, data, a, s);
      break;
    default:  // the DPP lane kernel: lane32 32 columns, two workgroups per CU; else 64
      if (shape.mid == TP_MID_LANE32) {
        if (n64) launch_mid<32, 4, 256, 2>(data, a, s);
        else launch_mid<32, 8, 256, 2>(data, a, s);
      } else {
        if (n64) launch_mid<64, 4, 256, 1>(data, a, s);
        else launch_mid<64, 8, 256, 1>(data, a, s);
      }
  }
  return hipGetLastError();
}

// Stage 1 of a z-slab rank (cfp_dist.hip) on its [n z][nyl][n x] block: the default shape's kernel
// on the rank's nyl / N2 local k1
hipError_t tp_mid_slab(int n, cd* data, const TPArgs& a, hipStream_t s) {
  if (n == 512) {  // 2 x times 16 y2 tiles, XCD order where the rounds are whole
    const int units = 256 * ((1 << a.lnyl) / 16);  // x tiles x local k1
    const unsigned g = grid_xcd(units, 1);
    if (g) TP_LAUNCH((k_tp_mid<0, 32, 16, 512, 16, true, 512, true>), dim3(g), dim3(1024), s, data, a, units);
    else TP_LAUNCH((k_tp_mid<0, 32, 16, 512, 16, true, 512, false>), dim3(grid_of(units, 1)), dim3(1024), s, data, a,
                   units);
    return hipGetLastError();
  }
  const int units = 32 * (a.lnyl ? (1 << a.lnyl) / 8 : 32);  // x tiles x local k1
  const dim3 g(grid_of(units, 1)), blk(1024);
  if (((uintptr_t)data & 15) == 0)  // the LDS-DMA prefetch needs 16-byte addresses
    hipLaunchKernelGGL((k_tp_mid_sw<64, 8, 256, 0, true, 256, 0, kP2LoadFlags>), g, blk, 0, s, data, a, units);
  else
    hipLaunchKernelGGL((k_tp_mid_sw<64, 8, 256, 0, false, 256, 0, kP2LoadFlags>), g, blk, 0, s, data, a, units);
  return hipGetLastError();
}

// The real plan's P2 (the schedule: cfp_tp_rows_r2c.hip): stage 1 on the half spectrum H
// (n/2 x n x n), stage 3 on the Nyquist column Q [n z][n y] (its N2 columns of each k1, NX = 1)
hipError_t tp_mid_real(int stage, int n, cd* H, cd* Q, const TPArgs& a, hipStream_t s) {
  if (stage == 3) {
    if (n == 128)
      hipLaunchKernelGGL((k_tp_mid<0, 4, 4, 128, 8, false, 1>), dim3(32), dim3(4 * 16), 0, s, Q, a, 32);
    else
      hipLaunchKernelGGL((k_tp_mid<0, 8, 8, 256, 4, false, 1>), dim3(32), dim3(8 * 64), 0, s, Q, a, 32);
  } else if (n == 128) {  // x tiles of the 64-wide half spectrum (8 x times 4 y2) x k1
    constexpr int units = (64 / 8) * 32;
    hipLaunchKernelGGL((k_tp_mid<0, 32, 4, 128, 8, false, 64>), dim3(grid_of(units, 2)), dim3(512), 0, s, H, a,
                       units);
  } else {
    constexpr int units = (128 / 8) * 32;  // x tiles of the half spectrum x k1
    const unsigned gx = CFP_REAL_MID_XCD ? grid_xcd(units, 1) : 0;  // whole rounds: 512 units, 256 workgroups
    if (gx)
      hipLaunchKernelGGL((k_tp_mid_sw<64, 8, 256, 0, true, 128, 0, 0, false, true>), dim3(gx), dim3(1024), 0, s, H, a,
                         units);
    else
      hipLaunchKernelGGL((k_tp_mid_sw<64, 8, 256, 0, true, 128>), dim3(grid_of(units, 1)), dim3(1024), 0, s, H, a,
                         units);
  }
  return hipGetLastError();
}

}  // namespace cfp
