// cfp_three_pass.hip -- the 3-sweep apply for 256^3 grids (PCApply in 96 N bytes instead of
// the 5-pass schedule's 160 N).
//
// The y transform is split four-step (Cooley-Tukey, ny = N1 * N2, N1 = 64 or 32): with
// y = y2 + N2 y1 and k = k1 + N1 k2,
//   X[k1 + N1 k2] = sum_{y2} W_N2^{y2 k2} W_256^{y2 k1} sum_{y1} W_N1^{y1 k1} x[y2 + N2 y1].
// The inner N1-point DFT rides with the x transform, the outer N2-point DFT with the z
// transform, and every intermediate stays in the slot it was read from (y1 <-> k1, y2 <-> k2):
//
//   P1  k_tp_rows<fwd>: one z-plane, rows y2 + N2 y1 (N1 rows, N1 x 4 KB): N1-point DFT down
//       the rows (column mode, lanes = x), LDS transpose, 256-point DFT along each row
//   P2  k_tp_mid_sw (default) / k_tp_mid: T/N2 x-columns x N2 rows y2 + N2 k1 x 256 z: twiddle
//       W_256^{y2 k1}, N2-point DFT across lanes (k_tp_mid_sw: radix-2 stages on permlane
//       register transposes; k_tp_mid: DPP lane permutations; frequencies left bit-reversed),
//       256-point z DFT, divide by the separable symbol at (kx, k1 + N1 k2, kz), then the same
//       transforms on the conjugate (inverse)
//       (k_tp_mid_rec, 256^3 default shape, a transport symbol with |a| <= 1 - 2^-13: the same
//       array and the same 8 rows x 128 B accesses (lane = x + 8 y2) without the z transforms:
//       y2 DFT across lane bits 3..5, z solved as the recurrence u_z = a u_{z-1} + w_z in the
//       registers of the lane that owns the column, one carry per wave)
//       (k_tp_mid_rec2, the same for an advection-diffusion symbol with mu_z != 0 and both z
//       ratios <= 1 - 2^-7: a forward and a backward recurrence, two carries per wave)
//       (k_tp_mid_recb, k_tp_mid_rec on the planes in reverse order: the upwind transport symbol
//       with lambda_z < 0, the recurrence u_z = a u_{z+1} + w_z)
//   P3  k_tp_rows<inv>: P1 on the conjugate, x 1/N
//
// P1/P3 workgroups are N1 x 16 threads x 16 points with a split-LDS exchange buffer of
// N1 x 2.1 KB: one per CU at N1 = 64, two at N1 = 32.  P2 holds T columns (T = 64: one
// 1024-thread workgroup per CU; T = 32: two of 512); its global runs are T/N2 x 16 bytes.
//
// This unit holds the row sweeps P1 / P3 (k_tp_rows) and every launcher that instantiates them: one
// GPU, z-slab ranks, the fused Krylov step.  P2: cfp_tp_mid.hip (FFT), cfp_tp_rec.hip (z by
// recurrence); the real plan's rows: cfp_tp_rows_r2c.hip; the dispatch: cfp_tp_dispatch.hip.
//
#include "cfp_tp_device.h"
#include "cfp_tp_launch.h"

namespace cfp {

// Persistent: a workgroup walks units blockIdx.x, + gridDim.x, ...  Prefetching the next unit
// into VGPRs across LDS-only barriers was tried and lost: at 1024 threads the extra registers
// spill (profiles/r01_schedule_sweep.txt); at 128^3 with 8 points per thread it fits (104
// VGPRs) and still lost, P1 20.7 -> 23.3 us with one workgroup per CU walking two units
// (profiles/r03m_128_three_sweep.md).  PTS points per thread (16 or 8); XS = the LDS exchanges
// split into real and imaginary halves (half the footprint, twice the barriers).
//
// LP (lane pair, N1 = 2 PTS): the two threads of a column x are lanes L and L + 32 of one wave
// (x = lane % 32 + 32 wave), so phase A's 32-point DFT is a 16-point DFT per lane (even / odd
// y1), the twiddle W_32^k on the odd lane, and a radix-2 across lane bit 5 on permlane32 swaps:
// no LDS exchange and no barrier pair in phase A.  Slot m then holds k1 = m % 8 + 8 ty + 16 (m / 8).
//
// BLK (blocked intermediate layout, r04): the N2 rows y2 + N2 k1 of one k1 (contiguous in every
// layout) hold [x / BLK][y2][x % BLK] instead of [y2][x], so a P2 unit of BLK x times N2 y2
// columns is one run of N2 BLK 16 bytes per z (1 KiB at BLK = 8); P1's stores and P3's loads
// become BLK x 16 B runs instead.  Only the intermediate between the sweeps changes; b and x
// stay natural.  BLK = 0: natural.  At 512^3 (N2 = 16) blocks of BLK = 2 x: 32-byte pieces for
// P1 / P3, 512-byte runs for P2's 2 x times 16 y2 tile.
// XCD: units in xcd_unit order (the host launches whole rounds), so the N2 units of one z-plane,
// whose blocked pieces share 128-byte lines, run under one L2.
//
// FUSE (r06, the stand-in GMRES's Krylov step; one GPU, natural layout): P1 (!INV) with FUSE = 1
// loads y = A b, A an x-row-local stencil (TPArgs pre_*): the neighbours b[i -+ 1] of a point are
// the same rows' lines, so the extra loads hit the caches and the sweep still reads b once from
// HBM.  P3 (INV) with FUSE = NP > 0 accumulates post_v[j]^H x over its stored points (j <
// a.post_nv <= NP; a NULL vector is x itself) across all its units and writes one partial per
// workgroup and value: the VecMDot that follows a PCApply in classical Gram-Schmidt, without the
// separate sweep that re-reads x.
//
// PF = NPF > 0 (the one-GPU 256^3 sweeps: N1 = 32, lane pairs, wave-local phase C, natural layout,
// whole rounds, `in` 16-byte aligned): slots 0 .. NPF-1 of the workgroup's next unit come by
// LDS-DMA (global_load_lds_dwordx4, lane-linear) into the issuing wave's own four rows of the
// exchange buffer, which only that wave touches from the last transpose barrier to the next
// unit's transpose.  The DMA goes out behind the unit's last arithmetic and in front of its
// stores (one burst); the next unit loads slots NPF .. 15 from global memory, waits once for
// everything and reads its own 16 bytes per slot back.  The barrier that closed the unit moves in
// front of the transpose's first write, behind every wave's read of its prefetched slots: the
// same number of barriers.  A workgroup's last unit prefetches nothing.
namespace rows {
// A unit's loads in the natural one-GPU layout.  A point's address = a wave-uniform base (unit
// u = (z, y2), the wave's 32 columns, slot m: rows 16 m further) + this lane's 32-bit byte offset
// (x % 32, ty): a scalar base plus one offset register for all 16 slots (as rec::Tile, cfp_tp_rec.hip)
struct Tile {
  static constexpr int TN = 256, N2 = 8;
  const cd* in;
  int wv;
  double* pf_l;  // this wave's rows of the exchange buffer
  // the lane's column x (its low 5 bits: the lane's place in the wave's 32 columns) and its ty
  static __device__ __forceinline__ unsigned lane_off(int x, int ty) {
    return 16u * ((unsigned)(x & 31) + (unsigned)(TN * N2) * (unsigned)ty);
  }
  static __device__ __forceinline__ const cd* at(const cd* base, unsigned off) {
    return reinterpret_cast<const cd*>(reinterpret_cast<const char*>(base) + off);
  }
  __device__ __forceinline__ const cd* slot_ptr(int u, int m) const {
    // (an opaque scalar per slot: with the slot stride visible as a compile-time constant the
    // lane's offset is added first and the 16 addresses become 64-bit vector additions)
    i64 e = (i64)(u / N2) * TN * TN + (u % N2) * TN + 32 * wv + 2 * TN * N2 * m;
    asm volatile("" : "+s"(e));
    return in + e;
  }
  // this wave's slots 0 .. NPF-1 of unit u -> LDS, lane-linear
  template <int NPF, int LD>
  __device__ __forceinline__ void prefetch(int u, unsigned loff) const {
    asm volatile("" : "+s"(u), "+v"(loff));
#pragma unroll
    for (int m = 0; m < NPF; ++m)
      __builtin_amdgcn_global_load_lds((glb_void_t*)at(slot_ptr(u, m), loff), (lds_void_t*)(pf_l + m * 128), 16, 0,
                                       (LD & (F_NT | F_NT_LD)) ? 2 : 0);
  }
  // slot m < NPF, which the prefetch brought
  __device__ __forceinline__ cd prefetched(int m, int lane) const {
    return fromv(*reinterpret_cast<const dv2*>(pf_l + m * 128 + 2 * lane));
  }
  template <int LD>
  __device__ __forceinline__ cd load(int u, int m, unsigned loff) const {
    return gload<LD>(at(slot_ptr(u, m), loff));
  }
};
}  // namespace rows

template <bool INV, int FLAGS, int N1, int TN, int PTS = 16, bool XS = true, bool LP = false, int BLK = 0,
          bool XCD = false, int PROBE = 0, int FUSE = 0, int NPF = 0>
__global__ void __launch_bounds__(N1 * (TN / PTS)) __attribute__((amdgpu_waves_per_eu(4)))
k_tp_rows(const cd* in, cd* out, TPArgs a, int nunits) {
#ifndef CFP_KEXP
  static_assert(PROBE == 0, "timing probes are built in tools/kexp only");
#endif
  constexpr bool PF = NPF > 0;
  static_assert(!PF || (N1 == 32 && TN == 256 && PTS == 16 && XS && LP && BLK == 0 && FUSE == 0 &&
                        (FLAGS & F_WAVE_LDS) != 0 && NPF <= 8),
                "prefetch: the one-GPU 256^3 sweeps, at most 8 slots in the wave's own rows");
  constexpr int N2 = TN / N1, TR = TN / PTS, NT = N1 * TR, TY = N1 / PTS;
  constexpr bool PRE = !INV && FUSE == 1, POST = INV && FUSE > 0;
  constexpr int NP = POST ? FUSE : 1;
  static_assert(!POST || NP <= TP_POST_MAX, "post dots: at most TP_POST_MAX vectors");
  static_assert(FUSE == 0 || (BLK == 0 && PROBE == 0), "fused work: natural layout, product kernels");
  constexpr bool BL = BLK > 0;
  constexpr int BX = BL ? BLK : 1, BW = N2 * BX;  // x per block column, values per block column
  static_assert(!LP || (TY == 2 && TN % 32 == 0), "lane pairs: two threads per column, 32 columns per wave");
  static_assert(!BL || (TR % BX == 0 && ((N2 == 8 && (BX == 4 || BX == 8)) || (N2 == 16 && (BX == 2 || BX == 8)))),
                "blocked layout: 4 or 8 x times 8 y2, or 2 or 8 x times 16 y2");
  constexpr int RS = TN + TN / 16;  // padded row stride of the row-mode LDS layout
  constexpr int F = FLAGS | (XS ? F_SPLIT_LDS : 0) | F_LDS_SYNC;
  // F_WAVE_LDS in FLAGS: phase C's row-FFT exchanges wave-local (a row's TR threads are
  // consecutive lanes of one wave and its LDS row is theirs alone); phase A (columns spread over
  // waves) and the transposes keep workgroup barriers
  constexpr int FA = F & ~F_WAVE_LDS;
  static_assert(!(FLAGS & F_WAVE_LDS) || 64 % TR == 0, "wave-local rows: whole rows per wave");
  __shared__ __attribute__((aligned(16))) double lds[N1 * RS * (XS ? 1 : 2)];  // both layouts fit
  __shared__ cd tw_l[N1];  // W_N1 for phase A; phase C reads W_256 from global memory (L2 hits),
                           // which keeps it out of scratch (20 B/lane with the table in LDS)
  // PRE: the stencil's classes as dense 3-slot rows (x - 1, x, x + 1) and their slot masks
  __shared__ cd pre_tab_l[PRE ? 3 * TP_PRE_MAX_CLS : 1];
  __shared__ unsigned pre_mk_l[PRE ? TP_PRE_MAX_CLS + 1 : 1];  // [ncls]: slot masks, [MAX]: their union
  __shared__ const unsigned char* pre_cls_l[1];
  __shared__ cd pre_edge_l[PRE ? NT : 1];  // PRE: per wave, the edge neighbours its lanes loaded
  // POST: per wave and value, the running sum of its lanes' dot contributions
  __shared__ double post_l[POST ? 2 * NP * (NT / 64) : 1];
  __shared__ const cd* post_ptr_l[POST ? NP : 1];
  __shared__ int post_n_l[2];  // post_nv, post_self
  const int tid = threadIdx.x;
  if constexpr (POST) {
    for (int i = tid; i < 2 * NP * (NT / 64); i += NT) post_l[i] = 0.0;
    if (tid < NP) post_ptr_l[tid] = a.post_v[tid];
    if (tid == 0) {
      post_n_l[0] = a.post_nv;
      post_n_l[1] = a.post_self;
    }
  }
  for (int i = tid; i < N1; i += NT) tw_l[i] = a.tw[N2 * i];
  if constexpr (PRE) {
    for (int c = tid; c < a.pre_ncls; c += NT) {
      const unsigned mk = a.pre_mask[c];
      unsigned dense = 0;
      pre_tab_l[3 * c] = pre_tab_l[3 * c + 1] = pre_tab_l[3 * c + 2] = make_cd(0.0, 0.0);
      for (int k = 0; k < a.pre_nd; ++k)
        if ((mk >> k) & 1u) {
          const int slot = a.pre_off[k] + 1;
          pre_tab_l[3 * c + slot] = a.pre_tab[c * a.pre_nd + k];
          dense |= 1u << slot;
        }
      pre_mk_l[c] = dense;
    }
    if (tid == 0) {
      unsigned all = 0;
      for (int k = 0; k < a.pre_nd; ++k) all |= 1u << (a.pre_off[k] + 1);
      pre_mk_l[TP_PRE_MAX_CLS] = all | (a.pre_cls_x ? 8u : 0u);  // bit 3: classes by x alone
      pre_cls_l[0] = a.pre_cls_x ? a.pre_cls_x : a.pre_cls;
    }
  }
  if constexpr (LP || PRE || POST) __syncthreads();  // phase A reads tw_l (and the stencil) before any barrier
  // phase A: column x, thread ty of TY
  const int x0 = LP ? (tid & 31) + 32 * (tid >> 6) : tid % TN, ty0 = LP ? (tid >> 5) & 1 : tid / TN;
  const int r0 = tid / TR, tx0 = tid % TR;  // phase C: row r, thread tx of TR
  // fresh (laundered) index copies (idx) at every use, as in k_tp_mid: nothing but the points
  // stays live across an FFT
  // rows of the chunked side (P1 output, P3 input): one GPU: nyl = TN, one chunk = natural
  const int lnyl = a.lnyl ? a.lnyl : ilog2(TN);
  const int nyl = 1 << lnyl;
  const auto crow = [&](int z, int y) -> i64 {
    return (i64)(y >> lnyl) * a.chunk + ((i64)z << lnyl) * TN + (i64)(y & (nyl - 1)) * TN;
  };
  // unit u = (z, y2): rows y2 + N2 y1 of (local) plane z; thread (column x, ty) loads rows
  // y2 + N2 (ty + TY m)
  const auto load = [&](int u, cd* v) {
    const int x = idx(x0), ty = idx(ty0);
    if constexpr ((PROBE & PR_NO_LOAD) != 0) {
#pragma unroll
      for (int m = 0; m < PTS; ++m) v[m] = make_cd(x + m, ty + u);
      return;
    }
    if (INV) {  // chunked rows: per-thread part + uniform part (nyl >= N2 TY)
      const cd* const src = BL ? in + crow(u / N2, N2 * ty) + (u % N2) * BX + (x / BX) * BW + x % BX
                               : in + crow(u / N2, u % N2 + N2 * ty) + x;
#pragma unroll
      for (int m = 0; m < PTS; ++m) v[m] = gload<FLAGS>(src + crow(0, N2 * TY * m));
    } else if constexpr (PRE) {
      // y = A b on the unit's rows.  With lane pairs (LP) lanes L and L + 1 of a wave hold x and
      // x + 1 of one row for L % 32 < 31, so a point's x-neighbours come from its neighbour lanes
      // (DPP wave_shr / wave_shl).  The neighbours across a wave's 32-column edge are loaded with
      // b, one per lane -- lane (ty, j < 16) the x - 1 edge of point j, (ty, 16 + j) the x + 1
      // edge -- and handed to the edge lanes through the wave's LDS slots: one memory round trip
      // per unit, as the plain load.  A neighbour outside the row is never used (its slot is
      // absent from the row's class), so its address is clamped into the row.
      static_assert(LP, "the fused stencil relies on the lane-pair layout");
      const i64 p0 = (i64)(u / N2) * TN * TN + (i64)TN * (u % N2 + N2 * ty);  // row of point 0
      const i64 i0 = p0 + x;
      const int l32 = (int)(threadIdx.x & 31), wv = (int)(threadIdx.x >> 6);
      // the slots any class uses, and the class array, from LDS at each use (kernel-argument
      // values would sit in SGPRs across the FFTs)
      const unsigned slots = ((volatile unsigned*)pre_mk_l)[TP_PRE_MAX_CLS];
      const bool hm = (slots & 1u) != 0, hp = (slots & 4u) != 0;
      const unsigned char* const cls = ((const unsigned char* const volatile*)pre_cls_l)[0];
      // classes by x alone (bit 3): one byte per thread (its column x), else one per point.
      // Every load here is non-temporal like b's: the edge and class lines must not stay in the
      // caches in place of this sweep's output, which P2 reads next.
      const bool by_x = (slots & 8u) != 0;
      int cl[PTS];
      const int clx = by_x ? (int)gload_u8<FLAGS>(cls + x) : 0;
#pragma unroll
      for (int m = 0; m < PTS; ++m) {
        const i64 i = i0 + (i64)TN * N2 * TY * m;
        v[m] = gload<FLAGS>(in + i);
        cl[m] = by_x ? clx : (int)gload_u8<FLAGS>(cls + i);
      }
      cd edge = make_cd(0.0, 0.0);
      {
        const bool left = l32 < 16;
        int xe = left ? x - l32 - 1 : x - l32 + 32;
        xe = xe < 0 ? 0 : (xe > TN - 1 ? TN - 1 : xe);
        if ((left && hm) || (!left && hp)) edge = gload<FLAGS>(in + p0 + (i64)TN * N2 * TY * (l32 & 15) + xe);
      }
      __builtin_amdgcn_sched_barrier(0);
      cd* const el = pre_edge_l + 64 * wv;
      el[threadIdx.x & 63] = edge;
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS writes are done
      __builtin_amdgcn_wave_barrier();
      // an absent diagonal has a zero coefficient in the dense table: fma(0, b, acc) = acc, so the
      // sum is the same as k_dia_spmv's, which skips it (finite b)
      const auto coefs = [&](int c, cd* t) {
        t[0] = pre_tab_l[3 * c];
        t[1] = pre_tab_l[3 * c + 1];
        t[2] = pre_tab_l[3 * c + 2];
      };
      cd tx[3];
      if (by_x) coefs(clx, tx);
#pragma unroll
      for (int m = 0; m < PTS; ++m) {
        cd t[3];
        if (by_x) {
          t[0] = tx[0], t[1] = tx[1], t[2] = tx[2];
        } else {
          coefs(cl[m], t);
        }
        // the same fma sequence, in the same diagonal order, as k_dia_spmv: bit-identical to
        // MatMult on the row-class form
        double ax = 0.0, ay = 0.0;
        const auto acc = [&](cd q, cd b) {
          ax = fma(q.x, b.x, fma(-q.y, b.y, ax));
          ay = fma(q.x, b.y, fma(q.y, b.x, ay));
        };
        if (hm) {
          cd bm = dpp_c<DPP_WAVE_SHR1>(v[m]);
          if (l32 == 0) bm = el[32 * ty + m];
          acc(t[0], bm);
        }
        acc(t[1], v[m]);
        if (hp) {
          cd bp = dpp_c<DPP_WAVE_SHL1>(v[m]);
          if (l32 == 31) bp = el[32 * ty + 16 + m];
          acc(t[2], bp);
        }
        v[m] = make_cd(ax, ay);
      }
    } else {
      const cd* const src = in + (i64)(u / N2) * TN * TN + x + (i64)TN * (u % N2 + N2 * ty);  // + uniform
#pragma unroll
      for (int m = 0; m < PTS; ++m) v[m] = gload<FLAGS>(src + (i64)TN * N2 * TY * m);
    }
    // all loads go out before the first butterfly: with runtime strides the scheduler
    // otherwise starts the DFT after 9 of them and issues the rest a memory latency later
    // (P3 100 -> 93 us at 256^3)
    __builtin_amdgcn_sched_barrier(0);
  };
  // PF: the wave's four rows (rows 4 wv .. 4 wv + 3: its phase-C rows) take the prefetch
  const auto pf_tile = [&]() {
    const int wv = __builtin_amdgcn_readfirstlane(idx(x0) >> 5);  // x0 = lane % 32 + 32 wave
    return rows::Tile{in, wv, lds + wv * (4 * RS)};
  };
  static_assert(!PF || (NPF * 128 <= 4 * RS && (4 * RS) % 2 == 0), "the prefetch fits the wave's rows, 16-byte aligned");
  static_assert(!PF || !(PROBE & PR_ZMAJOR), "prefetch: blockIdx or XCD unit order");
  if constexpr (PF && !(PROBE & PR_NO_LOAD)) {
    if ((int)blockIdx.x < nunits)
      pf_tile().template prefetch<NPF, FLAGS>(XCD ? xcd_unit(blockIdx.x, gridDim.x) : (int)blockIdx.x,
                                              rows::Tile::lane_off(idx(x0), idx(ty0)));
  }
  for (int it = blockIdx.x; it < nunits; it += gridDim.x) {
    int u = XCD ? xcd_unit(it, gridDim.x) : it;
    if constexpr ((PROBE & PR_ZMAJOR) != 0) u = (u % (nunits / N2)) * N2 + u / (nunits / N2);
    cd v[PTS];
    if constexpr (PF && !(PROBE & PR_NO_LOAD)) {
      // slots NPF .. 15 from global memory first, then one wait for everything in flight: these
      // loads, this wave's DMA and its stores of the previous unit
      const rows::Tile tile = pf_tile();
      {
        int ul = u;
        unsigned lo = rows::Tile::lane_off(idx(x0), idx(ty0));
        asm volatile("" : "+s"(ul), "+v"(lo));  // scalar base + this register, formed here
#pragma unroll
        for (int m = NPF; m < PTS; ++m) v[m] = tile.template load<FLAGS>(ul, m, lo);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      {
        const int lane = (idx(x0) & 31) + 32 * idx(ty0);
#pragma unroll
        for (int m = 0; m < NPF; ++m) v[m] = tile.prefetched(m, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
    } else {
      load(u, v);
    }
    if (INV) {
#pragma unroll
      for (int m = 0; m < PTS; ++m) v[m] = cconj(v[m]);
    }
    const auto k1_of = [](int m, int ty) {
      return LP ? (m & (PTS / 2 - 1)) + (PTS / 2) * ty + PTS * (m / (PTS / 2)) : ty + TY * m;
    };
    if constexpr ((PROBE & PR_NO_ZMATH) != 0) {
    } else if constexpr (LP) {
      // phase A on lane pairs: E / O = the 16-point DFTs of the even / odd y1 (lanes ty = 0 / 1)
      dft_reg<PTS>(v);
      {
        const int ty = idx(ty0);
#pragma unroll
        for (int k = 1; k < PTS; ++k) v[k] = cmul(v[k], tw_l[k * ty]);  // W_32^k on the odd lane
      }
      // lane ty = 0 takes (E[k], W^k O[k]), lane ty = 1 (E[k+8], W^(k+8) O[k+8]) -> X[k], X[k+16]
#pragma unroll
      for (int k = 0; k < PTS / 2; ++k) swap_c<5>(v[k], v[k + PTS / 2]);
#pragma unroll
      for (int k = 0; k < PTS / 2; ++k) {
        const cd p = v[k], q = v[k + PTS / 2];
        v[k] = cadd(p, q);
        v[k + PTS / 2] = csub(p, q);
      }
    } else {
      // phase A: N1-point DFT over y1 for every x (column mode, TN columns x TY threads)
      const int x = idx(x0), ty = idx(ty0);
      fft_stages<N1, PTS, r0_of(N1, PTS), false, TN, FA>(v, lds, tw_l, x, ty, true);  // v[m]: k1 = ty + TY m
      lds_barrier();  // phase A's last LDS reads are done
    }
    // PF: the unit's closing barrier stands here instead: every wave has read its prefetched slots
    // (and finished the previous unit's phase C) before the transpose overwrites the rows
    if constexpr (PF) lds_barrier();
    // phase B: transpose to rows k1, thread (row r, tx) gets x = tx + TR m
    if constexpr (!(PROBE & PR_NO_XCHG)) {
      const int x = idx(x0), ty = idx(ty0), r = idx(r0), tx = idx(tx0);
      if constexpr (XS) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
          for (int m = 0; m < PTS; ++m) lds[k1_of(m, ty) * RS + x + (x >> 4)] = half ? v[m].y : v[m].x;
          lds_barrier();
#pragma unroll
          for (int m = 0; m < PTS; ++m) {
            const int xx = tx + TR * m;
            const double val = lds[r * RS + xx + (xx >> 4)];
            if (half) v[m].y = val; else v[m].x = val;
          }
          lds_barrier();
        }
      } else {
        cd* const lc = reinterpret_cast<cd*>(lds);
#pragma unroll
        for (int m = 0; m < PTS; ++m) lc[k1_of(m, ty) * RS + x + (x >> 4)] = v[m];
        lds_barrier();
#pragma unroll
        for (int m = 0; m < PTS; ++m) {
          const int xx = tx + TR * m;
          v[m] = lc[r * RS + xx + (xx >> 4)];
        }
        lds_barrier();
      }
    }
    {
      // phase C: TN-point DFT along row r (row mode, N1 rows x TR threads)
      const int r = idx(r0), tx = idx(tx0);
      if constexpr (!(PROBE & PR_NO_ZMATH))
        fft_stages<TN, PTS, r0_of(TN, PTS), true, N1, F | F_TW_GLOBAL>(v, lds, a.tw, r, tx, true);  // v[m]: kx = tx + TR m
    }
    {
      const int r = idx(r0), tx = idx(tx0);
      const double sc = a.scale, sy = INV ? -sc : sc;
      if constexpr ((PROBE & PR_NO_STORE) != 0) {
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < PTS; ++m) acc += v[m].x * sc + v[m].y * sy;
        if (acc == 1.2345e300) out[tx] = make_cd(acc, 0.0);  // keeps the work live, never true
        if constexpr (PF && !(PROBE & PR_NO_LOAD)) {
          const int nx = it + (int)gridDim.x;
          if (nx < nunits)
            pf_tile().template prefetch<NPF, FLAGS>(XCD ? xcd_unit(nx, gridDim.x) : nx, rows::Tile::lane_off(idx(x0), idx(ty0)));
        }
      } else if (BL && !INV) {  // blocked: kx = tx + TR m at (kx / BX) 64 + y2 BX + kx % BX of row block r
        cd* dst = out + crow(u / N2, N2 * r) + (u % N2) * BX + (tx / BX) * BW + tx % BX;
#pragma unroll
        for (int m = 0; m < PTS; ++m) gstore<FLAGS>(dst + TR * N2 * m, make_cd(v[m].x * sc, v[m].y * sy));
      } else {
        const i64 e0 = (INV ? (i64)(u / N2) * TN * TN + (i64)TN * (u % N2 + N2 * r) : crow(u / N2, u % N2 + N2 * r)) + tx;
        cd* dst = out + e0;
        if constexpr (PF) {
          // the next unit's prefetch goes out behind all of this unit's arithmetic and in front of
          // its stores, which leave as one burst; no global load follows it inside the unit (a
          // wait for one would wait for the DMA as well)
#pragma unroll
          for (int m = 0; m < PTS; ++m) v[m] = make_cd(v[m].x * sc, v[m].y * sy);
          // (formed here: sunk below the branch round the prefetch, the row FFT's last stage
          // would wait for its twiddle loads with the DMA in flight, and so for the DMA)
#pragma unroll
          for (int m = 0; m < PTS; ++m) asm volatile("" : "+v"(v[m].x), "+v"(v[m].y));
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (!(PROBE & PR_NO_LOAD)) {
            const int nx = it + (int)gridDim.x;  // the last unit prefetches nothing
            if (nx < nunits)
              pf_tile().template prefetch<NPF, FLAGS>(XCD ? xcd_unit(nx, gridDim.x) : nx, rows::Tile::lane_off(idx(x0), idx(ty0)));
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int m = 0; m < PTS; ++m) gstore<FLAGS>(dst + TR * m, v[m]);
        } else {
#pragma unroll
          for (int m = 0; m < PTS; ++m) {
            v[m] = make_cd(v[m].x * sc, v[m].y * sy);
            gstore<FLAGS>(dst + TR * m, v[m]);
          }
        }
        if constexpr (POST) {
          // post_v[j]^H x over the unit's stored points (the other vectors read 4 points at a
          // time), reduced over the wave and added to the wave's slot in LDS: nothing stays live
          // across the next unit's FFTs
          const int lane = tid & 63, wv = tid >> 6;
          const int pnv = ((volatile int*)post_n_l)[0], pself = ((volatile int*)post_n_l)[1];
          constexpr int QB = 4;
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            if (j < pnv) {
              double sr = 0.0, si = 0.0;
              if ((pself >> j) & 1) {
#pragma unroll
                for (int m = 0; m < PTS; ++m) sr += v[m].x * v[m].x + v[m].y * v[m].y;
              } else {
                // the vector's address from LDS at each use (a kernel-argument pointer would be
                // held in SGPRs across the FFTs, which already use all of them)
                const cd* pv = ((const cd* volatile*)post_ptr_l)[j] + e0;
#pragma unroll
                for (int m0 = 0; m0 < PTS; m0 += QB) {
                  cd q[QB];
#pragma unroll
                  for (int m = 0; m < QB; ++m) q[m] = gload<kPostLoadFlags>(pv + TR * (m0 + m));
#pragma unroll
                  for (int m = 0; m < QB; ++m) {
                    const cd w = v[m0 + m];
                    sr += q[m].x * w.x + q[m].y * w.y;
                    si += q[m].x * w.y - q[m].y * w.x;
                  }
                }
              }
              sr = wave_sum_d(sr);
              si = wave_sum_d(si);
              if (lane == 0) {
                post_l[(2 * j) * (NT / 64) + wv] += sr;
                post_l[(2 * j + 1) * (NT / 64) + wv] += si;
              }
            }
          }
        }
      }
    }
    if constexpr (!PF) lds_barrier();  // the next unit's first exchange overwrites LDS
  }
  if constexpr (POST) {
    // one partial per workgroup and value: the waves' sums in a fixed order
    __syncthreads();
    if (tid < 2 * NP) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < NT / 64; ++q) s += post_l[tid * (NT / 64) + q];
      a.post_partial[(size_t)blockIdx.x * 16 + tid] = s;
    }
  }
}

// P1F / P3F: P1's load and P3's store policy out of place (kP1Flags / kP3Flags; 0 = plain)
// WR: phase C's exchanges wave-local (F_WAVE_LDS)
template <int N1, int TN, int PER_CU, int PTS = 16, bool XS = true, bool LP = false, int BL = 0, bool XCD = false,
          int P1F = kP1Flags, int P3F = kP3Flags, bool WR = kRowsWave>
static void launch_rows(int stage, const cd* in, cd* out, const TPArgs& a, hipStream_t s) {
  constexpr int units = TN * (TN / N1);  // z-planes x y2
  constexpr int W = WR ? F_WAVE_LDS : 0;
  const unsigned g = XCD ? grid_xcd(units, PER_CU) : grid_of(units, PER_CU);
  if constexpr (XCD) {
    if (g == 0) {  // fewer than 8 workgroups: the same kernel in plain unit order
      launch_rows<N1, TN, PER_CU, PTS, XS, LP, BL, false, P1F, P3F, WR>(stage, in, out, a, s);
      return;
    }
  }
  const dim3 blk(N1 * (TN / PTS));
  if (stage == 0 && in == out)  // in place (the direct solver's Un, Un)
    TP_LAUNCH((k_tp_rows<false, kP1InPlaceFlags | W, N1, TN, PTS, XS, LP, BL, XCD>), dim3(g), blk, s, in, out, a, units);
  else if (stage == 0)
    TP_LAUNCH((k_tp_rows<false, P1F | W, N1, TN, PTS, XS, LP, BL, XCD>), dim3(g), blk, s, in, out, a, units);
  else
    TP_LAUNCH((k_tp_rows<true, P3F | W, N1, TN, PTS, XS, LP, BL, XCD>), dim3(g), blk, s, in, out, a, units);
}
// the default row sweeps, or (alt, shape TP_MID_ROWSALT) the same with the other phase-C exchanges;
// units in XCD order (kRowsXCD)
template <int N1, int TN, int PER_CU, int PTS, bool XS, bool LP, int P1F = kP1Flags, int P3F = kP3Flags,
          bool XCD = kRowsXCD>
static void launch_rows_ab(bool alt, int stage, const cd* in, cd* out, const TPArgs& a, hipStream_t s) {
  if (alt) launch_rows<N1, TN, PER_CU, PTS, XS, LP, 0, XCD, P1F, P3F, !kRowsWave>(stage, in, out, a, s);
  else launch_rows<N1, TN, PER_CU, PTS, XS, LP, 0, XCD, P1F, P3F, kRowsWave>(stage, in, out, a, s);
}

// The 256^3 default row sweeps with the next unit's prefetch (k_tp_rows<.., kRowsNPF>): 0 where
// they must not run -- the build without them, another layout than one GPU's natural one, a grid
// that does not walk whole rounds (every workgroup then has the same number of units and only
// its last one goes without a prefetch), or a source that is not 16-byte aligned (`in`: the
// pointer the DMA reads in both sweeps) -- else the grid; the caller runs the plain sweeps on 0.
static unsigned rows_pf_grid(const cd* in, const TPArgs& a) {
  if (kRowsNPF == 0 || !kRowsXCD || !kRowsWave || !kRowsLP || a.lnyl != 0) return 0;
  if (((uintptr_t)in & 15) != 0) return 0;
  return grid_xcd(256 * 8, 2);
}
static void launch_rows_pf(int stage, const cd* in, cd* out, const TPArgs& a, hipStream_t s, unsigned g) {
  if constexpr (kRowsNPF > 0) {
    constexpr int W = F_WAVE_LDS, units = 256 * 8;
    if (stage == 0 && in == out)
      TP_LAUNCH((k_tp_rows<false, kP1InPlaceFlags | W, 32, 256, 16, true, true, 0, true, 0, 0, kRowsNPF>), dim3(g),
                dim3(512), s, in, out, a, units);
    else if (stage == 0)
      TP_LAUNCH((k_tp_rows<false, kP1Flags | W, 32, 256, 16, true, true, 0, true, 0, 0, kRowsNPF>), dim3(g), dim3(512), s,
                in, out, a, units);
    else
      TP_LAUNCH((k_tp_rows<true, kP3Flags | W, 32, 256, 16, true, true, 0, true, 0, 0, kRowsNPF>), dim3(g), dim3(512), s,
                in, out, a, units);
  }
}

// Stage 0 / 2 of one GPU (cfp_tp_launch.h).  The shapes' reasons and measurements stand with
// their P2 in cfp_tp_mid.hip (tp_mid); alt: the other phase-C exchanges (shape TP_MID_ROWSALT).
hipError_t tp_rows(int stage, int n, const cd* in, cd* out, const TPArgs& a, TPShape shape, bool alt, hipStream_t s) {
  if (n == 512) {
    // 32 rows of 512 (16 points per thread, 1024 threads, split exchanges: 136 KiB, one per CU).
    // blocked: blocks of 2 x, units in XCD order, so the 16 y2 units of a plane share their lines'
    // L2; blocked32: blocks of 8 x (whole 128-byte lines); lane64: phase A through LDS (A/B)
    if (shape.mid == TP_MID_BLOCKED) launch_rows<32, 512, 1, 16, true, kRowsLP, 2, true>(stage, in, out, a, s);
    else if (shape.mid == TP_MID_BLOCKED32) launch_rows<32, 512, 1, 16, true, kRowsLP, 8>(stage, in, out, a, s);
    else if (shape.mid == TP_MID_LANE64) launch_rows<32, 512, 1>(stage, in, out, a, s);
    else launch_rows_ab<32, 512, 1, 16, true, kRowsLP>(alt, stage, in, out, a, s);  // lane-pair phase A
    return hipGetLastError();
  }
  if (n == 128) {
    // Default since r04: y split 16 x 8 -- units of 16 rows (1,024 units, 256 threads, four
    // workgroups per CU, lane-pair phase A, 13.2 against 17.0 us), in blockIdx order (r05k: XCD
    // order 21,370-21,420 against 21,630-21,700 PCApply/s; one round of units whose b and x stay
    // in the Infinity Cache).  n1 = 32 (r03m to r04): 8 points per thread and whole-complex LDS
    // exchanges, 512 threads, 69 KiB (2 per CU); lane64 keeps the round-2 kernels (16 points per
    // thread, split exchanges) for A/B.
    const int n1 = shape.n1 ? shape.n1 : (shape.mid == TP_MID_LANE64 || shape.mid == TP_MID_SWAP64 ? 32 : 16);
    if (n1 == 16) launch_rows_ab<16, 128, 4, 8, false, true, 0, 0, false>(alt, stage, in, out, a, s);
    else if (shape.mid == TP_MID_LANE64) launch_rows<32, 128, 4>(stage, in, out, a, s);
    // b and x (32 MiB each) stay in the 256 MiB Infinity Cache between applies, so P1 loads and P3
    // stores keep the default policy (shape.mid = swap64: the 256^3 NT policy, A/B)
    else if (shape.mid == TP_MID_SWAP64) launch_rows<32, 128, 2, 8, false>(stage, in, out, a, s);
    else launch_rows<32, 128, 2, 8, false, false, 0, false, 0, 0>(stage, in, out, a, s);
    return hipGetLastError();
  }
  // 256^3: N1 = 32 unless the shape asks for 64
  if (shape.mid == TP_MID_BLOCKED) {  // blocked intermediate layout (k_tp_rows<.., 8>)
    launch_rows<32, 256, 2, 16, true, kRowsLP, 8>(stage, in, out, a, s);
  } else if (shape.mid == TP_MID_SWAP32X) {
    launch_rows<32, 256, 2, 16, true, kRowsLP>(stage, in, out, a, s);
  } else if (shape.mid == TP_MID_BLOCKED32) {
    // blocks of 4 x, in XCD order: the 8 y2 units of a plane share the 128-byte lines of their
    // 64-byte pieces (r04d without it: P3 130.6 us against 90.8 natural)
    launch_rows<32, 256, 2, 16, true, kRowsLP, 4, true>(stage, in, out, a, s);
  } else if (shape.n1 == 64) {
    launch_rows<64, 256, 1>(stage, in, out, a, s);
  } else if (const unsigned gpf = alt ? 0 : rows_pf_grid(in, a)) {
    launch_rows_pf(stage, in, out, a, s, gpf);
  } else {
    launch_rows_ab<32, 256, 2, 16, true, kRowsLP>(alt, stage, in, out, a, s);
  }
  return hipGetLastError();
}

// Stage 0 / 2 of a z-slab rank (cfp_dist.hip) on its nzl local planes through the per-peer chunks:
// the default shape's sweeps, two 512-thread workgroups per CU at 256^3, one of 1024 at 512^3.
// XCD order when the rounds are whole and fill the chip (r05l, profiles/r05l_rows_xcd_ab.txt:
// 512^3 P = 8 local kernels 423-431 against 439-445 us; P = 16 in 4 pieces of 128 units: 274-276
// against 256-258 us, so not below a full round).  Not through launch_rows: no in-place P1 here,
// and the 256^3 launches are not stamped.
template <int TN>
static void launch_rows_slab(int stage, const cd* in, cd* out, const TPArgs& a, int nzl, hipStream_t s) {
  constexpr int PER_CU = TN == 512 ? 1 : 2, W = kRowsWave ? F_WAVE_LDS : 0;
  const int units = nzl * (TN / 32);  // local z-planes x y2
  const unsigned gx = kRowsXCD && units >= (int)grid_of(1 << 30, PER_CU) ? grid_xcd(units, PER_CU) : 0;
  const dim3 g(gx ? gx : grid_of(units, PER_CU)), blk(32 * (TN / 16));
  by2(stage != 0, gx != 0, [&](auto inv, auto xcd) {
    constexpr bool INV = decltype(inv)::value, XCD = decltype(xcd)::value;
    constexpr int F = (INV ? F_NT_ST : F_NT_LD) | W;
    if constexpr (TN == 512)
      TP_LAUNCH((k_tp_rows<INV, F, 32, TN, 16, true, kRowsLP, 0, XCD>), g, blk, s, in, out, a, units);
    else
      hipLaunchKernelGGL((k_tp_rows<INV, F, 32, TN, 16, true, kRowsLP, 0, XCD>), g, blk, 0, s, in, out, a, units);
  });
}

hipError_t tp_rows_slab(int stage, int n, const cd* in, cd* out, const TPArgs& a, int nzl, hipStream_t s) {
  if (n == 512) launch_rows_slab<512>(stage, in, out, a, nzl, s);
  else launch_rows_slab<256>(stage, in, out, a, nzl, s);
  return hipGetLastError();
}

// The default 256^3 row sweeps with the stand-in GMRES's Krylov work fused in (FUSE): P1 on A b,
// P3 with the dots, on the dispatch's grid g
template <bool XCD>
static void launch_rows_fused(int stage, const cd* in, cd* out, const TPArgs& a, hipStream_t s, unsigned g) {
  constexpr int W = kRowsWave ? F_WAVE_LDS : 0, units = 256 * 8;
  if (stage == 0)
    TP_LAUNCH((k_tp_rows<false, kP1Flags | W, 32, 256, 16, true, kRowsLP, 0, XCD, 0, 1>), dim3(g), dim3(512), s, in,
              out, a, units);
  else
    TP_LAUNCH((k_tp_rows<true, kP3Flags | W, 32, 256, 16, true, kRowsLP, 0, XCD, 0, TP_POST_MAX>), dim3(g), dim3(512),
              s, in, out, a, units);
}

hipError_t tp_rows_fused(int stage, const cd* in, cd* out, const TPArgs& a, hipStream_t s, unsigned g, bool xcd) {
  if (xcd) launch_rows_fused<true>(stage, in, out, a, s, g);
  else launch_rows_fused<false>(stage, in, out, a, s, g);
  return hipGetLastError();
}

}  // namespace cfp
