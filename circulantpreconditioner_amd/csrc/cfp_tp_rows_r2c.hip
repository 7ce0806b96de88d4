// cfp_tp_rows_r2c.hip -- the row sweeps P1r / P3r of the real-data 3-sweep apply (k_tp_rows_r2c)
// and their launcher; its P2 runs the complex kernels (tp_mid_real, cfp_tp_mid.hip).
#include "cfp_tp_device.h"
#include "cfp_tp_launch.h"

namespace cfp {

// Real-data 3-sweep (cfp_real.hip, row f4) at 256^3: the half spectrum H = M x 256 x 256
// (M = 128) takes the complex schedule's four-step split of y with the x transform replaced by
// r2c / c2r (the even/odd split of k_rx):
//   P1r k_tp_rows_r2c<false>: one z-plane's rows y2 + 8 y1 (32 real rows of 2 KiB): r2c along x
//       (128-point FFT in row mode, mirror bin from the partner lane), LDS transpose, 32-point y1
//       DFT per kx (column mode), store H in slot layout; the Nyquist bins X[128] of the unit's
//       32 rows take the same y1 DFT (one wave, a direct 32-point DFT from LDS) into Q's slots
//   P2  k_tp_mid_sw<.., NX = 128> on H (y2 + z + divide + inverse), then the Nyquist column's
//       y2 + z + divide + inverse on Q (k_tp_mid on 8 columns of one k1: 32 small workgroups)
//   P3r k_tp_rows_r2c<true>: y1 inverse (H in column mode, Q by one wave from LDS), transpose,
//       c2r merge with Q, inverse 128-point FFT, x 2/N
// P1r/P3r move 8 N + 8 N bytes, P2 16 N: 32 N per apply against ~80 N for r2c + 3 half-spectrum
// passes + c2r.  (Folding the Nyquist column into P2 as a 17th x tile was measured slower: 544
// units on 256 CUs take a third round, P2 70 -> 89 us.  Until r04 the column took its own
// 3-launch y / z plan between P2 and P3r: 18.4 us of the 199 us apply.)
// 8 points per thread (512 threads): the even/odd split needs every point and its mirror live
// at once, which at 16 points per thread spills.
// At 128^3 (r03, AUTO there too): M = 64, y = y2 + 4 y1 (N1 = 32, N2 = 4), 256 threads; P2 is
// the lane-DFT k_tp_mid on the 64-wide half spectrum (NX = 64).
// MF: policy of the accesses to b (P1r loads) and x (P3r stores), which nothing in the apply
// reads again (the complex P1 / P3 policy, kP1Flags / kP3Flags); H and Q stay plain.
// OCC: waves per SIMD asked of the compiler (4: two 512-thread workgroups per CU; 6: three)
// WC: whole-complex LDS exchanges (ds_*_b128, one barrier pair per exchange instead of two;
// 70 KiB at M = 128, two workgroups per CU) instead of real / imaginary halves
// WL: wave-local FFT exchanges.  A row's TPC threads are consecutive lanes of one wave, and in
// column mode a wave takes 16 whole columns (lane = 16 ty + column) instead of 64 columns of one
// ty: the row FFT's and the y1 DFT's exchanges (3 of the unit's 5; 12 of its 18 barriers with
// split exchanges) then wait for the wave's own LDS accesses only; the two transposes keep their
// workgroup barriers.  Column-mode LDS rows are M + 16 doubles apart (the four ty rows of a
// wave's store then fall on different bank halves).
template <bool INV, int M = 128, int N1 = 32, int N2 = 8, int NY = 256, int MF = 0, int OCC = 4, bool WC = false,
          bool WL = false>
__global__ void __launch_bounds__(N1 * (M / 8)) __attribute__((amdgpu_waves_per_eu(OCC)))
k_tp_rows_r2c(const double* in_r, cd* H, cd* Q, double* out_r, TPArgs a, int nunits) {
  constexpr int PTS = 8;
  constexpr int TPC = M / PTS;  // threads per row (row mode)
  constexpr int TY = N1 / PTS;  // 4 threads per column (column mode)
  constexpr int NT = N1 * TPC;
  constexpr int RS = M + M / 16;
  constexpr int TC = WL ? M + 16 : M;  // column-mode row stride of the y1 DFT's exchange
  static_assert(!WL || (64 % TPC == 0 && TY * 16 == 64 && M % 16 == 0), "wave-local: whole rows and 16 columns per wave");
  constexpr int F = (WC ? 0 : F_SPLIT_LDS) | F_LDS_SYNC;
  constexpr int FW = F | (WL ? F_WAVE_LDS : 0);  // the row FFT's and the y1 DFT's exchanges
  constexpr int LDS_D = (N1 * RS > N1 * TC ? N1 * RS : N1 * TC) * (WC ? 2 : 1);
  __shared__ __attribute__((aligned(16))) double lds[LDS_D];  // row layout; the column layout (N1 x TC) fits
  cd* const lc = reinterpret_cast<cd*>(lds);
  __shared__ cd tw_m[M];   // W_M (row FFT)
  __shared__ cd tw_1[N1];  // W_N1 (y1 DFT)
  __shared__ cd qy[N1];    // the unit's Nyquist bins over y1 (P1r: before its y1 DFT; P3r: after)
  const int tid = threadIdx.x;
  for (int i = tid; i < M; i += NT) tw_m[i] = a.tw[2 * i];
  for (int i = tid; i < N1; i += NT) tw_1[i] = a.tw[(2 * M / N1) * i];
  if constexpr (WL) __syncthreads();  // no workgroup barrier precedes the first wave-local FFT's twiddle reads
  const int r0 = tid / TPC, tpc0 = tid % TPC;  // row mode: row r (= y1), thread tpc
  // column mode: column kx, thread ty
  const int x0 = WL ? (tid >> 6) * 16 + (tid & 15) : tid % M, ty0 = WL ? (tid >> 4) & 3 : tid / M;
  // row mode (row r, Z[k], k = tpc + TPC t) -> column mode (column kx, rows ty + TY m), with the
  // r2c even/odd split done on the way: each thread also reads its mirror bin Z[M - kx] of the
  // same rows from the transpose buffer (no cross-lane shuffles)
  const auto to_columns_r2c = [&](cd* v, int z, int y2) {
    const int r = idx(r0), tpc = idx(tpc0), x = idx(x0), ty = idx(ty0);
    const int xm = (M - x) & (M - 1);
    cd zm[PTS];
    if constexpr (WC) {
      lds_barrier();
#pragma unroll
      for (int t = 0; t < PTS; ++t) {
        const int k = tpc + TPC * t;
        lc[r * RS + k + (k >> 4)] = v[t];
      }
      lds_barrier();
#pragma unroll
      for (int m = 0; m < PTS; ++m) {
        const int row = (ty + TY * m) * RS;
        v[m] = lc[row + x + (x >> 4)];
        zm[m] = lc[row + xm + (xm >> 4)];
      }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        lds_barrier();
#pragma unroll
        for (int t = 0; t < PTS; ++t) {
          const int k = tpc + TPC * t;
          lds[r * RS + k + (k >> 4)] = h ? v[t].y : v[t].x;
        }
        lds_barrier();
#pragma unroll
        for (int m = 0; m < PTS; ++m) {
          const int row = (ty + TY * m) * RS;
          const double d = lds[row + x + (x >> 4)], dm = lds[row + xm + (xm >> 4)];
          if (h) { v[m].y = d; zm[m].y = dm; } else { v[m].x = d; zm[m].x = dm; }
        }
      }
    }
    lds_barrier();
    const cd w = a.tw[x];  // W_2M^kx
#pragma unroll
    for (int m = 0; m < PTS; ++m) {
      const cd e = make_cd(0.5 * (v[m].x + zm[m].x), 0.5 * (v[m].y - zm[m].y));
      const cd d = make_cd(v[m].x - zm[m].x, v[m].y + zm[m].y);  // Z[k] - conj Z[M-k]
      const cd o = make_cd(0.5 * d.y, -0.5 * d.x);                // d / 2i
      v[m] = cadd(e, cmul(w, o));
      if (x == 0) qy[ty + TY * m] = csub(e, o);  // Nyquist bin X[M] of row y1 = ty + TY m
    }
  };
  // column mode (column kx, rows y1 = ty + TY m, conjugated) -> row mode with the c2r merge: each
  // thread reads X[k] and its mirror X[M - k] of its row (X[M] = the Nyquist bin from Q)
  const auto to_rows_c2r = [&](cd* v, int z, int y2) {
    const int r = idx(r0), tpc = idx(tpc0), x = idx(x0), ty = idx(ty0);
    cd xm[PTS];
    if constexpr (WC) {
      lds_barrier();
#pragma unroll
      for (int m = 0; m < PTS; ++m) lc[(ty + TY * m) * RS + x + (x >> 4)] = cconj(v[m]);
      lds_barrier();
#pragma unroll
      for (int t = 0; t < PTS; ++t) {
        const int k = tpc + TPC * t, km = (M - k) & (M - 1);
        v[t] = lc[r * RS + k + (k >> 4)];
        xm[t] = lc[r * RS + km + (km >> 4)];
      }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        lds_barrier();
#pragma unroll
        for (int m = 0; m < PTS; ++m) lds[(ty + TY * m) * RS + x + (x >> 4)] = h ? -v[m].y : v[m].x;
        lds_barrier();
#pragma unroll
        for (int t = 0; t < PTS; ++t) {
          const int k = tpc + TPC * t, km = (M - k) & (M - 1);
          const double d = lds[r * RS + k + (k >> 4)], dm = lds[r * RS + km + (km >> 4)];
          if (h) { v[t].y = d; xm[t].y = dm; } else { v[t].x = d; xm[t].x = dm; }
        }
      }
    }
    lds_barrier();
    if (tpc == 0) xm[0] = qy[r];  // k = 0: the mirror is the Nyquist bin (row r's y1 inverse, from LDS)
#pragma unroll
    for (int t = 0; t < PTS; ++t) {
      const int k = tpc + TPC * t;
      const cd e = make_cd(0.5 * (v[t].x + xm[t].x), 0.5 * (v[t].y - xm[t].y));
      const cd d = make_cd(0.5 * (v[t].x - xm[t].x), 0.5 * (v[t].y + xm[t].y));
      const cd o = cmul(d, cconj(a.tw[k]));               // (X[k] - conj X[M-k]) W^-k / 2
      v[t] = cconj(make_cd(e.x - o.y, e.y + o.x));        // E + i O, conjugated: inverse by conjugation
    }
  };
  for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
    const int z = u / N2, y2 = u % N2;
    cd v[PTS];
    if constexpr (!INV) {
      {
        const int r = idx(r0), tpc = idx(tpc0);
        const cd* src = reinterpret_cast<const cd*>(in_r) + ((i64)z * NY + y2 + N2 * r) * M + tpc;
#pragma unroll
        for (int t = 0; t < PTS; ++t) v[t] = gload<MF>(src + TPC * t);
        __builtin_amdgcn_sched_barrier(0);  // all loads out before the first butterfly
        fft_stages<M, PTS, r0_of(M, PTS), true, N1, FW>(v, lds, tw_m, r, tpc, true);  // 128 = 2 x 8 x 8; v[t] = Z[tpc + TPC t]
      }
      to_columns_r2c(v, z, y2);
      {
        const int x = idx(x0), ty = idx(ty0);
        fft_stages<N1, PTS, r0_of(N1, PTS), false, TC, FW>(v, lds, tw_1, x, ty, true);  // 32 = 4 x 8; v[m]: k1 = ty + TY m
        cd* dst = H + ((i64)z * NY + y2 + N2 * ty) * M + x;
#pragma unroll
        for (int m = 0; m < PTS; ++m) dst[(i64)N2 * TY * M * m] = v[m];
      }
      if constexpr (WL) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // qy: written by this wave's x = 0 lanes
      if (tid < N1) {  // the Nyquist column's y1 DFT (qy is visible: fft_stages held barriers; with WL
                       // the x = 0 lanes that wrote it are lanes 0, 16, 32, 48 of this same wave)
        const int k = idx(tid);
        cd acc = make_cd(0.0, 0.0);
#pragma unroll 8
        for (int j = 0; j < N1; ++j) acc = cadd(acc, cmul(qy[j], tw_1[(j * k) & (N1 - 1)]));
        Q[(i64)z * NY + y2 + N2 * k] = acc;  // slot layout, k1 = k
      }
    } else {
      cd qk = make_cd(0.0, 0.0);  // the Nyquist column, k1 = tid (first wave), from the middle launch
      if (tid < N1) qk = Q[(i64)z * NY + y2 + N2 * idx(tid)];
      {
        const int x = idx(x0), ty = idx(ty0);
        const cd* src = H + ((i64)z * NY + y2 + N2 * ty) * M + x;
#pragma unroll
        for (int m = 0; m < PTS; ++m) v[m] = src[(i64)N2 * TY * M * m];
        __builtin_amdgcn_sched_barrier(0);  // all loads out before the first butterfly (measured neutral here)
#pragma unroll
        for (int m = 0; m < PTS; ++m) v[m] = cconj(v[m]);
        fft_stages<N1, PTS, r0_of(N1, PTS), false, TC, FW>(v, lds, tw_1, x, ty, true);  // v[m]: y1 = ty + TY m
      }
      if (tid < 64) {  // one wave: the Nyquist column's y1 inverse into qy (read by to_rows_c2r)
        if (tid < N1) qy[tid] = qk;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS writes before its reads
        cd acc = make_cd(0.0, 0.0);
        const int y1 = idx(tid) & (N1 - 1);
#pragma unroll 8
        for (int k = 0; k < N1; ++k) acc = cadd(acc, cmul(qy[k], cconj(tw_1[(y1 * k) & (N1 - 1)])));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane has read qy before it is overwritten
        if (tid < N1) qy[tid] = acc;
      }
      to_rows_c2r(v, z, y2);
      {
        const int r = idx(r0), tpc = idx(tpc0);
        fft_stages<M, PTS, r0_of(M, PTS), true, N1, FW>(v, lds, tw_m, r, tpc, true);
        const double sc = a.scale;
        cd* dst = reinterpret_cast<cd*>(out_r) + ((i64)z * NY + y2 + N2 * r) * M + tpc;
#pragma unroll
        for (int t = 0; t < PTS; ++t) gstore<MF>(dst + TPC * t, make_cd(v[t].x * sc, -v[t].y * sc));
      }
    }
    lds_barrier();  // the next unit's first exchange overwrites LDS
  }
}

// The real plan's stage 0 / 2 (cfp_tp_launch.h); alt_rows (CFP_RSCHEDULE_THREE_ALT, A/B): the row
// FFT's and y1 DFT's exchanges on workgroup barriers instead of wave-local (WL)
hipError_t tp_rows_real(int stage, int n, const double* b, cd* H, cd* Q, double* x, const TPArgs& a, hipStream_t s,
                        bool alt_rows) {
  if (n == 128) {
    constexpr int units = 128 * 4;  // z-planes x y2
    const unsigned g = grid_of(units, 4);
    // wave-local FFT exchanges (WL) by default since r04ab
    if (stage == 0 && alt_rows)
      hipLaunchKernelGGL((k_tp_rows_r2c<false, 64, 32, 4, 128>), dim3(g), dim3(256), 0, s, b, H, Q, nullptr, a,
                         units);
    else if (stage == 0)
      hipLaunchKernelGGL((k_tp_rows_r2c<false, 64, 32, 4, 128, 0, 4, false, true>), dim3(g), dim3(256), 0, s, b, H,
                         Q, nullptr, a, units);
    else if (alt_rows)
      hipLaunchKernelGGL((k_tp_rows_r2c<true, 64, 32, 4, 128>), dim3(g), dim3(256), 0, s, nullptr, H, Q, x, a,
                         units);
    else
      hipLaunchKernelGGL((k_tp_rows_r2c<true, 64, 32, 4, 128, 0, 4, false, true>), dim3(g), dim3(256), 0, s, nullptr,
                         H, Q, x, a, units);
    return hipGetLastError();
  }
  constexpr int units = 256 * 8;  // z-planes x y2
  const unsigned g = grid_of(units, 2);
  // WL (r04aa): 5,720 against 5,343 real PCApply/s, P1r 64 -> ~57 us
  // blockIdx order (r05l: XCD order 5,641-5,704 against 5,699-5,701 real PCApply/s)
  if (stage == 0 && !alt_rows)  // P1r: 80 VGPRs, three workgroups per CU
    hipLaunchKernelGGL((k_tp_rows_r2c<false, 128, 32, 8, 256, F_NT_LD, 6, false, true>), dim3(grid_of(units, 3)),
                       dim3(512), 0, s, b, H, Q, nullptr, a, units);
  else if (stage == 0)
    hipLaunchKernelGGL((k_tp_rows_r2c<false, 128, 32, 8, 256, F_NT_LD, 6>), dim3(grid_of(units, 3)), dim3(512), 0, s, b,
                       H, Q, nullptr, a, units);
  else if (!alt_rows)
    hipLaunchKernelGGL((k_tp_rows_r2c<true, 128, 32, 8, 256, F_NT_ST, 4, true, true>), dim3(g), dim3(512), 0, s,
                       nullptr, H, Q, x, a, units);
  else
    hipLaunchKernelGGL((k_tp_rows_r2c<true, 128, 32, 8, 256, F_NT_ST, 4, true>), dim3(g), dim3(512), 0, s, nullptr, H, Q, x, a,
                       units);
  return hipGetLastError();
}

}  // namespace cfp
