// cfp_wave_real.hip -- the wave-system block-circulant apply on real data
// (include/wave_system_real.h): r2c rows | y | fused last axis | inverse y | c2r rows, on the
// half spectrum kx <= nx/2 of the interleaved field idx = cell*C + comp, C = dim + 1.
//
// Row sweeps (k_wrx): component c of a row of nx = 2M cells is the real sequence
// b[ES ((row nx + i) C + c)], read as M complex values z[j] = (v[2j], v[2j+1]); Z = FFT_M(z),
// then cfp_real.hip's even/odd merge (k_rx) with Z[M-k] from the partner lane,
//     X[k] = E[k] + W_2M^k O[k]  (k < M)  -> H[row][kx][comp]  (a wave field of the grid M x ny x nz)
//     X[M] = E[0] - O[0]                  -> Q[row][comp]      (a wave field of the grid 1 x ny x nz)
// and backwards with 2/N folded into the stores.  A workgroup owns R whole cell-rows, R C nx
// contiguous values: it moves them between global memory and LDS in address order (every load
// and store instruction of b, x and H covers one contiguous run), and the FFT threads (one
// (row, comp) column per TPC lanes of a wavefront, k_rx's shapes) take their strided points from
// LDS.  The tile, the FFT's exchange buffer and the outgoing tile share one LDS buffer.
//
// y and fused passes: the complex wave plan's own kernels (launch_axis_pass, PASS_FUSED_WAVE)
// on H with the first M entries of the x table and on Q with its single entry kx = M.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/circulant_fft.h"
#include "../../include/wave_system_real.h"
#include "cfp_fft_device.h"
#include "cfp_host.h"
#include "cfp_wave_host.h"

namespace cfp {
namespace {

// k_rx's FFT shapes per M (TPC = M / PTS divides 64) and R = cell-rows per workgroup
template <int M> struct WRCfg;
template <> struct WRCfg<16> { static constexpr int PTS = 4, R0 = 4, R = 16; };
template <> struct WRCfg<32> { static constexpr int PTS = 8, R0 = 4, R = 16; };
template <> struct WRCfg<64> { static constexpr int PTS = 8, R0 = 8, R = 8; };
template <> struct WRCfg<128> { static constexpr int PTS = 8, R0 = 2, R = 4; };
template <> struct WRCfg<256> { static constexpr int PTS = 8, R0 = 4, R = 2; };
template <> struct WRCfg<512> { static constexpr int PTS = 16, R0 = 2, R = 1; };

// C components, M = nx/2, ES doubles per value of b / x, forward (r2c) or inverse (c2r).
// al16: b / x is 16-byte aligned (uniform): 16-byte accesses of it, else 8-byte ones.
template <int C, int M, int ES, bool INV>
__global__ void __launch_bounds__(WRCfg<M>::R* C*(M / WRCfg<M>::PTS))
    k_wrx(const double* in_r, cd* H, cd* Q, double* out_r, const cd* twn, i64 rows, double scale, int al16) {
  typedef WRCfg<M> G;
  constexpr int PTS = G::PTS, R0 = G::R0, R = G::R;
  constexpr int TPC = M / PTS;
  static_assert(64 % TPC == 0, "a column's threads must sit in one wavefront");
  constexpr int TCOLS = R * C;      // (row, comp) columns of the workgroup
  constexpr int NT = TCOLS * TPC;   // threads
  constexpr int NX = 2 * M;
  constexpr int TILE = R * C * M;   // complex values (pairs of reals) of the tile
  constexpr int F = F_SPLIT_LDS;
  static_assert(Shape<M, PTS, R0>::S > 1, "the exchange barriers order the shared buffer");
  static_assert(TCOLS * (M + M / 16) <= 2 * TILE, "the FFT exchange fits the tile buffer");
  __shared__ __attribute__((aligned(16))) double stage[2 * TILE];
  __shared__ cd tws[M];  // W_M[k] = W_2M[2k]
  const int tid = threadIdx.x;
  for (int i = tid; i < M; i += NT) tws[i] = twn[2 * i];
  const int tpc = tid % TPC, col = tid / TPC;
  const int r = col / C, c = col - r * C;
  const i64 row0 = (i64)blockIdx.x * R;
  const int nlive = rows - row0 < R ? (int)(rows - row0) : R;
  const bool live = r < nlive;
  const int lane = tid & 63;
  const int pl = lane - tpc + ((TPC - tpc) & (TPC - 1));  // lane of the mirror partner
  const int nd = nlive * NX * C;                          // live reals of the tile (even)
  cd* const st2 = reinterpret_cast<cd*>(stage);
  cd* const Ht = H + row0 * M * C;
  cd v[PTS];
  if (!INV) {
    const double* src = in_r + (i64)ES * (row0 * NX * C);
    if (ES == 1 && al16) {
#pragma unroll
      for (int i = 0; i < PTS; ++i) {
        const int e = tid + i * NT;
        dv2 z;
        z.x = z.y = 0.0;
        if (2 * e < nd) z = ldv(reinterpret_cast<const cd*>(src) + e);
        stv(st2 + e, z);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2 * PTS; ++i) {
        const int e = tid + i * NT;
        double x = 0.0;
        if (e < nd) x = (ES == 2 && al16) ? ldv(reinterpret_cast<const cd*>(src) + e).x : src[ES * e];
        stage[e] = x;
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < PTS; ++t) {
      const int j = tpc + t * TPC;
      v[t] = make_cd(stage[(r * NX + 2 * j) * C + c], stage[(r * NX + 2 * j + 1) * C + c]);
    }
    // first = false: the barrier before the exchange's writes also ends the reads of the tile
    fft_stages<M, PTS, R0, true, TCOLS, F>(v, stage, tws, col, tpc, false);  // v[t] = Z[tpc + t TPC]
    cd X[PTS], xq = make_cd(0.0, 0.0);
#pragma unroll
    for (int t = 0; t < PTS; ++t) {
      const int k = tpc + t * TPC;
      const cd za = shfl_cd(v[(PTS - t) % PTS], pl), zb = shfl_cd(v[PTS - 1 - t], pl);
      const cd zm = tpc == 0 ? za : zb;  // Z[M - k]
      const cd e = make_cd(0.5 * (v[t].x + zm.x), 0.5 * (v[t].y - zm.y));
      const cd d = make_cd(v[t].x - zm.x, v[t].y + zm.y);  // Z[k] - conj Z[M-k]
      const cd o = make_cd(0.5 * d.y, -0.5 * d.x);          // d / 2i
      X[t] = cadd(e, cmul(twn[k], o));
      if (t == 0) xq = csub(e, o);
    }
    __syncthreads();  // the last exchange's reads
#pragma unroll
    for (int t = 0; t < PTS; ++t) st2[(r * M + tpc + t * TPC) * C + c] = X[t];
    if (live && tpc == 0) Q[(row0 + r) * C + c] = xq;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PTS; ++i) {
      const int e = tid + i * NT;
      if (2 * e < nd) stv(Ht + e, ldv(st2 + e));
    }
  } else {
#pragma unroll
    for (int i = 0; i < PTS; ++i) {
      const int e = tid + i * NT;
      dv2 z;
      z.x = z.y = 0.0;
      if (2 * e < nd) z = ldv(Ht + e);
      stv(st2 + e, z);
    }
    const cd xn = (live && tpc == 0) ? Q[(row0 + r) * C + c] : make_cd(0.0, 0.0);
    __syncthreads();
    cd X[PTS];
#pragma unroll
    for (int t = 0; t < PTS; ++t) X[t] = st2[(r * M + tpc + t * TPC) * C + c];
#pragma unroll
    for (int t = 0; t < PTS; ++t) {
      const int k = tpc + t * TPC;
      const cd xa = shfl_cd(X[(PTS - t) % PTS], pl), xb = shfl_cd(X[PTS - 1 - t], pl);
      const cd xm = tpc == 0 ? (t == 0 ? xn : xa) : xb;  // X[M - k]
      const cd e = make_cd(0.5 * (X[t].x + xm.x), 0.5 * (X[t].y - xm.y));
      const cd d = make_cd(0.5 * (X[t].x - xm.x), 0.5 * (X[t].y + xm.y));
      const cd o = cmul(d, cconj(twn[k]));         // (X[k] - conj X[M-k]) W^-k / 2
      const cd z = make_cd(e.x - o.y, e.y + o.x);  // E + i O
      v[t] = cconj(z);                             // inverse FFT by conjugation
    }
    fft_stages<M, PTS, R0, true, TCOLS, F>(v, stage, tws, col, tpc, false);
    __syncthreads();  // the last exchange's reads
#pragma unroll
    for (int t = 0; t < PTS; ++t) {
      const int j = tpc + t * TPC;
      stage[(r * NX + 2 * j) * C + c] = v[t].x * scale;
      stage[(r * NX + 2 * j + 1) * C + c] = -v[t].y * scale;
    }
    __syncthreads();
    double* dst = out_r + (i64)ES * (row0 * NX * C);
    if (ES == 1 && al16) {
#pragma unroll
      for (int i = 0; i < PTS; ++i) {
        const int e = tid + i * NT;
        if (2 * e < nd) stv(reinterpret_cast<cd*>(dst) + e, ldv(st2 + e));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2 * PTS; ++i) {
        const int e = tid + i * NT;
        if (e < nd) {
          if (ES == 1) {
            dst[e] = stage[e];
          } else if (al16) {
            dv2 z;
            z.x = stage[e];
            z.y = 0.0;
            stv(reinterpret_cast<cd*>(dst) + e, z);
          } else {
            dst[2 * e] = stage[e];
            dst[2 * e + 1] = 0.0;
          }
        }
      }
    }
  }
}

template <int C, int M, int ES, bool INV>
hipError_t launch_wrx_t(const double* in, cd* H, cd* Q, double* out, const cd* twn, i64 rows, double sc,
                        hipStream_t s) {
  typedef WRCfg<M> G;
  const unsigned blocks = (unsigned)((rows + G::R - 1) / G::R);
  const int al16 = (((uintptr_t)(INV ? (const void*)out : (const void*)in)) & 15) == 0;
  hipLaunchKernelGGL((k_wrx<C, M, ES, INV>), dim3(blocks), dim3(G::R * C * (M / G::PTS)), 0, s, in, H, Q, out, twn,
                     rows, sc, al16);
  return hipGetLastError();
}

template <int C, int M>
hipError_t launch_wrx_m(int es, bool inv, const double* in, cd* H, cd* Q, double* out, const cd* twn, i64 rows,
                        double sc, hipStream_t s) {
  if (es == 1)
    return inv ? launch_wrx_t<C, M, 1, true>(in, H, Q, out, twn, rows, sc, s)
               : launch_wrx_t<C, M, 1, false>(in, H, Q, out, twn, rows, sc, s);
  return inv ? launch_wrx_t<C, M, 2, true>(in, H, Q, out, twn, rows, sc, s)
             : launch_wrx_t<C, M, 2, false>(in, H, Q, out, twn, rows, sc, s);
}

hipError_t launch_wrx(int C, int M, int es, bool inv, const double* in, cd* H, cd* Q, double* out, const cd* twn,
                      i64 rows, double sc, hipStream_t s) {
#define CFP_WRX(MM)                                                                       \
  case MM:                                                                                \
    return C == 4 ? launch_wrx_m<4, MM>(es, inv, in, H, Q, out, twn, rows, sc, s)         \
                  : launch_wrx_m<3, MM>(es, inv, in, H, Q, out, twn, rows, sc, s);
  if (C != 3 && C != 4) return hipErrorInvalidValue;
  switch (M) {
    CFP_WRX(16) CFP_WRX(32) CFP_WRX(64) CFP_WRX(128) CFP_WRX(256) CFP_WRX(512)
    default: return hipErrorInvalidValue;
  }
#undef CFP_WRX
}

}  // namespace
}  // namespace cfp

using namespace cfp;

struct cfp_wave_rplan_s {
  int device = 0;
  i64 n[3] = {1, 1, 1};
  i64 M = 1;
  int dim = 3;
  int ncomp = 4;
  cd* H = nullptr;    // [ny nz][M][ncomp]
  cd* Q = nullptr;    // [ny nz][ncomp]
  TwiddleCache tw;
  cd* twa[3] = {nullptr, nullptr, nullptr};  // tw's W_nx, W_ny, W_nz
  double2* tab[3] = {nullptr, nullptr, nullptr};  // x: kx = 0 .. M (M + 1 entries); y; z
  bool has_sym = false;
  double c0 = 0.0;
  std::vector<wave_real::Step> steps;
};

namespace {

void free_wrplan(cfp_wave_rplan_s* p) {
  if (p->H) hipFree(p->H);
  if (p->Q) hipFree(p->Q);
  p->tw.clear();
  for (int a = 0; a < 3; ++a)
    if (p->tab[a]) hipFree(p->tab[a]);
  delete p;
}

// the pass over `axis` (1 or 2) of H (field 0: the grid M x ny x nz) or Q (field 1: 1 x ny x nz),
// the x table starting at kx = 0 or at kx = M
PassDesc field_pass(const cfp_wave_rplan_s* p, int field, int axis, int mode) {
  const double2* const tab[3] = {field ? p->tab[0] + p->M : p->tab[0], p->tab[1], p->tab[2]};
  return wave_field_pass(p->ncomp, field ? 1 : p->M, p->n[1], p->n[2], tab, p->c0,
                         wave_real::fused_axis(p->n[1], p->n[2]), axis, mode, 1.0);
}

int run_wave_real(cfp_wave_rplan_s* p, const double* b, double* x, int es, hipStream_t s,
                  std::vector<hipEvent_t>* ev) {
  if (!p->has_sym) return set_error(CFP_ERR_ARG_WRONGSTATE, "no symbol set (call cfp_wave_rplan_set_symbol)");
  if (es != 1 && es != 2) return set_error(CFP_ERR_ARG_OUTOFRANGE, "es must be 1 or 2 (got %d)", es);
  if (((uintptr_t)b | (uintptr_t)x) & 7) return set_error(CFP_ERR_ARG_OUTOFRANGE, "b and x must be 8-byte aligned");
  const i64 rows = p->n[1] * p->n[2];
  const double sc = 2.0 / (double)(p->n[0] * rows);
  for (size_t i = 0; i < p->steps.size(); ++i) {
    const wave_real::Step& q = p->steps[i];
    if (ev) HIPCHK(hipEventRecord((*ev)[i], s));
    hipError_t e;
    if (q.kind == wave_real::AXIS) {
      cd* f = q.field ? p->Q : p->H;
      e = launch_axis_pass(field_pass(p, q.field, q.axis, q.mode), f, f, p->twa[q.axis], s);
    } else {
      const bool inv = q.kind == wave_real::C2R;
      e = launch_wrx(p->ncomp, (int)p->M, es, inv, b, p->H, p->Q, x, p->twa[0], rows, inv ? sc : 1.0, s);
    }
    if (e != hipSuccess) return hip_error(e, q.kind == wave_real::AXIS ? "real wave plan: axis pass" : "real wave plan: row sweep");
  }
  if (ev) HIPCHK(hipEventRecord((*ev)[p->steps.size()], s));
  return CFP_SUCCESS;
}

}  // namespace

extern "C" int cfp_wave_rplan_supported(int64_t nx, int64_t ny, int64_t nz, int dim) {
  return wave_real::refusal(nx, ny, nz, dim) ? 0 : 1;
}

extern "C" int cfp_wave_rplan_create(cfp_wave_rplan_t* plan, int64_t nx, int64_t ny, int64_t nz, int dim,
                                     int device) {
  if (!plan) return set_error(CFP_ERR_ARG_NULL, "plan is NULL");
  *plan = nullptr;
  if (const char* why = wave_real::refusal(nx, ny, nz, dim))
    return set_error(CFP_ERR_SUP, why, (long long)nx, (long long)ny, (long long)nz, dim);
  CFPCHK(check_device(device));
  DeviceGuard g(device);
  cfp_wave_rplan_s* p = new cfp_wave_rplan_s;
  p->device = device;
  p->n[0] = nx;
  p->n[1] = ny;
  p->n[2] = nz;
  p->M = nx / 2;
  p->dim = dim;
  p->ncomp = dim + 1;
  p->steps = wave_real::schedule(ny, nz);
  const size_t rows = (size_t)(ny * nz);
  hipError_t e = hipMalloc(&p->H, sizeof(cd) * rows * (size_t)p->M * p->ncomp);
  if (e == hipSuccess) e = hipMalloc(&p->Q, sizeof(cd) * rows * p->ncomp);
  int rc = e == hipSuccess ? CFP_SUCCESS : hip_error(e, "real wave plan buffers");
  for (int a = 0; a < 3 && !rc; ++a) rc = p->tw.get((int)p->n[a], &p->twa[a]);
  if (rc) {
    free_wrplan(p);
    return rc;
  }
  *plan = p;
  return CFP_SUCCESS;
}

extern "C" int cfp_wave_rplan_destroy(cfp_wave_rplan_t p) {
  if (!p) return CFP_SUCCESS;
  DeviceGuard g(p->device);
  free_wrplan(p);
  return CFP_SUCCESS;
}

extern "C" int cfp_wave_rplan_set_symbol(cfp_wave_rplan_t p, const double kappa[3], double c0) {
  if (!p || !kappa) return set_error(CFP_ERR_ARG_NULL, "NULL argument");
  if (const char* why = wave::symbol_refusal(kappa, c0)) return set_error(CFP_ERR_ARG_OUTOFRANGE, "%s", why);
  DeviceGuard g(p->device);
  for (int a = 0; a < 3; ++a) {
    const std::vector<double> t =
        a == 0 ? wave_real::x_table(p->n[0], kappa[0], c0) : wave::axis_table(p->n[a], p->n[a], kappa[a], c0, true);
    static_assert(sizeof(double2) == 2 * sizeof(double), "(p, q) pairs");
    if (!p->tab[a]) HIPCHK(hipMalloc(&p->tab[a], sizeof(double) * t.size()));
    HIPCHK(hipMemcpy(p->tab[a], t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice));
  }
  p->c0 = c0;
  p->has_sym = true;
  return CFP_SUCCESS;
}

extern "C" int cfp_wave_rplan_apply_strided(cfp_wave_rplan_t p, const double* b, double* x, int es, void* stream) {
  if (!p || !b || !x) return set_error(CFP_ERR_ARG_NULL, "NULL argument");
  DeviceGuard g(p->device);
  return run_wave_real(p, b, x, es, (hipStream_t)stream, nullptr);
}

extern "C" int cfp_wave_rplan_apply(cfp_wave_rplan_t p, const double* b, double* x, void* stream) {
  return cfp_wave_rplan_apply_strided(p, b, x, 1, stream);
}

extern "C" int cfp_wave_rplan_num_passes(cfp_wave_rplan_t p, int* passes) {
  if (!p || !passes) return set_error(CFP_ERR_ARG_NULL, "NULL argument");
  *passes = (int)p->steps.size();
  return CFP_SUCCESS;
}

extern "C" int cfp_wave_rplan_time_passes(cfp_wave_rplan_t p, const double* b, double* x, int es, int iters,
                                          double* ms_out, void* stream) {
  if (!p || !b || !x || !ms_out) return set_error(CFP_ERR_ARG_NULL, "NULL argument");
  DeviceGuard g(p->device);
  return time_passes(p->steps.size(), false, iters, [&](std::vector<hipEvent_t>* ev) {
    return run_wave_real(p, b, x, es, (hipStream_t)stream, ev);
  }, ms_out);
}
