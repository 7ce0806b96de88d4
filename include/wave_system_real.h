/*
 * wave_system_real.h -- the wave system's block-circulant apply on real data (r2c / half
 * spectrum / c2r) and its PCSHELL, in both scalar builds.
 *
 * The wave system's data are real: a real operator and a real right-hand side keep every Krylov
 * vector real.  The block symbol of include/wave_system.h is Hermitian, S(-k) = conj S(k),
 * because the matrices A^-(+-e_d) are real; so the half spectrum kx <= nx/2 carries everything.
 * The plan below transforms a real row of nx = 2M cells per component as M complex pairs (the
 * scalar real plan's trick, include/circulant_fft_real.h), runs the complex wave plan's y and
 * fused passes on the half-spectrum field H (an interleaved wave field of the grid M x ny x nz)
 * and on the Nyquist field Q (kx = M, the grid 1 x ny x nz), and transforms back: five sweeps
 * over half the data.  Bytes per cell and apply, C = dim + 1: 80 C (es = 1), 96 C (es = 2),
 * against 160 C of the complex plan's five passes.
 *
 * Everything in this header is compiled into libcirculant_fft.so (PetscScalar complex) and into
 * libcirculant_fft_real.so (PetscScalar = double).
 */
#ifndef CFP_WAVE_SYSTEM_REAL_H
#define CFP_WAVE_SYSTEM_REAL_H

#include <stdint.h>

#include "petsc_mini.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the real-data block-circulant plan (C ABI, device pointers; no PETSc types) */
typedef struct cfp_wave_rplan_s *cfp_wave_rplan_t;
/* 1 where cfp_wave_rplan_create serves the grid, else 0 (host arithmetic only, no HIP call):
 *   dim = 3, or dim = 2 with nz = 1 (dim = 1 is refused: the solve would sit inside the row kernel);
 *   nx even with nx/2 a power of two in [16, 512] (the scalar real plan's row lengths);
 *   1 <= ny, nz <= 4096, at least one of them > 1, and the last axis with n > 1 (the fused pass:
 *   DFT, block solve, inverse DFT of a whole column in one workgroup's LDS) at most 1024 long,
 *   the complex wave plan's own limit. */
int cfp_wave_rplan_supported(int64_t nx, int64_t ny, int64_t nz, int dim);
/* CFP_ERR_SUP with a message (cfp_last_error) on every grid cfp_wave_rplan_supported refuses */
int cfp_wave_rplan_create(cfp_wave_rplan_t *plan, int64_t nx, int64_t ny, int64_t nz, int dim, int device);
int cfp_wave_rplan_destroy(cfp_wave_rplan_t plan);
/* kappa[d] = dt / h_d, c0 = sound speed (as cfp_wave_plan_set_symbol); required before an apply
 * (CFP_ERR_ARG_WRONGSTATE otherwise) */
int cfp_wave_rplan_set_symbol(cfp_wave_rplan_t plan, const double kappa[3], double c0);
/* x = S^-1 b, b and x: (dim+1) nx ny nz doubles, idx = cell (dim+1) + comp; x may alias b; 8-byte
 * alignment is enough.  The plan owns its half-spectrum buffers: nothing is allocated per apply. */
int cfp_wave_rplan_apply(cfp_wave_rplan_t plan, const double *b, double *x, void *stream);
/* the same on the real parts of complex arrays: es = 2 reads value i at b[2 i] (the imaginary
 * parts are ignored) and writes x[2 i] and x[2 i + 1] = 0; es = 1 is cfp_wave_rplan_apply */
int cfp_wave_rplan_apply_strided(cfp_wave_rplan_t plan, const double *b, double *x, int es, void *stream);
/* the launches of an apply's schedule: r2c rows | y pass of H, of Q (3-D) | fused pass of H, of Q |
 * inverse y pass of H, of Q (3-D) | c2r rows */
int cfp_wave_rplan_num_passes(cfp_wave_rplan_t plan, int *passes);
/* mean device milliseconds of each of those launches over `iters` applies (events between them) */
int cfp_wave_rplan_time_passes(cfp_wave_rplan_t plan, const double *b, double *x, int es, int iters, double *ms_out,
                               void *stream);

/* ---- PCSHELL on the real-data plan (registration as applyFFT3DPrecWave: PCShellSetContext(pc,
 * &ctx), SetSetUp / SetApply / SetDestroy).  FFTPrecWaveContext's members in its order; `plan` is
 * a cfp_wave_rplan_t.
 *
 * Real-scalar library: b and x are the (dim+1) N real rows.
 * Complex library: b and x are complex Vecs whose data the caller promises to be real: the
 * callback reads the real parts only and writes a zero imaginary part (es = 2).  Inside GMRES on
 * the real wave operator with a real right-hand side (and a real initial guess) that is exact:
 * A, b and S^-1 are real, so every residual, every Krylov vector and every iterate is real, and
 * the preconditioner never sees a non-zero imaginary part to drop.
 *
 * One rank only: with PETSC_COMM_WORLD of several ranks setup returns PETSC_ERR_SUP, as it does
 * (with the plan's message) on a grid cfp_wave_rplan_supported refuses.  The shell offers no fused
 * dots: the KSP runs its own sweeps. */
struct FFTPrecWaveRealContext {
  PetscInt n_x, n_y, n_z;
  PetscReal kappa_x, kappa_y, kappa_z; /* dt / h_d */
  PetscReal c0;
  cfp_wave_rplan_t plan; /* created by setup, destroyed by destroy */
  PetscInt dim;          /* 2 or 3; 0 = 3 */
};
typedef struct FFTPrecWaveRealContext FFTPrecWaveRealContext;
PetscErrorCode setupFFTPrec3DWaveRealData(PC pc);
PetscErrorCode applyFFT3DPrecWaveRealData(PC pc, Vec b, Vec x);
PetscErrorCode destroyFFTPrec3DWaveRealData(PC pc);

#ifdef __cplusplus
}
#endif
#endif /* CFP_WAVE_SYSTEM_REAL_H */
