/*
 * diffusion_equation.h -- the implicit advection-diffusion step: the circulant FFT PCSHELL of its
 * symbol, the direct solver, the Cartesian operator and the GMRES time loop.
 *
 * The reference's to-do list asks for this operator next (ToDo.md: "ajouter l'equation de
 * diffusion pour tester la versatilite de la structure ... creer une structure
 * StructuredDiffusionContext et une structure FFTPrecDiffusionContext"); the names and the
 * argument order follow its transport interface (include/pcshell_fft3d.h,
 * include/transport_equation.h).
 *
 * One implicit step solves (I + dt L) U^{n+1} = U^n with
 *   L u = a . grad u - nu lap u,  upwind for the advection (the conservative sign,
 *   CFP_UPWIND_FIXED) and the centred 7-point stencil for the diffusion.
 * On a periodic grid I + dt L is the circulant with the symbol
 *   Diag[k] = 1 + sum_d [ lambda_d (1 - w_d) + mu_d (2 - w_d - conj(w_d)) ],  w_d = e^{-2 pi i k_d/n_d},
 *   lambda_d = a_d dt / h_d,  mu_d = nu dt / h_d^2   (cfp_plan_set_symbol_advdiff),
 * exactly for a_d >= 0 (the advection part couples a cell to its neighbour at index - 1, as the
 * transport symbol does).  For a velocity with a negative component the operator couples that axis
 * to index + 1 and its symbol is the upwind one (cfp_plan_set_symbol_upwind, circulant_fft.h):
 * setupFFTPrec3DDiffusionUpwind below sets it, for either sign of every a_d.  Registration by the
 * caller:
 *   PCSetType(pc, PCSHELL); PCShellSetContext(pc, &ctx);
 *   PCShellSetSetUp(pc, setupFFTPrec3DDiffusion); PCShellSetApply(pc, applyFFT3DPrecDiffusion);
 *   PCShellSetDestroy(pc, destroyFFTPrec3DDiffusion);
 * On PETSC_COMM_WORLD of P ranks (P | n_z) the FFT matrix is this rank's z slab
 * (include/circulant_fft_dist.h), every Vec holds the rank's z-planes and Diag is the rank's
 * planes of the symbol, as with the transport PCSHELL; a split with P not dividing n_z returns
 * PETSC_ERR_ARG_SIZ.
 *
 * Both scalar builds export every name below.  With real scalars (-DCFP_REAL_SCALAR,
 * libcirculant_fft_real.so) Vecs and U_out hold doubles, Diag and b_hat are the r2c half spectrum
 * [nz][ny][nx/2 + 1] (include/pcshell_fft3d.h), and the symbol is set on the real-data plan
 * (cfp_rplan_set_symbol_advdiff, include/circulant_fft_real.h) as well as on the complex plan that
 * serves the grids the real plan lacks and an explicit Diag.  On several ranks the real build
 * promotes to the complex slab plan, as its transport apply does, and Diag is the rank's planes
 * [nzl][ny][nx/2 + 1] of the half spectrum.
 */
#ifndef CFP_DIFFUSION_EQUATION_H
#define CFP_DIFFUSION_EQUATION_H

#include <stdint.h>

#include "petsc_mini.h"
#include "circulant_fft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* FFTPrecTransportContext's 12 members in its order (include/pcshell_fft3d.h), then the
 * diffusion numbers */
struct FFTPrecDiffusionContext {
  PetscInt spaceDim;
  PetscInt n_x;
  PetscInt n_y;
  PetscInt n_z;
  PetscScalar lambda_x;
  PetscScalar lambda_y;
  PetscScalar lambda_z;
  Mat FFT_MAT;
  Mat intersectionMatrix;
  Vec Diag;
  Vec b_hat;
  Vec b_cartesien;
  PetscScalar mu_x;
  PetscScalar mu_y;
  PetscScalar mu_z;
};
typedef struct FFTPrecDiffusionContext FFTPrecDiffusionContext;

struct StructuredDiffusionContext {
  PetscInt n_x;
  PetscInt n_y;
  PetscInt n_z;
  PetscScalar a_x;
  PetscScalar a_y;
  PetscScalar a_z;
  PetscScalar nu;
  PetscScalar dt;
  PetscScalar delta_x;
  PetscScalar delta_y;
  PetscScalar delta_z;
  Mat FFT_MAT;
};

/* Fills ctx for the n_x x n_y x n_z grid on [mins, maxs] with the matched numbers
 * lambda_d = a_d dt / h_d, mu_d = nu dt / h_d^2, h_d = (maxs_d - mins_d) / n_d; axes beyond ndim
 * (1, 2 or 3) get lambda = mu = 0. */
PetscErrorCode getFFTPrec3DDiffusionContext(PetscInt ndim, PetscScalar dt, PetscInt n_x, PetscInt n_y, PetscInt n_z,
                                            PetscScalar a_x, PetscScalar a_y, PetscScalar a_z, PetscScalar nu,
                                            const PetscReal mins[3], const PetscReal maxs[3],
                                            FFTPrecDiffusionContext *ctx);

/* ---- PCSHELL callbacks.  Setup creates the FFT matrix, the work vectors and Diag (materialised
 * from the plan's closed-form symbol); the apply divides by the plan's own symbol in registers
 * while Diag is untouched, as applyFFT3DPrecTransport does. */
PetscErrorCode setupFFTPrec3DDiffusion(PC pc);
/* setupFFTPrec3DDiffusion with the upwind symbol (cfp_plan_set_symbol_upwind): lambda_d of either
 * sign.  Diag is that symbol; apply and destroy are the callbacks below.  One rank or several. */
PetscErrorCode setupFFTPrec3DDiffusionUpwind(PC pc);
PetscErrorCode applyFFT3DPrecDiffusion(PC pc, Vec b, Vec x);
PetscErrorCode destroyFFTPrec3DDiffusion(PC pc);

/* ---- direct solver: x = (I + dt L_periodic)^{-1} b with customCtx.FFT_MAT from MatCreateFFT
 * (on PETSC_COMM_WORLD of several ranks: the slab-backed matrix, b and x the rank's z-planes); b
 * may be x.  The symbol is set once per (lambda, mu) and kept between calls. */
PetscErrorCode PetscFft3DDiffusionSolver(struct StructuredDiffusionContext customCtx, Vec b, Vec x);

/* ---- the operator */
enum { CFP_BC_WALL = 0, CFP_BC_PERIODIC = 1 };
/* Host-only CSR of  shift * I + dt L  on an nx*ny*nz Cartesian grid: upwind advection with the
 * conservative sign (un > 0 adds dt un / h to the diagonal, un < 0 adds dt un / h to the
 * neighbour's column) plus nu dt / h^2 (2, -1, -1) per axis.  CFP_BC_WALL: border faces are
 * skipped, as cfp_transport_csr does; CFP_BC_PERIODIC: they reach the cell across the grid (an
 * axis of one cell contributes nothing), and the operator is the circulant of the symbol above.
 * Every row stores its diagonal, columns ascend in each row, entries that are exactly zero are
 * not stored.  rowptr has n+1 entries, col/val room for 7n (val: interleaved re,im doubles).
 * Returns 0, CFP_ERR_ARG_NULL or CFP_ERR_ARG_OUTOFRANGE. */
int cfp_advdiff_csr(int64_t nx, int64_t ny, int64_t nz, const double h[3], double dt, const double a[3], double nu,
                    int bc, double shift, int64_t *rowptr, int64_t *col, double *val, int64_t *nnz);
/* dt L into a new AIJ matrix on comm (MatCreateAIJ with PETSC_DECIDE rows, each rank setting its
 * own rows; no MatShift) */
PetscErrorCode computeAdvectionDiffusionMatrixCartesianAIJ(MPI_Comm comm, PetscInt nx, PetscInt ny, PetscInt nz,
                                                           const PetscReal h[3], PetscReal dt, const PetscReal a[3],
                                                           PetscReal nu, PetscInt bc, Mat *A);

/* ---- the implicit time loop with GMRES */
/* FFT_UPWIND: the PCSHELL with setupFFTPrec3DDiffusionUpwind (the operator's symbol for a velocity
 * of either sign); FFT keeps setupFFTPrec3DDiffusion */
enum { CFP_ADVDIFF_PC_NONE = 0, CFP_ADVDIFF_PC_FFT = 1, CFP_ADVDIFF_PC_FFT_UPWIND = 2 };

typedef struct {
  int64_t nx, ny, nz;
  double xmin[3], xmax[3];
  double a[3];        /* advection velocity */
  double nu;          /* diffusivity */
  double dt;          /* time step */
  double tmax;
  int64_t ntmax;      /* time steps cap */
  double precision;   /* rtol = abstol = precision, stationarity threshold */
  int64_t max_its;    /* KSP max iterations */
  int64_t restart;    /* GMRES restart */
  int pc;             /* CFP_ADVDIFF_PC_* */
  int bc;             /* CFP_BC_* */
  int pc_side;        /* PC_LEFT (0) / PC_RIGHT (1) */
  int on_device;      /* 1: HIP Vecs, 0: host Vecs (PCNONE only) */
  int profile;        /* 1: device time of the loop's kernels by kind (res->dev_ms) */
} cfp_advdiff_config;

typedef struct {
  int64_t steps;
  double dt, time;
  int64_t total_its;      /* sum of KSP iterations over the steps */
  int64_t max_step_its;
  int64_t min_step_its;
  int last_reason;        /* KSPConvergedReason of the last solve */
  int all_converged;      /* every solve ended with reason 2 or 3 */
  double last_residual;
  double last_norm_dU;
  double solve_seconds;   /* wall time inside KSPSolve, summed */
  double pc_seconds;      /* host wall time inside PCApply, summed */
  int64_t pc_calls;
  double setup_seconds;   /* assembly + PC setup */
  double lambda[3], mu[3];
  double loop_seconds;
  double dev_ms[4];       /* cfg->profile: as cfp_transport_result */
  int64_t dev_launches[4];
  int64_t fused_dots, fused_norms;  /* 0: the 7-point stencil is not x-local, nothing is fused */
  int64_t rstart, nlocal; /* this rank's rows of the field [rstart, rstart + nlocal) (one rank: all) */
} cfp_advdiff_result;

/* [-0.5, 0.5]^3, n^3 cells, a = (1, 0, 0), nu = 0.01, dt = 0.01, one step, precision 1e-8, 1000
 * iterations, restart 30, the FFT PCSHELL, walls, left preconditioning, HIP Vecs */
void cfp_advdiff_config_default(cfp_advdiff_config *cfg, int64_t n);
/* The loop: U^0 = initial_conditions_shock_cartesian, then while steps < ntmax, time <= tmax and
 * ||U^{n+1} - U^n|| >= precision one KSPSolve of (I + dt L) U^{n+1} = U^n with the stand-in
 * GMRES and PCNONE or the diffusion PCSHELL (MatMult, PCApply and the dots as separate sweeps:
 * the 7-point stencil is not x-local, so there is no fused step).  U_out (optional): the final
 * field, N PetscScalars (interleaved (re, im) values; N doubles in the real-scalar build).  On
 * PETSC_COMM_WORLD of several ranks (PetscMiniSetCommWorld) the Vecs and the AIJ are distributed in
 * PETSC_DECIDE rows, as TransportEquationGMRES's: U_out then holds this rank's res->nlocal rows
 * from res->rstart on. */
PetscErrorCode AdvectionDiffusionGMRES(const cfp_advdiff_config *cfg, cfp_advdiff_result *res, double *U_out);
/* The direct-solver loop: each step is one PetscFft3DDiffusionSolver(ctx, Un, Un), i.e. the
 * periodic operator whatever cfg->bc says.  res: steps, dt, time, last_norm_dU, solve_seconds,
 * pc_calls, lambda, mu, rstart, nlocal (several ranks: as AdvectionDiffusionGMRES, needs P | nz). */
PetscErrorCode AdvectionDiffusionFFTDirect(const cfp_advdiff_config *cfg, cfp_advdiff_result *res, double *U_out);

#ifdef __cplusplus
}
#endif
#endif /* CFP_DIFFUSION_EQUATION_H */
