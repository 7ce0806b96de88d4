// transport_cartesian.cpp -- implicit upwind transport operator on a Cartesian grid and the
// GMRES time loop of the reference's transport driver, with the circulant FFT PCSHELL wired
// into the KSP.
//
//   cfp_transport_csr                  computeDivergenceMatrix, src/TransportEquation.cxx:75-133
//   initial_conditions_shock_cartesian initial_conditions_shock, src/TransportEquation.cxx:25-73
//   TransportEquationGMRES             TransportEquation_impl_mpi,
//                                      tests/TransportEquation_SphericalExplosion_impl_mpi.cxx:13-189,
//                                      plus the PCSHELL registration ToDo.md:1 asks for
//
// The operator is assembled on the host once (a 7-point CSR), handed to the stand-in AIJ
// (device SpMV), shifted by 1 (MatShift(A,1), :117) and solved with KSPGMRES each step.
#ifndef CFP_WITH_PETSC
#include <sys/time.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/circulant_fft.h"
#include "../../include/pcshell_fft3d.h"
#include "../../include/transport_equation.h"
#include "cartesian_driver.h"

using cfp_driver::wall;

// One row per cell; the six faces of cell (i,j,k) in the order -x,+x,-y,+y,-z,+z with outward
// normals; un = n . a.  Interior face: un > 0 adds dt |F|/|C| un to the diagonal (:109-110);
// otherwise the neighbour column gets -dt |F|/|C| un (reference sign, :111-112) or
// +dt |F|/|C| un (fixed sign).  Border faces add nothing (Neumann, :114-129).
// rows [r0, r1) of the operator: rowptr[c - r0], global columns
static int transport_csr_rows(int64_t nx, int64_t ny, int64_t nz, const double h[3], double dt, const double a[3],
                              int sign_mode, double shift, int64_t r0, int64_t r1, int64_t* rowptr, int64_t* col,
                              double* val, int64_t* nnz) {
  if (!h || !a || !rowptr || !col || !val || !nnz) return CFP_ERR_ARG_NULL;
  if (nx < 1 || ny < 1 || nz < 1 || h[0] <= 0 || h[1] <= 0 || h[2] <= 0) return CFP_ERR_ARG_OUTOFRANGE;
  if (sign_mode != CFP_UPWIND_REFERENCE && sign_mode != CFP_UPWIND_FIXED) return CFP_ERR_ARG_OUTOFRANGE;
  if (r0 < 0 || r1 < r0 || r1 > nx * ny * nz) return CFP_ERR_ARG_OUTOFRANGE;
  const int64_t n[3] = {nx, ny, nz};
  const int64_t stride[3] = {1, nx, nx * ny};
  const double sgn = sign_mode == CFP_UPWIND_REFERENCE ? -1.0 : 1.0;
  int64_t p = 0;
  rowptr[0] = 0;
  for (int64_t c = r0; c < r1; ++c) {
        const int64_t i = c % nx, j = (c / nx) % ny, k = c / (nx * ny);
        const int64_t idx[3] = {i, j, k};
        double diag = shift;
        double off[6] = {0, 0, 0, 0, 0, 0};  // neighbour coefficients: -x,+x,-y,+y,-z,+z
        bool has[6] = {false, false, false, false, false, false};
        for (int d = 0; d < 3; ++d) {
          const double coef = dt / h[d];  // dt |F| / |C|
          for (int s = 0; s < 2; ++s) {   // s = 0: face -d (normal -e_d), s = 1: face +d
            const bool border = s == 0 ? idx[d] == 0 : idx[d] == n[d] - 1;
            if (border) continue;
            const double un = s == 0 ? -a[d] : a[d];
            if (un > 0) {
              diag += coef * un;
            } else {
              off[2 * d + s] += sgn * coef * un;
              has[2 * d + s] = true;
            }
          }
        }
        // ascending columns: -z, -y, -x, diag, +x, +y, +z
        const int order[6] = {4, 2, 0, 1, 3, 5};
        for (int q = 0; q < 3; ++q) {
          const int f = order[q];
          if (has[f] && off[f] != 0.0) {
            col[p] = c - stride[f / 2];
            val[2 * p] = off[f];
            val[2 * p + 1] = 0.0;
            ++p;
          }
        }
        col[p] = c;
        val[2 * p] = diag;
        val[2 * p + 1] = 0.0;
        ++p;
        for (int q = 3; q < 6; ++q) {
          const int f = order[q];
          if (has[f] && off[f] != 0.0) {
            col[p] = c + stride[f / 2];
            val[2 * p] = off[f];
            val[2 * p + 1] = 0.0;
            ++p;
          }
        }
        rowptr[c - r0 + 1] = p;
  }
  *nnz = p;
  return CFP_SUCCESS;
}

extern "C" int cfp_transport_csr(int64_t nx, int64_t ny, int64_t nz, const double h[3], double dt, const double a[3],
                                 int sign_mode, double shift, int64_t* rowptr, int64_t* col, double* val,
                                 int64_t* nnz) {
  return transport_csr_rows(nx, ny, nz, h, dt, a, sign_mode, shift, 0, nx * ny * nz, rowptr, col, val, nnz);
}

extern "C" double cfp_cartesian_min_ratio_vol_surf(int dim, const double h[3]) {
  if (dim <= 1) return h[0] / 2.0;
  if (dim == 2) return h[0] * h[1] / (2.0 * (h[0] + h[1]));
  return h[0] * h[1] * h[2] / (2.0 * (h[0] * h[1] + h[1] * h[2] + h[2] * h[0]));
}

extern "C" PetscErrorCode computeDivergenceMatrixCartesian(PetscInt nx, PetscInt ny, PetscInt nz, const PetscReal h[3],
                                                           PetscReal dt, const PetscReal a[3], PetscInt sign_mode,
                                                           Mat* A) {
  PetscFunctionBeginUser;
  PetscCheck(A && h && a, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "computeDivergenceMatrixCartesian: NULL argument");
  PetscCheck(nx >= 1 && ny >= 1 && nz >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "grid sizes must be >= 1");
  const int64_t N = nx * ny * nz;
  std::vector<int64_t> rowptr((size_t)N + 1), col((size_t)(7 * N));
  std::vector<PetscScalar> val((size_t)(7 * N));
  int64_t nnz = 0;
  const int rc = cfp_transport_csr(nx, ny, nz, h, dt, a, (int)sign_mode, 0.0, rowptr.data(), col.data(),
                                   reinterpret_cast<double*>(val.data()), &nnz);
  PetscCheck(rc == CFP_SUCCESS, PETSC_COMM_SELF, rc, "computeDivergenceMatrixCartesian: bad arguments");
  PetscCall(MatCreateSeqAIJWithArrays(PETSC_COMM_SELF, N, N, rowptr.data(), col.data(), val.data(), A));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// computeDivergenceMatrix on a communicator (the reference's MatCreateAIJ on PETSC_COMM_WORLD,
// tests/TransportEquation_SphericalExplosion_impl_mpi.cxx:82-84): every rank sets its own rows
// (PETSC_DECIDE blocks = whole z-planes when the size divides n_z) and assembles
extern "C" PetscErrorCode computeDivergenceMatrixCartesianAIJ(MPI_Comm comm, PetscInt nx, PetscInt ny, PetscInt nz,
                                                              const PetscReal h[3], PetscReal dt, const PetscReal a[3],
                                                              PetscInt sign_mode, Mat* A) {
  PetscFunctionBeginUser;
  PetscCheck(A && h && a, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "computeDivergenceMatrixCartesianAIJ: NULL argument");
  PetscCheck(nx >= 1 && ny >= 1 && nz >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "grid sizes must be >= 1");
  const auto rows = [&](int64_t lo, int64_t hi, int64_t* rowptr, int64_t* col, double* val,
                        int64_t* nnz) -> PetscErrorCode {
    const int rc = transport_csr_rows(nx, ny, nz, h, dt, a, (int)sign_mode, 0.0, lo, hi, rowptr, col, val, nnz);
    PetscCheck(rc == CFP_SUCCESS, PETSC_COMM_SELF, rc, "computeDivergenceMatrixCartesianAIJ: bad arguments");
    return PETSC_SUCCESS;
  };
  PetscCall(cfp_driver::aij_from_rows(comm, nx * ny * nz, rows, A));
  PetscFunctionReturn(PETSC_SUCCESS);
}

extern "C" PetscErrorCode initial_conditions_shock_cartesian(PetscInt nx, PetscInt ny, PetscInt nz,
                                                             const PetscReal xmin[3], const PetscReal xmax[3], Vec U) {
  PetscFunctionBeginUser;
  PetscCall(cfp_driver::shock_initial_conditions(nx, ny, nz, xmin, xmax, U));
  PetscFunctionReturn(PETSC_SUCCESS);
}

extern "C" void cfp_transport_config_default(cfp_transport_config* cfg, int64_t n) {
  if (!cfg) return;
  std::memset((void*)cfg, 0, sizeof(*cfg));
  cfg->nx = cfg->ny = cfg->nz = n;
  for (int d = 0; d < 3; ++d) {
    cfg->xmin[d] = -0.5;
    cfg->xmax[d] = 0.5;
  }
  cfg->a[0] = 1.0;
  cfg->cfl = 1.0e3 / 3.0;
  cfg->tmax = 0.05;
  cfg->ntmax = 2000000;
  cfg->precision = 1e-5;
  cfg->max_its = 1000;
  cfg->restart = 30;
  cfg->pc = CFP_TRANSPORT_PC_FFT;
  cfg->sign_mode = CFP_UPWIND_REFERENCE;
  cfg->lambda_mode = CFP_LAMBDA_MATCHED;
  cfg->pc_side = PC_LEFT;
  cfg->on_device = 1;
  cfg->fuse = 1;
  cfg->profile = 0;
}

// TransportEquation_impl_mpi (one rank): the time loop of implicit upwind steps
// (I + dt A) U^{n+1} = U^n solved by GMRES, KSPSolve(ksp, Un, Un) as at :136.
extern "C" PetscErrorCode TransportEquationGMRES(const cfp_transport_config* cfg, cfp_transport_result* res,
                                                 double* U_out) {
  PetscFunctionBeginUser;
  PetscCheck(cfg && res, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "TransportEquationGMRES: NULL argument");
  PetscCheck(cfg->pc == CFP_TRANSPORT_PC_NONE || cfg->on_device, PETSC_COMM_SELF, PETSC_ERR_SUP,
             "the FFT preconditioner runs on HIP vectors only");
  std::memset((void*)res, 0, sizeof(*res));
  const double t_setup = wall();
  const PetscInt nx = cfg->nx, ny = cfg->ny, nz = cfg->nz, N = nx * ny * nz;
  const int dim = nz > 1 ? 3 : (ny > 1 ? 2 : 1);
  double h[3];
  cfp_driver::grid_spacing(cfg, h);
  const double anorm = std::sqrt(cfg->a[0] * cfg->a[0] + cfg->a[1] * cfg->a[1] + cfg->a[2] * cfg->a[2]);
  PetscCheck(anorm > 0, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "transport velocity is zero");
  const double dt = cfg->cfl * cfp_cartesian_min_ratio_vol_surf(dim, h) / anorm;  // :54
  res->dt = dt;

  // one rank: sequential Vecs and AIJ; several (PETSC_COMM_WORLD of PetscMiniSetCommWorld): the
  // reference's VecCreateMPI / MatCreateAIJ on PETSC_COMM_WORLD with PETSC_DECIDE rows (:59-84)
  int P = 1;
  PetscCallMPI(MPI_Comm_size(PETSC_COMM_WORLD, &P));
  Vec Un, dUn;
  PetscCall(cfp_driver::create_state(cfg, P, &Un, &dUn));
  PetscInt lo, nloc;
  PetscCall(VecGetOwnershipRange(Un, &lo, NULL));
  PetscCall(VecGetLocalSize(Un, &nloc));
  res->rstart = lo;
  res->nlocal = nloc;

  Mat A;
  if (P > 1) PetscCall(computeDivergenceMatrixCartesianAIJ(PETSC_COMM_WORLD, nx, ny, nz, h, dt, cfg->a, cfg->sign_mode, &A));
  else PetscCall(computeDivergenceMatrixCartesian(nx, ny, nz, h, dt, cfg->a, cfg->sign_mode, &A));
  PetscCall(MatShift(A, 1.0));  // :117

  KSP ksp;
  PC pc;
  PetscCall(cfp_driver::gmres_create(cfg, cfg->fuse ? PETSC_TRUE : PETSC_FALSE, &ksp, &pc));
  FFTPrecTransportContext ctx;
  std::memset((void*)&ctx, 0, sizeof(ctx));
  if (cfg->pc == CFP_TRANSPORT_PC_FFT) {
    // the wiring ToDo.md:1 asks for: context factory, then the three PCSHELL callbacks
    PetscCall(getFFTPrec3DContext(3, dt, N, cfg->a[0], cfg->a[1], cfg->a[2], cfg->xmin[0], cfg->xmin[1],
                                  cfg->xmin[2], cfg->xmax[0], cfg->xmax[1], cfg->xmax[2], &ctx));
    // the factory assumes a cube (n = cbrt(nbCells)); a box grid keeps its own sizes
    ctx.n_x = nx;
    ctx.n_y = ny;
    ctx.n_z = nz;
    const bool up = cfg->lambda_mode == CFP_LAMBDA_UPWIND;
    if (cfg->lambda_mode == CFP_LAMBDA_MATCHED || up) {
      ctx.lambda_x = cfg->a[0] * dt / h[0];
      ctx.lambda_y = cfg->a[1] * dt / h[1];
      ctx.lambda_z = cfg->a[2] * dt / h[2];
    }
    PetscCall(PCSetType(pc, PCSHELL));
    PetscCall(PCShellSetContext(pc, &ctx));
    PetscCall(PCShellSetSetUp(pc, up ? setupFFTPrec3DUpwind : setupFFTPrec3D));
    PetscCall(PCShellSetApply(pc, applyFFT3DPrecTransport));
    if (cfg->fuse) PetscCall(PCShellSetApplyBA(pc, applyFFT3DPrecTransportBA));
    PetscCall(PCShellSetDestroy(pc, destroyFFTPrec3D));
    PetscCall(PCShellSetName(pc, "circulant FFT (HIP)"));
    res->lambda[0] = ctx.lambda_x.real();
    res->lambda[1] = ctx.lambda_y.real();
    res->lambda[2] = ctx.lambda_z.real();
  } else {
    PetscCall(PCSetType(pc, PCNONE));
  }
  PetscCall(cfp_driver::gmres_setup(ksp, A, Un, dUn, cfg->on_device, t_setup, res));

  PetscCall(cfp_driver::gmres_time_loop(ksp, Un, dUn, dt, cfg, res));  // :131-170
  PetscCall(cfp_driver::copy_out(Un, nloc, U_out));
  PetscCall(KSPDestroy(&ksp));  // destroys the PC, whose destroy callback frees setup's objects
  PetscCall(MatDestroy(&A));
  PetscCall(VecDestroy(&Un));
  PetscCall(VecDestroy(&dUn));
  PetscFunctionReturn(PETSC_SUCCESS);
}
// TransportEquationFFT_impl_mpi, tests/TransportEquationFFT_SphericalExplosion_impl_mpi.cxx:20-150:
// the direct-solver loop.  The FFT matrix is made once (:97-99) and reused every step (the
// reference's Fft3DSolver destroys it after the first step, App. A item 6; here it survives).
extern "C" PetscErrorCode TransportEquationFFTDirect(const cfp_transport_config* cfg, cfp_transport_result* res,
                                                     double* U_out) {
  PetscFunctionBeginUser;
  PetscCheck(cfg && res, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "TransportEquationFFTDirect: NULL argument");
  std::memset((void*)res, 0, sizeof(*res));
  const double t_setup = wall();
  const PetscInt nx = cfg->nx, ny = cfg->ny, nz = cfg->nz, N = nx * ny * nz;
  PetscCheck(nx >= 1 && ny >= 1 && nz >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "grid sizes must be >= 1");
  const int dim = nz > 1 ? 3 : (ny > 1 ? 2 : 1);
  double h[3];
  cfp_driver::grid_spacing(cfg, h);
  // the velocity has dim components in the reference (Vector(getSpaceDimension())): the others are 0
  const double a[3] = {cfg->a[0], dim > 1 ? cfg->a[1] : 0.0, dim > 2 ? cfg->a[2] : 0.0};
  const double anorm = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  PetscCheck(anorm > 0, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "transport velocity is zero");
  const double dt = cfg->cfl * cfp_cartesian_min_ratio_vol_surf(dim, h) / anorm;  // :44-45
  res->dt = dt;
  for (int d = 0; d < 3; ++d) res->lambda[d] = a[d] * dt / h[d];

  Vec Un, dUn;
  PetscCall(cfp_driver::create_state(cfg, 1, &Un, &dUn));

  Mat FFT_MAT;
  const PetscInt dims[3] = {nz, ny, nx};
  PetscCall(MatCreateFFT(PETSC_COMM_WORLD, 3, dims, MATFFTW, &FFT_MAT));  // :97-99
  struct StructuredTransportContext ctx = {nx, ny, nz, a[0], a[1], a[2], dt, h[0], h[1], h[2], FFT_MAT};  // :100
  res->setup_seconds = wall() - t_setup;

  const auto solve = [&](Vec U) { return PetscFft3DTransportSolver(ctx, U, U); };
  PetscCall(cfp_driver::direct_time_loop(Un, dUn, dt, cfg, solve, res));
  PetscCall(cfp_driver::copy_out(Un, N, U_out));
  PetscCall(MatDestroy(&FFT_MAT));
  PetscCall(VecDestroy(&Un));
  PetscCall(VecDestroy(&dUn));
  PetscFunctionReturn(PETSC_SUCCESS);
}
#endif  // CFP_WITH_PETSC
