// cartesian_driver.h -- what the Cartesian time-loop drivers share: the transport ones
// (transport_cartesian.cpp) and the advection-diffusion ones (diffusion_cartesian.cpp).  The grid
// spacing, the state vectors with the initial condition, the KSP/GMRES set-up around the
// driver's own PCSHELL wiring, the two time loops (one KSPSolve(ksp, Un, Un) or one direct solve
// per step until ntmax steps, time > tmax or ||U^{n+1} - U^n|| < precision,
// tests/TransportEquation_SphericalExplosion_impl_mpi.cxx:131-170), the several-rank AIJ
// assembly and the copy of the result.  Config is cfp_transport_config or cfp_advdiff_config,
// Result cfp_transport_result or cfp_advdiff_result: they share these members by name.
#pragma once
#include <sys/time.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/circulant_fft.h"
#include "../../include/petsc_mini.h"

namespace cfp_driver {

inline double wall() {
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  return (double)tv.tv_sec + 1e-6 * (double)tv.tv_usec;
}

template <class Config>
void grid_spacing(const Config* cfg, double h[3]) {
  h[0] = (cfg->xmax[0] - cfg->xmin[0]) / (double)cfg->nx;
  h[1] = (cfg->xmax[1] - cfg->xmin[1]) / (double)cfg->ny;
  h[2] = (cfg->xmax[2] - cfg->xmin[2]) / (double)cfg->nz;
}

// The CSR builders write (re, im) pairs of doubles.  A complex PetscScalar is one pair; a real
// one (-DCFP_REAL_SCALAR) takes kPairScalars = 2 scalars of room per value, and pairs_to_scalars
// then keeps the real parts, in place (the operators are real: every imaginary part is 0).
constexpr size_t kPairScalars = 2 * sizeof(double) / sizeof(PetscScalar);
inline void pairs_to_scalars(PetscScalar* val, int64_t n) {
  if constexpr (kPairScalars == 2)
    for (int64_t k = 0; k < n; ++k) val[k] = val[2 * k];
}

// U = the shock initial condition on this rank's cells (initial_conditions_shock_cartesian,
// include/transport_equation.h, is this function)
inline PetscErrorCode shock_initial_conditions(PetscInt nx, PetscInt ny, PetscInt nz, const PetscReal xmin[3],
                                               const PetscReal xmax[3], Vec U) {
  PetscCheck(xmin && xmax, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "NULL domain bounds");
  PetscInt n, Ng, lo;
  PetscCall(VecGetLocalSize(U, &n));
  PetscCall(VecGetSize(U, &Ng));
  PetscCall(VecGetOwnershipRange(U, &lo, NULL));
  PetscCheck(Ng == nx * ny * nz, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ, "U size differs from nx*ny*nz");
  const double hx = (xmax[0] - xmin[0]) / (double)nx, hy = (xmax[1] - xmin[1]) / (double)ny,
               hz = (xmax[2] - xmin[2]) / (double)nz;
  const double cx = (xmin[0] + xmax[0]) / 2, cy = (xmin[1] + xmax[1]) / 2, cz = (xmin[2] + xmax[2]) / 2;
  const double rmax = 0.3;
  PetscScalar* u;
  PetscCall(VecGetArrayWrite(U, &u));
  for (PetscInt c = lo; c < lo + n; ++c) {  // this rank's cells
    const PetscInt i = c % nx, j = (c / nx) % ny, k = c / (nx * ny);
    const double x = xmin[0] + (i + 0.5) * hx, y = xmin[1] + (j + 0.5) * hy, z = xmin[2] + (k + 0.5) * hz;
    double r2 = (x - cx) * (x - cx);
    if (ny > 1) r2 += (y - cy) * (y - cy);
    if (nz > 1) r2 += (z - cz) * (z - cz);
    u[c - lo] = std::sqrt(r2) < rmax ? 650.0 : 600.0;
  }
  PetscCall(VecRestoreArrayWrite(U, &u));
  return PETSC_SUCCESS;
}

// Un and dUn with the shock initial condition in Un.  One rank (P = 1): sequential Vecs;
// several: the reference's VecCreateMPI on PETSC_COMM_WORLD with PETSC_DECIDE rows (:59-84)
template <class Config>
PetscErrorCode create_state(const Config* cfg, int P, Vec* Un, Vec* dUn) {
  const PetscInt N = cfg->nx * cfg->ny * cfg->nz;
  if (P > 1 && cfg->on_device) PetscCall(VecCreateMPIHIP(PETSC_COMM_WORLD, PETSC_DECIDE, N, Un));
  else if (P > 1) PetscCall(VecCreateMPI(PETSC_COMM_WORLD, PETSC_DECIDE, N, Un));
  else if (cfg->on_device) PetscCall(VecCreateSeqHIP(PETSC_COMM_SELF, N, Un));
  else PetscCall(VecCreateSeq(PETSC_COMM_SELF, N, Un));
  PetscCall(VecDuplicate(*Un, dUn));
  PetscCall(shock_initial_conditions(cfg->nx, cfg->ny, cfg->nz, cfg->xmin, cfg->xmax, *Un));
  return PETSC_SUCCESS;
}

// this rank's n rows of Un (all of them on one rank) -> U_out (n PetscScalars), if the caller asked for them
inline PetscErrorCode copy_out(Vec Un, PetscInt n, double* U_out) {
  if (!U_out) return PETSC_SUCCESS;
  const PetscScalar* u;
  PetscCall(VecGetArrayRead(Un, &u));
  std::memcpy(U_out, (const void*)u, sizeof(PetscScalar) * (size_t)n);
  PetscCall(VecRestoreArrayRead(Un, &u));
  return PETSC_SUCCESS;
}

// The several-rank AIJ of N rows: every rank sets its own rows [lo, hi) (PETSC_DECIDE blocks),
// which rows_fn(lo, hi, rowptr, col, val, &nnz) builds as CSR with global columns, and assembles
template <class RowsFn>
PetscErrorCode aij_from_rows(MPI_Comm comm, int64_t N, RowsFn rows_fn, Mat* A) {
  PetscCall(MatCreateAIJ(comm, PETSC_DECIDE, PETSC_DECIDE, N, N, 7, NULL, 6, NULL, A));
  PetscInt lo, hi;
  PetscCall(MatGetOwnershipRange(*A, &lo, &hi));
  const int64_t m = hi - lo;
  std::vector<int64_t> rowptr((size_t)m + 1), col((size_t)(7 * (m > 0 ? m : 1)));
  std::vector<PetscScalar> val((size_t)(7 * (m > 0 ? m : 1)) * kPairScalars);
  int64_t nnz = 0;
  PetscCall(rows_fn((int64_t)lo, (int64_t)hi, rowptr.data(), col.data(), reinterpret_cast<double*>(val.data()), &nnz));
  pairs_to_scalars(val.data(), nnz);
  for (int64_t r = 0; r < m; ++r) {
    const PetscInt row = lo + r, k = rowptr[(size_t)r + 1] - rowptr[(size_t)r];
    PetscCall(MatSetValues(*A, 1, &row, k, col.data() + rowptr[(size_t)r], val.data() + rowptr[(size_t)r], ADD_VALUES));
  }
  PetscCall(MatAssemblyBegin(*A, MAT_FINAL_ASSEMBLY));
  PetscCall(MatAssemblyEnd(*A, MAT_FINAL_ASSEMBLY));
  return PETSC_SUCCESS;
}

// GMRES with the config's tolerances, restart and side; the driver then wires its PC
template <class Config>
PetscErrorCode gmres_create(const Config* cfg, PetscBool fuse, KSP* ksp, PC* pc) {
  PetscCall(KSPCreate(PETSC_COMM_WORLD, ksp));
  PetscCall(KSPSetType(*ksp, KSPGMRES));
  PetscCall(KSPSetTolerances(*ksp, cfg->precision, cfg->precision, PETSC_DEFAULT, cfg->max_its));
  PetscCall(KSPGMRESSetRestart(*ksp, cfg->restart > 0 ? cfg->restart : 30));
  PetscCall(KSPSetPCSide(*ksp, (PCSide)cfg->pc_side));
  PetscCall(KSPMiniSetFusion(*ksp, fuse));
  PetscCall(KSPGetPC(*ksp, pc));
  return PETSC_SUCCESS;
}

// Set-up to its end (t_setup: its start).  The Krylov basis is allocated and the device copy of
// A made now, so the timed solves hold only the solver's own work (PETSc would do both inside
// the first KSPSolve)
template <class Result>
PetscErrorCode gmres_setup(KSP ksp, Mat A, Vec Un, Vec dUn, int on_device, double t_setup, Result* res) {
  PetscCall(KSPSetOperators(ksp, A, A));
  PetscCall(KSPSetUp(ksp));
  PetscCall(KSPMiniSetUpWork(ksp, Un));
  PetscCall(MatMult(A, Un, dUn));
  if (on_device)
    PetscCheck(cfp_stream_sync(nullptr) == CFP_SUCCESS, PETSC_COMM_SELF, PETSC_ERR_LIB, "stream sync failed");
  res->setup_seconds = wall() - t_setup;
  return PETSC_SUCCESS;
}

template <class Config, class Result>
PetscErrorCode gmres_time_loop(KSP ksp, Vec Un, Vec dUn, double dt, const Config* cfg, Result* res) {
  int64_t it = 0;
  double time = 0.0;
  bool stationary = false;
  res->all_converged = 1;
  res->min_step_its = -1;
  if (cfg->profile) PetscCall(PetscMiniProfileBegin(1 << 16));
  const double t_loop = wall();
  while (it < cfg->ntmax && time <= cfg->tmax && !stationary) {  // :131
    PetscCall(VecCopy(Un, dUn));
    const double v = wall();
    PetscCall(KSPSolve(ksp, Un, Un));
    const double w = wall();
    PetscCall(VecAXPY(dUn, -1.0, Un));
    time += dt;
    it += 1;
    PetscReal norm;
    PetscCall(VecNorm(dUn, NORM_2, &norm));
    stationary = norm < cfg->precision;
    KSPConvergedReason reason;
    PetscInt its;
    PetscReal residu;
    PetscCall(KSPGetConvergedReason(ksp, &reason));
    PetscCall(KSPGetIterationNumber(ksp, &its));
    PetscCall(KSPGetResidualNorm(ksp, &residu));
    PetscInt calls;
    PetscLogDouble pcs;
    PetscCall(KSPMiniGetPCApplyStats(ksp, &calls, &pcs));
    res->solve_seconds += w - v;
    res->pc_seconds += pcs;
    res->pc_calls += calls;
    res->total_its += its;
    res->max_step_its = std::max<int64_t>(res->max_step_its, its);
    res->min_step_its = res->min_step_its < 0 ? its : std::min<int64_t>(res->min_step_its, its);
    res->last_reason = (int)reason;
    res->last_residual = residu;
    res->last_norm_dU = norm;
    if (reason != KSP_CONVERGED_RTOL && reason != KSP_CONVERGED_ATOL) res->all_converged = 0;  // :166
    PetscInt fd, fn;
    PetscCall(KSPMiniGetFusedCounts(ksp, &fd, &fn));
    res->fused_dots += fd;
    res->fused_norms += fn;
  }
  res->loop_seconds = wall() - t_loop;
  if (cfg->profile) {
    PetscCall(PetscMiniProfileEnd(res->dev_ms, res->dev_launches));
    res->dev_ms[0] = 1e3 * res->pc_seconds;
    res->dev_launches[0] = res->pc_calls;
  }
  res->steps = it;
  res->time = time;
  return PETSC_SUCCESS;
}

// The direct-solver loop (tests/TransportEquationFFT_SphericalExplosion_impl_mpi.cxx:106-150):
// solve(Un) replaces Un by the step's solution
template <class Config, class Solve, class Result>
PetscErrorCode direct_time_loop(Vec Un, Vec dUn, double dt, const Config* cfg, Solve solve, Result* res) {
  int64_t it = 0;
  double time = 0.0;
  bool stationary = false;
  res->all_converged = 1;
  while (it < cfg->ntmax && time <= cfg->tmax && !stationary) {  // :106
    PetscCall(VecCopy(Un, dUn));
    // the copy above is queued on the Vec stream (PETSc's host VecCopy returns when done): drain
    // it, so that the clock brackets the solve only, as the reference's PetscTime pair (:110-112)
    PetscCall(VecMiniSynchronize(dUn));
    const double v = wall();
    PetscCall(solve(Un));  // :111
    PetscCall(VecMiniSynchronize(Un));  // a device-Vec solve is stream-ordered: time it to completion
    const double w = wall();
    PetscCall(VecAXPY(dUn, -1.0, Un));
    time += dt;
    it += 1;
    PetscReal norm;
    PetscCall(VecNorm(dUn, NORM_2, &norm));
    stationary = norm < cfg->precision;
    res->solve_seconds += w - v;
    res->pc_calls += 1;
    res->last_norm_dU = norm;
  }
  res->steps = it;
  res->time = time;
  return PETSC_SUCCESS;
}

}  // namespace cfp_driver
