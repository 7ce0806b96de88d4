// gmres_time_loop.h -- the implicit time loop's body shared by TransportEquationGMRES
// (transport_cartesian.cpp) and AdvectionDiffusionGMRES (diffusion_cartesian.cpp): one
// KSPSolve(ksp, Un, Un) per step until ntmax steps, time > tmax or ||U^{n+1} - U^n|| < precision
// (tests/TransportEquation_SphericalExplosion_impl_mpi.cxx:131-170), with the per-step
// bookkeeping both result structs share by field name.
#pragma once
#include <sys/time.h>

#include <algorithm>
#include <cstdint>

#include "../../include/petsc_mini.h"

namespace cfp_loop {

inline double wall() {
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  return (double)tv.tv_sec + 1e-6 * (double)tv.tv_usec;
}

// Result: cfp_transport_result or cfp_advdiff_result
template <class Result>
PetscErrorCode gmres_time_loop(KSP ksp, Vec Un, Vec dUn, double dt, int64_t ntmax, double tmax, double precision,
                               int profile, Result* res) {
  int64_t it = 0;
  double time = 0.0;
  bool stationary = false;
  res->all_converged = 1;
  res->min_step_its = -1;
  if (profile) PetscCall(PetscMiniProfileBegin(1 << 16));
  const double t_loop = wall();
  while (it < ntmax && time <= tmax && !stationary) {  // :131
    PetscCall(VecCopy(Un, dUn));
    const double v = wall();
    PetscCall(KSPSolve(ksp, Un, Un));
    const double w = wall();
    PetscCall(VecAXPY(dUn, -1.0, Un));
    time += dt;
    it += 1;
    PetscReal norm;
    PetscCall(VecNorm(dUn, NORM_2, &norm));
    stationary = norm < precision;
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
  if (profile) {
    PetscCall(PetscMiniProfileEnd(res->dev_ms, res->dev_launches));
    res->dev_ms[0] = 1e3 * res->pc_seconds;
    res->dev_launches[0] = res->pc_calls;
  }
  res->steps = it;
  res->time = time;
  return PETSC_SUCCESS;
}

}  // namespace cfp_loop
