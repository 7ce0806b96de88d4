// wave_system_real.cpp -- the PCSHELL of the real-data wave plan (include/wave_system_real.h):
// setupFFTPrec3DWaveRealData / applyFFT3DPrecWaveRealData / destroyFFTPrec3DWaveRealData.
//
// Compiled into both libraries.  What depends on the build is the element stride of the Vecs'
// arrays: PetscScalar = double reads and writes the (dim+1) N reals themselves (es = 1);
// PetscScalar complex reads the real parts and writes a zero imaginary part (es = 2), which is
// exact wherever the data are real (GMRES on the real wave operator with a real right-hand side).
// Host and device Vecs are handled as applyFFT3DPrecWave handles them (apply_on_device).
#include "../../include/circulant_fft.h"
#include "../../include/wave_system_real.h"
#include "pcshell_common.h"

using namespace cfp_pc;

namespace {
constexpr int kEs = (int)(sizeof(PetscScalar) / sizeof(double));  // doubles per Vec entry
static_assert(kEs == 1 || kEs == 2, "PetscScalar is double or complex double");
int ctx_dim(const FFTPrecWaveRealContext* ctx) { return ctx->dim ? (int)ctx->dim : 3; }
}  // namespace

extern "C" PetscErrorCode setupFFTPrec3DWaveRealData(PC pc) {
  PetscFunctionBeginUser;
  FFTPrecWaveRealContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  PetscCheck(ctx, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "setupFFTPrec3DWaveRealData: no context attached to the PC");
  int P = 1;
  PetscCallMPI(MPI_Comm_size(PETSC_COMM_WORLD, &P));
  PetscCheck(P == 1, PETSC_COMM_SELF, PETSC_ERR_SUP,
             "setupFFTPrec3DWaveRealData: the real-data wave plan runs on one rank (PETSC_COMM_WORLD has several)");
  int dev = 0;
  PetscCheck(hipGetDevice(&dev) == hipSuccess, PETSC_COMM_SELF, PETSC_ERR_LIB, "no HIP device");
  if (ctx->plan) CFPCALL(cfp_wave_rplan_destroy(ctx->plan));
  ctx->plan = nullptr;
  // an unsupported grid: CFP_ERR_SUP = PETSC_ERR_SUP with the plan's message
  CFPCALL(cfp_wave_rplan_create(&ctx->plan, ctx->n_x, ctx->n_y, ctx->n_z, ctx_dim(ctx), dev));
  const double kappa[3] = {ctx->kappa_x, ctx->kappa_y, ctx->kappa_z};
  const int rc = cfp_wave_rplan_set_symbol(ctx->plan, kappa, ctx->c0);
  if (rc != CFP_SUCCESS) {
    cfp_wave_rplan_destroy(ctx->plan);
    ctx->plan = nullptr;
  }
  CFPCALL(rc);
  PetscFunctionReturn(PETSC_SUCCESS);
}

extern "C" PetscErrorCode applyFFT3DPrecWaveRealData(PC pc, Vec b, Vec x) {
  PetscFunctionBeginUser;
  FFTPrecWaveRealContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  PetscCheck(ctx && ctx->plan, PETSC_COMM_SELF, PETSC_ERR_ARG_WRONGSTATE,
             "applyFFT3DPrecWaveRealData: setup has not run");
  const PetscInt M = (ctx_dim(ctx) + 1) * ctx->n_x * ctx->n_y * ctx->n_z;
  PetscCall(check_size(b, M, "applyFFT3DPrecWaveRealData: b has the wrong size"));
  PetscCall(check_size(x, M, "applyFFT3DPrecWaveRealData: x has the wrong size"));
  PetscCall(apply_on_device(b, x, M, __func__, [&](const double* bp, double* xp, void* st, bool) {
    return cfp_wave_rplan_apply_strided(ctx->plan, bp, xp, kEs, st);
  }));
  PetscFunctionReturn(PETSC_SUCCESS);
}

extern "C" PetscErrorCode destroyFFTPrec3DWaveRealData(PC pc) {
  PetscFunctionBeginUser;
  FFTPrecWaveRealContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  if (ctx && ctx->plan) {
    CFPCALL(cfp_wave_rplan_destroy(ctx->plan));
    ctx->plan = nullptr;
  }
  PetscFunctionReturn(PETSC_SUCCESS);
}
