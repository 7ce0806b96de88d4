// diffusion_cartesian.cpp -- the implicit advection-diffusion step on a Cartesian grid
// (include/diffusion_equation.h): the circulant FFT PCSHELL of its symbol, the direct solver, the
// 7-point operator and the GMRES time loop.  The reference's to-do list asks for this operator
// next (ToDo.md: "ajouter l'equation de diffusion ... StructuredDiffusionContext ...
// FFTPrecDiffusionContext"); the structure follows its transport boundary (pcshell_fft3d.cpp,
// pcshell_boundary.cpp, transport_cartesian.cpp).
//
// The PCSHELL's context starts with FFTPrecTransportContext's 12 members in its order, so the
// apply and the destroy callbacks are the transport ones: what they do (the solve with the plan's
// own symbol while Diag is untouched, the objects setup made) does not depend on which closed form
// filled the plan.  Only setup differs: it sets the advection-diffusion symbol.
//
// Compiled into both libraries (PetscScalar complex, and double with -DCFP_REAL_SCALAR).  What
// depends on the build sits behind cfp_pc::pc_set_advdiff_symbol and cfp_pc::pc_advdiff_diag
// (pcshell_common.h; pcshell_fft3d.cpp, pcshell_fft3d_real.cpp): which plans take the symbol and
// the layout of Diag.
#ifndef CFP_WITH_PETSC
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/circulant_fft.h"
#include "../../include/diffusion_equation.h"
#include "../../include/pcshell_fft3d.h"
#include "../../include/transport_equation.h"
#include "cartesian_driver.h"
#include "pcshell_common.h"

using namespace cfp_pc;
using cfp_driver::wall;

static_assert(offsetof(FFTPrecDiffusionContext, b_cartesien) == offsetof(FFTPrecTransportContext, b_cartesien) &&
                  offsetof(FFTPrecDiffusionContext, lambda_z) == offsetof(FFTPrecTransportContext, lambda_z) &&
                  offsetof(FFTPrecDiffusionContext, mu_x) == sizeof(FFTPrecTransportContext),
              "FFTPrecDiffusionContext starts with FFTPrecTransportContext's members");

namespace {

void pack6(PetscScalar x, PetscScalar y, PetscScalar z, double out[6]) {
  out[0] = std::real(x); out[1] = std::imag(x);
  out[2] = std::real(y); out[3] = std::imag(y);
  out[4] = std::real(z); out[5] = std::imag(z);
}

// Use (or refresh) the plan's advection-diffusion symbol for these numbers; equal numbers on an
// untouched plan reuse it (as ensure_transport_symbol, pcshell_fft3d.cpp)
// (upwind: through the upwind setters, lam of either sign)
PetscErrorCode ensure_advdiff_symbol(ShellBase* s, const double lam[6], const double mu[6], bool upwind = false) {
  PetscCheck(s->plan || s->slab.plan, PETSC_COMM_SELF, PETSC_ERR_ARG_WRONGSTATE, "the FFT matrix has no plan");
  double ad[12];
  std::memcpy(ad, lam, 6 * sizeof(double));
  std::memcpy(ad + 6, mu, 6 * sizeof(double));
  if (s->has_ad && s->ad_upwind == upwind && s->symbol_version() == s->ad_version &&
      std::memcmp(s->ad, ad, sizeof(ad)) == 0)
    return PETSC_SUCCESS;
  PetscCall(pc_set_advdiff_symbol(s, lam, mu, upwind));
  std::memcpy(s->ad, ad, sizeof(ad));
  s->has_ad = true;
  s->ad_upwind = upwind;
  s->ad_version = s->symbol_version();
  return PETSC_SUCCESS;
}

// rows [r0, r1) of shift I + dt L: rowptr[c - r0], global columns
int advdiff_csr_rows(int64_t nx, int64_t ny, int64_t nz, const double h[3], double dt, const double a[3], double nu,
                     int bc, double shift, int64_t r0, int64_t r1, int64_t* rowptr, int64_t* col, double* val,
                     int64_t* nnz) {
  if (!h || !a || !rowptr || !col || !val || !nnz) return CFP_ERR_ARG_NULL;
  if (nx < 1 || ny < 1 || nz < 1 || h[0] <= 0 || h[1] <= 0 || h[2] <= 0) return CFP_ERR_ARG_OUTOFRANGE;
  if (bc != CFP_BC_WALL && bc != CFP_BC_PERIODIC) return CFP_ERR_ARG_OUTOFRANGE;
  if (r0 < 0 || r1 < r0 || r1 > nx * ny * nz) return CFP_ERR_ARG_OUTOFRANGE;
  const int64_t n[3] = {nx, ny, nz};
  const int64_t stride[3] = {1, nx, nx * ny};
  int64_t p = 0;
  rowptr[0] = 0;
  for (int64_t c = r0; c < r1; ++c) {
    const int64_t idx[3] = {c % nx, (c / nx) % ny, c / (nx * ny)};
    double diag = shift;
    // the six faces' neighbour columns and coefficients (-x, +x, -y, +y, -z, +z); on a periodic
    // axis of two cells both faces reach the same cell and their coefficients add up
    int64_t ncol[6];
    double ncoef[6];
    int m = 0;
    for (int d = 0; d < 3; ++d) {
      const double adv = dt / h[d], dif = nu * dt / (h[d] * h[d]);
      if (bc == CFP_BC_PERIODIC && n[d] == 1) continue;  // the neighbour is the cell itself: net 0
      for (int s = 0; s < 2; ++s) {  // s = 0: face -d (normal -e_d), s = 1: face +d
        int64_t j = idx[d] + (s == 0 ? -1 : 1);
        if (j < 0 || j >= n[d]) {
          if (bc == CFP_BC_WALL) continue;
          j = (j + n[d]) % n[d];
        }
        const int64_t nb = c + (j - idx[d]) * stride[d];
        const double un = s == 0 ? -a[d] : a[d];
        double coef = -dif;
        diag += dif;
        if (un > 0) diag += adv * un;
        else coef += adv * un;
        int k = 0;
        while (k < m && ncol[k] != nb) ++k;
        if (k == m) {
          ncol[m] = nb;
          ncoef[m] = 0.0;
          ++m;
        }
        ncoef[k] += coef;
      }
    }
    // ascending columns, the diagonal (slot m) among them; exact zeros are not stored
    int64_t cols7[7];
    double vals7[7];
    int order[7];
    for (int k = 0; k < m; ++k) {
      cols7[k] = ncol[k];
      vals7[k] = ncoef[k];
    }
    cols7[m] = c;
    vals7[m] = diag;
    for (int k = 0; k <= m; ++k) order[k] = k;
    for (int k = 1; k <= m; ++k)
      for (int q = k; q > 0 && cols7[order[q]] < cols7[order[q - 1]]; --q) std::swap(order[q], order[q - 1]);
    for (int k = 0; k <= m; ++k) {
      const int o = order[k];
      if (o != m && vals7[o] == 0.0) continue;
      col[p] = cols7[o];
      val[2 * p] = vals7[o];
      val[2 * p + 1] = 0.0;
      ++p;
    }
    rowptr[c - r0 + 1] = p;
  }
  *nnz = p;
  return CFP_SUCCESS;
}

}  // namespace

// ------------------------------------------------------------------ context + PCSHELL callbacks
extern "C" PetscErrorCode getFFTPrec3DDiffusionContext(PetscInt ndim, PetscScalar dt, PetscInt n_x, PetscInt n_y,
                                                       PetscInt n_z, PetscScalar a_x, PetscScalar a_y, PetscScalar a_z,
                                                       PetscScalar nu, const PetscReal mins[3], const PetscReal maxs[3],
                                                       FFTPrecDiffusionContext* ctx) {
  PetscFunctionBeginUser;
  PetscCheck(ndim > 0 && ndim < 4, PETSC_COMM_WORLD, PETSC_ERR_ARG_OUTOFRANGE, "Dimension should be 1, 2 or 3");
  PetscCheck(ctx && mins && maxs, PETSC_COMM_WORLD, PETSC_ERR_ARG_NULL, "getFFTPrec3DDiffusionContext: NULL argument");
  PetscCheck(n_x >= 1 && n_y >= 1 && n_z >= 1, PETSC_COMM_WORLD, PETSC_ERR_ARG_OUTOFRANGE, "grid sizes must be >= 1");
  std::memset((void*)ctx, 0, sizeof(*ctx));
  ctx->spaceDim = ndim;
  ctx->n_x = n_x;
  ctx->n_y = n_y;
  ctx->n_z = n_z;
  const PetscInt n[3] = {n_x, n_y, n_z};
  const PetscScalar a[3] = {a_x, a_y, a_z};
  PetscScalar lam[3], mu[3];
  for (int d = 0; d < 3; ++d) {
    const double h = (maxs[d] - mins[d]) / (double)n[d];
    PetscCheck(d >= ndim || h > 0, PETSC_COMM_WORLD, PETSC_ERR_ARG_OUTOFRANGE, "empty domain");
    lam[d] = d < ndim ? a[d] * dt / h : PetscScalar(0.0);
    mu[d] = d < ndim ? nu * dt / (h * h) : PetscScalar(0.0);
  }
  ctx->lambda_x = lam[0];
  ctx->lambda_y = lam[1];
  ctx->lambda_z = lam[2];
  ctx->mu_x = mu[0];
  ctx->mu_y = mu[1];
  ctx->mu_z = mu[2];
  PetscFunctionReturn(PETSC_SUCCESS);
}

// setupFFTPrec3D with the advection-diffusion symbol: FFT matrix, work vectors and Diag
// (materialised from the plan's closed form, and remembered: while nobody writes to it the apply
// divides by the symbol in registers)
extern "C" PetscErrorCode setupFFTPrec3DDiffusion(PC pc) {
  PetscFunctionBeginUser;
  FFTPrecDiffusionContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  PetscCheck(ctx, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "setupFFTPrec3DDiffusion: no context attached to the PC");
  PetscCheck(ctx->n_x >= 1 && ctx->n_y >= 1 && ctx->n_z >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE,
             "setupFFTPrec3DDiffusion: n_x, n_y, n_z must be >= 1");
  // several ranks: this rank's z slab (MatCreateFFTHIP refuses a split that does not divide n_z
  // with PETSC_ERR_ARG_SIZ), Diag and the work vectors its z-planes
  const PetscInt dims[3] = {ctx->n_z, ctx->n_y, ctx->n_x};
  PetscCall(MatCreateFFTHIP(PETSC_COMM_WORLD, 3, dims, &ctx->FFT_MAT));
  PetscCall(MatCreateVecsFFTW(ctx->FFT_MAT, NULL, &ctx->Diag, NULL));
  PetscCall(MatCreateVecsFFTW(ctx->FFT_MAT, &ctx->b_cartesien, &ctx->b_hat, NULL));
  ShellBase* s;
  PetscCall(shell_base(ctx->FFT_MAT, &s));
  double lam[6], mu[6];
  pack6(ctx->lambda_x, ctx->lambda_y, ctx->lambda_z, lam);
  pack6(ctx->mu_x, ctx->mu_y, ctx->mu_z, mu);
  PetscCall(ensure_advdiff_symbol(s, lam, mu));
  PetscCall(pc_advdiff_diag(s, ctx->Diag, lam, mu));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// The two setups of the upwind symbol (cfp_plan_set_symbol_upwind: a cell coupled to index - 1 or
// index + 1 by the sign of lambda_d, the operators of cfp_transport_csr with CFP_UPWIND_FIXED and of
// cfp_advdiff_csr).  ctx: the 12 leading members the two contexts share; Diag is materialised from
// the advection-diffusion closed form of the mapped numbers (cfp_upwind_to_advdiff) and remembered
// as the plan's own, so apply, applyBA and destroy are the existing callbacks.
static PetscErrorCode setup_upwind(PC pc, FFTPrecTransportContext* ctx, const double lam[6], const double mu[6],
                                   const char* who) {
  PetscCheck(ctx, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, who);
  PetscCheck(ctx->n_x >= 1 && ctx->n_y >= 1 && ctx->n_z >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, who);
  const PetscInt dims[3] = {ctx->n_z, ctx->n_y, ctx->n_x};
  PetscCall(MatCreateFFTHIP(PETSC_COMM_WORLD, 3, dims, &ctx->FFT_MAT));
  PetscCall(MatCreateVecsFFTW(ctx->FFT_MAT, NULL, &ctx->Diag, NULL));
  PetscCall(MatCreateVecsFFTW(ctx->FFT_MAT, &ctx->b_cartesien, &ctx->b_hat, NULL));
  ShellBase* s;
  PetscCall(shell_base(ctx->FFT_MAT, &s));
  PetscCall(ensure_advdiff_symbol(s, lam, mu, true));
  double l2[6], m2[6];
  CFPCALL(cfp_upwind_to_advdiff(lam, mu, l2, m2));
  PetscCall(pc_advdiff_diag(s, ctx->Diag, l2, m2));
#ifndef CFP_REAL_SCALAR
  // the operator's row-class form for applyFFT3DPrecTransportBA, built now (as setupFFTPrec3D)
  Mat A = nullptr;
  PetscCall(PCGetOperators(pc, &A, NULL));
  MatType mt = nullptr;
  if (A && !s->slab.plan) PetscCall(MatGetType(A, &mt));
  if (mt && std::strcmp(mt, MATSEQAIJ) == 0) {
    PetscBool has, xl;
    PetscMiniDia dia;
    PetscCall(PetscMiniMatAIJGetDia(A, ctx->n_x, &has, &xl, &dia));
  }
#endif
  return PETSC_SUCCESS;
}

extern "C" PetscErrorCode setupFFTPrec3DUpwind(PC pc) {
  PetscFunctionBeginUser;
  FFTPrecTransportContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  PetscCheck(ctx, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "setupFFTPrec3DUpwind: no context attached to the PC");
  double lam[6];
  const double mu[6] = {0, 0, 0, 0, 0, 0};
  pack6(ctx->lambda_x, ctx->lambda_y, ctx->lambda_z, lam);
  PetscCall(setup_upwind(pc, ctx, lam, mu, "setupFFTPrec3DUpwind: n_x, n_y, n_z must be >= 1"));
  PetscFunctionReturn(PETSC_SUCCESS);
}

extern "C" PetscErrorCode setupFFTPrec3DDiffusionUpwind(PC pc) {
  PetscFunctionBeginUser;
  FFTPrecDiffusionContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  PetscCheck(ctx, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "setupFFTPrec3DDiffusionUpwind: no context attached to the PC");
  double lam[6], mu[6];
  pack6(ctx->lambda_x, ctx->lambda_y, ctx->lambda_z, lam);
  pack6(ctx->mu_x, ctx->mu_y, ctx->mu_z, mu);
  // (the leading members are FFTPrecTransportContext's, static_assert above)
  PetscCall(setup_upwind(pc, reinterpret_cast<FFTPrecTransportContext*>(ctx), lam, mu,
                         "setupFFTPrec3DDiffusionUpwind: n_x, n_y, n_z must be >= 1"));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// the plan's own-symbol apply: applyFFT3DPrecTransport's body on the shared leading members
extern "C" PetscErrorCode applyFFT3DPrecDiffusion(PC pc, Vec b, Vec x) { return applyFFT3DPrecTransport(pc, b, x); }
extern "C" PetscErrorCode destroyFFTPrec3DDiffusion(PC pc) { return destroyFFTPrec3D(pc); }

// ------------------------------------------------------------------ direct solver
extern "C" PetscErrorCode PetscFft3DDiffusionSolver(struct StructuredDiffusionContext c, Vec b, Vec x) {
  PetscFunctionBeginUser;
  ShellBase* s;
  PetscCall(shell_base(c.FFT_MAT, &s));
  PetscCheck(s->dims[0] == c.n_x && s->dims[1] == c.n_y && s->dims[2] == c.n_z, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ,
             "PetscFft3DDiffusionSolver: grid dims do not match FFT_MAT");
  double lam[6], mu[6];
  pack6(c.a_x * c.dt / c.delta_x, c.a_y * c.dt / c.delta_y, c.a_z * c.dt / c.delta_z, lam);
  pack6(c.nu * c.dt / (c.delta_x * c.delta_x), c.nu * c.dt / (c.delta_y * c.delta_y),
        c.nu * c.dt / (c.delta_z * c.delta_z), mu);
  PetscCall(ensure_advdiff_symbol(s, lam, mu));
  PetscCall(own_symbol_apply(c.FFT_MAT, x, b));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// ------------------------------------------------------------------ the operator
extern "C" int cfp_advdiff_csr(int64_t nx, int64_t ny, int64_t nz, const double h[3], double dt, const double a[3],
                               double nu, int bc, double shift, int64_t* rowptr, int64_t* col, double* val,
                               int64_t* nnz) {
  return advdiff_csr_rows(nx, ny, nz, h, dt, a, nu, bc, shift, 0, nx * ny * nz, rowptr, col, val, nnz);
}

extern "C" PetscErrorCode computeAdvectionDiffusionMatrixCartesianAIJ(MPI_Comm comm, PetscInt nx, PetscInt ny,
                                                                      PetscInt nz, const PetscReal h[3], PetscReal dt,
                                                                      const PetscReal a[3], PetscReal nu, PetscInt bc,
                                                                      Mat* A) {
  PetscFunctionBeginUser;
  PetscCheck(A && h && a, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL,
             "computeAdvectionDiffusionMatrixCartesianAIJ: NULL argument");
  PetscCheck(nx >= 1 && ny >= 1 && nz >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "grid sizes must be >= 1");
  const int64_t N = nx * ny * nz;
  int P = 1;
  PetscCallMPI(MPI_Comm_size(comm, &P));
  if (P == 1) {  // one rank: the arrays go in whole (MATSEQAIJ, as computeDivergenceMatrixCartesian)
    std::vector<int64_t> rowptr((size_t)N + 1), col((size_t)(7 * N));
    std::vector<PetscScalar> val((size_t)(7 * N) * cfp_driver::kPairScalars);
    int64_t nnz = 0;
    const int rc = cfp_advdiff_csr(nx, ny, nz, h, dt, a, nu, (int)bc, 0.0, rowptr.data(), col.data(),
                                   reinterpret_cast<double*>(val.data()), &nnz);
    PetscCheck(rc == CFP_SUCCESS, PETSC_COMM_SELF, rc, "computeAdvectionDiffusionMatrixCartesianAIJ: bad arguments");
    cfp_driver::pairs_to_scalars(val.data(), nnz);
    PetscCall(MatCreateSeqAIJWithArrays(comm, N, N, rowptr.data(), col.data(), val.data(), A));
    PetscFunctionReturn(PETSC_SUCCESS);
  }
  const auto rows = [&](int64_t lo, int64_t hi, int64_t* rowptr, int64_t* col, double* val,
                        int64_t* nnz) -> PetscErrorCode {
    const int rc = advdiff_csr_rows(nx, ny, nz, h, dt, a, nu, (int)bc, 0.0, lo, hi, rowptr, col, val, nnz);
    PetscCheck(rc == CFP_SUCCESS, PETSC_COMM_SELF, rc, "computeAdvectionDiffusionMatrixCartesianAIJ: bad arguments");
    return PETSC_SUCCESS;
  };
  PetscCall(cfp_driver::aij_from_rows(comm, N, rows, A));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// ------------------------------------------------------------------ time loops
extern "C" void cfp_advdiff_config_default(cfp_advdiff_config* cfg, int64_t n) {
  if (!cfg) return;
  std::memset((void*)cfg, 0, sizeof(*cfg));
  cfg->nx = cfg->ny = cfg->nz = n;
  for (int d = 0; d < 3; ++d) {
    cfg->xmin[d] = -0.5;
    cfg->xmax[d] = 0.5;
  }
  cfg->a[0] = 1.0;
  cfg->nu = 0.01;
  cfg->dt = 0.01;
  cfg->tmax = 1e300;
  cfg->ntmax = 1;
  cfg->precision = 1e-8;
  cfg->max_its = 1000;
  cfg->restart = 30;
  cfg->pc = CFP_ADVDIFF_PC_FFT;
  cfg->bc = CFP_BC_WALL;
  cfg->pc_side = PC_LEFT;
  cfg->on_device = 1;
  cfg->profile = 0;
}

extern "C" PetscErrorCode AdvectionDiffusionGMRES(const cfp_advdiff_config* cfg, cfp_advdiff_result* res,
                                                  double* U_out) {
  PetscFunctionBeginUser;
  PetscCheck(cfg && res, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "AdvectionDiffusionGMRES: NULL argument");
  PetscCheck(cfg->pc == CFP_ADVDIFF_PC_NONE || cfg->on_device, PETSC_COMM_SELF, PETSC_ERR_SUP,
             "the FFT preconditioner runs on HIP vectors only");
  PetscCheck(cfg->dt > 0 && cfg->nu >= 0, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "dt must be > 0 and nu >= 0");
  std::memset((void*)res, 0, sizeof(*res));
  const double t_setup = wall();
  const PetscInt nx = cfg->nx, ny = cfg->ny, nz = cfg->nz, N = nx * ny * nz;
  PetscCheck(nx >= 1 && ny >= 1 && nz >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "grid sizes must be >= 1");
  const int dim = nz > 1 ? 3 : (ny > 1 ? 2 : 1);
  double h[3];
  cfp_driver::grid_spacing(cfg, h);
  const double dt = cfg->dt;
  res->dt = dt;

  // one rank: sequential Vecs and AIJ; several (PETSC_COMM_WORLD of PetscMiniSetCommWorld):
  // distributed ones in PETSC_DECIDE rows, as TransportEquationGMRES
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
  PetscCall(computeAdvectionDiffusionMatrixCartesianAIJ(P > 1 ? PETSC_COMM_WORLD : PETSC_COMM_SELF, nx, ny, nz, h, dt,
                                                        cfg->a, cfg->nu, cfg->bc, &A));
  PetscCall(MatShift(A, 1.0));

  KSP ksp;
  PC pc;
  // the 7-point stencil is not x-local: MatMult, PCApply and the dots run as separate sweeps
  PetscCall(cfp_driver::gmres_create(cfg, PETSC_FALSE, &ksp, &pc));
  FFTPrecDiffusionContext ctx;
  std::memset((void*)&ctx, 0, sizeof(ctx));
  if (cfg->pc == CFP_ADVDIFF_PC_FFT || cfg->pc == CFP_ADVDIFF_PC_FFT_UPWIND) {
    PetscCall(getFFTPrec3DDiffusionContext(dim, dt, nx, ny, nz, cfg->a[0], cfg->a[1], cfg->a[2], cfg->nu, cfg->xmin,
                                           cfg->xmax, &ctx));
    PetscCall(PCSetType(pc, PCSHELL));
    PetscCall(PCShellSetContext(pc, &ctx));
    const bool up = cfg->pc == CFP_ADVDIFF_PC_FFT_UPWIND;
    PetscCall(PCShellSetSetUp(pc, up ? setupFFTPrec3DDiffusionUpwind : setupFFTPrec3DDiffusion));
    PetscCall(PCShellSetApply(pc, applyFFT3DPrecDiffusion));
    PetscCall(PCShellSetDestroy(pc, destroyFFTPrec3DDiffusion));
    PetscCall(PCShellSetName(pc, up ? "circulant FFT, upwind advection-diffusion (HIP)"
                                    : "circulant FFT, advection-diffusion (HIP)"));
    res->lambda[0] = std::real(ctx.lambda_x);
    res->lambda[1] = std::real(ctx.lambda_y);
    res->lambda[2] = std::real(ctx.lambda_z);
    res->mu[0] = std::real(ctx.mu_x);
    res->mu[1] = std::real(ctx.mu_y);
    res->mu[2] = std::real(ctx.mu_z);
  } else {
    PetscCall(PCSetType(pc, PCNONE));
  }
  PetscCall(cfp_driver::gmres_setup(ksp, A, Un, dUn, cfg->on_device, t_setup, res));

  PetscCall(cfp_driver::gmres_time_loop(ksp, Un, dUn, dt, cfg, res));
  PetscCall(cfp_driver::copy_out(Un, nloc, U_out));
  PetscCall(KSPDestroy(&ksp));  // destroys the PC, whose destroy callback frees setup's objects
  PetscCall(MatDestroy(&A));
  PetscCall(VecDestroy(&Un));
  PetscCall(VecDestroy(&dUn));
  PetscFunctionReturn(PETSC_SUCCESS);
}

extern "C" PetscErrorCode AdvectionDiffusionFFTDirect(const cfp_advdiff_config* cfg, cfp_advdiff_result* res,
                                                      double* U_out) {
  PetscFunctionBeginUser;
  PetscCheck(cfg && res, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "AdvectionDiffusionFFTDirect: NULL argument");
  PetscCheck(cfg->dt > 0 && cfg->nu >= 0, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "dt must be > 0 and nu >= 0");
  std::memset((void*)res, 0, sizeof(*res));
  const double t_setup = wall();
  const PetscInt nx = cfg->nx, ny = cfg->ny, nz = cfg->nz, N = nx * ny * nz;
  PetscCheck(nx >= 1 && ny >= 1 && nz >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "grid sizes must be >= 1");
  double h[3];
  cfp_driver::grid_spacing(cfg, h);
  const double dt = cfg->dt;
  res->dt = dt;
  const PetscInt n[3] = {nx, ny, nz};
  // an axis of one cell carries no operator (its symbol part is 0 whatever the numbers)
  for (int d = 0; d < 3; ++d) {
    res->lambda[d] = n[d] > 1 ? cfg->a[d] * dt / h[d] : 0.0;
    res->mu[d] = n[d] > 1 ? cfg->nu * dt / (h[d] * h[d]) : 0.0;
  }
  // several ranks: distributed Vecs in PETSC_DECIDE rows (whole z-planes: P | nz) on the slab-backed matrix
  int P = 1;
  PetscCallMPI(MPI_Comm_size(PETSC_COMM_WORLD, &P));
  PetscCheck(nz % P == 0, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ,
             "AdvectionDiffusionFFTDirect: the number of ranks must divide nz (whole z-planes per rank)");
  Vec Un, dUn;
  PetscCall(cfp_driver::create_state(cfg, P, &Un, &dUn));
  PetscInt lo, nloc;
  PetscCall(VecGetOwnershipRange(Un, &lo, NULL));
  PetscCall(VecGetLocalSize(Un, &nloc));
  res->rstart = lo;
  res->nlocal = nloc;
  Mat FFT_MAT;
  const PetscInt dims[3] = {nz, ny, nx};
  PetscCall(MatCreateFFT(PETSC_COMM_WORLD, 3, dims, MATFFTW, &FFT_MAT));
  struct StructuredDiffusionContext ctx = {nx, ny, nz, cfg->a[0], cfg->a[1], cfg->a[2], cfg->nu, dt, h[0], h[1], h[2],
                                           FFT_MAT};
  res->setup_seconds = wall() - t_setup;

  const auto solve = [&](Vec U) { return PetscFft3DDiffusionSolver(ctx, U, U); };
  PetscCall(cfp_driver::direct_time_loop(Un, dUn, dt, cfg, solve, res));
  PetscCall(cfp_driver::copy_out(Un, nloc, U_out));
  PetscCall(MatDestroy(&FFT_MAT));
  PetscCall(VecDestroy(&Un));
  PetscCall(VecDestroy(&dUn));
  PetscFunctionReturn(PETSC_SUCCESS);
}
#endif  // CFP_WITH_PETSC
