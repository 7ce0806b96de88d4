// pcshell_boundary.cpp -- the entry points of include/pcshell_fft3d.h that do not depend on the
// scalar type, compiled into both libraries: libcirculant_fft.so beside pcshell_fft3d.cpp (complex
// scalars) and libcirculant_fft_real.so beside pcshell_fft3d_real.cpp (-DCFP_REAL_SCALAR).  The
// PCSHELL callbacks' remap skeleton, the direct solver's forwarding wrappers, the context side
// table and the common part of the FFT matrix live here; the solves themselves are reached through
// the four hidden names of pcshell_common.h that each scalar build defines once.
#include <cmath>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "../../include/pcshell_fft3d.h"
#include "pcshell_common.h"

using namespace cfp_pc;

// cfp_plan.hip (internal): stop the current PCApply's dispatch stamping (cfp::g_apply_stamp)
extern "C" void cfp_apply_stamp_clear(void);

namespace {
// Per-context additions of this build, keyed by the context's address, so that the context
// keeps the reference's exact layout (src/PCSHELLFft_3D.hxx:8-21; include/pcshell_fft3d.h).
struct CtxExtra {
  Mat remapBack = nullptr;
};
std::mutex g_extra_mu;
std::unordered_map<const void*, CtxExtra> g_extra;

void ctx_forget(const FFTPrecTransportContext* ctx) {
  std::lock_guard<std::mutex> g(g_extra_mu);
  g_extra.erase(ctx);
}

#ifdef CFP_WITH_PETSC
// MatCreateVecsFFTW(A, x, y, z) on the shell: PETSc dispatches it through this composed method
// (a MATSHELL has no MatCreateVecsFFTW_C of its own)
PetscErrorCode create_vecs(Mat A, Vec* x, Vec* y, Vec* z) {
  if (x) PetscCall(MatCreateVecs(A, x, NULL));
  if (y) PetscCall(MatCreateVecs(A, NULL, y));
  if (z) PetscCall(MatCreateVecs(A, z, NULL));
  return PETSC_SUCCESS;
}
#endif
}  // namespace

Mat cfp_pc::ctx_remap_back(const FFTPrecTransportContext* ctx) {
  std::lock_guard<std::mutex> g(g_extra_mu);
  auto it = g_extra.find(ctx);
  return it == g_extra.end() ? nullptr : it->second.remapBack;
}

extern "C" PetscErrorCode FFTPrecTransportContextSetRemapBack(FFTPrecTransportContext* ctx, Mat remapBack) {
  PetscCheck(ctx, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "NULL context");
  std::lock_guard<std::mutex> g(g_extra_mu);
  if (remapBack) g_extra[ctx].remapBack = remapBack;
  else g_extra.erase(ctx);
  return PETSC_SUCCESS;
}
extern "C" PetscErrorCode FFTPrecTransportContextGetRemapBack(const FFTPrecTransportContext* ctx, Mat* remapBack) {
  PetscCheck(ctx && remapBack, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "NULL argument");
  *remapBack = ctx_remap_back(ctx);
  return PETSC_SUCCESS;
}

// ------------------------------------------------------------------ FFT matrix
PetscErrorCode cfp_pc::shell_base(Mat A, ShellBase** out) {
  void* ctx = nullptr;
  PetscCall(MatShellGetContext(A, &ctx));
  ShellBase* s = (ShellBase*)ctx;
  PetscCheck(s && s->magic == kShellMagic, PETSC_COMM_SELF, PETSC_ERR_ARG_WRONG,
             "FFT_MAT is not an FFT matrix made by MatCreateFFT/MatCreateFFTHIP");
  *out = s;
  return PETSC_SUCCESS;
}

PetscErrorCode cfp_pc::shell_create_plan(ShellBase* s, MPI_Comm comm, PetscInt ndim, const PetscInt dims[], Mat* A) {
  PetscCheck(ndim >= 1 && ndim <= 3, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE, "ndim must be 1, 2 or 3");
  PetscCheck(dims && A, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "NULL argument");
  PetscCallMPI(MPI_Comm_size(comm, &s->nranks));
  PetscCallMPI(MPI_Comm_rank(comm, &s->rank));
  // dims are row-major {n_z, n_y, n_x} (src/PCSHELLFft_3D.cxx:34): last = fastest = x
  for (PetscInt d = 0; d < ndim; ++d) s->dims[d] = dims[ndim - 1 - d];
  s->nzl = s->dims[2];
  s->nl = s->dims[0] * s->dims[1] * s->dims[2];
  int dev = 0;
  hipGetDevice(&dev);
  if (s->nranks == 1) return cfp_err(cfp_plan_create(&s->plan, s->dims[0], s->dims[1], s->dims[2], dev), "MatCreateFFTHIP");
  int64_t lay[8];
  const int rc = cfp_slab_layout(s->dims[0], s->dims[1], s->dims[2], s->nranks, s->rank, lay);
  const PetscErrorCode e =
      rc ? cfp_err(rc, "MatCreateFFTHIP") : slab_create(comm, s->nranks, s->rank, s->dims, dev, &s->slab);
  if (e) {
    slab_destroy(&s->slab);
    return e;
  }
  s->nzl = lay[0];
  s->z0 = lay[2];
  s->nl = lay[4];
  return PETSC_SUCCESS;
}

PetscErrorCode cfp_pc::shell_create_mat(ShellBase* s, MPI_Comm comm, PetscInt m, PetscInt n, PetscInt M, PetscInt N,
                                        ShellMult mult, ShellMult mult_transpose, PetscErrorCode (*destroy)(Mat),
                                        Mat* A) {
  PetscCall(MatCreateShell(comm, m, n, M, N, s, A));
  PetscCall(MatShellSetOperation(*A, MATOP_MULT, (void (*)(void))mult));
  PetscCall(MatShellSetOperation(*A, MATOP_MULT_TRANSPOSE, (void (*)(void))mult_transpose));
  PetscCall(MatShellSetOperation(*A, MATOP_DESTROY, (void (*)(void))destroy));
#ifdef CFP_WITH_PETSC
  PetscCall(PetscObjectComposeFunction((PetscObject)*A, "MatCreateVecsFFTW_C", create_vecs));
#endif
  return PETSC_SUCCESS;
}

// the single-GPU complex plan behind an FFT matrix (its symbol setters reach solve_3D's own path)
extern "C" PetscErrorCode MatFFTHIPGetPlan(Mat A, cfp_plan_t* plan) {
  ShellBase* s;
  PetscCall(shell_base(A, &s));
  *plan = s->plan;
  return PETSC_SUCCESS;
}
extern "C" PetscErrorCode MatFFTHIPGetDistPlan(Mat A, struct cfp_dist_plan_s** plan) {
  ShellBase* s;
  PetscCall(shell_base(A, &s));
  *plan = s->slab.plan;
  return PETSC_SUCCESS;
}
extern "C" PetscErrorCode MatFFTHIPGetSolveCounts(Mat A, PetscInt* own_symbol, PetscInt* explicit_diag) {
  ShellBase* s;
  PetscCall(shell_base(A, &s));
  if (own_symbol) *own_symbol = s->solves_own;
  if (explicit_diag) *explicit_diag = s->solves_diag;
  return PETSC_SUCCESS;
}
extern "C" PetscErrorCode MatFFTHIPGetFusedBACount(Mat A, PetscInt* fused_ba) {
  ShellBase* s;
  PetscCall(shell_base(A, &s));
  if (fused_ba) *fused_ba = s->fused_ba;
  return PETSC_SUCCESS;
}

// ------------------------------------------------------------------ direct solver
// build_transport_col, src/FftLinearSolver_3D.c:80-90
extern "C" PetscErrorCode build_transport_col(Vec c, PetscInt size) {
  PetscFunctionBeginUser;
  PetscCall(VecSet(c, 0.0));
  if (size > 1) {
    PetscCall(VecSetValue(c, 0, 1.0, INSERT_VALUES));
    PetscCall(VecSetValue(c, 1, -1.0, INSERT_VALUES));
  }
  PetscCall(VecAssemblyBegin(c));
  PetscCall(VecAssemblyEnd(c));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// Fft3DTransportSolver, :266-281: lambda_d = a_d dt / delta_d
extern "C" PetscErrorCode Fft3DTransportSolver(PetscInt nx, PetscInt ny, PetscInt nz, PetscScalar ax, PetscScalar ay,
                                               PetscScalar az, PetscScalar dt, PetscScalar dx, PetscScalar dy,
                                               PetscScalar dz, Vec X, Vec b, Mat FFT_MAT) {
  PetscFunctionBeginUser;
  const PetscScalar lx = ax * dt / dx, ly = ay * dt / dy, lz = az * dt / dz;
  PetscCall(FftTransportSolver(nx, ny, nz, lx, ly, lz, X, b, FFT_MAT));
  PetscFunctionReturn(PETSC_SUCCESS);
}
// :283-290
extern "C" PetscErrorCode Fft2DTransportSolver(PetscInt nx, PetscInt ny, PetscScalar ax, PetscScalar ay,
                                               PetscScalar dt, PetscScalar dx, PetscScalar dy, Vec X, Vec b,
                                               Mat FFT_MAT) {
  PetscFunctionBeginUser;
  PetscCall(Fft3DTransportSolver(nx, ny, 1, ax, ay, 0.0, dt, dx, dy, 1.0, X, b, FFT_MAT));
  PetscFunctionReturn(PETSC_SUCCESS);
}
// :292-301
extern "C" PetscErrorCode Fft1DTransportSolver(PetscInt nx, PetscScalar ax, PetscScalar dt, PetscScalar dx, Vec X,
                                               Vec b, Mat FFT_MAT) {
  PetscFunctionBeginUser;
  PetscCall(Fft3DTransportSolver(nx, 1, 1, ax, 0.0, 0.0, dt, dx, 1.0, 1.0, X, b, FFT_MAT));
  PetscFunctionReturn(PETSC_SUCCESS);
}
// :303-312 (context by value, as the reference)
extern "C" PetscErrorCode PetscFft3DTransportSolver(struct StructuredTransportContext c, Vec b, Vec x) {
  PetscFunctionBeginUser;
  PetscCall(Fft3DTransportSolver(c.n_x, c.n_y, c.n_z, c.a_x, c.a_y, c.a_z, c.dt, c.delta_x, c.delta_y, c.delta_z, x,
                                 b, c.FFT_MAT));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// ------------------------------------------------------------------ PCSHELL callbacks
// applyFFT3DPrecTransport, src/PCSHELLFft_3D.cxx:10-24
extern "C" PetscErrorCode applyFFT3DPrecTransport(PC pc, Vec b, Vec x) {
  PetscFunctionBeginUser;
  FFTPrecTransportContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  PetscCheck(ctx && ctx->FFT_MAT && ctx->Diag, PETSC_COMM_SELF, PETSC_ERR_ARG_WRONGSTATE,
             "applyFFT3DPrecTransport: setupFFTPrec3D has not run");
  const Mat back = ctx_remap_back(ctx);
  // the stand-in KSP times a PCApply by the plan's first and last kernel only when the plan
  // apply is the whole PCApply: not with remaps around it
  if (!kPlanApplyIsWholePCApply || ctx->intersectionMatrix || back) cfp_apply_stamp_clear();
  Vec src = b;
  if (ctx->intersectionMatrix) {  // mesh -> Cartesian remap (identity when NULL)
    PetscCall(MatMult(ctx->intersectionMatrix, b, ctx->b_cartesien));
    src = ctx->b_cartesien;
  }
  if (back) {  // extra (mesh_unstructured.h): solve on the grid, then back to the mesh
    if (src != ctx->b_cartesien) PetscCall(VecCopy(src, ctx->b_cartesien));
    PetscCall(pc_solve(nullptr, ctx, ctx->b_cartesien, ctx->b_cartesien));
    PetscCall(MatMult(back, ctx->b_cartesien, x));
    PetscFunctionReturn(PETSC_SUCCESS);
  }
  PetscCall(pc_solve(pc, ctx, x, src));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// PCShellSetApplyBA callback (PETSc's PCApplyBAorAB on a shell): y = B A x (left) or A B x
// (right) with A the PC's operator.  Left, no remaps and x != y: the scalar build may form A x
// inside the apply (pc_fused_ba).  Anything else: MatMult, then the apply, as PETSc does without
// an applyBA.
extern "C" PetscErrorCode applyFFT3DPrecTransportBA(PC pc, PCSide side, Vec x, Vec y, Vec work) {
  PetscFunctionBeginUser;
  FFTPrecTransportContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  PetscCheck(ctx && ctx->FFT_MAT && ctx->Diag, PETSC_COMM_SELF, PETSC_ERR_ARG_WRONGSTATE,
             "applyFFT3DPrecTransportBA: setupFFTPrec3D has not run");
  Mat A = nullptr;
  PetscCall(PCGetOperators(pc, &A, NULL));
  PetscCheck(A, PETSC_COMM_SELF, PETSC_ERR_ARG_WRONGSTATE, "applyFFT3DPrecTransportBA: the PC has no operator");
  if (side == PC_LEFT && !ctx->intersectionMatrix && !ctx_remap_back(ctx) && x != y) {
    bool taken = false;
    PetscCall(pc_fused_ba(pc, ctx, A, x, y, &taken));
    if (taken) PetscFunctionReturn(PETSC_SUCCESS);
  }
  if (side == PC_LEFT) {
    PetscCall(MatMult(A, x, work));
    PetscCall(applyFFT3DPrecTransport(pc, work, y));
  } else if (side == PC_RIGHT) {
    PetscCall(applyFFT3DPrecTransport(pc, x, work));
    PetscCall(MatMult(A, work, y));
  } else {
    PetscCheck(false, PETSC_COMM_SELF, PETSC_ERR_SUP, "applyFFT3DPrecTransportBA: left or right preconditioning");
  }
  PetscFunctionReturn(PETSC_SUCCESS);
}

// destroyFFTPrec3D, :86-99 (frees what setup created; the context itself stays the caller's)
extern "C" PetscErrorCode destroyFFTPrec3D(PC pc) {
  PetscFunctionBeginUser;
  FFTPrecTransportContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  if (!ctx) PetscFunctionReturn(PETSC_SUCCESS);
  PetscCall(VecDestroy(&ctx->Diag));
  PetscCall(VecDestroy(&ctx->b_cartesien));
  PetscCall(VecDestroy(&ctx->b_hat));
  PetscCall(MatDestroy(&ctx->FFT_MAT));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// getFFTPrec3DContext, :101-151 (fills the caller's ctx; lambda formula kept as the reference's)
extern "C" PetscErrorCode getFFTPrec3DContext(PetscInt ndim, PetscScalar dt, PetscInt nbCells, PetscScalar a_x,
                                              PetscScalar a_y, PetscScalar a_z, PetscScalar Xmin, PetscScalar Ymin,
                                              PetscScalar Zmin, PetscScalar Xmax, PetscScalar Ymax, PetscScalar Zmax,
                                              FFTPrecTransportContext* ctx) {
  PetscFunctionBeginUser;
  PetscCheck(ndim > 0 && ndim < 4, PETSC_COMM_WORLD, PETSC_ERR_ARG_OUTOFRANGE, "Dimension should be 1, 2 or 3");
  PetscCheck(ctx, PETSC_COMM_WORLD, PETSC_ERR_ARG_NULL, "getFFTPrec3DContext: ctx is NULL");
  PetscInt nx = nbCells, ny = 1, nz = 1;
  if (ndim == 3) nx = ny = nz = (PetscInt)std::floor(std::cbrt((double)nbCells));
  else if (ndim == 2) nx = ny = (PetscInt)std::floor(std::sqrt((double)nbCells));
  std::memset((void*)ctx, 0, sizeof(*ctx));
  ctx_forget(ctx);  // a fresh context: no remapBack left from a previous one at this address
  ctx->spaceDim = ndim;
  ctx->n_x = nx;
  ctx->n_y = ny;
  ctx->n_z = nz;
  ctx->lambda_x = a_x * dt * (Xmax - Xmin) / (double)nx;
  ctx->lambda_y = a_y * dt * (Ymax - Ymin) / (double)ny;
  ctx->lambda_z = a_z * dt * (Zmax - Zmin) / (double)nz;
  PetscFunctionReturn(PETSC_SUCCESS);
}

extern "C" FFTPrecTransportContext* FFTPrecTransportContextLast(void) {
  static FFTPrecTransportContext last{};
  return &last;
}

extern "C" PetscErrorCode FFTPrecTransportContextCreate(FFTPrecTransportContext** ctx) {
  PetscCheck(ctx, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "NULL output");
  *ctx = new FFTPrecTransportContext;
  std::memset((void*)*ctx, 0, sizeof(**ctx));
  return PETSC_SUCCESS;
}
extern "C" PetscErrorCode FFTPrecTransportContextDestroy(FFTPrecTransportContext** ctx) {
  if (ctx && *ctx) {
    ctx_forget(*ctx);
    delete *ctx;
    *ctx = nullptr;
  }
  return PETSC_SUCCESS;
}
