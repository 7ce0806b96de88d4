// pcshell_fft3d.cpp -- the reference's PCSHELL preconditioner and direct-solver entry points
// (src/PCSHELLFft_3D.cxx, src/FftLinearSolver_3D.c), re-implemented on the HIP plan.
//
// Written only against PETSc API calls (PCShellGetContext, Vec*AndMemType, MatShell*,
// MatMult, VecSet...), so it builds against the in-tree stand-in (petsc_mini.cpp) or a real
// PETSc (-DCFP_WITH_PETSC, PETSc configured with complex scalars and HIP).
//
// The FFT matrix is a MATSHELL whose context is a cfp plan: MatMult = unnormalised forward
// 3-D DFT, MatMultTranspose = backward (the MATFFTW semantics the reference relies on).
// solve_3D divides by the Diag it is given (src/FftLinearSolver_3D.c:174).  When that Diag is
// the one setupFFTPrec3D materialised from the plan's own symbol -- same object id, the
// object state recorded after the write (PetscObjectStateGet: every write access bumps it),
// and the plan's symbol unchanged since -- the apply evaluates the symbol in registers
// instead of streaming Diag from HBM; anything else takes the explicit-Diag apply.
//
// Several ranks (the reference's MATFFTW on PETSC_COMM_WORLD, src/PCSHELLFft_3D.cxx:34-37, and
// its MPI direct-solve driver, tests/TransportEquationFFT_SphericalExplosion_impl_mpi.cxx:66,
// 100,111): the FFT matrix is backed by the z-slab plan (include/circulant_fft_dist.h), every
// Vec holds its rank's PETSC_DECIDE rows = its z-planes, and the exchanges go through the
// communicator (RCCL, or the caller's collectives).  Whether solve_3D may use the register
// symbol, and whether an explicit Diag must be moved into the z-pencil layout again, is
// decided on every rank and agreed by one all-reduce, so all ranks run the same collectives.
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "../../include/circulant_fft.h"
#include "../../include/circulant_fft_dist.h"
#include "../../include/pcshell_fft3d.h"
#include "pcshell_common.h"

namespace {
using namespace cfp_pc;

struct FFTShell : ShellBase {
  FFTShell() : ShellBase(kShellMagic) {}
  // the explicit Diag last moved into slab.plan's z-pencil layout (0 id: none)
  PetscObjectId dt_id = 0;
  PetscObjectState dt_state = 0;
  void* stage = nullptr;  // in-place host-Vec staging of the slab path (nl values)
  double lam[6] = {0, 0, 0, 0, 0, 0};
};

// MatMult / MatMultTranspose: the unnormalised 3-D DFT; several ranks: of the slab-distributed
// grid, natural slab in and out (FFTW-MPI's non-transposed layout)
PetscErrorCode fft_mult_impl(Mat A, Vec x, Vec y, bool backward) {
  FFTShell* s;
  PetscCall(shell_of(A, &s));
  const PetscInt n = s->nl;
  PetscCall(check_size(x, n, "MatMult: x has the wrong size"));
  PetscCall(check_size(y, n, "MatMult: y has the wrong size"));
  PetscCheck(x != y || !s->slab.plan, PETSC_COMM_SELF, PETSC_ERR_ARG_IDN, "MatMult: x and y must differ");
  DevIn in;
  DevOut out;
  PetscCall(in.get(x, n));
  PetscCall(out.get(y, n));
  // on the Vec stream, behind the Vec kernels that produced x (a non-blocking stream does not
  // order against the null stream), then waited for: the transforms return complete
  Stream q;
  int rc;
  if (s->slab.plan)
    rc = backward ? cfp_dist_plan_backward(s->slab.plan, in.ptr(), out.ptr(), q.st)
                  : cfp_dist_plan_forward(s->slab.plan, in.ptr(), out.ptr(), q.st);
  else
    rc = backward ? cfp_plan_backward(s->plan, in.ptr(), out.ptr(), q.st)
                  : cfp_plan_forward(s->plan, in.ptr(), out.ptr(), q.st);
  if (rc == CFP_SUCCESS) rc = cfp_stream_sync(q.st);
  PetscCall(out.put());
  PetscCall(in.put());
  CFPCALL(rc);
  return PETSC_SUCCESS;
}
PetscErrorCode fft_mult(Mat A, Vec x, Vec y) { return fft_mult_impl(A, x, y, false); }
PetscErrorCode fft_mult_transpose(Mat A, Vec x, Vec y) { return fft_mult_impl(A, x, y, true); }
PetscErrorCode fft_destroy(Mat A) {
  FFTShell* s;
  PetscCall(shell_of(A, &s));
  if (s->plan) cfp_plan_destroy(s->plan);
  slab_destroy(&s->slab);
  if (s->stage) hipFree(s->stage);
  s->magic = 0;
  delete s;
  return PETSC_SUCCESS;
}

void lam6(PetscScalar lx, PetscScalar ly, PetscScalar lz, double out[6]) {
  out[0] = std::real(lx); out[1] = std::imag(lx);
  out[2] = std::real(ly); out[3] = std::imag(ly);
  out[4] = std::real(lz); out[5] = std::imag(lz);
}

// Use (or refresh) the plan's separable transport symbol for these lambdas (App. A item 9:
// the reference rebuilds Diag on every direct-solve call; equal lambdas reuse it here).
PetscErrorCode ensure_transport_symbol(FFTShell* s, const double lam[6]) {
  if (s->has_lam && s->symbol_version() == s->lam_version && std::memcmp(s->lam, lam, sizeof(s->lam)) == 0)
    return PETSC_SUCCESS;
  if (s->slab.plan) {
    CFPCALL(cfp_dist_plan_set_symbol_transport(s->slab.plan, lam));
    ++s->dist_version;
  } else {
    CFPCALL(cfp_plan_set_symbol_transport(s->plan, lam));
  }
  std::memcpy(s->lam, lam, sizeof(s->lam));
  s->has_lam = true;
  s->lam_version = s->symbol_version();
  return PETSC_SUCCESS;
}

}  // namespace

const int cfp_pc::kShellMagic = 0x46465448;  // "FFTH"
// a device-Vec PCApply without remaps is the plan apply alone
const bool cfp_pc::kPlanApplyIsWholePCApply = true;

// ------------------------------------------------------------------ FFT matrix
// MatCreateFFT(comm, ndim, dims, MATFFTW) of the reference (src/PCSHELLFft_3D.cxx:34-35): every
// Vec holds this rank's z-planes of the grid (pcshell_common.h, shell_create_plan)
extern "C" PetscErrorCode MatCreateFFTHIP(MPI_Comm comm, PetscInt ndim, const PetscInt dims[], Mat* A) {
  FFTShell* s = new FFTShell;
  PetscErrorCode e = shell_create_plan(s, comm, ndim, dims, A);
  if (e) {
    delete s;
    return e;
  }
  const PetscInt N = s->dims[0] * s->dims[1] * s->dims[2];
  return shell_create_mat(s, comm, s->nl, s->nl, N, N, fft_mult, fft_mult_transpose, fft_destroy, A);
}

// ------------------------------------------------------------------ direct solver
// Diag[k] = 1 + lx cx[kx] + ly cy[ky] + lz cz[kz] on this rank's planes [z0, z0 + nzl) (one
// device sweep; cx, cy, cz device arrays of the full axes)
PetscErrorCode build_diag_rows(double* diag, const double* cx, const double* cy, const double* cz, PetscInt nx,
                               PetscInt ny, PetscInt z0, PetscInt nzl, const double lam[6]) {
  int rc = cfp_build_diag_3d(diag, cx, cy, cz + 2 * z0, nx, ny, nzl, lam, nullptr);
  if (rc == CFP_SUCCESS) rc = cfp_stream_sync(nullptr);
  CFPCALL(rc);
  return PETSC_SUCCESS;
}

// build_diag_mat_vec_3D, :136-164: one device sweep instead of ~4N VecSetValue calls.  A
// distributed Diag gets its rank's rows (whole z-planes); the 1-D vectors hold the full axes.
extern "C" PetscErrorCode build_diag_mat_vec_3D(Vec Diag, Vec cx, Vec cy, Vec cz, PetscInt nx, PetscInt ny,
                                                PetscInt nz, PetscScalar lx, PetscScalar ly, PetscScalar lz) {
  PetscFunctionBeginUser;
  PetscInt Ng, nloc, lo, hi;
  PetscCall(VecGetSize(Diag, &Ng));
  PetscCall(VecGetLocalSize(Diag, &nloc));
  PetscCall(VecGetOwnershipRange(Diag, &lo, &hi));
  PetscCheck(Ng == nx * ny * nz, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ, "build_diag_mat_vec_3D: Diag size != n_x n_y n_z");
  PetscCheck(lo % (nx * ny) == 0 && nloc % (nx * ny) == 0, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ,
             "build_diag_mat_vec_3D: a distributed Diag must hold whole z-planes");
  PetscCall(check_size(cx, nx, "build_diag_mat_vec_3D: c_x_hat size != n_x"));
  PetscCall(check_size(cy, ny, "build_diag_mat_vec_3D: c_y_hat size != n_y"));
  PetscCall(check_size(cz, nz, "build_diag_mat_vec_3D: c_z_hat size != n_z"));
  DevIn a, b, c;
  DevOut d;
  PetscCall(a.get(cx, nx));
  PetscCall(b.get(cy, ny));
  PetscCall(c.get(cz, nz));
  PetscCall(d.get(Diag, nloc));
  double lam[6];
  lam6(lx, ly, lz, lam);
  PetscErrorCode e = build_diag_rows(d.ptr(), a.ptr(), b.ptr(), c.ptr(), nx, ny, lo / (nx * ny), nloc / (nx * ny), lam);
  PetscCall(d.put());  // a write access: Diag's state moves on, so no plan treats it as its own symbol
  PetscCall(c.put());
  PetscCall(b.put());
  PetscCall(a.put());
  PetscCall(e);
  PetscFunctionReturn(PETSC_SUCCESS);
}

// One apply of FFT_MAT's plan, X = (1/N) IDFT(DFT(b) ./ symbol): the register symbol (own) or
// the explicit Diag (single rank: streamed; slab plan: the z-pencil copy already set).  b may be
// X (the direct solver's Un, Un).  Host Vecs are staged: single rank through the plan's own
// persistent buffer (cfp_plan_apply_host), slab plan through the shell's; those applies, and
// every slab apply (its exchanges are host-driven), return complete.  A single-rank apply on
// device Vecs is ordered on the Vec stream (cfp_pc::device_stream).
// ex (single rank, register symbol, b != X): the fused Krylov step (cfp_plan_apply_ex); ex->fused
// stays -1 when this apply could not take it.
PetscErrorCode shell_apply(FFTShell* s, Vec X, Vec b, bool own, Vec Diag, cfp_apply_ex_t* ex = nullptr) {
  const PetscInt n = s->nl;
  DevIn din;
  if (!own && !s->slab.plan) PetscCall(din.get(Diag, n));
  if (s->slab.plan) CFPCALL(cfp_dist_plan_use_diag(s->slab.plan, own ? 0 : 1));
  // device Vecs: on the Vec stream, behind the Vec kernels that produced b (the slab apply too,
  // which then waits: its exchanges are host-driven)
  Stream q;
  if (ex) ex->fused = -1;
  auto dev_apply = [&](const double* in, double* out) -> int {
    if (s->slab.plan) return cfp_dist_plan_apply(s->slab.plan, in, out, q.st);
    if (ex && own && in != out) return cfp_plan_apply_ex(s->plan, in, out, q.st, ex);
    return own ? cfp_plan_apply(s->plan, in, out, q.st) : cfp_plan_apply_with_diag(s->plan, din.ptr(), in, out, q.st);
  };
  // device Vecs: wait only where the caller cannot rely on stream order
  auto dev_sync = [&]() -> int {
    if (s->slab.plan || q.wait || din.tmp) return cfp_stream_sync(q.st);  // din.tmp: a staged host Diag is freed below
    return CFP_SUCCESS;
  };
  int rc;
  int stage_err = 0;  // slab path: failed host staging (PETSC_ERR_MEM / PETSC_ERR_LIB)
  if (b == X) {
    // in-place direct solve (PetscFft3DTransportSolver(ctx, Un, Un)): read-write access
    PetscScalar* arr;
    PetscMemType mt;
    PetscCall(VecGetArrayAndMemType(X, &arr, &mt));
    double* p = (double*)arr;
    if (mt == PETSC_MEMTYPE_HOST && !s->slab.plan) {
      // staged through the plan's persistent device buffer; both copies are checked, so a
      // failed copy returns PETSC_ERR_LIB instead of leaving stale data behind
      rc = own ? cfp_plan_apply_host(s->plan, p, p) : cfp_plan_apply_with_diag_host(s->plan, din.ptr(), p, p);
    } else if (mt == PETSC_MEMTYPE_HOST) {
      const size_t bytes = sizeof(PetscScalar) * (size_t)n;
      rc = CFP_SUCCESS;
      if (!s->stage && hipMalloc(&s->stage, bytes) != hipSuccess) stage_err = PETSC_ERR_MEM;
      if (!stage_err && hipMemcpy(s->stage, p, bytes, hipMemcpyHostToDevice) != hipSuccess) stage_err = PETSC_ERR_LIB;
      if (!stage_err) rc = dev_apply((const double*)s->stage, (double*)s->stage);
      if (!stage_err && !rc) rc = cfp_stream_sync(q.st);
      if (!stage_err && !rc && hipMemcpy(p, s->stage, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        stage_err = PETSC_ERR_LIB;
    } else {
      rc = dev_apply(p, p);
      if (rc == CFP_SUCCESS) rc = dev_sync();
    }
    PetscCall(VecRestoreArrayAndMemType(X, &arr));
  } else {
    DevIn bin;
    DevOut xout;
    PetscCall(bin.get(b, n));
    PetscCall(xout.get(X, n));
    rc = dev_apply(bin.ptr(), xout.ptr());
    // a staged host side (DevIn/DevOut copies) needs the result now
    if (rc == CFP_SUCCESS) rc = (bin.tmp || xout.tmp) ? cfp_stream_sync(q.st) : dev_sync();
    PetscCall(xout.put());
    PetscCall(bin.put());
  }
  if (!own && !s->slab.plan) PetscCall(din.put());
  PetscCheck(!stage_err, PETSC_COMM_SELF, stage_err, "solve: host staging of the slab failed");
  CFPCALL(rc);
  return PETSC_SUCCESS;
}

// solve_3D, :166-190: X = (1/size) F^T( F(b) ./ Diag ), fused into one 3- or 5-launch apply.
// b_hat is the reference's scratch vector; the fused apply needs none and leaves it untouched.
// ex: the stand-in KSP's dots of X, computed with the apply where it can (shell_apply).
PetscErrorCode solve_impl(Mat FFT_MAT, Vec X, Vec Diag, Vec b, PetscInt size, cfp_apply_ex_t* ex) {
  PetscFunctionBeginUser;
  FFTShell* s;
  PetscCall(shell_of(FFT_MAT, &s));
  const PetscInt N = s->dims[0] * s->dims[1] * s->dims[2];
  PetscCheck(size == N, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ, "solve_3D: size != number of grid cells of FFT_MAT");
  PetscCall(check_size(X, s->nl, "solve_3D: X has the wrong size"));
  PetscCall(check_size(b, s->nl, "solve_3D: b has the wrong size"));
  PetscCall(check_size(Diag, s->nl, "solve_3D: Diag has the wrong size"));
  // the plan's own symbol, if Diag was materialised from it and nothing has written to it since
  bool own = false;
  PetscCall(s->diag_is_own_symbol(Diag, &own));
  if (s->slab.plan) {
    // every rank must take the same path (the apply holds collectives): agree on it, and on
    // whether the explicit Diag has to be moved into the z-pencil layout again
    PetscObjectId id;
    PetscObjectState st;
    PetscCall(PetscObjectGetId((PetscObject)Diag, &id));
    PetscCall(PetscObjectStateGet((PetscObject)Diag, &st));
    double f[2] = {own ? 0.0 : 1.0, (id == s->dt_id && st == s->dt_state) ? 0.0 : 1.0};
    PetscCall(comm_max(s->slab.comm, s->nranks, f, 2));
    own = f[0] == 0.0;
    if (!own && f[1] != 0.0) {
      DevIn din;
      PetscCall(din.get(Diag, s->nl));
      Stream q;
      int rc = cfp_dist_plan_set_diag(s->slab.plan, din.ptr(), q.st);
      if (rc == CFP_SUCCESS) rc = cfp_stream_sync(q.st);
      PetscCall(din.put());
      CFPCALL(rc);
      s->dt_id = id;
      s->dt_state = st;
    }
  }
  ++(own ? s->solves_own : s->solves_diag);
  PetscCall(shell_apply(s, X, b, own, Diag, ex));
  PetscFunctionReturn(PETSC_SUCCESS);
}
extern "C" PetscErrorCode solve_3D(Mat FFT_MAT, Vec X, Vec Diag, Vec b, Vec b_hat, PetscInt size) {
  (void)b_hat;
  return solve_impl(FFT_MAT, X, Diag, b, size, nullptr);
}

#ifndef CFP_WITH_PETSC
// The stand-in KSP's pending dots request (PCMiniApplyDots) as the post-op of a plan apply -- taken
// only when the plan computes them inside its sweeps (with the stencil `pre`, if any); otherwise
// the KSP's own multi-dot is the same work
cfp_apply_ex_t* take_dots(PC pc, cfp_apply_ex_t* ex, PCMiniApplyDots** req, const cfp_stencil_t* pre = nullptr) {
  *req = nullptr;
  if (PCMiniGetApplyDots(pc, req) || !*req || (*req)->done || (*req)->nv < 1 || (*req)->nv > 8) {
    *req = nullptr;
    return nullptr;
  }
  FFTPrecTransportContext* ctx = nullptr;
  FFTShell* s = nullptr;
  int fusable = 0;
  if (PCShellGetContext(pc, &ctx) || !ctx || !ctx->FFT_MAT || shell_of(ctx->FFT_MAT, &s) || !s->plan ||
      cfp_plan_apply_ex_fusable(s->plan, pre, (int)(*req)->nv, &fusable) || !fusable) {
    *req = nullptr;
    return nullptr;
  }
  ex->post_nv = (int)(*req)->nv;
  for (PetscInt j = 0; j < (*req)->nv; ++j) ex->post_v[j] = (const double*)(*req)->v[j];
  ex->post_out = (*req)->out;
  return ex;
}
#endif

// FftTransportSolver, :218-264.  The reference builds three 1-D FFTs of the transport column
// and the Kronecker Diag on every call, then destroys the caller's FFT_MAT (App. A item 6).
// Here the closed-form symbol of the same columns is set once per lambda and FFT_MAT survives.
extern "C" PetscErrorCode FftTransportSolver(PetscInt nx, PetscInt ny, PetscInt nz, PetscScalar lx, PetscScalar ly,
                                             PetscScalar lz, Vec X, Vec b, Mat FFT_MAT) {
  PetscFunctionBeginUser;
  FFTShell* s;
  PetscCall(shell_of(FFT_MAT, &s));
  PetscCheck(s->dims[0] * s->dims[1] * s->dims[2] == nx * ny * nz, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ,
             "FftTransportSolver: n_x n_y n_z does not match FFT_MAT");
  PetscCheck(s->dims[0] == nx && s->dims[1] == ny && s->dims[2] == nz, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ,
             "FftTransportSolver: grid dims do not match FFT_MAT");
  double lam[6];
  lam6(lx, ly, lz, lam);
  PetscCall(ensure_transport_symbol(s, lam));
  PetscCall(check_size(X, s->nl, "FftTransportSolver: X has the wrong size"));
  PetscCall(check_size(b, s->nl, "FftTransportSolver: b has the wrong size"));
  PetscCall(shell_apply(s, X, b, true, nullptr));
  PetscFunctionReturn(PETSC_SUCCESS);
}

PetscErrorCode cfp_pc::own_symbol_apply(Mat FFT_MAT, Vec X, Vec b) {
  FFTShell* s;
  PetscCall(shell_of(FFT_MAT, &s));
  PetscCall(check_size(X, s->nl, "own_symbol_apply: X has the wrong size"));
  PetscCall(check_size(b, s->nl, "own_symbol_apply: b has the wrong size"));
  ++s->solves_own;
  PetscCall(shell_apply(s, X, b, true, nullptr));
  return PETSC_SUCCESS;
}

// the diffusion boundary's build-specific pieces (pcshell_common.h): one complex plan; Diag is the
// plan's own closed-form symbol on the full grid
PetscErrorCode cfp_pc::pc_set_advdiff_symbol(ShellBase* s, const double lam[6], const double mu[6], bool upwind) {
  if (s->slab.plan) {  // several ranks: this rank's z slab
    if (upwind) CFPCALL(cfp_dist_plan_set_symbol_upwind(s->slab.plan, lam, mu));
    else CFPCALL(cfp_dist_plan_set_symbol_advdiff(s->slab.plan, lam, mu));
    ++s->dist_version;
  } else if (upwind) {
    CFPCALL(cfp_plan_set_symbol_upwind(s->plan, lam, mu));
  } else {
    CFPCALL(cfp_plan_set_symbol_advdiff(s->plan, lam, mu));
  }
  return PETSC_SUCCESS;
}
PetscErrorCode cfp_pc::pc_advdiff_diag(ShellBase* s, Vec Diag, const double lam[6], const double mu[6]) {
  DevOut d;
  PetscCall(d.get(Diag, s->nl));
  int rc = CFP_SUCCESS;
  if (s->slab.plan) {  // this rank's z-planes [nzl][ny][nx] of the closed form, from the axes' parts
    const PetscInt nx = s->dims[0], ny = s->dims[1];
    std::vector<double> c[3];
    for (int a = 0; a < 3 && !rc; ++a) {
      c[a].resize(2 * (size_t)s->dims[a]);
      rc = cfp_advdiff_symbol_1d(s->dims[a], lam + 2 * a, mu + 2 * a, c[a].data());
    }
    std::vector<double> h(2 * (size_t)s->nl);
    for (PetscInt kz = s->z0; kz < s->z0 + s->nzl && !rc; ++kz)
      for (PetscInt ky = 0; ky < ny; ++ky)
        for (PetscInt kx = 0; kx < nx; ++kx) {
          const size_t i = 2 * (size_t)(((kz - s->z0) * ny + ky) * nx + kx);
          h[i] = 1.0 + c[0][2 * kx] + c[1][2 * ky] + c[2][2 * kz];
          h[i + 1] = c[0][2 * kx + 1] + c[1][2 * ky + 1] + c[2][2 * kz + 1];
        }
    if (!rc && hipMemcpy(d.ptr(), h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice) != hipSuccess)
      rc = CFP_ERR_LIB;
  } else {
    rc = cfp_plan_get_diag(s->plan, d.ptr(), nullptr);
    if (rc == CFP_SUCCESS) rc = cfp_stream_sync(nullptr);
  }
  PetscCall(d.put());
  CFPCALL(rc);
  PetscCall(s->remember_diag(Diag));
  return PETSC_SUCCESS;
}

// ------------------------------------------------------------------ PCSHELL callbacks
// the solve of applyFFT3DPrecTransport (pcshell_boundary.cpp)
PetscErrorCode cfp_pc::pc_solve(PC pc, FFTPrecTransportContext* ctx, Vec X, Vec src) {
  const PetscInt N = ctx->n_x * ctx->n_y * ctx->n_z;
  cfp_apply_ex_t* ex = nullptr;
#ifndef CFP_WITH_PETSC
  // the stand-in KSP may ask for dots of x with its basis (PCMiniApplyDots): they ride in the apply
  cfp_apply_ex_t exd{};
  PCMiniApplyDots* req = nullptr;
  if (pc) ex = take_dots(pc, &exd, &req);
#endif
  PetscCall(solve_impl(ctx->FFT_MAT, X, ctx->Diag, src, N, ex));
#ifndef CFP_WITH_PETSC
  if (req && exd.fused >= 0) req->done = PETSC_TRUE;
#endif
  return PETSC_SUCCESS;
}

// The fused step of applyFFT3DPrecTransportBA (pcshell_boundary.cpp).  One rank, register symbol,
// and A the stand-in AIJ in row-class form: A x is formed inside the apply's first sweep
// (cfp_apply_ex_t, P1 reads x once) instead of a MatMult sweep into `work` -- config 3's transport
// operator couples cells along x only, so the whole stencil of a row is in the rows P1 loads.
PetscErrorCode cfp_pc::pc_fused_ba(PC pc, FFTPrecTransportContext* ctx, Mat A, Vec x, Vec y, bool* taken) {
  *taken = false;
#ifndef CFP_WITH_PETSC
  FFTShell* s;
  PetscCall(shell_of(ctx->FFT_MAT, &s));
  bool own = false;
  PetscCall(s->diag_is_own_symbol(ctx->Diag, &own));
  PetscInt am, an;
  PetscCall(MatGetSize(A, &am, &an));
  const PetscInt N = ctx->n_x * ctx->n_y * ctx->n_z;
  if (s->slab.plan || !own || am != N || an != N) return PETSC_SUCCESS;
  PetscBool has = PETSC_FALSE, xl = PETSC_FALSE;
  PetscMiniDia dia;
  PetscCall(PetscMiniMatAIJGetDia(A, ctx->n_x, &has, &xl, &dia));
  if (!has) return PETSC_SUCCESS;
  cfp_stencil_t st;
  int fusable = 0;
  std::memset((void*)&st, 0, sizeof(st));
  st.cls = dia.cls;
  st.mask = dia.mask;
  st.tab = (const double*)dia.tab;
  for (int k = 0; k < 8; ++k) st.off[k] = dia.off[k];
  st.nd = dia.nd;
  st.ncls = dia.ncls;
  st.x_local = xl ? 1 : 0;
  st.cls_x = dia.cls_x;
  CFPCALL(cfp_plan_apply_ex_fusable(s->plan, &st, 0, &fusable));
  if (!fusable) return PETSC_SUCCESS;  // the caller's MatMult, then the apply: the same kernels
  cfp_apply_ex_t ex{};
  PCMiniApplyDots* req = nullptr;
  take_dots(pc, &ex, &req, &st);
  ex.pre = &st;
  ++s->solves_own;
  PetscCall(shell_apply(s, y, x, true, nullptr, &ex));
  PetscCheck(ex.fused >= 0, PETSC_COMM_SELF, PETSC_ERR_PLIB, "applyFFT3DPrecTransportBA: fused apply not taken");
  if (req) req->done = PETSC_TRUE;
  ++s->fused_ba;
  *taken = true;
#endif
  return PETSC_SUCCESS;
}

// setupFFTPrec3D, :26-84: FFT matrix, work vectors and Diag (materialised from the closed form
// of the 1-D DFTs of the transport columns, which is what :39-69 compute with FFTW).
extern "C" PetscErrorCode setupFFTPrec3D(PC pc) {
  PetscFunctionBeginUser;
  FFTPrecTransportContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  PetscCheck(ctx, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "setupFFTPrec3D: no context attached to the PC");
  PetscCheck(ctx->n_x >= 1 && ctx->n_y >= 1 && ctx->n_z >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE,
             "setupFFTPrec3D: n_x, n_y, n_z must be >= 1");
  // all three dims always (the reference passes spaceDim with {n_z, n_y, n_x}, which picks the
  // wrong axes for spaceDim = 2, App. A item 7)
  const PetscInt dims[3] = {ctx->n_z, ctx->n_y, ctx->n_x};
  PetscCall(MatCreateFFTHIP(PETSC_COMM_WORLD, 3, dims, &ctx->FFT_MAT));
  PetscCall(MatCreateVecsFFTW(ctx->FFT_MAT, NULL, &ctx->Diag, NULL));
  PetscCall(MatCreateVecsFFTW(ctx->FFT_MAT, &ctx->b_cartesien, &ctx->b_hat, NULL));
  FFTShell* s;
  PetscCall(shell_of(ctx->FFT_MAT, &s));
  double lam[6];
  lam6(ctx->lambda_x, ctx->lambda_y, ctx->lambda_z, lam);
  PetscCall(ensure_transport_symbol(s, lam));
  DevOut d;
  PetscCall(d.get(ctx->Diag, s->nl));
  PetscErrorCode e = PETSC_SUCCESS;
  if (s->slab.plan) {  // this rank's z-planes of the closed-form Diag
    const PetscInt nx = ctx->n_x, ny = ctx->n_y, nz = ctx->n_z;
    std::vector<double> h(2 * (size_t)(nx + ny + nz));
    int rc = cfp_transport_symbol_1d(nx, h.data());
    if (!rc) rc = cfp_transport_symbol_1d(ny, h.data() + 2 * nx);
    if (!rc) rc = cfp_transport_symbol_1d(nz, h.data() + 2 * (nx + ny));
    void* t = nullptr;
    if (!rc && hipMalloc(&t, sizeof(double) * h.size()) != hipSuccess) rc = CFP_ERR_MEM;
    if (!rc && hipMemcpy(t, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice) != hipSuccess) rc = CFP_ERR_LIB;
    PetscInt lo;
    PetscCall(VecGetOwnershipRange(ctx->Diag, &lo, NULL));
    const double* td = (const double*)t;
    if (!rc) e = build_diag_rows(d.ptr(), td, td + 2 * nx, td + 2 * (nx + ny), nx, ny, lo / (nx * ny),
                                 s->nl / (nx * ny), lam);
    if (t) hipFree(t);
    if (rc) e = cfp_err(rc, "setupFFTPrec3D");
  } else {
    int rc = cfp_plan_get_diag(s->plan, d.ptr(), nullptr);
    if (rc == CFP_SUCCESS) rc = cfp_stream_sync(nullptr);
    e = cfp_err(rc, "setupFFTPrec3D");
  }
  PetscCall(d.put());
  PetscCall(e);
#ifndef CFP_WITH_PETSC
  // the operator's row-class form for applyFFT3DPrecTransportBA, built (and its x-locality
  // checked) now rather than inside the first timed solve
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
  PetscCall(s->remember_diag(ctx->Diag));
  PetscFunctionReturn(PETSC_SUCCESS);
}
