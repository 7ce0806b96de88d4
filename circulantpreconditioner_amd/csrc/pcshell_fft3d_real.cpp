// pcshell_fft3d_real.cpp -- the PETSc-named boundary of include/pcshell_fft3d.h for a PETSc
// built with real scalars (PetscScalar = double, !PETSC_USE_COMPLEX): the reference's real
// branches of src/FftLinearSolver_3D.c (:6-78 VecPointwiseDivideForRealFFT, :166-190 solve_3D
// with the r2c MATFFTW) and src/PCSHELLFft_3D.cxx (:10-99).  Compiled with -DCFP_REAL_SCALAR
// into libcirculant_fft_real.so, beside the real-scalar stand-in PETSc (petsc_mini.cpp).
//
// Layouts (FFTW's r2c conventions, which a real-scalar MATFFTW uses; third-party semantics):
//   - the grid side of FFT_MAT (b, X, b_cartesien): N = nx ny nz reals, x fastest;
//   - the spectral side (Diag, b_hat, MatMult's output): the half spectrum [nz][ny][nx/2 + 1]
//     of complex values stored as interleaved (re, im) reals, NS = 2 (nx/2 + 1) ny nz reals.
// Arithmetic: the correct real solve X = C^{-1} b = (1/N) c2r( r2c(b) ./ Diag_half ), i.e. the
// complex build's result for real b and real lambda.  The reference's real branch divides only
// the first 2 (size/4 + 1) entries (:54) and scales by 2/size (:186); neither is reproduced
// (parity is against the correct real arithmetic, the oracle's solve of b).
//
// One rank: the register-symbol path runs the real plan (cfp_rplan: r2c rows, half-spectrum
// passes, c2r; 3 sweeps at 128^3 and 256^3) where it supports the grid, else the complex plan on
// b promoted to complex (one extra read and write of N complex values).  An explicit Diag (any
// change to the Diag setup made) takes the complex plan with the Hermitian extension of the
// half-spectrum Diag.  The diffusion boundary (diffusion_cartesian.cpp, include/diffusion_equation.h)
// sets the advection-diffusion symbol on both plans through pc_set_advdiff_symbol below and takes
// the same paths.
//
// Several ranks (r05; the reference's real branch runs on PETSC_COMM_WORLD
// like the complex one, src/FftLinearSolver_3D.c:6-78,176,186 and src/PCSHELLFft_3D.cxx:34-35):
// the FFT matrix is backed by the complex z-slab plan (include/circulant_fft_dist.h) on b promoted
// to complex.  Every Vec holds its rank's z-planes: the grid side nzl ny nx reals, the spectral
// side FFTW-MPI's non-transposed r2c slab, [nzl][ny][nx/2 + 1] complex.  The half spectrum's
// Hermitian extension would need the X(-kz) planes of another rank, so the c2r side instead
// pads each row locally (cfp_half_spectrum_pad: weight 2 on the paired columns, 0 above nx/2),
// whose real part after the backward transform is the same c2r.
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstring>
#include <vector>

#include "../../include/circulant_fft.h"
#include "../../include/circulant_fft_real.h"
#include "../../include/pcshell_fft3d.h"
#include "pcshell_common.h"

#if defined(PETSC_USE_COMPLEX)
#error "pcshell_fft3d_real.cpp is the real-scalar boundary: build it with -DCFP_REAL_SCALAR (stand-in) or against a real-scalar PETSc"
#endif

namespace {
using namespace cfp_pc;

struct RShell : ShellBase {
  RShell() : ShellBase(kShellMagic) {}
  // plan (the base's complex plan): transforms, explicit Diag, grids cfp_rplan lacks.  Several
  // ranks: the complex slab plan (slab.plan) on this rank's z-planes, nl grid reals.
  PetscInt N = 1, NS = 2;       // grid reals, half-spectrum reals
  PetscInt nsl = 2;             // this rank's half-spectrum reals (one rank: NS)
  cfp_rplan_t rplan = nullptr;  // real plan (NULL where it does not support the grid)
  double* zbuf = nullptr;       // N complex: promoted b / spectrum
  double* fbuf = nullptr;       // N complex: the full (Hermitian-extended) explicit Diag
  double lam[3] = {0, 0, 0};    // lam_version: rplan is valid only at that symbol version
};

PetscErrorCode ensure_bufs(RShell* s, bool full_diag) {
  const size_t bytes = 2 * sizeof(double) * (size_t)s->nl;
  if (!s->zbuf) PetscCheck(hipMalloc(&s->zbuf, bytes) == hipSuccess, PETSC_COMM_SELF, PETSC_ERR_MEM, "work buffer");
  if (full_diag && !s->fbuf)
    PetscCheck(hipMalloc(&s->fbuf, bytes) == hipSuccess, PETSC_COMM_SELF, PETSC_ERR_MEM, "Diag buffer");
  return PETSC_SUCCESS;
}

// MatMult: y = r2c(x) (FFTW_FORWARD, unnormalised), the half spectrum
PetscErrorCode rfft_mult(Mat A, Vec x, Vec y) {
  RShell* s;
  PetscCall(shell_of(A, &s));
  PetscCall(check_size(x, s->nl, "MatMult: x has the wrong size (n_x n_y n_z reals)"));
  PetscCall(check_size(y, s->nsl, "MatMult: y has the wrong size (2 (n_x/2 + 1) n_y n_z reals)"));
  PetscCall(ensure_bufs(s, s->slab.plan != nullptr));
  DevIn in;
  DevOut out;
  PetscCall(in.get(x, s->nl));
  PetscCall(out.get(y, s->nsl));
  Stream q;
  int rc = cfp_real_to_complex(in.ptr(), s->zbuf, s->nl, q.st);
  double* spec = s->zbuf;
  if (s->slab.plan) {  // natural slab out (FFTW-MPI's non-transposed layout): the half per plane
    if (!rc) rc = cfp_dist_plan_forward(s->slab.plan, s->zbuf, s->fbuf, q.st);
    spec = s->fbuf;
  } else if (!rc) {
    rc = cfp_plan_forward(s->plan, s->zbuf, s->zbuf, q.st);
  }
  if (!rc) rc = cfp_half_spectrum_extract(spec, out.ptr(), s->dims[0], s->dims[1], s->nzl, q.st);
  if (!rc) rc = cfp_stream_sync(q.st);
  PetscCall(out.put());
  PetscCall(in.put());
  CFPCALL(rc);
  return PETSC_SUCCESS;
}
// MatMultTranspose: x = c2r(y) (FFTW_BACKWARD, unnormalised) of a Hermitian half spectrum
PetscErrorCode rfft_mult_transpose(Mat A, Vec y, Vec x) {
  RShell* s;
  PetscCall(shell_of(A, &s));
  PetscCall(check_size(y, s->nsl, "MatMultTranspose: x has the wrong size (2 (n_x/2 + 1) n_y n_z reals)"));
  PetscCall(check_size(x, s->nl, "MatMultTranspose: y has the wrong size (n_x n_y n_z reals)"));
  PetscCall(ensure_bufs(s, s->slab.plan != nullptr));
  DevIn in;
  DevOut out;
  PetscCall(in.get(y, s->nsl));
  PetscCall(out.get(x, s->nl));
  Stream q;
  int rc;
  if (s->slab.plan) {  // row-local padding instead of the extension (its -kz planes live elsewhere)
    rc = cfp_half_spectrum_pad(in.ptr(), nullptr, s->zbuf, s->dims[0], s->dims[1] * s->nzl, q.st);
    if (!rc) rc = cfp_dist_plan_backward(s->slab.plan, s->zbuf, s->fbuf, q.st);
    if (!rc) rc = cfp_complex_real_part(s->fbuf, out.ptr(), s->nl, 1.0, q.st);
  } else {
    rc = cfp_half_spectrum_extend(in.ptr(), s->zbuf, s->dims[0], s->dims[1], s->dims[2], q.st);
    if (!rc) rc = cfp_plan_backward(s->plan, s->zbuf, s->zbuf, q.st);
    if (!rc) rc = cfp_complex_real_part(s->zbuf, out.ptr(), s->N, 1.0, q.st);
  }
  if (!rc) rc = cfp_stream_sync(q.st);
  PetscCall(out.put());
  PetscCall(in.put());
  CFPCALL(rc);
  return PETSC_SUCCESS;
}
PetscErrorCode rfft_destroy(Mat A) {
  RShell* s;
  PetscCall(shell_of(A, &s));
  if (s->plan) cfp_plan_destroy(s->plan);
  if (s->rplan) cfp_rplan_destroy(s->rplan);
  slab_destroy(&s->slab);
  if (s->zbuf) hipFree(s->zbuf);
  if (s->fbuf) hipFree(s->fbuf);
  s->magic = 0;
  delete s;
  return PETSC_SUCCESS;
}

PetscErrorCode ensure_transport_symbol(RShell* s, const double lam[3]) {
  if (s->has_lam && s->symbol_version() == s->lam_version && std::memcmp(s->lam, lam, sizeof(s->lam)) == 0)
    return PETSC_SUCCESS;
  const double l6[6] = {lam[0], 0.0, lam[1], 0.0, lam[2], 0.0};
  if (s->slab.plan) {
    CFPCALL(cfp_dist_plan_set_symbol_transport(s->slab.plan, l6));
    ++s->dist_version;
  } else {
    CFPCALL(cfp_plan_set_symbol_transport(s->plan, l6));
  }
  if (s->rplan) CFPCALL(cfp_rplan_set_symbol_transport(s->rplan, lam));
  std::memcpy(s->lam, lam, sizeof(s->lam));
  s->has_lam = true;
  s->lam_version = s->symbol_version();
  return PETSC_SUCCESS;
}

// rplan holds the complex plan's current symbol: the shell set both, last, by either setter
// (ensure_transport_symbol's lam / lam_version, the diffusion boundary's ad / ad_version)
bool rplan_current(const RShell* s) {
  const uint64_t v = s->symbol_version();
  return v == s->lam_version || (s->has_ad && v == s->ad_version);
}

// X = C^{-1} b with the plan's own symbol (own) or the half-spectrum Diag given; b may be X
PetscErrorCode rshell_apply(RShell* s, Vec X, Vec b, bool own, Vec Diag) {
  PetscCall(ensure_bufs(s, !own));
  DevIn bin, din;
  DevOut xout;
  PetscCall(bin.get(b, s->nl));
  if (!own) PetscCall(din.get(Diag, s->nsl));
  PetscCall(xout.get(X, s->nl));
  Stream q;
  int rc;
  if (s->slab.plan) {  // the complex slab plan on the promoted slab; its exchanges are host-driven
    rc = cfp_real_to_complex(bin.ptr(), s->zbuf, s->nl, q.st);
    if (own) {
      if (!rc) rc = cfp_dist_plan_use_diag(s->slab.plan, 0);
      if (!rc) rc = cfp_dist_plan_apply(s->slab.plan, s->zbuf, s->zbuf, q.st);
      if (!rc) rc = cfp_complex_real_part(s->zbuf, xout.ptr(), s->nl, 1.0, q.st);
    } else {  // (1/N) c2r(r2c(b) ./ Diag): forward, divide the half and pad per row, backward
      if (!rc) rc = cfp_dist_plan_forward(s->slab.plan, s->zbuf, s->fbuf, q.st);
      if (!rc) rc = cfp_half_spectrum_pad(nullptr, din.ptr(), s->fbuf, s->dims[0], s->dims[1] * s->nzl, q.st);
      if (!rc) rc = cfp_dist_plan_backward(s->slab.plan, s->fbuf, s->zbuf, q.st);
      if (!rc) rc = cfp_complex_real_part(s->zbuf, xout.ptr(), s->nl, 1.0 / (double)s->N, q.st);
    }
    if (!rc) rc = cfp_stream_sync(q.st);
  } else if (own && s->rplan && rplan_current(s)) {  // the real plan: 8-byte grid values end to end
    rc = cfp_rplan_apply(s->rplan, bin.ptr(), xout.ptr(), q.st);
  } else {  // the complex plan on the promoted b, real part out (x is real for a Hermitian symbol)
    rc = cfp_real_to_complex(bin.ptr(), s->zbuf, s->N, q.st);
    if (!rc && own) rc = cfp_plan_apply(s->plan, s->zbuf, s->zbuf, q.st);
    if (!rc && !own) rc = cfp_half_spectrum_extend(din.ptr(), s->fbuf, s->dims[0], s->dims[1], s->dims[2], q.st);
    if (!rc && !own) rc = cfp_plan_apply_with_diag(s->plan, s->fbuf, s->zbuf, s->zbuf, q.st);
    if (!rc) rc = cfp_complex_real_part(s->zbuf, xout.ptr(), s->N, 1.0, q.st);
  }
  // staged host sides, and the shared work buffers of the promoted path, need the result now
  if (!rc && (q.wait || bin.tmp || xout.tmp || din.tmp)) rc = cfp_stream_sync(q.st);
  PetscCall(xout.put());
  if (!own) PetscCall(din.put());
  PetscCall(bin.put());
  CFPCALL(rc);
  return PETSC_SUCCESS;
}

// the half-spectrum symbol 1 + sum_d lam_d c_d(k_d) on the host, planes kz in [z0, z0 + nzl);
// c_d: the axes' 1-D symbols (n_d interleaved complex values each), lam_d their weights
std::vector<double> half_symbol(const PetscInt d[3], const std::vector<double> c[3], const double lam[3], PetscInt z0,
                                PetscInt nzl) {
  const PetscInt nx = d[0], ny = d[1], M = nx / 2 + 1;
  std::vector<double> h(2 * (size_t)(M * ny * nzl));
  for (PetscInt kz = z0; kz < z0 + nzl; ++kz)
    for (PetscInt ky = 0; ky < ny; ++ky)
      for (PetscInt kx = 0; kx < M; ++kx) {
        const size_t i = 2 * (size_t)(((kz - z0) * ny + ky) * M + kx);
        h[i] = 1.0 + lam[0] * c[0][2 * kx] + lam[1] * c[1][2 * ky] + lam[2] * c[2][2 * kz];
        h[i + 1] = lam[0] * c[0][2 * kx + 1] + lam[1] * c[1][2 * ky + 1] + lam[2] * c[2][2 * kz + 1];
      }
  return h;
}

}  // namespace

const int cfp_pc::kShellMagic = 0x52464654;  // "RFFT"
// the real apply is timed by the stand-in KSP's own events (not a 3-sweep-only apply)
const bool cfp_pc::kPlanApplyIsWholePCApply = false;

// MatCreateFFT(comm, ndim, dims, MATFFTW) of a real-scalar PETSc (src/PCSHELLFft_3D.cxx:34-35):
// columns = the N reals of the grid, rows = the half spectrum's NS reals
extern "C" PetscErrorCode MatCreateFFTHIP(MPI_Comm comm, PetscInt ndim, const PetscInt dims[], Mat* A) {
  RShell* s = new RShell;
  PetscErrorCode e = shell_create_plan(s, comm, ndim, dims, A);
  if (e) {
    delete s;
    return e;
  }
  const PetscInt* d = s->dims;
  s->N = d[0] * d[1] * d[2];
  s->NS = 2 * (d[0] / 2 + 1) * d[1] * d[2];
  s->nsl = 2 * (d[0] / 2 + 1) * d[1] * s->nzl;
  int dev = 0;
  hipGetDevice(&dev);
  if (s->plan && cfp_rplan_create(&s->rplan, d[0], d[1], d[2], dev) != CFP_SUCCESS) s->rplan = nullptr;
  return shell_create_mat(s, comm, s->nsl, s->nl, s->NS, s->N, rfft_mult, rfft_mult_transpose, rfft_destroy, A);
}

// real-scalar build only: the real plan behind the matrix (NULL where it lacks the grid)
extern "C" PetscErrorCode MatFFTHIPGetRealPlan(Mat A, cfp_rplan_t* plan) {
  RShell* s;
  PetscCall(shell_of(A, &s));
  *plan = s->rplan;
  return PETSC_SUCCESS;
}

// build_diag_mat_vec_3D, :136-164, real scalars: the c_d_hat are the 1-D r2c half spectra
// (2 (n_d/2 + 1) reals, a 1-D real MATFFTW's MatMult of build_transport_col), Diag the 3-D half
// spectrum; the mirrored halves of c_y, c_z come from c(n - k) = conj c(k).
extern "C" PetscErrorCode build_diag_mat_vec_3D(Vec Diag, Vec cx, Vec cy, Vec cz, PetscInt nx, PetscInt ny,
                                                PetscInt nz, PetscScalar lx, PetscScalar ly, PetscScalar lz) {
  PetscFunctionBeginUser;
  const PetscInt M = nx / 2 + 1;
  // a distributed Diag holds its rank's whole z-planes of the half spectrum
  PetscInt Ng, nloc, lo;
  PetscCall(VecGetSize(Diag, &Ng));
  PetscCall(VecGetLocalSize(Diag, &nloc));
  PetscCall(VecGetOwnershipRange(Diag, &lo, NULL));
  PetscCheck(Ng == 2 * M * ny * nz, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ,
             "build_diag_mat_vec_3D: Diag size != 2 (n_x/2 + 1) n_y n_z");
  PetscCheck(lo % (2 * M * ny) == 0 && nloc % (2 * M * ny) == 0, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ,
             "build_diag_mat_vec_3D: a distributed Diag must hold whole z-planes");
  const PetscInt z0 = lo / (2 * M * ny), nzl = nloc / (2 * M * ny);
  PetscCall(check_size(cx, 2 * (nx / 2 + 1), "build_diag_mat_vec_3D: c_x_hat size != 2 (n_x/2 + 1)"));
  PetscCall(check_size(cy, 2 * (ny / 2 + 1), "build_diag_mat_vec_3D: c_y_hat size != 2 (n_y/2 + 1)"));
  PetscCall(check_size(cz, 2 * (nz / 2 + 1), "build_diag_mat_vec_3D: c_z_hat size != 2 (n_z/2 + 1)"));
  const PetscScalar *ax, *ay, *az;
  PetscCall(VecGetArrayRead(cx, &ax));
  PetscCall(VecGetArrayRead(cy, &ay));
  PetscCall(VecGetArrayRead(cz, &az));
  const auto full = [](const PetscScalar* c, PetscInt n, PetscInt k) {
    return k <= n / 2 ? std::complex<double>(c[2 * k], c[2 * k + 1])
                      : std::complex<double>(c[2 * (n - k)], -c[2 * (n - k) + 1]);
  };
  PetscScalar* d;
  PetscCall(VecGetArrayWrite(Diag, &d));
  for (PetscInt kz = z0; kz < z0 + nzl; ++kz)
    for (PetscInt ky = 0; ky < ny; ++ky)
      for (PetscInt kx = 0; kx < M; ++kx) {
        const std::complex<double> v = 1.0 + lx * full(ax, nx, kx) + ly * full(ay, ny, ky) + lz * full(az, nz, kz);
        const size_t i = 2 * (size_t)(((kz - z0) * ny + ky) * M + kx);
        d[i] = v.real();
        d[i + 1] = v.imag();
      }
  PetscCall(VecRestoreArrayWrite(Diag, &d));
  PetscCall(VecRestoreArrayRead(cz, &az));
  PetscCall(VecRestoreArrayRead(cy, &ay));
  PetscCall(VecRestoreArrayRead(cx, &ax));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// solve_3D, :166-190 (real scalars): X = (1/size) c2r( r2c(b) ./ Diag ) -- the correct real
// solve (see the file header for the reference's loop bound and 2/size); b_hat is untouched.
extern "C" PetscErrorCode solve_3D(Mat FFT_MAT, Vec X, Vec Diag, Vec b, Vec b_hat, PetscInt size) {
  PetscFunctionBeginUser;
  (void)b_hat;
  RShell* s;
  PetscCall(shell_of(FFT_MAT, &s));
  PetscCheck(size == s->N, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ, "solve_3D: size != number of grid cells of FFT_MAT");
  PetscCall(check_size(X, s->nl, "solve_3D: X has the wrong size"));
  PetscCall(check_size(b, s->nl, "solve_3D: b has the wrong size"));
  PetscCall(check_size(Diag, s->nsl, "solve_3D: Diag has the wrong size (2 (n_x/2 + 1) n_y n_z reals)"));
  bool own = false;
  PetscCall(s->diag_is_own_symbol(Diag, &own));
  if (s->slab.plan) {  // every rank takes the same path (the apply holds collectives)
    double f = own ? 0.0 : 1.0;
    PetscCall(comm_max(s->slab.comm, s->nranks, &f, 1));
    own = f == 0.0;
  }
  ++(own ? s->solves_own : s->solves_diag);
  PetscCall(rshell_apply(s, X, b, own, Diag));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// FftTransportSolver, :218-264 (the symbol of real lambdas, cached; FFT_MAT survives)
extern "C" PetscErrorCode FftTransportSolver(PetscInt nx, PetscInt ny, PetscInt nz, PetscScalar lx, PetscScalar ly,
                                             PetscScalar lz, Vec X, Vec b, Mat FFT_MAT) {
  PetscFunctionBeginUser;
  RShell* s;
  PetscCall(shell_of(FFT_MAT, &s));
  PetscCheck(s->dims[0] == nx && s->dims[1] == ny && s->dims[2] == nz, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ,
             "FftTransportSolver: grid dims do not match FFT_MAT");
  const double lam[3] = {lx, ly, lz};
  PetscCall(ensure_transport_symbol(s, lam));
  PetscCall(check_size(X, s->nl, "FftTransportSolver: X has the wrong size"));
  PetscCall(check_size(b, s->nl, "FftTransportSolver: b has the wrong size"));
  PetscCall(rshell_apply(s, X, b, true, nullptr));
  PetscFunctionReturn(PETSC_SUCCESS);
}

// X = C^{-1} b with the plans' own symbol (the diffusion direct solver)
PetscErrorCode cfp_pc::own_symbol_apply(Mat FFT_MAT, Vec X, Vec b) {
  RShell* s;
  PetscCall(shell_of(FFT_MAT, &s));
  PetscCall(check_size(X, s->nl, "own_symbol_apply: X has the wrong size"));
  PetscCall(check_size(b, s->nl, "own_symbol_apply: b has the wrong size"));
  ++s->solves_own;
  PetscCall(rshell_apply(s, X, b, true, nullptr));
  return PETSC_SUCCESS;
}

// The diffusion boundary's build-specific pieces (pcshell_common.h).  The symbol goes on the
// complex plan (grids the real plan lacks, the explicit-Diag path) and on the real plan; the
// caller (ensure_advdiff_symbol) then records ad / ad_version, which rplan_current reads.
PetscErrorCode cfp_pc::pc_set_advdiff_symbol(ShellBase* base, const double lam[6], const double mu[6], bool upwind) {
  RShell* s = static_cast<RShell*>(base);
  if (s->slab.plan) {  // several ranks: the complex slab plan on the promoted slab, as the transport apply
    if (upwind) CFPCALL(cfp_dist_plan_set_symbol_upwind(s->slab.plan, lam, mu));
    else CFPCALL(cfp_dist_plan_set_symbol_advdiff(s->slab.plan, lam, mu));
    ++s->dist_version;
    return PETSC_SUCCESS;
  }
  const double l3[3] = {lam[0], lam[2], lam[4]}, m3[3] = {mu[0], mu[2], mu[4]};
  if (upwind) {
    CFPCALL(cfp_plan_set_symbol_upwind(s->plan, lam, mu));
    if (s->rplan) CFPCALL(cfp_rplan_set_symbol_upwind(s->rplan, l3, m3));
    return PETSC_SUCCESS;
  }
  CFPCALL(cfp_plan_set_symbol_advdiff(s->plan, lam, mu));
  if (s->rplan) CFPCALL(cfp_rplan_set_symbol_advdiff(s->rplan, l3, m3));
  return PETSC_SUCCESS;
}
// Diag: the half spectrum [nz][ny][nx/2 + 1] of the symbol, from the axes' closed forms
PetscErrorCode cfp_pc::pc_advdiff_diag(ShellBase* s, Vec Diag, const double lam[6], const double mu[6]) {
  std::vector<double> c[3];
  for (int a = 0; a < 3; ++a) {
    c[a].resize(2 * (size_t)s->dims[a]);
    CFPCALL(cfp_advdiff_symbol_1d(s->dims[a], lam + 2 * a, mu + 2 * a, c[a].data()));
  }
  const double one[3] = {1.0, 1.0, 1.0};
  const std::vector<double> h = half_symbol(s->dims, c, one, s->z0, s->nzl);
  PetscScalar* d;
  PetscCall(VecGetArrayWrite(Diag, &d));
  std::memcpy(d, h.data(), sizeof(double) * h.size());
  PetscCall(VecRestoreArrayWrite(Diag, &d));
  PetscCall(s->remember_diag(Diag));
  return PETSC_SUCCESS;
}

// the solve of applyFFT3DPrecTransport (pcshell_boundary.cpp); no dots ride in a real apply
PetscErrorCode cfp_pc::pc_solve(PC, FFTPrecTransportContext* ctx, Vec X, Vec src) {
  return solve_3D(ctx->FFT_MAT, X, ctx->Diag, src, ctx->b_hat, ctx->n_x * ctx->n_y * ctx->n_z);
}
// real scalars have no fused form of applyFFT3DPrecTransportBA
PetscErrorCode cfp_pc::pc_fused_ba(PC, FFTPrecTransportContext*, Mat, Vec, Vec, bool* taken) {
  *taken = false;
  return PETSC_SUCCESS;
}

// setupFFTPrec3D, :26-84 (real scalars: Diag and b_hat are half spectra, b_cartesien N reals)
extern "C" PetscErrorCode setupFFTPrec3D(PC pc) {
  PetscFunctionBeginUser;
  FFTPrecTransportContext* ctx = nullptr;
  PetscCall(PCShellGetContext(pc, &ctx));
  PetscCheck(ctx, PETSC_COMM_SELF, PETSC_ERR_ARG_NULL, "setupFFTPrec3D: no context attached to the PC");
  PetscCheck(ctx->n_x >= 1 && ctx->n_y >= 1 && ctx->n_z >= 1, PETSC_COMM_SELF, PETSC_ERR_ARG_OUTOFRANGE,
             "setupFFTPrec3D: n_x, n_y, n_z must be >= 1");
  const PetscInt dims[3] = {ctx->n_z, ctx->n_y, ctx->n_x};
  PetscCall(MatCreateFFTHIP(PETSC_COMM_WORLD, 3, dims, &ctx->FFT_MAT));
  PetscCall(MatCreateVecsFFTW(ctx->FFT_MAT, NULL, &ctx->Diag, NULL));
  PetscCall(MatCreateVecsFFTW(ctx->FFT_MAT, &ctx->b_cartesien, &ctx->b_hat, NULL));
  RShell* s;
  PetscCall(shell_of(ctx->FFT_MAT, &s));
  const double lam[3] = {ctx->lambda_x, ctx->lambda_y, ctx->lambda_z};
  PetscCall(ensure_transport_symbol(s, lam));
  std::vector<double> c[3];  // the 1-D DFTs of the transport columns, from their closed form
  for (int a = 0; a < 3; ++a) {
    c[a].resize(2 * (size_t)s->dims[a]);
    cfp_transport_symbol_1d(s->dims[a], c[a].data());
  }
  const std::vector<double> h = half_symbol(s->dims, c, lam, s->z0, s->nzl);
  PetscScalar* d;
  PetscCall(VecGetArrayWrite(ctx->Diag, &d));
  std::memcpy(d, h.data(), sizeof(double) * h.size());
  PetscCall(VecRestoreArrayWrite(ctx->Diag, &d));
  PetscCall(s->remember_diag(ctx->Diag));
  PetscFunctionReturn(PETSC_SUCCESS);
}
