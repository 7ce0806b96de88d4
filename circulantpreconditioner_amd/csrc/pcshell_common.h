// pcshell_common.h -- helpers shared by the PCSHELL implementations (pcshell_boundary.cpp,
// pcshell_fft3d.cpp, pcshell_fft3d_real.cpp, wave_system.cpp): cfp error -> PETSc error, device
// views of Vecs (device arrays used in place, host arrays staged through a temporary device
// buffer; apply_on_device: one PCApply on such views), slab plans on a communicator, and -- for
// the transport PCSHELL only -- the part of an FFT matrix that both scalar builds share and the
// interface between the scalar-independent boundary (pcshell_boundary.cpp) and the scalar build
// behind it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/circulant_fft.h"
#include "../../include/circulant_fft_dist.h"
#include "../../include/petsc_mini.h"

struct FFTPrecTransportContext;  // include/pcshell_fft3d.h

namespace cfp_pc {

inline PetscErrorCode cfp_err(int rc, const char* where) {
  if (rc == CFP_SUCCESS) return PETSC_SUCCESS;
#ifndef CFP_WITH_PETSC
  return PetscErrorSet(rc, where, cfp_last_error());
#else
  SETERRQ(PETSC_COMM_SELF, rc, "%s: %s", where, cfp_last_error());
#endif
}

// The stream an apply on device Vecs is ordered on, and whether it must be waited for: the
// stand-in's Vec stream, stream-ordered like PETSc's VECHIP operations (the next Vec operation,
// e.g. GMRES's VecMAXPY, queues behind the apply; a host read synchronises), so PCApply costs no
// host round trip.  Built against a real PETSc: the default stream, waited for.
inline void device_stream(void** st, bool* wait) {
#ifdef CFP_WITH_PETSC
  *st = nullptr;
  *wait = true;
#else
  VecMiniGetStream(st);
  *wait = false;
#endif
}
// that stream and the final wait, looked up where an apply starts
struct Stream {
  void* st = nullptr;
  bool wait = true;
  Stream() { device_stream(&st, &wait); }
};

// Device view of a Vec for the duration of one solve: device arrays are used in place,
// host arrays are staged through a temporary device buffer (PCIe-inclusive path).
struct DevIn {
  Vec v = nullptr;
  const PetscScalar* arr = nullptr;
  PetscMemType mt = PETSC_MEMTYPE_HOST;
  void* tmp = nullptr;
  const double* ptr() const { return tmp ? (const double*)tmp : (const double*)arr; }
  PetscErrorCode get(Vec vec, PetscInt n) {
    v = vec;
    PetscCall(VecGetArrayReadAndMemType(v, &arr, &mt));
    if (mt == PETSC_MEMTYPE_HOST) {
      PetscCheck(hipMalloc(&tmp, sizeof(PetscScalar) * (size_t)n) == hipSuccess, PETSC_COMM_SELF, PETSC_ERR_MEM,
                 "staging buffer");
      PetscCheck(hipMemcpy(tmp, arr, sizeof(PetscScalar) * (size_t)n, hipMemcpyHostToDevice) == hipSuccess,
                 PETSC_COMM_SELF, PETSC_ERR_LIB, "host to device copy");
    }
    return PETSC_SUCCESS;
  }
  PetscErrorCode put() {
    if (tmp) hipFree(tmp);
    tmp = nullptr;
    return VecRestoreArrayReadAndMemType(v, &arr);
  }
};
struct DevOut {
  Vec v = nullptr;
  PetscScalar* arr = nullptr;
  PetscMemType mt = PETSC_MEMTYPE_HOST;
  void* tmp = nullptr;
  PetscInt n = 0;
  double* ptr() const { return tmp ? (double*)tmp : (double*)arr; }
  PetscErrorCode get(Vec vec, PetscInt nn) {
    v = vec;
    n = nn;
    PetscCall(VecGetArrayWriteAndMemType(v, &arr, &mt));
    if (mt == PETSC_MEMTYPE_HOST)
      PetscCheck(hipMalloc(&tmp, sizeof(PetscScalar) * (size_t)n) == hipSuccess, PETSC_COMM_SELF, PETSC_ERR_MEM,
                 "staging buffer");
    return PETSC_SUCCESS;
  }
  PetscErrorCode put() {
    if (tmp) {
      hipDeviceSynchronize();
      PetscCheck(hipMemcpy(arr, tmp, sizeof(PetscScalar) * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess,
                 PETSC_COMM_SELF, PETSC_ERR_LIB, "device to host copy");
      hipFree(tmp);
      tmp = nullptr;
    }
    return VecRestoreArrayWriteAndMemType(v, &arr);
  }
};

// One PCApply on the device views of b and x (n entries each): run(b, x, stream, staged) queues
// the work.  Device Vecs are ordered on the Vec stream without a host round trip (device_stream);
// with a staged host Vec (staged: the default stream) the work is waited for, since put() copies
// the buffers back and frees them.  `where` names the caller in the error.
template <class Run>
PetscErrorCode apply_on_device(Vec b, Vec x, PetscInt n, const char* where, Run run) {
  DevIn in;
  DevOut out;
  PetscCall(in.get(b, n));
  PetscCall(out.get(x, n));
  const bool staged = in.tmp || out.tmp;
  void* st = nullptr;
  bool wait = true;
  if (!staged) device_stream(&st, &wait);
  int rc = run(in.ptr(), out.ptr(), st, staged);
  if (rc == CFP_SUCCESS && (wait || staged)) rc = cfp_stream_sync(st);
  PetscCall(out.put());
  PetscCall(in.put());
  return cfp_err(rc, where);
}

// ------------------------------------------------------------------ slab plans on a communicator
// The z-slab plan behind an FFT matrix of several ranks (the complex build, pcshell_fft3d.cpp, and
// the real-scalar build, pcshell_fft3d_real.cpp): the reference's MATFFTW on PETSC_COMM_WORLD
// (src/PCSHELLFft_3D.cxx:34-35).
#ifdef CFP_WITH_PETSC
// Exchange piece over a real MPI communicator (cfp_dist_exchange_fn): host-staged
// MPI_Alltoall of the [size][count] pieces.
struct MpiExchange {
  MPI_Comm comm;
  int size;
  std::vector<char> hs, hr;
};
inline int mpi_exchange(void* user, const double* src, double* dst, int64_t chunk, int64_t off, int64_t count,
                        void* stream) {
  MpiExchange* m = (MpiExchange*)user;
  const size_t bytes = 16 * (size_t)count, pitch = 16 * (size_t)chunk;
  if (bytes > (size_t)INT32_MAX) return 1;
  m->hs.resize(bytes * m->size);
  m->hr.resize(bytes * m->size);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpy2DAsync(m->hs.data(), bytes, src + 2 * off, pitch, bytes, m->size, hipMemcpyDeviceToHost, st) ||
      hipStreamSynchronize(st))
    return 1;
  if (MPI_Alltoall(m->hs.data(), (int)bytes, MPI_BYTE, m->hr.data(), (int)bytes, MPI_BYTE, m->comm)) return 1;
  if (hipMemcpy2DAsync(dst + 2 * off, pitch, m->hr.data(), bytes, bytes, m->size, hipMemcpyHostToDevice, st) ||
      hipStreamSynchronize(st))
    return 1;
  return 0;
}
#endif

// max over the ranks of an FFT matrix' communicator (one rank: itself)
inline PetscErrorCode comm_max(MPI_Comm comm, int nranks, double* v, int n) {
  if (nranks == 1) return PETSC_SUCCESS;
#ifdef CFP_WITH_PETSC
  PetscCallMPI(MPI_Allreduce(MPI_IN_PLACE, v, n, MPI_DOUBLE, MPI_MAX, comm));
#else
  PetscCall(PetscMiniAllreduce(comm, v, n, PETSCMINI_OP_MAX));
#endif
  return PETSC_SUCCESS;
}

// This rank's slab plan of the nx x ny x nz grid, its exchanges over `comm`: an RCCL communicator
// of the stand-in -> grouped ncclSend / ncclRecv on it; a callback communicator -> the caller's
// collectives, host-staged; a real MPI communicator -> host-staged MPI_Alltoall.  *resolved: the
// communicator to release (stand-in: PETSC_COMM_WORLD resolved, retained); *mx: the MPI exchange
// state (CFP_WITH_PETSC).
struct SlabBacking {
  cfp_dist_plan_t plan = nullptr;
  MPI_Comm comm = PETSC_COMM_SELF;
  void* mx = nullptr;
};
inline PetscErrorCode slab_create(MPI_Comm comm, int nranks, int rank, const PetscInt dims[3], int dev,
                                  SlabBacking* sb) {
#ifdef CFP_WITH_PETSC
  PetscCall(cfp_err(cfp_dist_plan_create_external(&sb->plan, dims[0], dims[1], dims[2], nranks, rank, dev), __func__));
  MpiExchange* m = new MpiExchange{comm, nranks, {}, {}};
  sb->mx = m;
  sb->comm = comm;
  PetscCall(cfp_err(cfp_dist_plan_set_exchange(sb->plan, mpi_exchange, m), __func__));
#else
  MPI_Comm c;
  PetscCall(PetscMiniCommResolve(comm, &c));
  void* nccl = nullptr;
  PetscCall(PetscMiniCommGetNCCL(c, &nccl));
  if (nccl) {
    PetscCall(cfp_err(cfp_dist_plan_create_with_comm(&sb->plan, dims[0], dims[1], dims[2], nranks, rank, nccl, dev),
                      __func__));
  } else {
    PetscCall(cfp_err(cfp_dist_plan_create_external(&sb->plan, dims[0], dims[1], dims[2], nranks, rank, dev), __func__));
    PetscCall(cfp_err(cfp_dist_plan_set_exchange(sb->plan, PetscMiniCommExchange, (void*)(intptr_t)c), __func__));
  }
  PetscCall(PetscMiniCommRetain(c));  // PetscMiniCommDestroy refuses until slab_destroy releases it
  sb->comm = c;
#endif
  return PETSC_SUCCESS;
}
inline void slab_destroy(SlabBacking* sb) {
  if (sb->plan) {
    cfp_dist_plan_destroy(sb->plan);
#ifndef CFP_WITH_PETSC
    PetscMiniCommRelease(sb->comm);
#endif
  }
#ifdef CFP_WITH_PETSC
  delete (MpiExchange*)sb->mx;
#endif
  sb->plan = nullptr;
  sb->mx = nullptr;
}

inline PetscErrorCode check_size(Vec v, PetscInt n, const char* name) {
  PetscInt m;
  PetscCall(VecGetLocalSize(v, &m));
  PetscCheck(m == n, PETSC_COMM_SELF, PETSC_ERR_ARG_SIZ, name);
  return PETSC_SUCCESS;
}

// ------------------------------------------------------------------ the transport FFT matrix
// What the MATSHELL context of both scalar builds holds (FFTShell of pcshell_fft3d.cpp, RShell of
// pcshell_fft3d_real.cpp derive from it): the grid, the plan behind it and the bookkeeping that
// decides whether a Diag still is the plan's own symbol.  Hidden, like everything below: a process
// may hold both libraries, and neither may bind to (or export) the other's.
#define CFP_INTERNAL __attribute__((visibility("hidden")))
struct CFP_INTERNAL ShellBase {
  int magic;                     // the build's kShellMagic while the matrix lives
  PetscInt dims[3] = {1, 1, 1};  // n_x, n_y, n_z
  int nranks = 1, rank = 0;
  cfp_plan_t plan = nullptr;     // one rank: the complex plan
  SlabBacking slab;              // several ranks: this rank's z slab (slab.plan) and its communicator
  PetscInt z0 = 0, nzl = 1, nl = 1;  // this rank's z-planes [z0, z0 + nzl) and grid values (one rank: all)
  uint64_t dist_version = 0;     // symbol version of slab.plan (its setters are called by its shell only)
  bool has_lam = false;
  uint64_t lam_version = 0;      // the symbol version right after the shell's lam was set
  // the Diag setupFFTPrec3D materialised from the plan's symbol of version diag_version: its
  // object id and its state right after that write (0 id: none).  The version is the plan's
  // own counter (cfp_plan_symbol_version), so a symbol set on the plan directly through
  // MatFFTHIPGetPlan also invalidates the fast path.
  PetscObjectId diag_id = 0;
  PetscObjectState diag_state = 0;
  uint64_t diag_version = 0;
  PetscInt solves_own = 0, solves_diag = 0;  // solve_3D calls per path (MatFFTHIPGetSolveCounts)
  PetscInt fused_ba = 0;                     // applyBA calls that took pc_fused_ba (MatFFTHIPGetFusedBACount)
  // the advection-diffusion numbers (lam[6], mu[6]) the diffusion boundary last set on the plan
  // (diffusion_cartesian.cpp) and the symbol version right after: equal numbers reuse the symbol
  // ad_upwind: they went through the upwind setter (the numbers kept are the caller's; the same
  // tables as the advdiff setter with the mapped pair, but a routing of their own)
  bool has_ad = false;
  bool ad_upwind = false;
  double ad[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t ad_version = 0;

  explicit ShellBase(int m) : magic(m) {}
  uint64_t symbol_version() const {
    if (slab.plan) return dist_version;
    uint64_t v = 0;
    cfp_plan_symbol_version(plan, &v);
    return v;
  }
  // Diag holds exactly the plan's current symbol (materialised by setupFFTPrec3D, untouched since)
  PetscErrorCode diag_is_own_symbol(Vec Diag, bool* own) const {
    *own = false;
    if (!diag_id || diag_version != symbol_version()) return PETSC_SUCCESS;
    PetscObjectId id;
    PetscObjectState st;
    PetscCall(PetscObjectGetId((PetscObject)Diag, &id));
    PetscCall(PetscObjectStateGet((PetscObject)Diag, &st));
    *own = id == diag_id && st == diag_state;
    return PETSC_SUCCESS;
  }
  // remember which object and state hold the symbol (solve_3D's register-symbol fast path)
  PetscErrorCode remember_diag(Vec Diag) {
    PetscCall(PetscObjectGetId((PetscObject)Diag, &diag_id));
    PetscCall(PetscObjectStateGet((PetscObject)Diag, &diag_state));
    diag_version = symbol_version();
    return PETSC_SUCCESS;
  }
};

// ---- pcshell_boundary.cpp <-> the scalar build linked beside it
// defined by the scalar build: two constants and two functions, one definition per library
extern CFP_INTERNAL const int kShellMagic;  // "FFTH" / "RFFT"
// the plan apply is the whole PCApply when no remap surrounds it (the stand-in KSP then times a
// PCApply by the plan's first and last kernel; otherwise by its own events)
extern CFP_INTERNAL const bool kPlanApplyIsWholePCApply;
// X = C^{-1} src with ctx's FFT_MAT and Diag (X may be src).  pc: the PC whose pending dots
// request (PCMiniApplyDots) may ride in the apply, NULL when X is not the PCApply's result.
CFP_INTERNAL PetscErrorCode pc_solve(PC pc, FFTPrecTransportContext* ctx, Vec X, Vec src);
// y = B A x as one fused apply, where the build has one and this PC, A and x allow it (no remaps,
// x != y: checked by the caller); *taken says whether y was written
CFP_INTERNAL PetscErrorCode pc_fused_ba(PC pc, FFTPrecTransportContext* ctx, Mat A, Vec x, Vec y, bool* taken);

// X = C^{-1} b with the plan's own symbol, whatever set it (one apply of FFT_MAT's plan; b may
// be X) -- the diffusion direct solver
CFP_INTERNAL PetscErrorCode own_symbol_apply(Mat FFT_MAT, Vec X, Vec b);
// The two build-specific pieces of the diffusion boundary (diffusion_cartesian.cpp).
// pc_set_advdiff_symbol: the advection-diffusion symbol of lam[6], mu[6] (re, im per axis) on
// every plan behind the matrix (the real build: its complex plan and its real plan, real parts;
// several ranks, both builds: slab.plan, with dist_version moved on); upwind: by the upwind setters
// (cfp_plan_set_symbol_upwind and its siblings) instead, lam of either sign.
// pc_advdiff_diag: Diag := this rank's z-planes of that symbol in the build's spectral layout
// (complex: [nzl][ny][nx]; real: the half spectrum [nzl][ny][nx/2 + 1]), remembered as the plan's
// own (remember_diag).
CFP_INTERNAL PetscErrorCode pc_set_advdiff_symbol(ShellBase* s, const double lam[6], const double mu[6],
                                                  bool upwind = false);
CFP_INTERNAL PetscErrorCode pc_advdiff_diag(ShellBase* s, Vec Diag, const double lam[6], const double mu[6]);

// defined by pcshell_boundary.cpp
CFP_INTERNAL PetscErrorCode shell_base(Mat A, ShellBase** out);  // the context of an FFT matrix of this build
CFP_INTERNAL Mat ctx_remap_back(const FFTPrecTransportContext* ctx);
// MatCreateFFTHIP in two steps, the build's own sizes and plans in between.  shell_create_plan:
// argument checks, rank and size, dims (row-major {n_z, n_y, n_x} in), then the single-GPU plan or
// this rank's z slab (needs nranks | n_z; n_y is split in FFTW-MPI's blocks of ceil(n_y / nranks)
// rows, any n_y); on failure nothing is left behind but *s.  shell_create_mat: the MATSHELL.
CFP_INTERNAL PetscErrorCode shell_create_plan(ShellBase* s, MPI_Comm comm, PetscInt ndim, const PetscInt dims[], Mat* A);
typedef PetscErrorCode (*ShellMult)(Mat, Vec, Vec);
CFP_INTERNAL PetscErrorCode shell_create_mat(ShellBase* s, MPI_Comm comm, PetscInt m, PetscInt n, PetscInt M, PetscInt N,
                                             ShellMult mult, ShellMult mult_transpose, PetscErrorCode (*destroy)(Mat),
                                             Mat* A);

template <class S>
PetscErrorCode shell_of(Mat A, S** out) {
  ShellBase* b;
  PetscCall(shell_base(A, &b));
  *out = static_cast<S*>(b);
  return PETSC_SUCCESS;
}

}  // namespace cfp_pc

#define CFPCALL(expr) PetscCall(cfp_pc::cfp_err((expr), __func__))
