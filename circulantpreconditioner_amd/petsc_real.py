"""The real-scalar PETSc boundary (PetscScalar = double): ``libcirculant_fft_real.so``.

The same PETSc-named entry points as ``petsc.py`` (include/pcshell_fft3d.h, include/petsc_mini.h)
built with -DCFP_REAL_SCALAR: a PETSc configured with real scalars, which is what the
reference's ``#if !defined(PETSC_USE_COMPLEX)`` branches compile against
(src/FftLinearSolver_3D.c:6-78, 166-190).  Vecs hold doubles; FFT_MAT maps the N reals of the
grid to FFTW's r2c half spectrum ([nz][ny][nx/2 + 1] complex as interleaved reals), which is
also the layout of Diag and b_hat (pcshell_fft3d_real.cpp).

This module is the REAL binding of ``_boundary.py`` (the classes, structs and reference-named
functions of ``petsc.py``, under the same names) plus handle-level helpers over those classes
that give and take raw ``c_void_p`` handles, as the real-scalar tests pass them straight to
``lib().X(...)``.  The library is loaded with RTLD_LOCAL and linked -Bsymbolic, so it coexists
with the complex ``libcirculant_fft.so`` in one process.  No CPU fallback: a missing library raises.
"""
from __future__ import annotations

import ctypes

from ._boundary import (ADD_VALUES, INSERT_VALUES, KSP_REASONS, MATOP_MULT, NORM_1, NORM_2,  # noqa: F401
                        NORM_INFINITY, PC_LEFT, PC_RIGHT, PETSC_COMM_SELF, PETSC_COMM_WORLD, PETSC_DEFAULT,
                        REAL as B, PetscError)
from ._lib import REAL_LIB_PATH as LIB_PATH  # noqa: F401
from ._lib_ext import AdvDiffConfig, AdvDiffResult, AIJInfo, FFTPrecWaveRealContext  # noqa: F401

# the names of petsc.py, bound to this library
lib, PetscCall, fn, set_comm_world = B.lib, B.call, B.fn, B.set_comm_world
Vec, Comm, Mat, PC, KSP = B.Vec, B.Comm, B.Mat, B.PC, B.KSP
FFTPrecTransportContext, FFTPrecDiffusionContext = B.structs.FFTPrecTransportContext, B.structs.FFTPrecDiffusionContext
StructuredTransportContext = B.structs.StructuredTransportContext
StructuredDiffusionContext = B.structs.StructuredDiffusionContext

getFFTPrec3DContext, make_context, diffusion_context = B.getFFTPrec3DContext, B.make_context, B.diffusion_context
context_plan, context_remap_back = B.context_plan, B.context_remap_back
applyFFT3DPrecTransport, applyFFT3DPrecTransportBA = B.applyFFT3DPrecTransport, B.applyFFT3DPrecTransportBA
setupFFTPrec3D, destroyFFTPrec3D = B.setupFFTPrec3D, B.destroyFFTPrec3D
solve_3D, build_transport_col, build_diag_mat_vec_3D = B.solve_3D, B.build_transport_col, B.build_diag_mat_vec_3D
FftTransportSolver, Fft3DTransportSolver = B.FftTransportSolver, B.Fft3DTransportSolver
Fft2DTransportSolver, Fft1DTransportSolver = B.Fft2DTransportSolver, B.Fft1DTransportSolver
StructuredContext, PetscFft3DTransportSolver = B.StructuredContext, B.PetscFft3DTransportSolver
structured_diffusion_context, PetscFft3DDiffusionSolver = B.structured_diffusion_context, B.PetscFft3DDiffusionSolver


# ---- handle-level helpers: raw c_void_p handles in and out, one or two lines over the classes
def mat_create_fft(dims):
    """MatCreateFFT(PETSC_COMM_WORLD, ndim, dims = {n_z, n_y, n_x} row-major, MATFFTW)."""
    return Mat.create_fft(dims).release()


def mat_create_vecs_fftw(A) -> tuple:
    return tuple(Mat.borrow(A).create_vecs(3))


def mat_aij(A_csr):
    """MatCreateSeqAIJWithArrays from a real scipy CSR matrix."""
    return Mat.aij(A_csr.indptr, A_csr.indices, A_csr.data, A_csr.shape).release()


def mat_aij_info(M) -> dict:
    return Mat.borrow(M).aij_info()


def mat_aij_format(M) -> str:
    return Mat.borrow(M).aij_format()


def mat_mult(M, x, y):
    return Mat.borrow(M).mult(x, y)


def mat_shift(M, a: float) -> None:
    Mat.borrow(M).shift(a)


def mat_destroy(M) -> None:
    Mat(M).destroy()


def mat_real_plan_mid_kernel(A) -> str:
    """The half-spectrum middle kernel of the real plan behind an FFT matrix (MatFFTHIPGetRealPlan,
    which only this library holds, then cfp_rplan_mid_kernel): 'fft', 'zrec2', or 'none' where the
    real plan lacks the grid."""
    h, k = ctypes.c_void_p(), ctypes.c_int()
    PetscCall(lib().MatFFTHIPGetRealPlan(Mat.borrow(A).h, ctypes.byref(h)))
    if not h.value:
        return "none"
    B.check(lib().cfp_rplan_mid_kernel(h, ctypes.byref(k)))
    return "zrec2" if k.value == 2 else "fft"


def pc_shell(ctx, upwind: bool = False):
    """The PCSHELL of ctx's kind (PC.shell), set up; the caller destroys the handle and keeps ctx alive."""
    return PC.shell(ctx, upwind).setup().release()
