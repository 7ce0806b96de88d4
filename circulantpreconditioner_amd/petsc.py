"""Python mirror of the reference's PETSc-facing interface, over the C ABI of the complex-scalar
library ``libcirculant_fft.so``: the COMPLEX binding of ``_boundary.py``, where the classes and
functions are written once for both scalar builds (``petsc_real.py`` is the other binding and
exports the same names; tests/test_boundary_cpu.py holds the two lists together).

The functions carry the reference's names and argument order, so the parity tests read like the
reference's own drivers:

    ctx = getFFTPrec3DContext(3, dt, N, ax, ay, az, xmin, ymin, zmin, xmax, ymax, zmax)
    pc = PC.shell(ctx)                        # PCSetType(PCSHELL) + PCShellSet*
    pc.setup()                                # setupFFTPrec3D
    pc.apply(b, x)                            # PCApply -> applyFFT3DPrecTransport
"""
from __future__ import annotations

from ._boundary import (ADD_VALUES, COMPLEX as B, INSERT_VALUES, KSP_REASONS, MATOP_MULT, NORM_1,  # noqa: F401
                        NORM_2, NORM_INFINITY, PC_LEFT, PC_RIGHT, PETSC_COMM_SELF, PETSC_COMM_WORLD, PETSC_DEFAULT,
                        PetscError)
from ._lib_ext import FFTPrecWaveContext, FFTPrecWaveRealContext, PetscScalar  # noqa: F401

lib, PetscCall, fn, set_comm_world, _S = B.lib, B.call, B.fn, B.set_comm_world, B.S
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
