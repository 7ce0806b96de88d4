"""Implicit advection-diffusion on a Cartesian grid: the operator, the circulant FFT PCSHELL of
its symbol inside the stand-in KSPGMRES, and the direct solver (include/diffusion_equation.h,
csrc/diffusion_cartesian.cpp).  The mirror of transport.py for the operator the reference's to-do
list asks for next.

Both libraries hold these functions.  The default is the complex-scalar one; ``real=True`` runs
the real-scalar library (PetscScalar = double, fields of N doubles, the real-data plan behind the
PCSHELL).  Each function picks its binding (_boundary.COMPLEX or REAL) once and runs one body.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from ._boundary import COMPLEX, PETSC_COMM_SELF, REAL
from ._lib_ext import AdvDiffConfig, AdvDiffResult

BC_WALL, BC_PERIODIC = 0, 1
PC_NONE, PC_FFT, PC_FFT_UPWIND = 0, 1, 2

_BC = {"wall": BC_WALL, "periodic": BC_PERIODIC}
_PC = {"none": PC_NONE, "fft": PC_FFT, "fft_upwind": PC_FFT_UPWIND}


def _d3(v) -> ctypes.Array:
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def _binding(real: bool):
    return REAL if real else COMPLEX


def advdiff_csr(dims: Sequence[int], h: Sequence[float], dt: float, a: Sequence[float], nu: float,
                bc: str | int = "wall", shift: float = 0.0, real: bool = False):
    """(rowptr, col, val) of shift*I + dt (a . grad - nu lap) on the grid (host only): upwind
    advection with the conservative sign plus the centred 7-point diffusion; bc 'wall' skips the
    border faces, 'periodic' gives the circulant the FFT preconditioner inverts.  Bad arguments
    raise CirculantError with the library's message from either library (real=True used to raise a
    bare ValueError, when the real-scalar module had no check())."""
    B = _binding(real)
    nx, ny, nz = (int(v) for v in dims)
    n = nx * ny * nz
    b = _BC[bc] if isinstance(bc, str) else int(bc)
    rowptr = np.empty(n + 1, dtype=np.int64)
    col = np.empty(7 * n, dtype=np.int64)
    val = np.empty(7 * n, dtype=np.complex128)
    nnz = ctypes.c_int64()
    P64 = ctypes.POINTER(ctypes.c_int64)
    B.check(B.lib().cfp_advdiff_csr(nx, ny, nz, _d3(h), float(dt), _d3(a), float(nu), b, float(shift),
                                    rowptr.ctypes.data_as(P64), col.ctypes.data_as(P64),
                                    val.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(nnz)))
    k = nnz.value
    return rowptr, col[:k].copy(), val[:k].copy()


def operator(dims: Sequence[int], h: Sequence[float], dt: float, a: Sequence[float], nu: float,
             bc: str | int = "wall", comm: int = PETSC_COMM_SELF, real: bool = False):
    """computeAdvectionDiffusionMatrixCartesianAIJ: dt (a . grad - nu lap) as a stand-in AIJ Mat
    (no MatShift), of the complex library or with real=True of the real-scalar one."""
    B = _binding(real)
    nx, ny, nz = (int(v) for v in dims)
    b = _BC[bc] if isinstance(bc, str) else int(bc)
    hdl = ctypes.c_void_p()
    B.call(B.lib().computeAdvectionDiffusionMatrixCartesianAIJ(int(comm), nx, ny, nz, _d3(h), float(dt), _d3(a),
                                                               float(nu), b, ctypes.byref(hdl)))
    return B.Mat(hdl)


def config(n: int | Sequence[int] = 32, real: bool = False, **kw) -> AdvDiffConfig:
    """cfp_advdiff_config_default ([-0.5, 0.5]^3, a = (1, 0, 0), nu = 0.01, dt = 0.01, one step,
    precision 1e-8, the FFT PCSHELL, walls) with keyword overrides: pc='none'|'fft'|'fft_upwind',
    bc='wall'|'periodic', steps=ntmax, device=True/False, plus any AdvDiffConfig field."""
    cfg = AdvDiffConfig()
    dims = (int(n),) * 3 if np.isscalar(n) else tuple(int(v) for v in n)
    _binding(real).lib().cfp_advdiff_config_default(ctypes.byref(cfg), dims[0])
    cfg.nx, cfg.ny, cfg.nz = dims
    for k, v in kw.items():
        if k == "pc":
            cfg.pc = _PC[v] if isinstance(v, str) else int(v)
        elif k == "bc":
            cfg.bc = _BC[v] if isinstance(v, str) else int(v)
        elif k == "steps":
            cfg.ntmax = int(v)
            cfg.tmax = 1e300
        elif k == "device":
            cfg.on_device = 1 if v else 0
        elif k in ("xmin", "xmax", "a"):
            setattr(cfg, k, _d3(v))
        else:
            if not hasattr(cfg, k):
                raise KeyError(k)
            setattr(cfg, k, v)
    return cfg


def _run(name: str, cfg: AdvDiffConfig, return_field: bool, real: bool):
    B = _binding(real)
    res = AdvDiffResult()
    n = int(cfg.nx * cfg.ny * cfg.nz)
    out = np.empty(n, dtype=B.dtype) if return_field else None
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if out is not None else None
    B.call(getattr(B.lib(), name)(ctypes.byref(cfg), ctypes.byref(res), ptr))
    d = res.as_dict()
    if out is not None:  # this rank's rows (all of them on one rank)
        out = out[:d["nlocal"]].copy()
    return (d, out) if return_field else d


def run(cfg: AdvDiffConfig, return_field: bool = False, real: bool = False):
    """AdvectionDiffusionGMRES: the implicit time loop with the stand-in GMRES and PCNONE or the
    diffusion PCSHELL; returns the result dict (and the final field when asked: N complex values,
    or N doubles with real=True, the real-scalar library).  When PETSC_COMM_WORLD has several ranks
    (petsc.set_comm_world) the field is this rank's rows res['rstart'] .. + res['nlocal']."""
    return _run("AdvectionDiffusionGMRES", cfg, return_field, real)


def run_direct(cfg: AdvDiffConfig, return_field: bool = False, real: bool = False):
    """AdvectionDiffusionFFTDirect: one PetscFft3DDiffusionSolver(ctx, Un, Un) per implicit step
    (the periodic operator); real=True: the real-scalar library."""
    return _run("AdvectionDiffusionFFTDirect", cfg, return_field, real)


def pc_shell(ctx, upwind: bool = False):
    """A PC of type PCSHELL with the diffusion callbacks registered on ctx (setupFFTPrec3DDiffusion,
    applyFFT3DPrecDiffusion, destroyFFTPrec3DDiffusion; PC.shell picks them by ctx's type) and set
    up.  On PETSC_COMM_WORLD of several ranks the FFT matrix is this rank's z slab and ctx.Diag its
    z-planes of the symbol.  upwind=True: setupFFTPrec3DDiffusionUpwind, the operator's symbol for
    a velocity of either sign."""
    return COMPLEX.PC.shell(ctx, upwind).setup()


# the complex binding's reference-named functions (petsc_real exports the real binding's)
context = COMPLEX.diffusion_context
StructuredContext = COMPLEX.structured_diffusion_context
PetscFft3DDiffusionSolver = COMPLEX.PetscFft3DDiffusionSolver
