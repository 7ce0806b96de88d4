"""Implicit advection-diffusion on a Cartesian grid: the operator, the circulant FFT PCSHELL of
its symbol inside the stand-in KSPGMRES, and the direct solver (include/diffusion_equation.h,
csrc/diffusion_cartesian.cpp).  The mirror of transport.py for the operator the reference's to-do
list asks for next.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from ._lib import check, lib
from ._lib_ext import AdvDiffConfig, AdvDiffResult, PetscScalar, StructuredDiffusionContext
from .petsc import PETSC_COMM_SELF, Mat, PetscCall, Vec

BC_WALL, BC_PERIODIC = 0, 1
PC_NONE, PC_FFT = 0, 1

_BC = {"wall": BC_WALL, "periodic": BC_PERIODIC}
_PC = {"none": PC_NONE, "fft": PC_FFT}


def _d3(v) -> ctypes.Array:
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def advdiff_csr(dims: Sequence[int], h: Sequence[float], dt: float, a: Sequence[float], nu: float,
                bc: str | int = "wall", shift: float = 0.0):
    """(rowptr, col, val) of shift*I + dt (a . grad - nu lap) on the grid (host only): upwind
    advection with the conservative sign plus the centred 7-point diffusion; bc 'wall' skips the
    border faces, 'periodic' gives the circulant the FFT preconditioner inverts."""
    nx, ny, nz = (int(v) for v in dims)
    n = nx * ny * nz
    b = _BC[bc] if isinstance(bc, str) else int(bc)
    rowptr = np.empty(n + 1, dtype=np.int64)
    col = np.empty(7 * n, dtype=np.int64)
    val = np.empty(7 * n, dtype=np.complex128)
    nnz = ctypes.c_int64()
    P64 = ctypes.POINTER(ctypes.c_int64)
    check(lib().cfp_advdiff_csr(nx, ny, nz, _d3(h), float(dt), _d3(a), float(nu), b, float(shift),
                                rowptr.ctypes.data_as(P64), col.ctypes.data_as(P64),
                                val.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(nnz)))
    k = nnz.value
    return rowptr, col[:k].copy(), val[:k].copy()


def operator(dims: Sequence[int], h: Sequence[float], dt: float, a: Sequence[float], nu: float,
             bc: str | int = "wall", comm: int = PETSC_COMM_SELF) -> Mat:
    """computeAdvectionDiffusionMatrixCartesianAIJ: dt (a . grad - nu lap) as a stand-in AIJ Mat
    (no MatShift)."""
    nx, ny, nz = (int(v) for v in dims)
    b = _BC[bc] if isinstance(bc, str) else int(bc)
    hdl = ctypes.c_void_p()
    PetscCall(lib().computeAdvectionDiffusionMatrixCartesianAIJ(int(comm), nx, ny, nz, _d3(h), float(dt), _d3(a),
                                                                float(nu), b, ctypes.byref(hdl)))
    return Mat(hdl)


def config(n: int | Sequence[int] = 32, **kw) -> AdvDiffConfig:
    """cfp_advdiff_config_default ([-0.5, 0.5]^3, a = (1, 0, 0), nu = 0.01, dt = 0.01, one step,
    precision 1e-8, the FFT PCSHELL, walls) with keyword overrides: pc='none'|'fft',
    bc='wall'|'periodic', steps=ntmax, device=True/False, plus any AdvDiffConfig field."""
    cfg = AdvDiffConfig()
    dims = (int(n),) * 3 if np.isscalar(n) else tuple(int(v) for v in n)
    lib().cfp_advdiff_config_default(ctypes.byref(cfg), dims[0])
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


def _run(fn, cfg: AdvDiffConfig, return_field: bool):
    res = AdvDiffResult()
    n = int(cfg.nx * cfg.ny * cfg.nz)
    out = np.empty(n, dtype=np.complex128) if return_field else None
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if out is not None else None
    PetscCall(fn(ctypes.byref(cfg), ctypes.byref(res), ptr))
    d = res.as_dict()
    return (d, out) if return_field else d


def run(cfg: AdvDiffConfig, return_field: bool = False):
    """AdvectionDiffusionGMRES: the implicit time loop with the stand-in GMRES and PCNONE or the
    diffusion PCSHELL; returns the result dict (and the final field when asked)."""
    return _run(lib().AdvectionDiffusionGMRES, cfg, return_field)


def run_direct(cfg: AdvDiffConfig, return_field: bool = False):
    """AdvectionDiffusionFFTDirect: one PetscFft3DDiffusionSolver(ctx, Un, Un) per implicit step
    (the periodic operator)."""
    return _run(lib().AdvectionDiffusionFFTDirect, cfg, return_field)


def StructuredContext(n_x, n_y, n_z, a_x, a_y, a_z, nu, dt, delta_x, delta_y, delta_z, FFT_MAT: Mat
                      ) -> StructuredDiffusionContext:
    c = StructuredDiffusionContext()
    c.n_x, c.n_y, c.n_z = int(n_x), int(n_y), int(n_z)
    for name, v in (("a_x", a_x), ("a_y", a_y), ("a_z", a_z), ("nu", nu), ("dt", dt), ("delta_x", delta_x),
                    ("delta_y", delta_y), ("delta_z", delta_z)):
        setattr(c, name, PetscScalar.of(v))
    c.FFT_MAT = FFT_MAT.h
    return c


def PetscFft3DDiffusionSolver(customCtx: StructuredDiffusionContext, b: Vec, x: Vec) -> None:
    PetscCall(lib().PetscFft3DDiffusionSolver(customCtx, b.h, x.h))
