"""Implicit advection-diffusion on a Cartesian grid: the operator, the circulant FFT PCSHELL of
its symbol inside the stand-in KSPGMRES, and the direct solver (include/diffusion_equation.h,
csrc/diffusion_cartesian.cpp).  The mirror of transport.py for the operator the reference's to-do
list asks for next.

Both libraries hold these functions.  The default is the complex-scalar one; ``real=True`` runs
the real-scalar library (petsc_real.py: PetscScalar = double, fields of N doubles, the real-data
plan behind the PCSHELL).
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from ._lib import check, lib
from ._lib_ext import AdvDiffConfig, AdvDiffResult, PetscScalar, StructuredDiffusionContext
from .petsc import PETSC_COMM_SELF, Mat, PetscCall, Vec

BC_WALL, BC_PERIODIC = 0, 1
PC_NONE, PC_FFT, PC_FFT_UPWIND = 0, 1, 2

_BC = {"wall": BC_WALL, "periodic": BC_PERIODIC}
_PC = {"none": PC_NONE, "fft": PC_FFT, "fft_upwind": PC_FFT_UPWIND}


def _d3(v) -> ctypes.Array:
    return (ctypes.c_double * 3)(*[float(x) for x in v])


def _real_lib():
    from . import petsc_real
    return petsc_real


def advdiff_csr(dims: Sequence[int], h: Sequence[float], dt: float, a: Sequence[float], nu: float,
                bc: str | int = "wall", shift: float = 0.0, real: bool = False):
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
    fn = _real_lib().lib().cfp_advdiff_csr if real else lib().cfp_advdiff_csr
    rc = fn(nx, ny, nz, _d3(h), float(dt), _d3(a), float(nu), b, float(shift), rowptr.ctypes.data_as(P64),
            col.ctypes.data_as(P64), val.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(nnz))
    if rc and real:
        raise ValueError(f"cfp_advdiff_csr: bad arguments (code {rc})")
    check(rc)
    k = nnz.value
    return rowptr, col[:k].copy(), val[:k].copy()


def operator(dims: Sequence[int], h: Sequence[float], dt: float, a: Sequence[float], nu: float,
             bc: str | int = "wall", comm: int = PETSC_COMM_SELF, real: bool = False):
    """computeAdvectionDiffusionMatrixCartesianAIJ: dt (a . grad - nu lap) as a stand-in AIJ Mat
    (no MatShift).  real=True: the real-scalar library's Mat handle (petsc_real.mat_mult,
    petsc_real.mat_destroy)."""
    nx, ny, nz = (int(v) for v in dims)
    b = _BC[bc] if isinstance(bc, str) else int(bc)
    hdl = ctypes.c_void_p()
    if real:
        R = _real_lib()
        R.PetscCall(R.lib().computeAdvectionDiffusionMatrixCartesianAIJ(int(comm), nx, ny, nz, _d3(h), float(dt),
                                                                        _d3(a), float(nu), b, ctypes.byref(hdl)))
        return hdl
    PetscCall(lib().computeAdvectionDiffusionMatrixCartesianAIJ(int(comm), nx, ny, nz, _d3(h), float(dt), _d3(a),
                                                                float(nu), b, ctypes.byref(hdl)))
    return Mat(hdl)


def config(n: int | Sequence[int] = 32, real: bool = False, **kw) -> AdvDiffConfig:
    """cfp_advdiff_config_default ([-0.5, 0.5]^3, a = (1, 0, 0), nu = 0.01, dt = 0.01, one step,
    precision 1e-8, the FFT PCSHELL, walls) with keyword overrides: pc='none'|'fft'|'fft_upwind',
    bc='wall'|'periodic', steps=ntmax, device=True/False, plus any AdvDiffConfig field."""
    cfg = AdvDiffConfig()
    dims = (int(n),) * 3 if np.isscalar(n) else tuple(int(v) for v in n)
    (_real_lib().lib() if real else lib()).cfp_advdiff_config_default(ctypes.byref(cfg), dims[0])
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
    res = AdvDiffResult()
    n = int(cfg.nx * cfg.ny * cfg.nz)
    out = np.empty(n, dtype=np.float64 if real else np.complex128) if return_field else None
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if out is not None else None
    if real:
        R = _real_lib()
        R.PetscCall(getattr(R.lib(), name)(ctypes.byref(cfg), ctypes.byref(res), ptr))
    else:
        PetscCall(getattr(lib(), name)(ctypes.byref(cfg), ctypes.byref(res), ptr))
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


def context(ndim: int, dt: float, dims: Sequence[int], a: Sequence[float], nu: float, mins, maxs):
    """getFFTPrec3DDiffusionContext: the PCSHELL context with the matched numbers
    lambda_d = a_d dt / h_d, mu_d = nu dt / h_d^2."""
    from ._lib_ext import FFTPrecDiffusionContext
    ctx = FFTPrecDiffusionContext()
    S = PetscScalar.of
    PetscCall(lib().getFFTPrec3DDiffusionContext(int(ndim), S(dt), int(dims[0]), int(dims[1]), int(dims[2]),
                                                 S(a[0]), S(a[1]), S(a[2]), S(nu), _d3(mins), _d3(maxs),
                                                 ctypes.byref(ctx)))
    return ctx


def pc_shell(ctx, upwind: bool = False):
    """A PC of type PCSHELL with the diffusion callbacks registered on ctx (setupFFTPrec3DDiffusion,
    applyFFT3DPrecDiffusion, destroyFFTPrec3DDiffusion) and set up.  On PETSC_COMM_WORLD of several
    ranks the FFT matrix is this rank's z slab and ctx.Diag its z-planes of the symbol.
    upwind=True: setupFFTPrec3DDiffusionUpwind, the operator's symbol for a velocity of either sign."""
    from .petsc import PC, _fn
    pc = PC()
    PetscCall(lib().PCSetType(pc.h, b"shell"))
    pc.ctx = ctx
    PetscCall(lib().PCShellSetContext(pc.h, ctypes.addressof(ctx)))
    PetscCall(lib().PCShellSetSetUp(pc.h, _fn("setupFFTPrec3DDiffusionUpwind" if upwind else "setupFFTPrec3DDiffusion")))
    PetscCall(lib().PCShellSetApply(pc.h, _fn("applyFFT3DPrecDiffusion")))
    PetscCall(lib().PCShellSetDestroy(pc.h, _fn("destroyFFTPrec3DDiffusion")))
    return pc.setup()


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
