"""The advection-diffusion symbol on the real-data plan and in the real-scalar library, without a
GPU: the exports (cfp_rplan_set_symbol_advdiff, the middle-kernel selector, every name of
include/diffusion_equation.h in libcirculant_fft_real.so), the real library's operator against
the dense restatement, and its GMRES time loop on host Vecs."""
import ctypes
import os

import numpy as np
import pytest

from advdiff_cases import apply_operator, dense_operator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dif():
    from circulantpreconditioner_amd import diffusion
    return diffusion


def test_real_plan_entry_points_are_exported_by_both_libraries():
    from circulantpreconditioner_amd import _lib, petsc_real
    names = _lib._parse_decls(os.path.join(ROOT, "include", "circulant_fft_real.h"))
    new = ["cfp_rplan_set_symbol_advdiff", "cfp_rplan_set_mid_kernel", "cfp_rplan_mid_kernel"]
    assert set(new) <= set(names)
    for path in (_lib.LIB_PATH, petsc_real.LIB_PATH):
        L = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        for n in new:
            assert hasattr(L, n), f"{os.path.basename(path)} does not export {n}"


def test_diffusion_header_is_exported_by_the_real_scalar_library():
    from circulantpreconditioner_amd import _lib, petsc_real
    names = _lib._parse_decls(os.path.join(ROOT, "include", "diffusion_equation.h"))
    assert {"getFFTPrec3DDiffusionContext", "setupFFTPrec3DDiffusion", "applyFFT3DPrecDiffusion",
            "destroyFFTPrec3DDiffusion", "PetscFft3DDiffusionSolver", "cfp_advdiff_csr",
            "computeAdvectionDiffusionMatrixCartesianAIJ", "cfp_advdiff_config_default", "AdvectionDiffusionGMRES",
            "AdvectionDiffusionFFTDirect"} <= set(names)
    L = ctypes.CDLL(petsc_real.LIB_PATH, mode=ctypes.RTLD_LOCAL)
    for n in names:
        assert hasattr(L, n), f"libcirculant_fft_real.so does not export {n}"


def test_real_context_structures_match_the_header_layout():
    """PetscScalar = double: 4 PetscInt, 3 scalars, 5 handles, 3 scalars; the transport context first."""
    from circulantpreconditioner_amd import petsc_real as R
    assert ctypes.sizeof(R.FFTPrecDiffusionContext) == 8 * 15
    assert R.FFTPrecDiffusionContext.mu_x.offset == ctypes.sizeof(R.FFTPrecTransportContext)
    assert ctypes.sizeof(R.StructuredDiffusionContext) == 8 * 12


@pytest.mark.parametrize("bc", ["wall", "periodic"])
def test_real_library_csr_matches_dense(dif, bc):
    dims = (4, 3, 2)
    h, dt, a, nu = (0.25, 0.5, 0.2), 0.07, (1.0, 0.5, 2.0), 0.3
    rowptr, col, val = dif.advdiff_csr(dims, h, dt, a, nu, bc, 1.0, real=True)
    n = int(np.prod(dims))
    got = np.zeros((n, n), dtype=np.complex128)
    for r in range(n):
        for k in range(rowptr[r], rowptr[r + 1]):
            got[r, col[k]] += val[k]
    ref = dense_operator(dims, h, dt, a, nu, bc == "periodic", 1.0)
    assert np.abs(got.imag).max() == 0
    assert np.abs(got.real - ref).max() <= 8 * np.finfo(float).eps * np.abs(ref).max()
    # the same arrays as the complex library's
    r2, c2, v2 = dif.advdiff_csr(dims, h, dt, a, nu, bc, 1.0)
    assert np.array_equal(rowptr, r2) and np.array_equal(col, c2) and np.array_equal(val, v2)


@pytest.mark.parametrize("bc", ["wall", "periodic"])
def test_real_library_operator_matmult_on_host_vecs(dif, bc):
    """computeAdvectionDiffusionMatrixCartesianAIJ with real scalars: dt L (no shift) as a host MatMult."""
    from circulantpreconditioner_amd import petsc_real as R
    dims = (4, 3, 2)
    h, dt, a, nu = (0.25, 0.5, 0.2), 0.07, (1.0, 0.5, 2.0), 0.3
    n = int(np.prod(dims))
    A = dif.operator(dims, h, dt, a, nu, bc, real=True)
    u = np.random.default_rng(2).normal(size=n)
    x, y = R.Vec.seq(n).set_array(u), R.Vec.seq(n)
    A.mult(x, y)
    ref = dense_operator(dims, h, dt, a, nu, bc == "periodic", 0.0) @ u
    assert np.abs(y.array() - ref).max() <= 16 * np.finfo(float).eps * np.abs(ref).max()
    x.destroy()
    y.destroy()
    A.destroy()


@pytest.mark.parametrize("bc", ["wall", "periodic"])
def test_real_library_time_loop_pcnone_on_host_vecs(dif, bc):
    """AdvectionDiffusionGMRES of the real-scalar library without a device (host Vecs, PCNONE): it
    converges, the field is N doubles, and one step solves the operator."""
    dims = (8, 6, 5)
    kw = dict(bc=bc, pc="none", device=False, a=(1.0, 0.5, 0.0), nu=0.1, dt=0.01, real=True)
    _, u0 = dif.run(dif.config(dims, steps=0, **kw), return_field=True, real=True)
    assert u0.dtype == np.float64 and set(np.unique(u0)) == {600.0, 650.0}
    cfg = dif.config(dims, steps=1, **kw)
    res, u1 = dif.run(cfg, return_field=True, real=True)
    h = [(cfg.xmax[d] - cfg.xmin[d]) / n for d, n in enumerate(dims)]
    err = np.linalg.norm(apply_operator(u1, dims, h, cfg.dt, list(cfg.a), cfg.nu, bc == "periodic") - u0) / np.linalg.norm(u0)
    print(f"real library, host GMRES {bc}: its {res['total_its']} |A U1 - U0| / |U0| = {err:.2e}")
    assert res["steps"] == 1 and res["all_converged"] == 1 and res["total_its"] > 1
    assert err <= 10 * cfg.precision
    # the same field as the complex library's time loop
    kwc = {k: v for k, v in kw.items() if k != "real"}
    _, uc = dif.run(dif.config(dims, steps=1, **kwc), return_field=True)
    assert np.abs(uc.imag).max() == 0
    assert np.linalg.norm(uc.real - u1) / np.linalg.norm(u1) <= 10 * cfg.precision


def test_real_library_fft_pc_needs_hip_vecs(dif):
    from circulantpreconditioner_amd import petsc_real as R
    PETSC_ERR_SUP = 56
    with pytest.raises(R.PetscError) as e:
        dif.run(dif.config((8, 6, 5), pc="fft", device=False, real=True), real=True)
    assert e.value.code == PETSC_ERR_SUP


def test_real_plan_python_surface_rejects_complex_numbers():
    """set_advdiff_symbol validates before it touches the library's plan: a complex lambda or mu is
    no Hermitian symbol."""
    from circulantpreconditioner_amd.plan import RealPlan
    assert RealPlan._real3((0.5, 1, np.float64(2.0)), "lambda")[:] == [0.5, 1.0, 2.0]
    assert RealPlan._real3((0.5 + 0j, 1, 2), "mu")[:] == [0.5, 1.0, 2.0]
    with pytest.raises(ValueError):
        RealPlan._real3((0.5 + 0.1j, 1, 2), "lambda")
    with pytest.raises(ValueError):
        RealPlan._real3((0.5, 1), "mu")
    assert RealPlan.MID_KERNELS == {"auto": 0, "fft": 1, "rec": 2}
