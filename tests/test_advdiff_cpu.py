"""The advection-diffusion symbol's host side (no GPU): the closed-form 1-D symbol, the z
factorisation beta (1 - a e^{-i t}) (1 - b e^{i t}) and its ratios, a numpy model of the two-sided
recurrence kernel's algorithm against the FFT solve -- the proof that the bound the GPU tests use
is one the algorithm meets -- and the advection-diffusion CSR operator against a dense one."""
import ctypes
import os

import numpy as np
import pytest

from advdiff_cases import (COLUMNS, ELIGIBLE, apply_operator, bound, column_reference, dense_operator, kernel_model,
                           symbol_1d, z_factors, z_ratios)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    return cp


def transport_ratio(nx, ny, lam):
    from circulantpreconditioner_amd._lib import check, lib
    l6 = (ctypes.c_double * 6)(*[t for v in lam for t in (complex(v).real, complex(v).imag)])
    out = ctypes.c_double()
    check(lib().cfp_transport_z_ratio(nx, ny, l6, ctypes.byref(out)))
    return out.value


@pytest.mark.parametrize("n", [1, 2, 7, 100, 256])
@pytest.mark.parametrize("lam,mu", [(0.6, 0.2), (0.3 + 0.2j, 0.7 - 0.1j), (0, 1000), (-0.4, 3.0), (0.6, 0)])
def test_symbol_1d_closed_form(cp, n, lam, mu):
    got = cp.advdiff_symbol_1d(n, lam, mu)
    ref = symbol_1d(n, lam, mu)
    # 4 ulp of the terms' size (the two parts may cancel, so not of the result's)
    scale = (abs(complex(lam)) + 2 * abs(complex(mu))) * 2 + 1e-300
    assert got.shape == (n,)
    assert np.abs(got - ref).max() <= 4 * np.finfo(float).eps * scale


def test_symbol_1d_mu0_is_the_transport_symbol(cp):
    for n in (1, 2, 7, 256):
        assert np.array_equal(cp.advdiff_symbol_1d(n, 1.0, 0.0), cp.transport_symbol_1d(n))


@pytest.mark.parametrize("name", list(ELIGIBLE))
@pytest.mark.parametrize("nxy", [(256, 256), (7, 5), (1, 1)])
def test_z_ratio_matches_brute_force(cp, name, nxy):
    lam, mu = ELIGIBLE[name]
    ra, rb = cp.advdiff_z_ratio(nxy[0], nxy[1], lam, mu)
    ea, eb = z_ratios(nxy[0], nxy[1], lam, mu)
    assert ra == pytest.approx(ea, rel=1e-12)
    assert rb == pytest.approx(eb, rel=1e-12)
    if nxy == (256, 256):
        assert max(ra, rb) <= 1 - 2.0 ** -7  # the eligible cases are eligible


@pytest.mark.parametrize("lam", [(0.6, 0.15, 0.02), (0.6, 0.15, 333.3), (0.3 + 0.2j, 1.1, 0.7 - 0.4j), (0.6, 0.15, -0.6)])
def test_z_ratio_mu0_is_the_transport_ratio(cp, lam):
    ra, rb = cp.advdiff_z_ratio(256, 256, lam, (0, 0, 0))
    assert ra == transport_ratio(256, 256, lam)
    assert rb == 0.0


def test_z_ratio_over_the_cap_and_singular(cp):
    ra, rb = cp.advdiff_z_ratio(256, 256, (0, 0, 0), (0.3, 0.3, 1e6))
    assert max(ra, rb) > 1 - 2.0 ** -7
    # c = 1, lam_z = -1, mu_z = 0: d = 0 and p q = 0, so beta = 0 -> infinity
    ra, rb = cp.advdiff_z_ratio(1, 1, (0, 0, -1.0), (0, 0, 0))
    assert ra == float("inf") and rb == 0.0


@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_factorisation_identity(name):
    lam, mu = ELIGIBLE[name]
    sx, sy = symbol_1d(256, lam[0], mu[0]), symbol_1d(256, lam[1], mu[1])
    rng = np.random.default_rng(5)
    zeta = np.exp(2j * np.pi * np.arange(256) / 256)
    for kx, ky in [(0, 0), (128, 128), (1, 255)] + [tuple(rng.integers(0, 256, 2)) for _ in range(13)]:
        c = 1 + sx[kx] + sy[ky]
        beta, a, b = z_factors(c, lam[2], mu[2])
        assert abs(a) < 1 and abs(b) < 1
        lhs = beta * (1 - a / zeta) * (1 - b * zeta)
        ref = c + symbol_1d(256, lam[2], mu[2])
        assert np.abs(lhs - ref).max() <= 16 * np.finfo(float).eps * np.abs(ref).max()


@pytest.mark.parametrize("name", list(COLUMNS))
def test_kernel_model_meets_the_bound(name):
    c, lz, mz = COLUMNS[name]
    rng = np.random.default_rng(11)
    v = rng.uniform(-1, 1, 256) + 1j * rng.uniform(-1, 1, 256)
    _, a, b = z_factors(c, lz, mz)
    got, ref = kernel_model(v, c, lz, mz), column_reference(v, c, lz, mz)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    bd = bound(abs(a), abs(b))
    print(f"model [{name}]: |a| {abs(a):.5f} |b| {abs(b):.5f} rel L2 {err:.3e} bound {bd:.3e}")
    assert err < bd


def csr_dense(cp, dims, h, dt, a, nu, bc, shift):
    from circulantpreconditioner_amd import diffusion
    rp, col, val = diffusion.advdiff_csr(dims, h, dt, a, nu, bc, shift)
    N = int(np.prod(dims))
    A = np.zeros((N, N), dtype=np.complex128)
    for r in range(N):
        cols = col[rp[r]:rp[r + 1]]
        assert np.all(np.diff(cols) > 0), "columns ascend"
        assert r in cols, "every row stores its diagonal"
        assert np.all(val[rp[r]:rp[r + 1]][cols != r] != 0), "exact zeros are not stored"
        A[r, cols] = val[rp[r]:rp[r + 1]]
    return A


@pytest.mark.parametrize("dims", [(4, 3, 5), (6, 1, 1), (2, 2, 3)])
@pytest.mark.parametrize("bc", ["wall", "periodic"])
def test_advdiff_csr_matches_dense(cp, dims, bc):
    h, dt, a, nu = (0.25, 0.5, 0.2), 0.07, (1.0, 0.5, 2.0), 0.3
    got = csr_dense(cp, dims, h, dt, a, nu, bc, 1.0)
    ref = dense_operator(dims, h, dt, a, nu, bc == "periodic", 1.0)
    assert np.abs(got.imag).max() == 0
    assert np.abs(got.real - ref).max() <= 8 * np.finfo(float).eps * np.abs(ref).max()


@pytest.mark.parametrize("dims", [(4, 3, 5), (6, 1, 1), (2, 2, 3)])
@pytest.mark.parametrize("periodic", [False, True])
def test_matrix_free_restatement_is_the_dense_operator(dims, periodic):
    """test_diffusion_gpu.py checks the time loop's step with apply_operator: it is the same operator."""
    h, dt, a, nu = (0.25, 0.5, 0.2), 0.07, (1.0, 0.5, 2.0), 0.3
    u = np.random.default_rng(3).normal(size=int(np.prod(dims)))
    ref = dense_operator(dims, h, dt, a, nu, periodic, 1.0) @ u
    assert np.abs(apply_operator(u, dims, h, dt, a, nu, periodic) - ref).max() <= 16 * np.finfo(float).eps * np.abs(ref).max()


@pytest.mark.parametrize("dims", [(4, 3, 5), (6, 1, 1)])
def test_periodic_operator_is_the_circulant_of_the_symbol(cp, dims):
    h, dt, a, nu = (0.25, 0.5, 0.2), 0.07, (1.0, 0.5, 2.0), 0.3
    A = csr_dense(cp, dims, h, dt, a, nu, "periodic", 1.0)
    nx, ny, nz = dims
    first = A[:, 0].reshape(nz, ny, nx)
    lam = [a[d] * dt / h[d] for d in range(3)]
    mu = [nu * dt / h[d] ** 2 for d in range(3)]
    sym = 1 + sum(symbol_1d(n, l, m).reshape(sh) for n, l, m, sh in
                  zip(dims, lam, mu, [(1, 1, nx), (1, ny, 1), (nz, 1, 1)]))
    assert np.abs(np.fft.fftn(first) - sym).max() <= 64 * np.finfo(float).eps * np.abs(sym).max()


def test_header_declarations_are_exported(cp):
    from circulantpreconditioner_amd import _lib
    names = _lib._parse_decls(os.path.join(ROOT, "include", "diffusion_equation.h"))
    assert {"setupFFTPrec3DDiffusion", "applyFFT3DPrecDiffusion", "destroyFFTPrec3DDiffusion",
            "getFFTPrec3DDiffusionContext", "PetscFft3DDiffusionSolver", "cfp_advdiff_csr",
            "computeAdvectionDiffusionMatrixCartesianAIJ", "AdvectionDiffusionGMRES"} <= set(names)
    assert set(names) <= set(_lib.exported_symbols())  # the header is in the library's list
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names + ["cfp_plan_set_symbol_advdiff", "cfp_advdiff_symbol_1d", "cfp_advdiff_z_ratio"]:
        assert hasattr(L, n), n


def test_real_scalar_library_still_loads():
    from circulantpreconditioner_amd import petsc_real
    assert petsc_real.lib() is not None


@pytest.mark.parametrize("bc", ["wall", "periodic"])
def test_time_loop_pcnone_on_host_vecs(bc):
    """AdvectionDiffusionGMRES without a device (host Vecs, PCNONE): one step solves the operator."""
    from circulantpreconditioner_amd import diffusion as dif
    dims = (8, 6, 5)
    kw = dict(bc=bc, pc="none", device=False, a=(1.0, 0.5, 0.0), nu=0.1, dt=0.01)
    _, u0 = dif.run(dif.config(dims, steps=0, **kw), return_field=True)
    cfg = dif.config(dims, steps=1, **kw)
    res, u1 = dif.run(cfg, return_field=True)
    h = [1.0 / n for n in dims]
    err = np.linalg.norm(apply_operator(u1, dims, h, cfg.dt, list(cfg.a), cfg.nu, bc == "periodic") - u0) / np.linalg.norm(u0)
    assert res["steps"] == 1 and res["all_converged"] == 1 and res["total_its"] > 1
    assert err <= 10 * cfg.precision
    with pytest.raises(Exception):
        dif.run(dif.config(dims, pc="fft", device=False))  # the FFT preconditioner needs HIP Vecs
