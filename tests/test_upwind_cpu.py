"""The upwind symbol's host side (no GPU): the exported names, the mapping onto the
advection-diffusion pair, the closed form, the periodic operator it is the symbol of (and the
literal lam (1 - w) is not, for a negative velocity), a numpy model of the backward recurrence
kernel against the FFT solve -- the proof that the bound the GPU tests use is one the algorithm
meets -- and the z ratios of the mapped pair."""
import numpy as np
import pytest

from upwind_cases import (MUS, SIGNS, back_ratio, bound, column_reference, diag, literal_symbol_1d,
                          reversed_scan_model, signed, upwind_symbol_1d)

NEW_NAMES = ["cfp_upwind_to_advdiff", "cfp_plan_set_symbol_upwind", "cfp_rplan_set_symbol_upwind",
             "cfp_dist_plan_set_symbol_upwind", "cfp_group_set_symbol_upwind", "setupFFTPrec3DUpwind",
             "setupFFTPrec3DDiffusionUpwind"]


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    return cp


@pytest.mark.parametrize("real", [False, True])
def test_new_names_are_exported(real):
    if real:
        from circulantpreconditioner_amd import petsc_real
        L = petsc_real.lib()
    else:
        from circulantpreconditioner_amd import lib
        L = lib()
    for name in NEW_NAMES:
        assert hasattr(L, name), name


def test_enum_values_and_python_names(cp):
    from circulantpreconditioner_amd import diffusion, transport
    from circulantpreconditioner_amd.distributed import SlabGroup, SlabPlan
    assert transport.config(8, lambda_mode="upwind").lambda_mode == 2
    assert transport.config(8, lam="upwind").lambda_mode == 2
    assert transport.config(8).lambda_mode == 1  # the default stays MATCHED
    assert diffusion.config(8, pc="fft_upwind").pc == 2
    assert diffusion.config(8).pc == 1  # the default stays the literal FFT PCSHELL
    for cls in (cp.CirculantPlan, cp.RealPlan, SlabPlan, SlabGroup):
        assert callable(getattr(cls, "set_upwind_symbol"))


@pytest.mark.parametrize("signs", SIGNS)
@pytest.mark.parametrize("mu", list(MUS))
def test_mapping_on_every_sign_pattern(cp, signs, mu):
    lam = signed(signs)
    lo, mo = cp.upwind_to_advdiff(lam, MUS[mu])
    for d in range(3):
        assert lo[d] == lam[d]
        assert mo[d] == (MUS[mu][d] - lam[d] if lam[d] < 0 else MUS[mu][d])


def test_mapping_on_complex_numbers(cp):
    lam = (-0.3 + 0.2j, 0.4 - 0.7j, -1e-3 - 2j)
    mu = (0.1 + 0.05j, 0.2, 0.3 - 0.1j)
    lo, mo = cp.upwind_to_advdiff(lam, mu)
    assert list(lo) == [complex(v) for v in lam]
    assert mo[0] == complex(mu[0]) - complex(lam[0])  # Re lam < 0: both components move
    assert mo[1] == complex(mu[1])                    # Re lam >= 0 whatever the imaginary part
    assert mo[2] == complex(mu[2]) - complex(lam[2])
    lo, mo = cp.upwind_to_advdiff((0.0, -0.0, 0.0 - 1j), (0, 0, 0))  # zero real part: a copy
    assert list(mo) == [0, 0, 0]


@pytest.mark.parametrize("n", [1, 2, 7, 100, 256])
@pytest.mark.parametrize("lam,mu", [(-0.6, 0.0), (-0.6, 0.2), (0.6, 0.2), (-1e3 / 3, 0.0), (-0.3 + 0.2j, 0.7 - 0.1j),
                                    (-0.4, 3.0)])
def test_symbol_of_the_mapped_numbers_is_the_upwind_closed_form(cp, n, lam, mu):
    lo, mo = cp.upwind_to_advdiff((lam, 0, 0), (mu, 0, 0))
    got = cp.advdiff_symbol_1d(n, lo[0], mo[0])
    ref = upwind_symbol_1d(n, lam, mu)
    scale = np.abs(ref).max() if n > 1 else 1.0
    assert got.shape == (n,)
    # relative to the symbol's size: the mapped form adds terms of that size
    assert np.abs(got - ref).max() <= 1e-14 * scale


def test_periodic_operator_has_the_upwind_symbol_not_the_literal_one(cp):
    from circulantpreconditioner_amd import diffusion
    dims, a, nu, dt = (6, 5, 4), (-1.0, 0.5, -0.3), 0.01, 0.05
    h = [1.0 / n for n in dims]
    rowptr, col, val = diffusion.advdiff_csr(dims, h, dt, a, nu, bc="periodic", shift=1.0)
    N = dims[0] * dims[1] * dims[2]
    first = np.zeros(N, dtype=np.complex128)
    for r in range(N):
        for p in range(rowptr[r], rowptr[r + 1]):
            if col[p] == 0:
                first[r] += val[p]
    eig = np.fft.fftn(first.reshape(dims[2], dims[1], dims[0])).reshape(-1)
    lam = [a[d] * dt / h[d] for d in range(3)]
    mu = [nu * dt / h[d] ** 2 for d in range(3)]
    up = diag(dims, lam, mu)
    lit = diag(dims, lam, mu, sym=literal_symbol_1d)
    err_up, err_lit = np.abs(eig - up).max(), np.abs(eig - lit).max()
    print(f"periodic operator {dims}: |eig - upwind| {err_up:.2e}, |eig - literal| {err_lit:.2e}")
    assert err_up <= 1e-13
    assert err_lit > 1e-2
    # and through the library's own closed form on the mapped pair
    lo, mo = cp.upwind_to_advdiff(lam, mu)
    s = [cp.advdiff_symbol_1d(n, lo[d], mo[d]) for d, n in enumerate(dims)]
    lib_diag = (1 + s[0][None, None, :] + s[1][None, :, None] + s[2][:, None, None]).reshape(-1)
    assert np.abs(eig - lib_diag).max() <= 1e-13


@pytest.mark.parametrize("c", [1.0, 1.2 - 0.4j])
def test_reversed_scan_model_meets_the_bound(c):
    """nz = 256 at amax = 0.997, the reference driver's cfl of 1e3 / 3 against z."""
    amax = 0.997
    q = amax * abs(complex(c)) / (1 - amax)  # |q / (c + q)| close to amax
    a = abs(q / (complex(c) + q))
    rng = np.random.default_rng(11)
    v = rng.uniform(-1, 1, 256) + 1j * rng.uniform(-1, 1, 256)
    got = reversed_scan_model(v, c, q)
    ref = column_reference(v, c, q)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"reversed scan model c={c}: |a| {a:.6f} rel L2 {err:.3e} bound {bound(max(a, amax)):.3e}")
    assert err <= 8 * 2.2e-16 / (1 - amax)
    # an impulse at the block edges and the cyclic wrap
    for z0 in (0, 15, 16, 255):
        e = np.zeros(256, dtype=np.complex128)
        e[z0] = 1.0
        g, r = reversed_scan_model(e, c, q), column_reference(e, c, q)
        assert np.linalg.norm(g - r) / np.linalg.norm(r) <= 8 * 2.2e-16 / (1 - amax)


@pytest.mark.parametrize("lam", [(0.6, 0.15, -0.6), (55.6, 0, -1e3 / 3), (-0.6, -0.15, -0.4), (0.3 + 0.2j, 1.1, -0.7 + 0.4j)])
def test_ratios_of_the_mapped_pure_transport_numbers(cp, lam):
    lo, mo = cp.upwind_to_advdiff(lam, (0, 0, 0))
    ra, rb = cp.advdiff_z_ratio(256, 256, lo, mo)
    assert ra == 0.0
    assert rb == pytest.approx(back_ratio(256, 256, lam), rel=1e-12)
    assert rb < 1.0


def test_reference_driver_cfl_is_under_the_backward_cap_and_over_the_two_sided_one(cp):
    lam = (55.6, 0, -1e3 / 3)
    _, rb = cp.advdiff_z_ratio(256, 256, *cp.upwind_to_advdiff(lam))
    assert 1 - 2.0 ** -7 < rb <= 1 - 2.0 ** -13
