"""The recurrence middle kernel (k_tp_mid_rec) with y2 on the lanes and z in the registers: a
wave-wide access is the 8 rows of one z-plane, the y2 DFT runs across lane bits 3..5 and leaves
lane (x, y2) with column (x, brev3(y2)), and the scan is a register loop over the wave's 16 z with
one carry per wave.  These cases aim at what that layout can get wrong: every input lane of the
y2 DFT, the thread-block and wave edges of the scan, the cyclic wrap, the closure 1 / (1 - a^256),
the bit-reversed symbol index with a non-real a, and the instantiation the fused Krylov step runs.

256^3 is the only grid the kernel exists for.  The reference in every comparison is the same plan
with shape 'swap64pf' (the FFT middle kernel always), under test_zrec_gpu.py's bound."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
N3 = (256, 256, 256)
N = 256 ** 3

CFL333 = (0.6, 0.15, 333.3)             # a = 0.997: carries and closure all matter
NEAR_CAP = (0.6, 0.15, 8000.0)          # amax just under the eligibility cap 1 - 2^-13
COMPLEX = (0.3 + 0.2j, 1.1, 0.7 - 0.4j)  # test_zrec_gpu.py's "complex" set

# (x0, y0, z0): x0 mod 8 and y0 mod 8 each cover 0..7 (every x lane and every input lane of the
# y2 DFT); z0 covers the first and last slot of a wave's block, a wave edge inside the grid, the
# middle, and the wrap
IMPULSES = [(0, 8, 0), (9, 17, 15), (18, 250, 16), (27, 3, 31), (100, 100, 128), (253, 37, 240),
            (6, 254, 254), (255, 255, 255)]


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return cp


def amax_of(lam):
    from circulantpreconditioner_amd._lib import check, lib
    l6 = (ctypes.c_double * 6)(*[t for v in lam for t in (complex(v).real, complex(v).imag)])
    out = ctypes.c_double()
    check(lib().cfp_transport_z_ratio(256, 256, l6, ctypes.byref(out)))
    return out.value


def bound(lam):
    a = amax_of(lam)
    return 1e-13 if a <= 0.5 else 8 * 2.2e-16 / (1.0 - a)


def rel(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


@pytest.fixture(scope="module")
def plans(cp):
    """(recurrence plan, FFT plan) per lambda set, created once and closed at the end."""
    made = {}

    def get(lam):
        if lam not in made:
            rec = cp.CirculantPlan(N3)
            rec.set_transport_symbol(lam)
            fft = cp.CirculantPlan(N3)
            fft.set_transport_symbol(lam).set_three_pass_shape(0, "swap64pf")
            assert rec.mid_kernel() == "zrec" and fft.mid_kernel() == "fft"
            made[lam] = (rec, fft)
        return made[lam]
    yield get
    for rec, fft in made.values():
        rec.close()
        fft.close()


def both(plans, lam, b):
    rec, fft = plans(lam)
    x = rec.apply(b)
    xf = fft.apply(b)
    torch.cuda.synchronize()
    return x, xf


def impulse(x0, y0, z0):
    b = torch.zeros(N, dtype=torch.complex128, device="cuda")
    b[x0 + 256 * (y0 + 256 * z0)] = 1.0
    return b


@pytest.mark.parametrize("x0,y0,z0", IMPULSES)
def test_unit_impulse(plans, x0, y0, z0):
    x, xf = both(plans, CFL333, impulse(x0, y0, z0))
    err = rel(x, xf)
    print(f"zrec impulse ({x0}, {y0}, {z0}): rel L2 {err:.3e} bound {bound(CFL333):.3e}")
    assert err < bound(CFL333)
    if z0 >= 240:
        col = x.view(256, 256, 256)[:, y0, x0]
        assert bool((col[0:6].abs() > 0).all())  # the wrap-around happened


def test_constant_along_z(cp, plans):
    """b constant along z: every wave-local scan sees the same input and the closure
    1 / (1 - a^256) carries the whole answer."""
    plane = torch.empty(256 * 256, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(plane, 91)
    b = plane.repeat(256)
    x, xf = both(plans, CFL333, b)
    err = rel(x, xf)
    print(f"zrec constant along z: rel L2 {err:.3e} bound {bound(CFL333):.3e}")
    assert err < bound(CFL333)
    xv = x.view(256, 256 * 256)
    assert rel(xv[255], xv[0]) < bound(CFL333)  # the answer is constant along z as well


def test_near_the_cap(cp, plans):
    b = torch.empty(N, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(b, 77)
    a = amax_of(NEAR_CAP)
    assert 0.999 < a <= 1.0 - 2.0 ** -13
    x, xf = both(plans, NEAR_CAP, b)
    err = rel(x, xf)
    print(f"zrec near the cap: amax {a:.8f} rel L2 {err:.3e} bound {bound(NEAR_CAP):.3e}")
    assert err < bound(NEAR_CAP)


def test_complex_lambda_impulse(plans):
    """A non-real a: a wrong (bit-reversed) symbol index changes the column's phase."""
    x, xf = both(plans, COMPLEX, impulse(77, 203, 129))
    err = rel(x, xf)
    print(f"zrec complex impulse: rel L2 {err:.3e} bound {bound(COMPLEX):.3e}")
    assert err < bound(COMPLEX)


def test_fused_gmres_step_same_iterations():
    """One GMRES step of the 256^3 transport solve with the Krylov step fused into the apply
    (graph replay, the kernel's second instantiation) against MatMult + PCApply + VecMDot."""
    from circulantpreconditioner_amd import transport as T
    rf = T.run(T.config(256, pc="fft", sign="fixed", device=True, steps=1, fuse=1))
    ru = T.run(T.config(256, pc="fft", sign="fixed", device=True, steps=1, fuse=0))
    assert rf["all_converged"] == ru["all_converged"] == 1
    assert rf["total_its"] == ru["total_its"] and rf["pc_calls"] == ru["pc_calls"]
    assert rf["fused_dots"] == rf["total_its"] and ru["fused_dots"] == 0
