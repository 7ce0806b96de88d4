"""The recurrence middle kernel of the 256^3 3-sweep apply (k_tp_mid_rec): for a transport symbol
whose z ratio a = lam_z / (1 + s_x + s_y + lam_z) stays below 1 - 2^-13 the z DFT, the divide and
the inverse z DFT are the cyclic recurrence u_z = a u_{z-1} + w_z.  The reference in every test
is the same plan with shape 'swap64pf', which is the FFT middle kernel always.

Bounds: two schedules of the same apply agree to 1e-13 (the project's schedule-against-schedule
bar) where amax <= 0.5; above that the recurrence's rounding grows like eps / (1 - amax), and
the bound is 8 * 2.2e-16 / (1 - amax) (5.9e-13 at amax = 0.997)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-10
N3 = (256, 256, 256)
N = 256 ** 3

ELIGIBLE = {
    "bench": (0.6, 0.15, 0.02),
    "cfl333": (0.6, 0.15, 333.3),
    "complex": (0.3 + 0.2j, 1.1, 0.7 - 0.4j),
    "xonly": (55.6, 0, 0),
}
NEGZ = (0.6, 0.15, -0.6)  # amax = 1.5: not eligible


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


def apply_with(cp, lam, b, mid):
    with cp.CirculantPlan(N3) as plan:
        plan.set_transport_symbol(lam).set_three_pass_shape(0, mid)
        kind = plan.mid_kernel()
        x = plan.apply(b)
        torch.cuda.synchronize()
    return x, kind


@pytest.fixture(scope="module")
def b_rand(cp):
    b = torch.empty(N, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(b, 77)
    return b


@pytest.fixture(scope="module")
def solved(cp, b_rand):
    """(x of the recurrence kernel, x of the FFT kernel) per eligible lambda set, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            lam = ELIGIBLE[name]
            x, kind = apply_with(cp, lam, b_rand, "default")
            assert kind == "zrec"
            xf, kindf = apply_with(cp, lam, b_rand, "swap64pf")
            assert kindf == "fft"
            cache[name] = (x, xf)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_agrees_with_fft_kernel(solved, name):
    x, xf = solved(name)
    err = rel(x, xf)
    print(f"zrec vs fft [{name}]: amax {amax_of(ELIGIBLE[name]):.6f} rel L2 {err:.3e} bound {bound(ELIGIBLE[name]):.3e}")
    assert err < bound(ELIGIBLE[name])


@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_residual(solved, b_rand, name):
    from bench import transport_residual
    x, _ = solved(name)
    res = transport_residual(b_rand, x, N3, ELIGIBLE[name])
    print(f"zrec residual [{name}]: {res:.3e}")
    assert res < 1e-12


def test_oracle_cfl333(solved, b_rand, oracle):
    lam = ELIGIBLE["cfl333"]
    x, _ = solved("cfl333")
    ref = oracle.c_solve_3d(oracle.c_build_diag_transport(N3, lam), b_rand.cpu().numpy(), N3)
    err = oracle.rel_l2(x.cpu().numpy(), ref)
    print(f"zrec vs oracle [cfl333]: {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("z0", [250, 15])
def test_impulse_carries_and_wrap(cp, z0):
    """At lam_z = 0.02 a^16 is 1e-27 and a broken carry is invisible; at 333.3 (a = 0.997) the
    carries between the threads, lanes and waves and the cyclic closure all matter.  z0 = 15 is a
    block edge (the last point of wave 0)."""
    lam = ELIGIBLE["cfl333"]
    x0, y0 = 37, 101
    b = torch.zeros(N, dtype=torch.complex128, device="cuda")
    b[x0 + 256 * (y0 + 256 * z0)] = 1.0
    x, kind = apply_with(cp, lam, b, "default")
    assert kind == "zrec"
    xf, _ = apply_with(cp, lam, b, "swap64pf")
    err = rel(x, xf)
    print(f"zrec impulse z0={z0}: rel L2 {err:.3e} bound {bound(lam):.3e}")
    assert err < bound(lam)
    col = x.view(256, 256, 256)[:, y0, x0]
    assert bool((col[0:6].abs() > 0).all())  # the wrap-around happened


def test_fallback_not_eligible(cp, b_rand):
    x, kind = apply_with(cp, NEGZ, b_rand, "default")
    assert kind == "fft"
    xf, _ = apply_with(cp, NEGZ, b_rand, "swap64pf")
    assert torch.equal(x, xf)


@pytest.mark.parametrize("graph", [False, True])
def test_live_plan_follows_symbol(cp, b_rand, graph):
    """One plan through eligible -> not eligible -> eligible: each apply equals a fresh plan's."""
    seq = [(ELIGIBLE["bench"], "zrec"), (NEGZ, "fft"), (ELIGIBLE["cfl333"], "zrec")]
    with cp.CirculantPlan(N3) as plan:
        plan.set_graph(graph)
        out = torch.empty_like(b_rand)
        for lam, kind in seq:
            plan.set_transport_symbol(lam)
            assert plan.mid_kernel() == kind
            plan.apply(b_rand, out=out)
            if graph:
                plan.apply(b_rand, out=out)  # the second apply of the pair replays the captured graph
            torch.cuda.synchronize()
            fresh, fkind = apply_with(cp, lam, b_rand, "default")
            assert fkind == kind
            assert torch.equal(out, fresh)


def test_other_symbols_and_shapes_stay_fft(cp):
    with cp.CirculantPlan(N3) as plan:
        plan.set_transport_symbol(ELIGIBLE["bench"])
        assert plan.mid_kernel() == "zrec"
        for mid in ("swap64pf", "swap64", "lane64", "blocked"):
            plan.set_three_pass_shape(0, mid)
            assert plan.mid_kernel() == "fft"
        plan.set_three_pass_shape(64, "default")
        assert plan.mid_kernel() == "fft"
        plan.set_three_pass_shape(0, "default").set_schedule("five")
        assert plan.mid_kernel() == "fft"
        plan.set_schedule("auto")
        assert plan.mid_kernel() == "zrec"
        s = cp.transport_symbol_1d(256)
        plan.set_separable_symbol(s, s, s, ELIGIBLE["bench"])  # the same symbol, given as vectors
        assert plan.mid_kernel() == "fft"
    with cp.CirculantPlan((128, 128, 128)) as plan:
        plan.set_transport_symbol(ELIGIBLE["bench"])
        assert plan.mid_kernel() == "fft"


def test_deterministic_and_in_place(cp, b_rand):
    lam = ELIGIBLE["cfl333"]
    with cp.CirculantPlan(N3) as plan:
        plan.set_transport_symbol(lam)
        assert plan.mid_kernel() == "zrec"
        x1 = plan.apply(b_rand)
        x2 = plan.apply(b_rand)
        assert torch.equal(x1, x2)
        t = b_rand.clone()
        plan.apply(t, out=t)
        assert torch.equal(t, x1)


def test_8_byte_aligned(cp, b_rand, solved):
    """b and x 8 bytes past a 16-byte boundary: the kernel runs without its LDS-DMA prefetch."""
    from circulantpreconditioner_amd._lib import check, lib
    lam = ELIGIBLE["cfl333"]
    x, xf = solved("cfl333")
    raw = torch.empty(2 * N + 1, dtype=torch.float64, device="cuda")
    raw[1:].copy_(torch.view_as_real(b_rand).reshape(-1))
    ptr = raw.data_ptr() + 8
    with cp.CirculantPlan(N3) as plan:
        plan.set_transport_symbol(lam)
        assert plan.mid_kernel() == "zrec"
        check(lib().cfp_plan_apply(plan._h, ptr, ptr, None))
        torch.cuda.synchronize()
    got = torch.view_as_complex(raw[1:].clone().reshape(-1, 2))
    err = rel(got, xf)
    print(f"zrec unaligned vs fft: {err:.3e}; vs aligned zrec: {rel(got, x):.3e}")
    assert err < bound(lam)
    assert rel(got, x) < bound(lam)
