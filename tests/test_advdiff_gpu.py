"""The advection-diffusion symbol on the GPU (CirculantPlan.set_advdiff_symbol) and the two-sided
recurrence middle kernel of the 256^3 3-sweep apply (k_tp_mid_rec2): along z the symbol is
beta (1 - a e^{-i t}) (1 - b e^{i t}), so "z DFT, divide, inverse z DFT" is a forward and a
backward cyclic first-order recurrence.  The reference in every 256^3 test is the same plan with
shape 'swap64pf', which is the FFT middle kernel always.

Bounds: two schedules of the same apply agree to 1e-13 (the project's schedule-against-schedule
bar) where both z ratios are <= 0.5; above that the recurrence's rounding grows like
eps / (1 - |a|) once per scan direction, and the bound is 8 * 2.2e-16 / ((1 - ra) (1 - rb)) with
ra, rb the maxima over the columns (test_advdiff_cpu.py checks a numpy model of the kernel's
algorithm against it).  The oracle bar is the project's 1e-10."""
import ctypes

import numpy as np
import pytest
import torch

from advdiff_cases import ELIGIBLE, bound as ratio_bound, diag as np_diag

pytestmark = pytest.mark.gpu
TOL = 1e-10
N3 = (256, 256, 256)
N = 256 ** 3
OVER_CAP = ((0, 0, 0), (0.3, 0.3, 1e6))
TRANSPORT = (0.6, 0.15, 0.02)


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return cp


def bound(cp, case):
    ra, rb = cp.advdiff_z_ratio(256, 256, *case)
    return 1e-13 if max(ra, rb) <= 0.5 else ratio_bound(ra, rb)


def rel(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


def apply_with(cp, case, b, mid):
    with cp.CirculantPlan(N3) as plan:
        plan.set_advdiff_symbol(*case).set_three_pass_shape(0, mid)
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
    """(x of the two-sided recurrence kernel, x of the FFT kernel) per eligible case, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            x, kind = apply_with(cp, ELIGIBLE[name], b_rand, "default")
            assert kind == "zrec2"
            xf, kindf = apply_with(cp, ELIGIBLE[name], b_rand, "swap64pf")
            assert kindf == "fft"
            cache[name] = (x, xf)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_agrees_with_fft_kernel(cp, solved, name):
    x, xf = solved(name)
    err = rel(x, xf)
    ra, rb = cp.advdiff_z_ratio(256, 256, *ELIGIBLE[name])
    print(f"zrec2 vs fft [{name}]: ratios {ra:.6f} {rb:.6f} rel L2 {err:.3e} bound {bound(cp, ELIGIBLE[name]):.3e}")
    assert err < bound(cp, ELIGIBLE[name])


def circulant_apply(x, case):
    """C x of the advection-diffusion circulant, by rolls in both directions of every axis."""
    lam, mu = case
    v = x.view(256, 256, 256)
    y = v.clone()
    for d, dim in enumerate((2, 1, 0)):  # x is the fastest axis = the last dim
        l, m = complex(lam[d]), complex(mu[d])
        down, up = torch.roll(v, 1, dim), torch.roll(v, -1, dim)  # v[i - 1], v[i + 1]
        y += (l + 2 * m) * v - (l + m) * down - m * up
    return y.reshape(-1)


@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_residual(cp, solved, b_rand, name):
    x, _ = solved(name)
    res = rel(circulant_apply(x, ELIGIBLE[name]), b_rand)
    print(f"zrec2 residual [{name}]: {res:.3e} bound {bound(cp, ELIGIBLE[name]):.3e}")
    assert res < bound(cp, ELIGIBLE[name])


def test_oracle_diff1000(solved, b_rand, oracle):
    x, _ = solved("diff1000")
    ref = oracle.c_solve_3d(np_diag(N3, *ELIGIBLE["diff1000"]), b_rand.cpu().numpy(), N3)
    err = oracle.rel_l2(x.cpu().numpy(), ref)
    print(f"zrec2 vs oracle [diff1000]: {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("z0", [0, 15, 16, 255])
def test_impulse_carries_and_wrap(cp, z0):
    """mu_z = 1000: |a| = |b| = 0.97, so a^16 = 0.6 and the carries between slots, waves and
    across the cyclic closure matter in both directions.  z0 = 15 / 16 are a block's last and the
    next block's first point, 0 / 255 the two ends of the wrap."""
    case = ELIGIBLE["diff1000"]
    x0, y0 = 37, 101
    b = torch.zeros(N, dtype=torch.complex128, device="cuda")
    b[x0 + 256 * (y0 + 256 * z0)] = 1.0
    x, kind = apply_with(cp, case, b, "default")
    assert kind == "zrec2"
    xf, _ = apply_with(cp, case, b, "swap64pf")
    err = rel(x, xf)
    print(f"zrec2 impulse z0={z0}: rel L2 {err:.3e} bound {bound(cp, case):.3e}")
    assert err < bound(cp, case)
    col = x.view(256, 256, 256)[:, y0, x0]
    assert bool((col[0:6].abs() > 0).all()) and bool((col[250:256].abs() > 0).all())  # both sides of the wrap


def test_mu_z_zero_takes_the_transport_kernel(cp, b_rand):
    lam = TRANSPORT
    with cp.CirculantPlan(N3) as plan:
        plan.set_advdiff_symbol(lam, (0.2, 0.1, 0))
        assert plan.mid_kernel() == "zrec"
        plan.set_advdiff_symbol(lam, (0, 0, 0))
        assert plan.mid_kernel() == "zrec"
        x = plan.apply(b_rand)
        plan.set_transport_symbol(lam)
        assert plan.mid_kernel() == "zrec"
        xt = plan.apply(b_rand)
        assert torch.equal(x, xt)


def test_mu_z_zero_with_diffusion_in_xy_agrees_with_fft(cp, b_rand):
    case = (TRANSPORT, (0.2, 0.1, 0))
    x, kind = apply_with(cp, case, b_rand, "default")
    assert kind == "zrec"
    xf, kindf = apply_with(cp, case, b_rand, "swap64pf")
    assert kindf == "fft"
    assert rel(x, xf) < 1e-13  # z ratio 0.02: the schedule-against-schedule bar


def test_over_the_cap_keeps_the_fft_kernel(cp, b_rand):
    x, kind = apply_with(cp, OVER_CAP, b_rand, "default")
    assert kind == "fft"
    xf, _ = apply_with(cp, OVER_CAP, b_rand, "swap64pf")
    assert torch.equal(x, xf)


def test_other_shapes_schedules_grids_and_symbols_stay_fft(cp):
    case = ELIGIBLE["advdiff"]
    with cp.CirculantPlan(N3) as plan:
        plan.set_advdiff_symbol(*case)
        assert plan.mid_kernel() == "zrec2"
        for mid in ("swap64pf", "swap64", "lane64", "lane32", "blocked"):
            plan.set_three_pass_shape(0, mid)
            assert plan.mid_kernel() == "fft"
        plan.set_three_pass_shape(64, "default")
        assert plan.mid_kernel() == "fft"
        plan.set_three_pass_shape(0, "default").set_schedule("five")
        assert plan.mid_kernel() == "fft"
        plan.set_schedule("auto")
        assert plan.mid_kernel() == "zrec2"
        s = [cp.advdiff_symbol_1d(256, l, m) for l, m in zip(*case)]
        plan.set_separable_symbol(s[0], s[1], s[2], (1, 1, 1))  # the same symbol, given as vectors
        assert plan.mid_kernel() == "fft"
    with cp.CirculantPlan((128, 128, 128)) as plan:
        plan.set_advdiff_symbol(*case)
        assert plan.mid_kernel() == "fft"


@pytest.mark.parametrize("graph", [False, True])
def test_live_plan_follows_symbol(cp, b_rand, graph):
    """One plan through transport -> advdiff -> over-cap advdiff -> transport: each apply equals a
    fresh plan's."""
    def fresh(setter):
        with cp.CirculantPlan(N3) as plan:
            setter(plan)
            k = plan.mid_kernel()
            x = plan.apply(b_rand)
            torch.cuda.synchronize()
        return x, k

    seq = [(lambda p: p.set_transport_symbol(TRANSPORT), "zrec"),
           (lambda p: p.set_advdiff_symbol(*ELIGIBLE["diff1000"]), "zrec2"),
           (lambda p: p.set_advdiff_symbol(*OVER_CAP), "fft"),
           (lambda p: p.set_advdiff_symbol(*ELIGIBLE["complex"]), "zrec2"),
           (lambda p: p.set_transport_symbol(TRANSPORT), "zrec")]
    with cp.CirculantPlan(N3) as plan:
        plan.set_graph(graph)
        out = torch.empty_like(b_rand)
        for setter, kind in seq:
            setter(plan)
            assert plan.mid_kernel() == kind
            plan.apply(b_rand, out=out)
            if graph:
                plan.apply(b_rand, out=out)  # the second apply of the pair replays the captured graph
            torch.cuda.synchronize()
            want, fkind = fresh(setter)
            assert fkind == kind
            assert torch.equal(out, want)


def test_deterministic_and_in_place(cp, b_rand):
    with cp.CirculantPlan(N3) as plan:
        plan.set_advdiff_symbol(*ELIGIBLE["diff1000"])
        assert plan.mid_kernel() == "zrec2"
        x1 = plan.apply(b_rand)
        x2 = plan.apply(b_rand)
        assert torch.equal(x1, x2)
        t = b_rand.clone()
        plan.apply(t, out=t)
        assert torch.equal(t, x1)


def test_8_byte_aligned(cp, b_rand, solved):
    """b and x 8 bytes past a 16-byte boundary: the kernel runs without its LDS-DMA prefetch."""
    from circulantpreconditioner_amd._lib import check, lib
    case = ELIGIBLE["diff1000"]
    x, xf = solved("diff1000")
    raw = torch.empty(2 * N + 1, dtype=torch.float64, device="cuda")
    raw[1:].copy_(torch.view_as_real(b_rand).reshape(-1))
    ptr = raw.data_ptr() + 8
    with cp.CirculantPlan(N3) as plan:
        plan.set_advdiff_symbol(*case)
        assert plan.mid_kernel() == "zrec2"
        check(lib().cfp_plan_apply(plan._h, ptr, ptr, None))
        torch.cuda.synchronize()
    got = torch.view_as_complex(raw[1:].clone().reshape(-1, 2))
    err = rel(got, xf)
    print(f"zrec2 unaligned vs fft: {err:.3e}; vs aligned zrec2: {rel(got, x):.3e}")
    assert err < bound(cp, case)
    assert rel(got, x) < bound(cp, case)


@pytest.mark.parametrize("dims", [(32, 16, 24), (100, 100, 100), (128, 128, 128)])
def test_other_grids_vs_oracle(cp, oracle, dims):
    case = ELIGIBLE["advdiff"]
    n = dims[0] * dims[1] * dims[2]
    b = torch.empty(n, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(b, 5)
    with cp.CirculantPlan(dims) as plan:
        plan.set_advdiff_symbol(*case)
        x = plan.apply(b)
        torch.cuda.synchronize()
    ref = oracle.c_solve_3d(np_diag(dims, *case), b.cpu().numpy(), dims)
    err = oracle.rel_l2(x.cpu().numpy(), ref)
    print(f"advdiff setter {dims} vs oracle: {err:.3e}")
    assert err < TOL


def test_get_diag_is_the_closed_form(cp):
    dims = (32, 16, 24)
    case = ELIGIBLE["complex"]
    with cp.CirculantPlan(dims) as plan:
        plan.set_advdiff_symbol(*case)
        d = plan.get_diag().cpu().numpy()
    ref = np_diag(dims, *case)
    assert np.abs(d - ref).max() <= 16 * np.finfo(float).eps * np.abs(ref).max()
