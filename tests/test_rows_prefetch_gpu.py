"""The 256^3 row sweeps P1 / P3 with the LDS-DMA prefetch of the next unit (k_tp_rows<.., NPF>).

The prefetching form exists at 256^3 only (one GPU, default y split, natural layout), so every
case runs there; an apply takes 0.3 ms.  References: the 5-pass schedule in the same process and
the residual ||C x - b|| / ||b|| that bench.py checks.  b comes from fill_uniform, so every point
is distinct and a slot taken from the wrong unit, row or lane shows up.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

G = (256, 256, 256)
N = 256 ** 3
LAM = (0.6, 0.15, 0.02)  # bench.py's symbol (z by recurrence under the default shape)


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return cp


def _fill(cp, seed):
    b = torch.empty(N, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(b, seed)
    return b


@pytest.fixture(scope="module")
def case(cp):
    """b, its 5-pass solution and its 3-sweep solution under the default shape (computed once, read only)."""
    b = _fill(cp, 20251017)
    with cp.CirculantPlan(G) as plan:
        plan.set_transport_symbol(LAM).set_schedule("five")
        x5 = plan.apply(b)
        plan.set_schedule("three")
        x3 = plan.apply(b)
    torch.cuda.synchronize()
    return b, x5, x3


def _relmax(x, ref):
    return float((x - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("mid", ["default", "swap64pf"])
def test_against_five_pass_and_residual(cp, case, mid):
    """Default plan and swap64pf (the FFT P2 between the same sweeps): against the 5-pass schedule
    (the bound test_gpu_parity uses for shape changes) and the residual of the circulant."""
    from bench import transport_residual
    b, x5, _ = case
    with cp.CirculantPlan(G) as plan:
        plan.set_transport_symbol(LAM).set_schedule("three").set_three_pass_shape(0, mid)
        assert [p["mode"] for p in plan.passes()] == ["rows_fwd", "mid_fused", "rows_inv"]
        x = plan.apply(b)
    d, res = _relmax(x, x5), transport_residual(b, x, G, LAM)
    print(f"{mid}: rel max diff to five {d:.3e}, residual {res:.3e}")
    assert d < 1e-13
    assert res < 1e-10


def test_in_place_bit_equal(cp, case):
    b, _, x3 = case
    t = b.clone()
    with cp.CirculantPlan(G) as plan:
        plan.set_transport_symbol(LAM)
        plan.apply(t, out=t)
    assert torch.equal(t, x3)


@pytest.mark.parametrize("which", ["b", "x"])
def test_unaligned_source_runs_the_plain_sweep_bit_equal(cp, case, which):
    """b (P1's source) or x (P3's source, and P2's array) 8 bytes past a 16-byte boundary: that
    sweep runs without the prefetch, the other with it, and the result is bit-equal to the aligned
    run -- the alignment test looks at the pointer the DMA reads, and both forms do the same
    arithmetic."""
    from circulantpreconditioner_amd._lib import check, lib
    b, _, x3 = case
    raw = torch.empty(2 * N + 1, dtype=torch.float64, device="cuda")  # raw[1:] starts 8 bytes past a 16-byte boundary
    assert raw.data_ptr() % 16 == 0
    with cp.CirculantPlan(G) as plan:
        plan.set_transport_symbol(LAM)
        if which == "b":
            raw[1:].copy_(torch.view_as_real(b).reshape(-1))
            x = torch.empty_like(b)
            check(lib().cfp_plan_apply(plan._h, raw.data_ptr() + 8, x.data_ptr(), None))
            torch.cuda.synchronize()
        else:
            check(lib().cfp_plan_apply(plan._h, b.data_ptr(), raw.data_ptr() + 8, None))
            torch.cuda.synchronize()
            x = torch.view_as_complex(raw[1:].clone().reshape(-1, 2))
    assert torch.equal(x, x3)


def test_three_applies_on_one_plan(cp, case):
    """Three right-hand sides in a row on one plan: each matches its own 5-pass result (nothing of
    one apply's last prefetch reaches the next)."""
    bs = [case[0], _fill(cp, 7), _fill(cp, 99)]
    with cp.CirculantPlan(G) as plan:
        plan.set_transport_symbol(LAM).set_schedule("three")
        xs = [plan.apply(b) for b in bs]
        plan.set_schedule("five")
        for i, (b, x) in enumerate(zip(bs, xs)):
            x5 = case[1] if i == 0 else plan.apply(b)
            d = _relmax(x, x5)
            print(f"apply {i}: rel max diff to five {d:.3e}")
            assert d < 1e-13
