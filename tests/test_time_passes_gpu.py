"""time_passes of the four plan classes (cfp_plan / cfp_rplan / cfp_wave_plan / cfp_wave_rplan
_time_passes, one shared pass timer): one mean per pass of the schedule, every mean a finite
positive time, the timed applies leave x = apply(b) bit for bit, and iters < 1 is refused.  Small
grids on every schedule shape the timer meets: a start and a stop event per pass (CirculantPlan),
one event per boundary (the others), 3-D and 2-D wave grids, the real wave plan on float64 and on
the real parts of complex128 (es = 1 and 2)."""
import math

import pytest

pytestmark = pytest.mark.gpu
LAM = (0.6, 0.15, 0.02)
KAPPA = (0.079, 0.05, 0.11)


def make(kind):
    """(plan with its symbol set, number of passes, seeded b on the device)"""
    import torch

    import circulantpreconditioner_amd as cp
    from circulantpreconditioner_amd import wave as W
    g = torch.Generator(device="cuda").manual_seed(20251021)
    if kind == "plan":
        plan = cp.CirculantPlan((32, 6, 5)).set_transport_symbol(LAM)
        return plan, len(plan.passes()), torch.randn(plan.N, dtype=torch.complex128, device="cuda", generator=g)
    if kind == "rplan":
        plan = cp.RealPlan((32, 6, 5)).set_transport_symbol(LAM)
        return plan, 4, torch.randn(plan.N, dtype=torch.float64, device="cuda", generator=g)
    if kind in ("wave3d", "wave2d"):
        plan = W.WavePlan((16, 6, 5)) if kind == "wave3d" else W.WavePlan((50, 50), dim=2)
        plan.set_symbol(KAPPA if kind == "wave3d" else (KAPPA[0], KAPPA[1], 0.0))
        return plan, plan.num_passes(), torch.randn(plan.size, dtype=torch.complex128, device="cuda", generator=g)
    dims, dim = {"rwave3d": ((32, 6, 5), 3), "rwave2d": ((32, 24), 2)}[kind[:-4]]
    dtype = torch.float64 if kind.endswith("es1") else torch.complex128
    plan = W.RealWavePlan(dims, dim=dim).set_symbol(KAPPA if dim == 3 else (KAPPA[0], KAPPA[1], 0.0))
    b = torch.randn(plan.size, dtype=torch.float64, device="cuda", generator=g)
    return plan, plan.num_passes(), b if dtype == torch.float64 else b.to(torch.complex128)


KINDS = ["plan", "rplan", "wave3d", "wave2d", "rwave3d_es1", "rwave3d_es2", "rwave2d_es1", "rwave2d_es2"]


@pytest.mark.parametrize("kind", KINDS)
def test_time_passes(kind):
    import torch
    plan, npass, b = make(kind)
    ref = plan.apply(b)
    x = torch.zeros_like(b)
    ms = plan.time_passes(b, x, iters=3)
    torch.cuda.synchronize()
    print(f"{kind}: {npass} passes, ms {['%.4f' % v for v in ms]}")
    assert len(ms) == npass and npass >= 1
    assert all(math.isfinite(v) and v > 0.0 for v in ms)
    assert torch.equal(x, ref)
    plan.close()


@pytest.mark.parametrize("kind", KINDS)
def test_time_passes_refuses_zero_iters(kind):
    import torch

    import circulantpreconditioner_amd as cp
    plan, _, b = make(kind)
    with pytest.raises(cp.CirculantError, match="iters must be >= 1") as ei:
        plan.time_passes(b, torch.zeros_like(b), iters=0)
    assert ei.value.code == 63  # CFP_ERR_ARG_OUTOFRANGE
    plan.close()
