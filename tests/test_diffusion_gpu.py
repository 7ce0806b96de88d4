"""The advection-diffusion boundary on the GPU (include/diffusion_equation.h): the diffusion
PCSHELL inside the stand-in GMRES time loop, the direct solver and the operator's device form.

With periodic boundaries the operator is the circulant the PCSHELL inverts, so every solve takes
one iteration; with walls the preconditioner is approximate and must still beat PCNONE."""
import numpy as np
import pytest
import torch

from advdiff_cases import apply_operator, diag as np_diag

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope="module")
def dif():
    from circulantpreconditioner_amd import diffusion
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return diffusion


def grid_h(cfg):
    return [(cfg.xmax[d] - cfg.xmin[d]) / n for d, n in enumerate((cfg.nx, cfg.ny, cfg.nz))]


@pytest.mark.parametrize("dims", [(16, 16, 16), (32, 16, 24)])
def test_periodic_converges_in_one_iteration(dif, dims):
    cfg = dif.config(dims, bc="periodic", pc="fft", steps=3, a=(1.0, 0.5, 0.25), nu=0.5, dt=0.01)
    res = dif.run(cfg)
    print(f"periodic {dims}: its per step {res['min_step_its']}..{res['max_step_its']} residual {res['last_residual']:.2e}")
    assert res["steps"] == 3 and res["all_converged"] == 1
    assert res["min_step_its"] == 1 and res["max_step_its"] == 1
    h = grid_h(cfg)
    assert res["lambda"] == pytest.approx([cfg.a[d] * cfg.dt / h[d] for d in range(3)], rel=1e-14)
    assert res["mu"] == pytest.approx([cfg.nu * cfg.dt / h[d] ** 2 for d in range(3)], rel=1e-14)


def test_periodic_step_inverts_the_operator_and_matches_the_direct_solver(dif):
    dims = (32, 16, 24)
    kw = dict(bc="periodic", a=(1.0, 0.5, 0.25), nu=0.5, dt=0.01)
    _, u0 = dif.run(dif.config(dims, steps=0, **kw), return_field=True)
    cfg = dif.config(dims, pc="fft", steps=1, **kw)
    _, u1 = dif.run(cfg, return_field=True)
    res = np.linalg.norm(apply_operator(u1, dims, grid_h(cfg), cfg.dt, list(cfg.a), cfg.nu, True) - u0) / np.linalg.norm(u0)
    print(f"periodic one step: |A U1 - U0| / |U0| = {res:.2e}")
    assert res <= 10 * cfg.precision
    rd, ud = dif.run_direct(dif.config(dims, steps=1, **kw), return_field=True)
    assert rd["steps"] == 1
    assert np.linalg.norm(ud - u1) / np.linalg.norm(u1) <= 10 * cfg.precision


def test_wall_converges_and_beats_pcnone(dif):
    dims = (24, 24, 24)
    kw = dict(bc="wall", a=(1.0, 0.0, 0.0), nu=0.1, dt=0.01, steps=2)
    fft = dif.run(dif.config(dims, pc="fft", **kw))
    none = dif.run(dif.config(dims, pc="none", **kw))
    print(f"wall {dims}: total its fft {fft['total_its']} none {none['total_its']}")
    assert fft["all_converged"] == 1 and none["all_converged"] == 1
    assert fft["steps"] == 2 and none["steps"] == 2
    assert fft["total_its"] < none["total_its"]
    assert fft["pc_calls"] > 0 and fft["fused_dots"] == 0


def test_wall_step_solves_the_operator(dif):
    dims = (24, 24, 24)
    kw = dict(bc="wall", a=(1.0, 0.0, 0.0), nu=0.1, dt=0.01)
    _, u0 = dif.run(dif.config(dims, steps=0, **kw), return_field=True)
    assert set(np.unique(u0.real)) == {600.0, 650.0}
    cfg = dif.config(dims, pc="fft", steps=1, **kw)
    r, u1 = dif.run(cfg, return_field=True)
    res = np.linalg.norm(apply_operator(u1, dims, grid_h(cfg), cfg.dt, list(cfg.a), cfg.nu, False) - u0) / np.linalg.norm(u0)
    print(f"wall one step: its {r['total_its']} |A U1 - U0| / |U0| = {res:.2e}")
    assert r["all_converged"] == 1
    assert res <= 10 * cfg.precision


@pytest.mark.parametrize("in_place", [False, True])
def test_direct_solver_vs_oracle(dif, oracle, in_place):
    import circulantpreconditioner_amd as cp
    from circulantpreconditioner_amd.petsc import Mat, Vec
    dims = (32, 16, 24)
    a, nu, dt, h = (1.0, 0.5, 2.0), 0.3, 0.07, (0.25, 0.5, 0.2)
    n = dims[0] * dims[1] * dims[2]
    b = torch.empty(n, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(b, 9)
    b_host = b.cpu().numpy()
    b2, x2 = b.clone(), torch.zeros_like(b)
    x = b if in_place else torch.zeros_like(b)
    F = Mat.create_fft((dims[2], dims[1], dims[0]))
    ctx = dif.StructuredContext(*dims, *a, nu, dt, *h, F)
    vb = Vec.from_tensor(b)
    dif.PetscFft3DDiffusionSolver(ctx, vb, vb if in_place else Vec.from_tensor(x))
    dif.PetscFft3DDiffusionSolver(ctx, Vec.from_tensor(b2), Vec.from_tensor(x2))  # equal numbers: the symbol is kept
    torch.cuda.synchronize()
    assert torch.equal(x, x2)
    lam = [a[d] * dt / h[d] for d in range(3)]
    mu = [nu * dt / h[d] ** 2 for d in range(3)]
    ref = oracle.c_solve_3d(np_diag(dims, lam, mu), b_host, dims)
    err = oracle.rel_l2(x.cpu().numpy(), ref)
    print(f"PetscFft3DDiffusionSolver {dims} in_place={in_place} vs oracle: {err:.3e}")
    assert err < TOL
    assert F.solve_counts() == (2, 0)


def test_operator_takes_a_device_storage_form(dif):
    dims = (24, 24, 24)
    A = dif.operator(dims, (1 / 24,) * 3, 0.01, (1.0, 0.0, 0.0), 0.1, "wall")
    info = A.aij_info()
    print(f"advection-diffusion operator {dims}: {info}")
    assert info["format"] == "dia"
    assert info["nd"] == 7
