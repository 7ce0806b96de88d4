"""The advection-diffusion symbol on the real-data plan (RealPlan.set_advdiff_symbol), the
two-sided z recurrence as the 256^3 half-spectrum middle sweep (k_tp_mid_rec2_half,
RealPlan.set_mid_kernel("rec")) and the diffusion boundary of the real-scalar library
(include/diffusion_equation.h in libcirculant_fft_real.so).

References: the oracle's solve of the same real b; the same plan with the FFT middle kernel; and
the complex plan with shape 'swap64pf' on the promoted b, which shares no table and no kernel with
the real plan's recurrence.

Bounds (the rule of test_advdiff_gpu.py): the oracle bar is 1e-10; two schedules of the same apply
agree to 1e-13 where both z ratios are <= 0.5; above that 8 * 2.2e-16 / ((1 - ra) (1 - rb)) with
ra, rb = advdiff_z_ratio(256, 256, lam, mu), the maxima over the columns (for real lam, mu a
half-spectrum column and its mirror have conjugate factors: the full grid's maxima are the half's)."""
import ctypes

import numpy as np
import pytest
import torch

from advdiff_cases import ELIGIBLE, apply_operator, bound as ratio_bound, diag as np_diag

pytestmark = pytest.mark.gpu
TOL = 1e-10
N3 = (256, 256, 256)
N = 256 ** 3
REAL_CASES = [k for k in ELIGIBLE if k != "complex"]  # 'complex' is no Hermitian symbol
OVER_CAP = ((0, 0, 0), (0.3, 0.3, 1e6))
TRANSPORT = (0.6, 0.15, 0.02)
PURE_DIFFUSION = ((0, 0, 0), (0.3, 0.2, 0.7))
# what CFP_RMID_AUTO launches for an eligible symbol at 256^3: the measured default (DESIGN.md
# "256^3 real P2", profiles/r12_real_zrec2_ab.txt)
AUTO_KERNEL = "zrec2"


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


def real_rand(cp, n, seed):
    """real random b: fill_uniform on a complex buffer, real part"""
    z = torch.empty(n, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(z, seed)
    return z.real.contiguous()


def real_apply(cp, dims, setter, b, mid="auto", schedule="auto"):
    with cp.RealPlan(dims) as plan:
        setter(plan)
        plan.set_schedule(schedule).set_mid_kernel(mid)
        kind = plan.mid_kernel()
        x = plan.apply(b)
        torch.cuda.synchronize()
    return x, kind


def advdiff(case):
    return lambda p: p.set_advdiff_symbol(*case)


def complex_fft_apply(cp, case, b):
    """the complex plan, FFT middle kernel always, on the promoted b: real part"""
    with cp.CirculantPlan(N3) as plan:
        plan.set_advdiff_symbol(*case).set_three_pass_shape(0, "swap64pf")
        assert plan.mid_kernel() == "fft"
        z = plan.apply(torch.complex(b, torch.zeros_like(b)))
        torch.cuda.synchronize()
    return z.real.contiguous()


@pytest.fixture(scope="module")
def b_rand(cp):
    return real_rand(cp, N, 77)


@pytest.fixture(scope="module")
def solved(cp, b_rand):
    """(x of the recurrence, x of the same plan's FFT kernel, x of the complex plan) per case, once."""
    cache = {}

    def get(name):
        if name not in cache:
            x, kind = real_apply(cp, N3, advdiff(ELIGIBLE[name]), b_rand, "rec")
            assert kind == "zrec2"
            xf, kindf = real_apply(cp, N3, advdiff(ELIGIBLE[name]), b_rand, "fft")
            assert kindf == "fft"
            cache[name] = (x, xf, complex_fft_apply(cp, ELIGIBLE[name], b_rand))
        return cache[name]
    return get


# ------------------------------------------------------------------ the setter on other grids
GRIDS = [((32, 16, 24), "auto"), ((64, 20, 12), "auto"), ((128, 128, 128), "auto"), ((128, 128, 128), "five")]


@pytest.mark.parametrize("case", [ELIGIBLE["advdiff"], PURE_DIFFUSION], ids=["advdiff", "lam0"])
@pytest.mark.parametrize("dims,schedule", GRIDS, ids=[f"{d[0]}x{d[1]}x{d[2]}-{s}" for d, s in GRIDS])
def test_setter_vs_oracle(cp, oracle, dims, schedule, case):
    n = dims[0] * dims[1] * dims[2]
    b = real_rand(cp, n, 5)
    with cp.RealPlan(dims) as plan:
        plan.set_advdiff_symbol(*case).set_schedule(schedule).set_mid_kernel("rec")
        assert plan.mid_kernel() == "fft"  # the recurrence exists at 256^3 only
        assert plan.three_sweep == (dims[0] == 128 and schedule == "auto")
        x = plan.apply(b)
        torch.cuda.synchronize()
    ref = oracle.c_solve_3d(np_diag(dims, *case), b.cpu().numpy().astype(np.complex128), dims)
    assert np.linalg.norm(ref.imag) / np.linalg.norm(ref) < 1e-13  # real b, Hermitian symbol
    err = oracle.rel_l2(x.cpu().numpy(), ref.real)
    print(f"real advdiff setter {dims} {schedule}: rel L2 vs oracle {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("dims,schedule", GRIDS + [(N3, "auto"), (N3, "five")],
                         ids=[f"{d[0]}x{d[1]}x{d[2]}-{s}" for d, s in GRIDS + [(N3, "auto"), (N3, "five")]])
def test_mu_zero_is_the_transport_setter_bit_for_bit(cp, dims, schedule):
    b = real_rand(cp, dims[0] * dims[1] * dims[2], 6)
    xa, ka = real_apply(cp, dims, lambda p: p.set_advdiff_symbol(TRANSPORT, (0, 0, 0)), b, "rec", schedule)
    xt, kt = real_apply(cp, dims, lambda p: p.set_transport_symbol(TRANSPORT), b, "rec", schedule)
    assert ka == "fft" and kt == "fft"
    assert torch.equal(xa, xt)


def test_complex_numbers_are_rejected(cp):
    with cp.RealPlan((32, 16, 24)) as plan:
        with pytest.raises(ValueError):
            plan.set_advdiff_symbol((0.3 + 0.2j, 1.1, 0.3), (0.1, 0.1, 0.7))
        with pytest.raises(ValueError):
            plan.set_advdiff_symbol((0.3, 1.1, 0.3), (0.1, 0.1, 0.7 - 0.1j))
        with pytest.raises(Exception) as e:
            plan.apply(torch.zeros(32 * 16 * 24, dtype=torch.float64, device="cuda"))
        assert "cfp_rplan_set_symbol_advdiff" in str(e.value) and "cfp_rplan_set_symbol_transport" in str(e.value)


# ------------------------------------------------------------------ 256^3, the recurrence
@pytest.mark.parametrize("name", REAL_CASES)
def test_agrees_with_the_fft_kernel(cp, solved, name):
    x, xf, _ = solved(name)
    err = rel(x, xf)
    ra, rb = cp.advdiff_z_ratio(256, 256, *ELIGIBLE[name])
    print(f"real zrec2 vs fft [{name}]: ratios {ra:.6f} {rb:.6f} rel L2 {err:.3e} bound {bound(cp, ELIGIBLE[name]):.3e}")
    assert err < bound(cp, ELIGIBLE[name])


@pytest.mark.parametrize("name", REAL_CASES)
def test_agrees_with_the_complex_plan(cp, solved, name):
    x, _, xc = solved(name)
    err = rel(x, xc)
    print(f"real zrec2 vs complex swap64pf [{name}]: rel L2 {err:.3e} bound {bound(cp, ELIGIBLE[name]):.3e}")
    assert err < bound(cp, ELIGIBLE[name])


def circulant_apply(x, case):
    """C x of the advection-diffusion circulant on a real field, by rolls in both directions of every axis."""
    lam, mu = case
    v = x.view(256, 256, 256)
    y = v.clone()
    for d, dim in enumerate((2, 1, 0)):  # x is the fastest axis = the last dim
        l, m = float(lam[d]), float(mu[d])
        down, up = torch.roll(v, 1, dim), torch.roll(v, -1, dim)  # v[i - 1], v[i + 1]
        y += (l + 2 * m) * v - (l + m) * down - m * up
    return y.reshape(-1)


@pytest.mark.parametrize("name", REAL_CASES)
def test_residual(cp, solved, b_rand, name):
    x, _, _ = solved(name)
    res = rel(circulant_apply(x, ELIGIBLE[name]), b_rand)
    print(f"real zrec2 residual [{name}]: {res:.3e} bound {bound(cp, ELIGIBLE[name]):.3e}")
    assert res < bound(cp, ELIGIBLE[name])


def test_oracle_diff1000(solved, b_rand, oracle):
    x, _, _ = solved("diff1000")
    ref = oracle.c_solve_3d(np_diag(N3, *ELIGIBLE["diff1000"]), b_rand.cpu().numpy().astype(np.complex128), N3)
    err = oracle.rel_l2(x.cpu().numpy(), ref.real)
    print(f"real zrec2 vs oracle [diff1000]: {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("z0", [0, 15, 16, 255])
def test_impulse_carries_and_wrap(cp, z0):
    """mu_z = 1000: |a| = |b| = 0.97, so a^16 = 0.6 and the carries between slots, waves and across
    the cyclic closure matter in both directions.  z0 = 15 / 16: a block's last and the next
    block's first point; 0 / 255: the two ends of the wrap."""
    case = ELIGIBLE["diff1000"]
    x0, y0 = 37, 101
    b = torch.zeros(N, dtype=torch.float64, device="cuda")
    b[x0 + 256 * (y0 + 256 * z0)] = 1.0
    x, kind = real_apply(cp, N3, advdiff(case), b, "rec")
    assert kind == "zrec2"
    xf, _ = real_apply(cp, N3, advdiff(case), b, "fft")
    err = rel(x, xf)
    print(f"real zrec2 impulse z0={z0}: rel L2 {err:.3e} bound {bound(cp, case):.3e}")
    assert err < bound(cp, case)
    col = x.view(256, 256, 256)[:, y0, x0]
    assert bool((col[0:6].abs() > 0).all()) and bool((col[250:256].abs() > 0).all())  # both sides of the wrap


def test_impulses_at_the_row_ends(cp):
    """Impulses at x0 = 0 and x0 = 255 excite every Fourier mode in x: kx = 0, the last
    half-spectrum column kx = 127 and the Nyquist column (which keeps its FFT kernel) all count."""
    case = ELIGIBLE["diff1000"]
    y0 = 101
    b = torch.zeros(N, dtype=torch.float64, device="cuda")
    b[0 + 256 * (y0 + 256 * 100)] = 1.0
    b[255 + 256 * (y0 + 256 * 200)] = -0.5
    x, kind = real_apply(cp, N3, advdiff(case), b, "rec")
    assert kind == "zrec2"
    xf, _ = real_apply(cp, N3, advdiff(case), b, "fft")
    err = rel(x, xf)
    print(f"real zrec2 impulses at x0 = 0 and 255: rel L2 {err:.3e} bound {bound(cp, case):.3e}")
    assert err < bound(cp, case)
    v = x.view(256, 256, 256)
    assert float(v[100, y0, 0]) > 0 > float(v[200, y0, 255])


# ------------------------------------------------------------------ routing
def test_routing(cp):
    case = ELIGIBLE["advdiff"]
    with cp.RealPlan(N3) as plan:
        plan.set_mid_kernel("rec")
        plan.set_advdiff_symbol(*case)
        assert plan.mid_kernel() == "zrec2"
        plan.set_advdiff_symbol(*OVER_CAP)
        assert plan.mid_kernel() == "fft"
        plan.set_advdiff_symbol(case[0], (0.2, 0.2, 0))  # mu_z = 0
        assert plan.mid_kernel() == "fft"
        plan.set_transport_symbol(TRANSPORT)
        assert plan.mid_kernel() == "fft"
        plan.set_advdiff_symbol(*case)
        assert plan.mid_kernel() == "zrec2"
        plan.set_schedule("five")
        assert plan.mid_kernel() == "fft"
        plan.set_schedule("three")
        assert plan.mid_kernel() == "zrec2"
        plan.set_mid_kernel("fft")
        assert plan.mid_kernel() == "fft"
        plan.set_mid_kernel("auto")
        assert plan.mid_kernel() == AUTO_KERNEL
        with pytest.raises(Exception):
            plan.set_mid_kernel(7)
    with cp.RealPlan((128, 128, 128)) as plan:
        plan.set_advdiff_symbol(*case).set_mid_kernel("rec")
        assert plan.three_sweep and plan.mid_kernel() == "fft"


@pytest.mark.parametrize("alias", [False, True], ids=["out_of_place", "in_place"])
def test_live_plan_follows_symbol(cp, b_rand, alias):
    """One live plan through eligible advdiff -> transport -> over-cap advdiff -> another eligible
    advdiff: each apply equals a fresh plan's, bit for bit."""
    seq = [(advdiff(ELIGIBLE["diff1000"]), "zrec2"),
           (lambda p: p.set_transport_symbol(TRANSPORT), "fft"),
           (advdiff(OVER_CAP), "fft"),
           (advdiff(ELIGIBLE["advdiff"]), "zrec2")]
    with cp.RealPlan(N3) as plan:
        plan.set_mid_kernel("rec")
        for setter, kind in seq:
            setter(plan)
            assert plan.mid_kernel() == kind
            if alias:
                out = b_rand.clone()
                plan.apply(out, out=out)
            else:
                out = plan.apply(b_rand)
            torch.cuda.synchronize()
            want, fkind = real_apply(cp, N3, setter, b_rand, "rec")
            assert fkind == kind
            assert torch.equal(out, want)


# ------------------------------------------------------------------ the real-scalar library
@pytest.fixture(scope="module")
def R():
    from circulantpreconditioner_amd import petsc_real as R
    R.lib()
    return R


@pytest.fixture(scope="module")
def dif():
    from circulantpreconditioner_amd import diffusion
    return diffusion


def _half(full, nx):
    """[nz][ny][nx] complex -> the r2c half spectrum as interleaved reals"""
    return np.ascontiguousarray(full[..., : nx // 2 + 1]).view(np.float64).reshape(-1)


def _oracle_real(oracle, dims, case, b, scale=1.0):
    x = oracle.c_solve_3d(scale * np_diag(dims, *case), b.astype(np.complex128), dims)
    assert np.linalg.norm(x.imag) / np.linalg.norm(x) < 1e-13
    return x.real


def _diffusion_ctx(R, dims, case):
    lam, mu = case
    return R.FFTPrecDiffusionContext(3, dims[0], dims[1], dims[2], lam[0], lam[1], lam[2], None, None, None, None,
                                     None, mu[0], mu[1], mu[2])


def _destroy_pc(R, pc):
    pcp = ctypes.c_void_p(pc.value)
    R.PetscCall(R.lib().PCDestroy(ctypes.byref(pcp)))


# (32, 16, 24): the real plan serves it; (20, 12, 8): it lacks the grid, the promoted complex plan runs
@pytest.mark.parametrize("dims", [(32, 16, 24), (20, 12, 8)])
def test_real_diffusion_pcshell(R, oracle, dims):
    """The diffusion PCSHELL on real HIP Vecs: PCApply with the symbol setup materialised, Diag
    after setup, then PCApply with a Diag the caller changed (the explicit-Diag path)."""
    nx, ny, nz = dims
    n = nx * ny * nz
    case = ELIGIBLE["advdiff"]
    ctx = _diffusion_ctx(R, dims, case)
    pc = R.pc_shell(ctx)
    assert (R.mat_real_plan_mid_kernel(ctypes.c_void_p(ctx.FFT_MAT)) == "none") == (dims == (20, 12, 8))
    b = oracle.c_fill_uniform(n, 43).real.copy()
    vb, vx = R.Vec.seq(n, hip=True).set_array(b), R.Vec.seq(n, hip=True)
    R.PetscCall(R.lib().PCApply(pc, vb.h, vx.h))
    ref = _oracle_real(oracle, dims, case, b)
    err = np.linalg.norm(vx.array() - ref) / np.linalg.norm(ref)
    print(f"real diffusion PCSHELL {dims}: rel L2 vs oracle {err:.3e}")
    assert err < TOL
    diag = R.Vec.borrow(ctx.Diag)
    np.testing.assert_allclose(diag.array(), _half(np_diag(dims, *case).reshape(nz, ny, nx), nx), rtol=0, atol=1e-14)
    R.PetscCall(R.lib().VecScale(diag.h, 2.0))  # the caller changes Diag: solve_3D divides by it
    R.PetscCall(R.lib().PCApply(pc, vb.h, vx.h))
    err2 = np.linalg.norm(vx.array() - ref / 2) / np.linalg.norm(ref / 2)
    assert err2 < TOL
    own, expl = ctypes.c_int64(), ctypes.c_int64()
    R.PetscCall(R.lib().MatFFTHIPGetSolveCounts(ctypes.c_void_p(ctx.FFT_MAT), ctypes.byref(own), ctypes.byref(expl)))
    assert (own.value, expl.value) == (1, 1)
    vb.destroy()
    vx.destroy()
    _destroy_pc(R, pc)


def test_real_diffusion_pcshell_256_routing_and_result(cp, R, solved, b_rand):
    """After setupFFTPrec3DDiffusion with an eligible symbol the Mat's real plan reports the kernel a
    bare RealPlan reports under AUTO, and PCApply is that plan's apply."""
    case = ELIGIBLE["advdiff"]
    ctx = _diffusion_ctx(R, N3, case)
    pc = R.pc_shell(ctx)
    with cp.RealPlan(N3) as plan:
        plan.set_advdiff_symbol(*case)
        bare = plan.mid_kernel()
    assert bare == AUTO_KERNEL
    assert R.mat_real_plan_mid_kernel(ctypes.c_void_p(ctx.FFT_MAT)) == bare
    vb, vx = R.Vec.seq(N, hip=True).set_array(b_rand.cpu().numpy()), R.Vec.seq(N, hip=True)
    R.PetscCall(R.lib().PCApply(pc, vb.h, vx.h))
    x, xf, _ = solved("advdiff")
    want = (x if bare == "zrec2" else xf).cpu().numpy()
    assert np.array_equal(vx.array(), want)
    vb.destroy()
    vx.destroy()
    _destroy_pc(R, pc)


@pytest.mark.parametrize("in_place", [False, True])
def test_real_direct_solver_vs_oracle(R, oracle, in_place):
    dims = (32, 16, 24)
    nx, ny, nz = dims
    n = nx * ny * nz
    a, nu, dt, h = (1.0, 0.5, 2.0), 0.3, 0.07, (0.25, 0.5, 0.2)
    b = oracle.c_fill_uniform(n, 9).real.copy()
    F = R.mat_create_fft([nz, ny, nx])
    ctx = R.StructuredDiffusionContext(nx, ny, nz, a[0], a[1], a[2], nu, dt, h[0], h[1], h[2], F)
    vb = R.Vec.seq(n, hip=True).set_array(b)
    vx = vb if in_place else R.Vec.seq(n, hip=True)
    R.PetscCall(R.lib().PetscFft3DDiffusionSolver(ctx, vb.h, vx.h))
    got = vx.array()
    vb2, vx2 = R.Vec.seq(n, hip=True).set_array(b), R.Vec.seq(n, hip=True)
    R.PetscCall(R.lib().PetscFft3DDiffusionSolver(ctx, vb2.h, vx2.h))  # equal numbers: the symbol is kept
    assert np.array_equal(got, vx2.array())
    case = ([a[d] * dt / h[d] for d in range(3)], [nu * dt / h[d] ** 2 for d in range(3)])
    ref = _oracle_real(oracle, dims, case, b)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"real PetscFft3DDiffusionSolver {dims} in_place={in_place} vs oracle: {err:.3e}")
    assert err < TOL
    own, expl = ctypes.c_int64(), ctypes.c_int64()
    R.PetscCall(R.lib().MatFFTHIPGetSolveCounts(F, ctypes.byref(own), ctypes.byref(expl)))
    assert (own.value, expl.value) == (2, 0)
    for v in {vb, vx, vb2, vx2}:
        v.destroy()
    R.PetscCall(R.lib().MatDestroy(ctypes.byref(F)))


def grid_h(cfg):
    return [(cfg.xmax[d] - cfg.xmin[d]) / n for d, n in enumerate((cfg.nx, cfg.ny, cfg.nz))]


def test_real_gmres_periodic_converges_in_one_iteration(dif):
    dims = (32, 32, 32)
    kw = dict(bc="periodic", a=(1.0, 0.5, 0.25), nu=0.5, dt=0.01, real=True)
    cfg = dif.config(dims, pc="fft", steps=3, **kw)
    res = dif.run(cfg, real=True)
    print(f"real periodic {dims}: its per step {res['min_step_its']}..{res['max_step_its']} residual {res['last_residual']:.2e}")
    assert res["steps"] == 3 and res["all_converged"] == 1
    assert res["min_step_its"] == 1 and res["max_step_its"] == 1
    h = grid_h(cfg)
    assert res["lambda"] == pytest.approx([cfg.a[d] * cfg.dt / h[d] for d in range(3)], rel=1e-14)
    assert res["mu"] == pytest.approx([cfg.nu * cfg.dt / h[d] ** 2 for d in range(3)], rel=1e-14)
    # one step inverts the periodic operator and matches the direct solver
    _, u0 = dif.run(dif.config(dims, steps=0, **kw), return_field=True, real=True)
    cfg1 = dif.config(dims, pc="fft", steps=1, **kw)
    _, u1 = dif.run(cfg1, return_field=True, real=True)
    assert u1.dtype == np.float64
    r = np.linalg.norm(apply_operator(u1, dims, h, cfg1.dt, list(cfg1.a), cfg1.nu, True) - u0) / np.linalg.norm(u0)
    assert r <= 10 * cfg1.precision
    rd, ud = dif.run_direct(dif.config(dims, steps=1, **kw), return_field=True, real=True)
    assert rd["steps"] == 1
    assert np.linalg.norm(ud - u1) / np.linalg.norm(u1) <= 10 * cfg1.precision


def test_real_gmres_wall_beats_pcnone_and_solves_the_operator(dif):
    dims = (24, 24, 24)
    kw = dict(bc="wall", a=(1.0, 0.0, 0.0), nu=0.1, dt=0.01, real=True)
    fft = dif.run(dif.config(dims, pc="fft", steps=2, **kw), real=True)
    none = dif.run(dif.config(dims, pc="none", steps=2, **kw), real=True)
    print(f"real wall {dims}: total its fft {fft['total_its']} none {none['total_its']}")
    assert fft["all_converged"] == 1 and none["all_converged"] == 1
    assert fft["steps"] == 2 and none["steps"] == 2
    assert fft["total_its"] < none["total_its"]
    assert fft["pc_calls"] > 0 and fft["fused_dots"] == 0
    _, u0 = dif.run(dif.config(dims, steps=0, **kw), return_field=True, real=True)
    assert set(np.unique(u0)) == {600.0, 650.0}
    cfg = dif.config(dims, pc="fft", steps=1, **kw)
    r, u1 = dif.run(cfg, return_field=True, real=True)
    res = np.linalg.norm(apply_operator(u1, dims, grid_h(cfg), cfg.dt, list(cfg.a), cfg.nu, False) - u0) / np.linalg.norm(u0)
    print(f"real wall one step: its {r['total_its']} |A U1 - U0| / |U0| = {res:.2e}")
    assert r["all_converged"] == 1
    assert res <= 10 * cfg.precision
