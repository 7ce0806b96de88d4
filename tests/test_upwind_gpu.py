"""The upwind symbol on the GPU: set_upwind_symbol on the three plan kinds against the numpy closed
form through the oracle, the backward recurrence middle kernel of the 256^3 3-sweep apply
(k_tp_mid_recb: k_tp_mid_rec on the planes in reverse order), its routing, the two upwind PCSHELL
setups in both scalar builds and the drivers' upwind modes.

Bounds, the project's own: against the oracle 1e-10; the recurrence against the FFT kernel
upwind_cases.bound(amax) = 8 * 2.2e-16 / (1 - amax) above amax = 0.5 (tests/test_zrec_gpu.py), amax
the backward ratio max |q / (1 + s_x + s_y + q)|, q = -lam_z; the circulant residual 1e-12."""
import ctypes

import numpy as np
import pytest
import torch

from upwind_cases import LAM0, MUS, SIGNS, apply_operator, back_ratio, bound, diag as up_diag, mapped, signed

pytestmark = pytest.mark.gpu
TOL = 1e-10
N3 = (256, 256, 256)
N = 256 ** 3
LAMB = (0.6, 0.15, -0.6)          # amax = 0.375
LAMB_MIRROR = (0.6, 0.15, 0.6)    # the forward kernel's symbol of the flip test
LAMC = (55.6, 0, -1e3 / 3)        # the reference driver's cfl against z: amax = 0.997
MU_Z = (0.2, 0.2, 2.5)
SMALL = [(32, 16, 24), (64, 20, 12)]


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return cp


@pytest.fixture(scope="module")
def SlabGroup():
    from circulantpreconditioner_amd.distributed import SlabGroup
    return SlabGroup


def rel(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


def group_apply(g, b):
    torch.cuda.synchronize()  # b is complete: the group's streams do not wait for torch's
    x = torch.cat(g.apply(g.scatter(b)))
    torch.cuda.synchronize()
    return x


# ---------------------------------------------------------------- small grids, every sign pattern
@pytest.fixture(scope="module")
def small_ref(oracle):
    """(b, oracle solve) per (dims, signs, mu name), computed once and shared by the plan kinds"""
    cache = {}

    def get(dims, signs, mu):
        key = (dims, signs, mu)
        if key not in cache:
            b = oracle.c_fill_uniform(int(np.prod(dims)), 23)
            ref = oracle.c_solve_3d(up_diag(dims, signed(signs), MUS[mu]), b, dims)
            cache[key] = (b, ref)
        return cache[key]
    return get


@pytest.mark.parametrize("mu", list(MUS))
@pytest.mark.parametrize("signs", SIGNS, ids=lambda s: "".join("+" if v > 0 else "-" for v in s))
@pytest.mark.parametrize("dims", SMALL)
def test_complex_plan_vs_oracle(cp, oracle, small_ref, dims, signs, mu):
    b, ref = small_ref(dims, signs, mu)
    with cp.CirculantPlan(dims) as plan:
        plan.set_upwind_symbol(signed(signs), MUS[mu])
        x = plan.apply(torch.from_numpy(b).cuda()).cpu().numpy()
    err = oracle.rel_l2(x, ref)
    print(f"upwind {dims} {signs} [{mu}]: vs oracle {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("schedule", ["three", "five"])
def test_complex_plan_128_vs_oracle(cp, oracle, schedule):
    dims, lam, mu = (128, 128, 128), (-0.6, 0.15, -0.4), MU_Z
    b = oracle.c_fill_uniform(128 ** 3, 29)
    ref = oracle.c_solve_3d(up_diag(dims, lam, mu), b, dims)
    with cp.CirculantPlan(dims) as plan:
        plan.set_schedule(schedule).set_upwind_symbol(lam, mu)
        assert plan.mid_kernel() == "fft"
        x = plan.apply(torch.from_numpy(b).cuda()).cpu().numpy()
    err = oracle.rel_l2(x, ref)
    print(f"upwind 128^3 [{schedule}]: vs oracle {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("mu", list(MUS))
@pytest.mark.parametrize("dims", SMALL)
def test_real_plan_vs_oracle(cp, oracle, small_ref, dims, mu):
    with cp.RealPlan(dims) as plan:
        for signs in SIGNS:
            b, _ = small_ref(dims, signs, mu)
            br = np.ascontiguousarray(b.real)
            ref = oracle.c_solve_3d(up_diag(dims, signed(signs), MUS[mu]), br.astype(np.complex128), dims)
            assert np.linalg.norm(ref.imag) <= 1e-13 * np.linalg.norm(ref)
            plan.set_upwind_symbol(signed(signs), MUS[mu])
            x = plan.apply(torch.from_numpy(br).cuda()).cpu().numpy()
            err = np.linalg.norm(x - ref.real) / np.linalg.norm(ref.real)
            print(f"real upwind {dims} {signs} [{mu}]: vs oracle {err:.3e}")
            assert err < TOL


@pytest.mark.parametrize("mu", list(MUS))
@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("dims", SMALL)
def test_slab_group_vs_oracle(SlabGroup, oracle, small_ref, dims, P, mu):
    with SlabGroup(dims, P) as g:
        for signs in SIGNS:
            b, ref = small_ref(dims, signs, mu)
            g.set_upwind_symbol(signed(signs), MUS[mu])
            assert g.mid_kernel() == "fft"
            x = group_apply(g, torch.from_numpy(b).cuda()).cpu().numpy()
            err = oracle.rel_l2(x, ref)
            print(f"slab upwind {dims} P={P} {signs} [{mu}]: vs oracle {err:.3e}")
            assert err < TOL


def test_slab_refill_keeps_the_mapped_numbers(SlabGroup, oracle, small_ref):
    """set_schedule and set_pieces refill the tables from what the plan remembers"""
    dims, signs = (32, 16, 24), (-1, 1, -1)
    b, ref = small_ref(dims, signs, "mu")
    with SlabGroup(dims, 2) as g:
        g.set_upwind_symbol(signed(signs), MUS["mu"])
        g.set_schedule("five")
        x = group_apply(g, torch.from_numpy(b).cuda()).cpu().numpy()
    assert oracle.rel_l2(x, ref) < TOL


@pytest.mark.parametrize("dims", [(32, 16, 24), N3])
def test_non_negative_numbers_are_the_existing_setters_bit_for_bit(cp, SlabGroup, dims):
    n = int(np.prod(dims))
    b = torch.empty(n, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(b, 5)
    br = b.real.contiguous()
    P = 2 if dims != N3 else 8
    for mu, other in ((MU_Z, "advdiff"), ((0, 0, 0), "transport")):
        def set_other(p):
            return p.set_advdiff_symbol(LAM0, mu) if other == "advdiff" else p.set_transport_symbol(LAM0)
        with cp.CirculantPlan(dims) as plan:
            x = plan.set_upwind_symbol(LAM0, mu).apply(b)
            kind = plan.mid_kernel()
            xo = set_other(plan).apply(b)
            assert plan.mid_kernel() == kind  # the routing too ('zrec2' / 'zrec' at 256^3)
            assert torch.equal(x, xo)
            if dims == N3:
                assert kind == ("zrec2" if other == "advdiff" else "zrec")
                xa = plan.set_advdiff_symbol(LAM0, mu).apply(b)
                assert torch.equal(x, xa)
        with cp.RealPlan(dims) as plan:
            x = plan.set_upwind_symbol(LAM0, mu).apply(br)
            kind = plan.mid_kernel()
            xo = set_other(plan).apply(br)
            assert torch.equal(x, xo)
            if other == "advdiff":
                assert plan.mid_kernel() == kind
        with SlabGroup(dims, P) as g:
            g.set_upwind_symbol(LAM0, mu)
            x, kind = group_apply(g, b), g.mid_kernel()
            set_other(g)
            assert torch.equal(x, group_apply(g, b))
            if other == "advdiff":
                assert g.mid_kernel() == kind


# ---------------------------------------------------------------- 256^3: the backward recurrence
@pytest.fixture(scope="module")
def b256(cp):
    b = torch.empty(N, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(b, 77)
    return b


def upwind_apply(cp, lam, b, mid="default", mu=(0, 0, 0)):
    with cp.CirculantPlan(N3) as plan:
        plan.set_upwind_symbol(lam, mu).set_three_pass_shape(0, mid)
        kind = plan.mid_kernel()
        x = plan.apply(b)
        torch.cuda.synchronize()
    return x, kind


@pytest.fixture(scope="module")
def solved(cp, b256):
    """(x of the backward recurrence, x of the FFT kernel) per lambda set, computed once"""
    cache = {}

    def get(lam):
        if lam not in cache:
            x, kind = upwind_apply(cp, lam, b256)
            assert kind == "zrecb"
            xf, kindf = upwind_apply(cp, lam, b256, "swap64pf")
            assert kindf == "fft"
            cache[lam] = (x, xf)
        return cache[lam]
    return get


def flip_z(t):
    return t.view(256, 256, 256).flip(0).reshape(-1)


def test_flip_of_the_forward_kernel_bit_for_bit(cp, b256, solved):
    """apply(b) == flip_z(apply'(flip_z(b))), apply' the forward kernel on the mirrored symbol: P1 and
    P3 work per plane and P2 runs the same instructions on the same values (the two kernels' vector
    instructions are the same, only the scalar address arithmetic differs)."""
    x, _ = solved(LAMB)
    with cp.CirculantPlan(N3) as plan:
        plan.set_transport_symbol(LAMB_MIRROR)
        assert plan.mid_kernel() == "zrec"
        xm = plan.apply(flip_z(b256).contiguous())
        torch.cuda.synchronize()
    assert torch.equal(x, flip_z(xm))


@pytest.mark.parametrize("lam", [LAMB, LAMC], ids=["a0375", "a0997"])
def test_agrees_with_fft_kernel(solved, lam):
    x, xf = solved(lam)
    amax = back_ratio(256, 256, lam)
    err = rel(x, xf)
    print(f"zrecb vs fft {lam}: amax {amax:.6f} rel L2 {err:.3e} bound {bound(amax):.3e}")
    assert err < bound(amax)


def circulant_apply(x, lam):
    """C x of the upwind transport circulant: index - 1 for lam_d >= 0, index + 1 for lam_d < 0"""
    v = x.view(256, 256, 256)
    y = v.clone()
    for d, dim in enumerate((2, 1, 0)):  # x is the fastest axis = the last dim
        l = float(lam[d])
        if l != 0.0:
            y += abs(l) * (v - torch.roll(v, 1 if l > 0 else -1, dim))
    return y.reshape(-1)


@pytest.mark.parametrize("lam", [LAMB, LAMC], ids=["a0375", "a0997"])
def test_residual(solved, b256, lam):
    x, _ = solved(lam)
    res = rel(circulant_apply(x, lam), b256)
    print(f"zrecb residual {lam}: {res:.3e}")
    assert res < 1e-12


@pytest.mark.parametrize("lam", [LAMB, LAMC], ids=["a0375", "a0997"])
def test_oracle(solved, b256, oracle, lam):
    x, _ = solved(lam)
    ref = oracle.c_solve_3d(up_diag(N3, lam), b256.cpu().numpy(), N3)
    err = oracle.rel_l2(x.cpu().numpy(), ref)
    print(f"zrecb vs oracle {lam}: {err:.3e}")
    assert err < TOL


@pytest.fixture(scope="module")
def plans_c(cp):
    """the backward-recurrence plan and the FFT-kernel plan of LAMC, shared by the impulse cases"""
    with cp.CirculantPlan(N3) as pr, cp.CirculantPlan(N3) as pf:
        pr.set_upwind_symbol(LAMC)
        pf.set_upwind_symbol(LAMC).set_three_pass_shape(0, "swap64pf")
        assert pr.mid_kernel() == "zrecb" and pf.mid_kernel() == "fft"
        yield pr, pf


@pytest.mark.parametrize("z0", [0, 15, 16, 255])
def test_impulse_carries_and_wrap(plans_c, z0):
    """a = 0.997: the carries between slots, waves and across the cyclic closure all matter; planes
    0 and 255 are the last and the first the reversed scan visits, 15 / 16 a wave's edge"""
    pr, pf = plans_c
    x0, y0 = 37, 101
    b = torch.zeros(N, dtype=torch.complex128, device="cuda")
    b[x0 + 256 * (y0 + 256 * z0)] = 1.0
    x, xf = pr.apply(b), pf.apply(b)
    torch.cuda.synchronize()
    err, bd = rel(x, xf), bound(back_ratio(256, 256, LAMC))
    print(f"zrecb impulse z0={z0}: rel L2 {err:.3e} bound {bd:.3e}")
    assert err < bd
    col = x.view(256, 256, 256)[:, y0, x0]
    # information travels towards smaller z and wraps from plane 0 to plane 255
    assert bool((col[(z0 - torch.arange(1, 7)) % 256].abs() > 0).all())


def test_deterministic_and_in_place(cp, b256, solved):
    x, _ = solved(LAMC)
    with cp.CirculantPlan(N3) as plan:
        plan.set_upwind_symbol(LAMC)
        assert plan.mid_kernel() == "zrecb"
        x1 = plan.apply(b256)
        x2 = plan.apply(b256)
        assert torch.equal(x1, x2) and torch.equal(x1, x)
        t = b256.clone()
        plan.apply(t, out=t)
        assert torch.equal(t, x1)


def test_8_byte_aligned(cp, b256, solved):
    """b and x 8 bytes past a 16-byte boundary: the kernel runs without its LDS-DMA prefetch."""
    from circulantpreconditioner_amd._lib import check, lib
    x, xf = solved(LAMC)
    raw = torch.empty(2 * N + 1, dtype=torch.float64, device="cuda")
    raw[1:].copy_(torch.view_as_real(b256).reshape(-1))
    ptr = raw.data_ptr() + 8
    with cp.CirculantPlan(N3) as plan:
        plan.set_upwind_symbol(LAMC)
        assert plan.mid_kernel() == "zrecb"
        check(lib().cfp_plan_apply(plan._h, ptr, ptr, None))
        torch.cuda.synchronize()
    got = torch.view_as_complex(raw[1:].clone().reshape(-1, 2))
    bd = bound(back_ratio(256, 256, LAMC))
    print(f"zrecb unaligned vs fft: {rel(got, xf):.3e}; vs aligned zrecb: {rel(got, x):.3e}")
    assert rel(got, xf) < bd
    assert rel(got, x) < bd


# ---------------------------------------------------------------- routing
def test_routing_table(cp):
    with cp.CirculantPlan(N3) as plan:
        plan.set_upwind_symbol(LAMB)
        assert plan.mid_kernel() == "zrecb"
        for mid in ("swap64pf", "swap64", "lane64", "blocked"):
            assert plan.set_three_pass_shape(0, mid).mid_kernel() == "fft"
        assert plan.set_three_pass_shape(64, "default").mid_kernel() == "fft"
        assert plan.set_three_pass_shape(0, "default").set_schedule("five").mid_kernel() == "fft"
        assert plan.set_schedule("auto").mid_kernel() == "zrecb"
        # over the cap 1 - 2^-13: the FFT kernel
        over = (0.0, 0.0, -1e4)
        assert back_ratio(256, 256, over) > 1 - 2.0 ** -13
        assert plan.set_upwind_symbol(over).mid_kernel() == "fft"
        assert plan.set_upwind_symbol(LAMC).mid_kernel() == "zrecb"  # under it, over zrec2's 1 - 2^-7
        # mu_z != 0: the advdiff rule on the mapped numbers
        for lam, mu in ((LAMB, MU_Z), (LAMC, (0, 0, 1e-3))):
            want = plan.set_advdiff_symbol(*mapped(lam, mu)).mid_kernel()
            assert plan.set_upwind_symbol(lam, mu).mid_kernel() == want
        assert plan.set_upwind_symbol(LAMB, MU_Z).mid_kernel() == "zrec2"
        assert plan.set_upwind_symbol(LAMC, (0, 0, 1e-3)).mid_kernel() == "fft"
        # lam_z >= 0: the existing kernels
        assert plan.set_upwind_symbol((-0.6, -0.15, 0.6)).mid_kernel() == "zrec"
        assert plan.set_upwind_symbol((-0.6, -0.15, 0.0)).mid_kernel() == "zrec"
        # the advdiff setter with the mapped numbers never takes the new kernel
        for lam in (LAMB, LAMC):
            assert plan.set_advdiff_symbol(*mapped(lam)).mid_kernel() in ("zrec2", "fft")
        # and the other setters clear it
        plan.set_upwind_symbol(LAMB)
        assert plan.set_transport_symbol(LAMB).mid_kernel() == "fft"
        s = cp.transport_symbol_1d(256)
        plan.set_upwind_symbol(LAMB)
        assert plan.set_separable_symbol(s, s, s, LAMB).mid_kernel() == "fft"
    with cp.CirculantPlan((128, 128, 128)) as plan:
        assert plan.set_upwind_symbol(LAMB).mid_kernel() == "fft"


@pytest.mark.parametrize("graph", [False, True])
def test_live_plan_follows_symbol(cp, b256, graph):
    """One plan through transport -> upwind(-) -> advdiff -> upwind(+): each apply equals a fresh plan's."""
    seq = [("transport", (LAMB_MIRROR,), "zrec"), ("upwind", (LAMB,), "zrecb"),
           ("advdiff", (LAMB_MIRROR, MU_Z), "zrec2"), ("upwind", (LAMB_MIRROR,), "zrec")]
    with cp.CirculantPlan(N3) as plan:
        plan.set_graph(graph)
        out = torch.empty_like(b256)
        for name, args, kind in seq:
            getattr(plan, f"set_{name}_symbol")(*args)
            assert plan.mid_kernel() == kind
            plan.apply(b256, out=out)
            if graph:
                plan.apply(b256, out=out)  # the second apply of the pair replays the captured graph
            torch.cuda.synchronize()
            with cp.CirculantPlan(N3) as fresh:
                getattr(fresh, f"set_{name}_symbol")(*args)
                assert fresh.mid_kernel() == kind
                want = fresh.apply(b256)
                torch.cuda.synchronize()
            assert torch.equal(out, want)


# ---------------------------------------------------------------- boundary, both scalar builds
BDIMS = (32, 16, 24)
BLAM = (-0.6, 0.15, -0.4)
BMU = (0.2, 0.2, 2.5)


def plan_kernel(handle):
    from circulantpreconditioner_amd._lib import check, lib
    k = ctypes.c_int()
    check(lib().cfp_plan_mid_kernel(ctypes.c_void_p(handle), ctypes.byref(k)))
    return {1: "zrec", 2: "zrec2", 3: "zrecb"}.get(k.value, "fft")


@pytest.mark.parametrize("kind", ["transport", "diffusion"])
def test_complex_pcshell_setups(oracle, kind):
    from circulantpreconditioner_amd import diffusion as dif
    from circulantpreconditioner_amd import petsc as P
    from circulantpreconditioner_amd._lib_ext import FFTPrecDiffusionContext, PetscScalar
    nx, ny, nz = BDIMS
    n = nx * ny * nz
    mu = BMU if kind == "diffusion" else (0, 0, 0)
    if kind == "transport":
        ctx = P.make_context(BDIMS, BLAM)
        pc = P.PC.shell(ctx, upwind=True).setup()
    else:
        ctx = FFTPrecDiffusionContext()
        ctx.spaceDim = 3
        ctx.n_x, ctx.n_y, ctx.n_z = BDIMS
        ctx.lambda_x, ctx.lambda_y, ctx.lambda_z = (PetscScalar.of(v) for v in BLAM)
        ctx.mu_x, ctx.mu_y, ctx.mu_z = (PetscScalar.of(v) for v in mu)
        pc = dif.pc_shell(ctx, upwind=True)
    d0 = up_diag(BDIMS, BLAM, mu)
    d = P.Vec.borrow(ctx.Diag).array()
    assert np.abs(d - d0).max() <= 1e-14 * np.abs(d0).max()
    b = oracle.c_fill_uniform(n, 41)
    tb, tx = torch.from_numpy(b).cuda(), torch.zeros(n, dtype=torch.complex128, device="cuda")
    pc.apply(P.Vec.from_tensor(tb), P.Vec.from_tensor(tx))
    torch.cuda.synchronize()
    err = oracle.rel_l2(tx.cpu().numpy(), oracle.c_solve_3d(d0, b, BDIMS))
    print(f"upwind PCSHELL [{kind}] {BDIMS}: vs oracle {err:.3e}")
    assert err < TOL
    F = P.Mat(ctx.FFT_MAT, owned=False)
    assert F.solve_counts() == (1, 0)  # Diag is the plan's own symbol: divided in registers
    pc.destroy()


@pytest.mark.parametrize("kind", ["transport", "diffusion"])
def test_real_pcshell_setups(oracle, kind):
    from circulantpreconditioner_amd import petsc_real as R
    nx, ny, nz = BDIMS
    n = nx * ny * nz
    mu = BMU if kind == "diffusion" else (0, 0, 0)
    if kind == "transport":
        ctx = R.FFTPrecTransportContext(3, nx, ny, nz, BLAM[0], BLAM[1], BLAM[2], None, None, None, None, None)
    else:
        ctx = R.FFTPrecDiffusionContext(3, nx, ny, nz, BLAM[0], BLAM[1], BLAM[2], None, None, None, None, None,
                                        mu[0], mu[1], mu[2])
    pc = R.pc_shell(ctx, upwind=True)
    d0 = up_diag(BDIMS, BLAM, mu)
    half = np.ascontiguousarray(d0.reshape(nz, ny, nx)[..., : nx // 2 + 1]).view(np.float64).reshape(-1)
    diag = R.Vec.borrow(ctx.Diag)
    assert np.abs(diag.array() - half).max() <= 1e-14 * np.abs(half).max()
    b = oracle.c_fill_uniform(n, 43).real.copy()
    vb, vx = R.Vec.seq(n, hip=True).set_array(b), R.Vec.seq(n, hip=True)
    R.PetscCall(R.lib().PCApply(pc, vb.h, vx.h))
    ref = oracle.c_solve_3d(d0, b.astype(np.complex128), BDIMS)
    assert np.linalg.norm(ref.imag) <= 1e-13 * np.linalg.norm(ref)
    err = np.linalg.norm(vx.array() - ref.real) / np.linalg.norm(ref.real)
    print(f"real upwind PCSHELL [{kind}] {BDIMS}: vs oracle {err:.3e}")
    assert err < TOL
    own, expl = ctypes.c_int64(), ctypes.c_int64()
    R.PetscCall(R.lib().MatFFTHIPGetSolveCounts(ctypes.c_void_p(ctx.FFT_MAT), ctypes.byref(own), ctypes.byref(expl)))
    assert (own.value, expl.value) == (1, 0)
    vb.destroy()
    vx.destroy()
    pcp = ctypes.c_void_p(pc.value)
    R.PetscCall(R.lib().PCDestroy(ctypes.byref(pcp)))


# ---------------------------------------------------------------- drivers
A_NEG, NU, DT = (-1.0, 0.5, -0.3), 0.01, 0.05


def grid_h(cfg):
    return [(cfg.xmax[d] - cfg.xmin[d]) / n for d, n in enumerate((cfg.nx, cfg.ny, cfg.nz))]


def test_diffusion_periodic_converges_in_one_iteration():
    from circulantpreconditioner_amd import diffusion as dif
    cfg = dif.config(32, bc="periodic", pc="fft_upwind", steps=3, a=A_NEG, nu=NU, dt=DT)
    res = dif.run(cfg)
    print(f"periodic, a = {A_NEG}: its per step {res['min_step_its']}..{res['max_step_its']}")
    assert res["steps"] == 3 and res["all_converged"] == 1
    assert res["min_step_its"] == 1 and res["max_step_its"] == 1
    h = grid_h(cfg)
    assert res["lambda"] == pytest.approx([cfg.a[d] * cfg.dt / h[d] for d in range(3)], rel=1e-14)


def test_diffusion_walls_beat_pcnone_and_solve_the_operator():
    from circulantpreconditioner_amd import diffusion as dif
    dims = (32, 32, 32)
    kw = dict(bc="wall", a=A_NEG, nu=NU, dt=DT)
    _, u0 = dif.run(dif.config(32, steps=0, **kw), return_field=True)
    cfg = dif.config(32, pc="fft_upwind", steps=1, **kw)
    up, u1 = dif.run(cfg, return_field=True)
    none = dif.run(dif.config(32, pc="none", steps=1, **kw))
    res = np.linalg.norm(apply_operator(u1, dims, grid_h(cfg), cfg.dt, list(cfg.a), cfg.nu, False) - u0) / np.linalg.norm(u0)
    print(f"walls, a = {A_NEG}: its upwind {up['total_its']} none {none['total_its']} |A U1 - U0| / |U0| = {res:.2e}")
    assert up["all_converged"] == 1
    assert up["total_its"] < none["total_its"]
    assert res <= 10 * cfg.precision


@pytest.mark.parametrize("a", [(-1.0, 0.0, 0.0), (0.0, 0.0, -1.0)], ids=["-x", "-z"])
def test_transport_upwind_mode_beats_pcnone(a):
    from circulantpreconditioner_amd import transport as T
    up = T.run(T.config(32, pc="fft", sign="fixed", lambda_mode="upwind", a=a, device=True))
    none = T.run(T.config(32, pc="none", sign="fixed", a=a, device=True))
    print(f"transport a = {a}: its upwind {up['total_its']} none {none['total_its']} (converged {none['all_converged']})")
    assert up["all_converged"] == 1
    assert up["total_its"] < none["total_its"]
    assert up["lambda"] == pytest.approx([v * up["dt"] * 32 for v in a], rel=1e-14)


def test_transport_256_step_takes_the_backward_kernel():
    """One 256^3 step against z: converged, the fused and the unfused Krylov step agree, and a
    PCSHELL set up with the driver's numbers runs the backward recurrence."""
    from circulantpreconditioner_amd import petsc as P
    from circulantpreconditioner_amd import transport as T
    a = (0.0, 0.0, -1.0)
    kw = dict(pc="fft", sign="fixed", lambda_mode="upwind", a=a, device=True, steps=1)
    r1, u1 = T.run(T.config(256, **kw), return_field=True)
    r0, u0 = T.run(T.config(256, fuse=0, **kw), return_field=True)
    assert r1["all_converged"] == 1 and r1["steps"] == 1
    assert r0["all_converged"] == 1 and r0["total_its"] == r1["total_its"]
    d = np.linalg.norm(u1 - u0) / np.linalg.norm(u0)
    print(f"256^3 step a = {a}: its {r1['total_its']} lambda {r1['lambda']} fused vs unfused {d:.3e}")
    assert d <= 1e-11
    assert r1["lambda"][2] < 0
    ctx = P.make_context(N3, r1["lambda"])
    pc = P.PC.shell(ctx, upwind=True).setup()
    assert plan_kernel(P.context_plan(ctx)) == "zrecb"
    pc.destroy()
