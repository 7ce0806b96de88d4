"""The advection-diffusion symbol on the z-slab plan (SlabGroup / SlabPlan.set_advdiff_symbol) and
the two-sided z recurrence as the middle kernel of a 256^3 slab rank (k_tp_mid_rec2 on the rank's
[256 z][256 / P][256 x] block, set_mid_kernel('rec')).

Bounds, the project's own: against the oracle 1e-10; two schedules of the FFT path 1e-13; the
recurrence against the FFT kernel advdiff_cases.bound(ra, rb) with the ratios of the whole grid
(1e-13 where both are <= 0.5), test_advdiff_gpu.py's rule."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

from advdiff_cases import ELIGIBLE, bound as ratio_bound, diag as np_diag

pytestmark = pytest.mark.gpu
TOL = 1e-10
N3 = (256, 256, 256)
N = 256 ** 3
SEED = 31
OVER_CAP = ((0, 0, 0), (0.3, 0.3, 1e6))  # test_advdiff_gpu.py test_over_the_cap_keeps_the_fft_kernel
TRANSPORT = (0.6, 0.15, 0.02)


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return cp


@pytest.fixture(scope="module")
def SlabGroup():
    from circulantpreconditioner_amd.distributed import SlabGroup
    return SlabGroup


def bound(cp, case):
    ra, rb = cp.advdiff_z_ratio(256, 256, *case)
    return 1e-13 if max(ra, rb) <= 0.5 else ratio_bound(ra, rb)


def rel(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


@pytest.fixture(scope="module")
def b256(cp):
    b = torch.empty(N, dtype=torch.complex128, device="cuda")
    cp.fill_uniform(b, SEED)
    return b


@pytest.fixture(scope="module")
def ref256(b256, oracle):
    """the oracle's solve of the 'advdiff' symbol, once for every P (and the process test)"""
    ref = oracle.c_solve_3d(np_diag(N3, *ELIGIBLE["advdiff"]), b256.cpu().numpy(), N3)
    return torch.from_numpy(ref).cuda()


def group_apply(g, b):
    torch.cuda.synchronize()  # b is complete: the group's streams do not wait for torch's
    bs = g.scatter(b)
    x = torch.cat(g.apply(bs))
    torch.cuda.synchronize()
    return x


# ---------------------------------------------------------------- small grids: the 5-pass tables
@pytest.mark.parametrize("name", ["advdiff", "complex"])
@pytest.mark.parametrize("dims,P", [((32, 16, 24), 2), ((32, 16, 24), 4), ((16, 3, 8), 4), ((64, 30, 32), 4),
                                    ((1, 8, 8), 2), ((100, 50, 30), 3)])
def test_small_grids_vs_oracle(SlabGroup, oracle, dims, P, name):
    """padded layouts (P not dividing ny) and ranks without rows among them"""
    case = ELIGIBLE[name]
    n = int(np.prod(dims))
    b = oracle.c_fill_uniform(n, 17)
    ref = oracle.c_solve_3d(np_diag(dims, *case), b, dims)
    with SlabGroup(dims, P) as g:
        g.set_advdiff_symbol(*case)
        assert g.mid_kernel() == "fft"
        got = group_apply(g, torch.from_numpy(b).cuda()).cpu().numpy()
    err = oracle.rel_l2(got, ref)
    print(f"slab advdiff {dims} P={P} [{name}]: vs oracle {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("dims,P", [((32, 16, 24), 4), (N3, 8)])
def test_mu_zero_is_the_transport_setter_bit_for_bit(cp, SlabGroup, dims, P):
    lam = ELIGIBLE["complex"][0]
    b = torch.empty(int(np.prod(dims)), dtype=torch.complex128, device="cuda")
    cp.fill_uniform(b, 5)
    with SlabGroup(dims, P) as g:
        g.set_advdiff_symbol(lam, (0, 0, 0))
        assert g.mid_kernel() == "fft"
        x = group_apply(g, b)
        g.set_transport_symbol(lam)
        xt = group_apply(g, b)
    assert torch.equal(x, xt)


# ---------------------------------------------------------------- 256^3: the slab recurrence
@pytest.mark.parametrize("P", [1, 2, 4, 8, 16])
def test_rec_agrees_with_fft_and_oracle(cp, SlabGroup, b256, ref256, P):
    case = ELIGIBLE["advdiff"]
    with SlabGroup(N3, P) as g:
        g.set_advdiff_symbol(*case)
        g.set_mid_kernel("rec")
        assert g.mid_kernel() == "zrec2"
        x = group_apply(g, b256)
        g.set_mid_kernel("fft")
        assert g.mid_kernel() == "fft"
        xf = group_apply(g, b256)
        g.set_mid_kernel("rec").set_schedule("five")
        assert g.mid_kernel() == "fft"
        x5 = group_apply(g, b256)
    e_fft, e_or, e_five = rel(x, xf), rel(x, ref256), rel(x5, xf)
    print(f"slab zrec2 P={P}: vs fft {e_fft:.3e} (bound {bound(cp, case):.3e}) vs oracle {e_or:.3e}; "
          f"five vs three (fft) {e_five:.3e}")
    assert e_fft < bound(cp, case)
    assert e_or < TOL
    assert rel(xf, ref256) < TOL
    assert e_five < 1e-13


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


def test_hardest_eligible_case(cp, SlabGroup, b256):
    """diff1000: |a| = |b| = 0.969 on the worst column; P = 8, one unit per workgroup"""
    case = ELIGIBLE["diff1000"]
    with SlabGroup(N3, 8) as g:
        g.set_advdiff_symbol(*case).set_mid_kernel("rec")
        assert g.mid_kernel() == "zrec2"
        x = group_apply(g, b256)
        g.set_mid_kernel("fft")
        xf = group_apply(g, b256)
    err, res = rel(x, xf), rel(circulant_apply(x, case), b256)
    print(f"slab zrec2 P=8 [diff1000]: vs fft {err:.3e} residual {res:.3e} bound {bound(cp, case):.3e}")
    assert err < bound(cp, case)
    assert res < bound(cp, case)


@pytest.mark.parametrize("z0", [0, 15, 16, 63, 64, 255])
def test_impulses_cross_the_blocks_the_seam_and_the_wrap(cp, SlabGroup, z0):
    """P = 4 (nzl = 64): z0 = 15 / 16 a wave block's last and the next one's first point, 63 / 64
    the two sides of a slab seam, 0 / 255 the two ends of the cyclic wrap"""
    case = ELIGIBLE["diff1000"]
    x0, y0 = 3, 37
    b = torch.zeros(N, dtype=torch.complex128, device="cuda")
    b[x0 + 256 * (y0 + 256 * z0)] = 1.0
    with SlabGroup(N3, 4) as g:
        g.set_advdiff_symbol(*case).set_mid_kernel("rec")
        assert g.mid_kernel() == "zrec2"
        x = group_apply(g, b)
        g.set_mid_kernel("fft")
        xf = group_apply(g, b)
    err = rel(x, xf)
    print(f"slab zrec2 impulse z0={z0}: {err:.3e} bound {bound(cp, case):.3e}")
    assert err < bound(cp, case)
    col = x.view(256, 256, 256)[:, y0, x0]
    assert bool((col[0:6].abs() > 0).all()) and bool((col[250:256].abs() > 0).all())  # both sides of the wrap


def test_pieces_and_in_place(cp, SlabGroup, b256):
    """one piece: the z-pencil buffer is the caller's x; four: the second work buffer"""
    case = ELIGIBLE["advdiff"]
    with SlabGroup(N3, 4) as g:
        g.set_advdiff_symbol(*case).set_mid_kernel("rec")
        g.set_pieces(1)
        assert g.mid_kernel() == "zrec2"
        x1 = group_apply(g, b256)
        g.set_pieces(4)
        assert g.mid_kernel() == "zrec2"  # set_steps refilled the symbol and its table
        x4 = group_apply(g, b256)
        err = rel(x4, x1)
        print(f"slab zrec2 pieces 4 vs 1: {err:.3e}")
        assert err < bound(cp, case)
        for K, want in ((1, x1), (4, x4)):
            g.set_pieces(K)
            bs = [t.clone() for t in g.scatter(b256)]  # (scatter on one device gives views of b256)
            torch.cuda.synchronize()  # the group's streams do not wait for torch's
            g.apply(bs, bs)
            torch.cuda.synchronize()
            assert torch.equal(torch.cat(bs), want), K


def test_8_byte_aligned_x(cp, SlabGroup, b256):
    """P = 2, one piece: x is the z-pencil buffer; 8 bytes past a 16-byte boundary the kernel runs
    without its LDS-DMA prefetch"""
    from circulantpreconditioner_amd._lib import check, lib
    case = ELIGIBLE["advdiff"]
    with SlabGroup(N3, 2) as g:
        g.set_advdiff_symbol(*case).set_mid_kernel("rec").set_pieces(1)
        assert g.mid_kernel() == "zrec2"
        want = group_apply(g, b256)
        g.set_mid_kernel("fft")
        xf = group_apply(g, b256)
        g.set_mid_kernel("rec")
        bs = g.scatter(b256)
        n = bs[0].numel()
        raws = [torch.empty(2 * n + 1, dtype=torch.float64, device="cuda") for _ in bs]
        assert all(r.data_ptr() % 16 == 0 for r in raws)
        bp = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in bs])
        xp = (ctypes.c_void_p * 2)(*[r.data_ptr() + 8 for r in raws])
        check(lib().cfp_group_apply(g._h, bp, xp))
        torch.cuda.synchronize()
    got = torch.cat([torch.view_as_complex(r[1:].clone().reshape(-1, 2)) for r in raws])
    print(f"slab zrec2 unaligned x: vs fft {rel(got, xf):.3e}; vs aligned zrec2 {rel(got, want):.3e}")
    assert rel(got, xf) < bound(cp, case)
    assert rel(got, want) < bound(cp, case)


# ---------------------------------------------------------------- routing
def test_routing(cp, SlabGroup, b256):
    case = ELIGIBLE["advdiff"]
    with SlabGroup(N3, 4) as g:
        g.set_mid_kernel("rec")
        g.set_advdiff_symbol(case[0], (0.2, 0.2, 0))  # mu_z = 0
        assert g.mid_kernel() == "fft"
        g.set_advdiff_symbol(*OVER_CAP)
        assert g.mid_kernel() == "fft"
        g.set_advdiff_symbol(*case)
        assert g.mid_kernel() == "zrec2"
        g.set_transport_symbol(TRANSPORT)
        assert g.mid_kernel() == "fft"
        with pytest.raises(Exception):
            g.set_mid_kernel(7)
    with SlabGroup(N3, 32) as g:  # no 3-sweep schedule at P = 32
        g.set_advdiff_symbol(*case).set_mid_kernel("rec")
        assert g.mid_kernel() == "fft"


def test_512_keeps_the_fft_kernel():
    """one rank of 16 (its two work buffers: 256 MiB), 3 sweeps: the tables only"""
    from circulantpreconditioner_amd.distributed import SlabPlan
    plan = SlabPlan((512, 512, 512), rank=3, world=16, device=0, exchange="torch")
    try:
        plan.set_advdiff_symbol(*ELIGIBLE["advdiff"]).set_mid_kernel("rec")
        assert any(s["kind"] == 2 for s in plan.steps())
        assert plan.mid_kernel() == "fft"
    finally:
        plan.close()


def test_live_group_follows_symbol_and_schedule(cp, SlabGroup, b256):
    """advdiff -> transport -> advdiff with a schedule change in between: each apply equals a
    fresh group's"""
    case = ELIGIBLE["advdiff"]

    def fresh(setter):
        with SlabGroup(N3, 4) as f:
            f.set_mid_kernel("rec")
            setter(f)
            return group_apply(f, b256), f.mid_kernel()

    adv = lambda q: q.set_advdiff_symbol(*case)  # noqa: E731
    tra = lambda q: q.set_transport_symbol(TRANSPORT)  # noqa: E731
    with SlabGroup(N3, 4) as g:
        g.set_mid_kernel("rec")
        for setter, sched, kind in ((adv, "auto", "zrec2"), (tra, "auto", "fft"), (tra, "five", "fft"),
                                    (adv, "five", "fft"), (adv, "three", "zrec2")):
            setter(g)
            g.set_schedule(sched)
            assert g.mid_kernel() == kind, (sched, kind)
            x = group_apply(g, b256)
            if sched != "five":
                want, fkind = fresh(setter)
                assert fkind == kind
                assert torch.equal(x, want)
        g.set_schedule("five")
        x5 = group_apply(g, b256)
        g.set_schedule("auto")  # back to three sweeps: the table is rebuilt with the symbol
        assert g.mid_kernel() == "zrec2"
        assert rel(group_apply(g, b256), x5) < bound(cp, case)


def test_auto_takes_one_of_the_two_kernels(cp, SlabGroup, b256):
    case = ELIGIBLE["advdiff"]
    with SlabGroup(N3, 2) as g:
        g.set_advdiff_symbol(*case)
        assert g.mid_kernel() in ("fft", "zrec2")
        x = group_apply(g, b256)
        g.set_mid_kernel("fft")
        xf = group_apply(g, b256)
    assert rel(x, xf) < bound(cp, case)


# ---------------------------------------------------------------- SlabPlan, one process per rank
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _slab_rank(rank, world, port, q):
    """One rank of a SlabPlan in its own process (exchange through torch.distributed / gloo)."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import circulantpreconditioner_amd as cp
        from circulantpreconditioner_amd.distributed import SlabPlan
        torch.cuda.set_device(0)
        plan = SlabPlan(N3, rank=rank, world=world, device=0, exchange="torch")
        plan.set_advdiff_symbol(*ELIGIBLE["advdiff"]).set_mid_kernel("rec")
        kind = plan.mid_kernel()
        b = torch.empty(plan.local_size, dtype=torch.complex128, device="cuda:0")
        cp.fill_uniform(b, SEED, offset=plan.local_offset)
        x = plan.apply(b)
        torch.cuda.synchronize()
        q.put((rank, plan.local_offset, x.cpu().numpy(), kind))
        plan.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_slab_plan_processes_vs_oracle(world, ref256):
    """`world` fresh processes, one SlabPlan rank each, on cuda:0; gathered x vs the oracle"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_slab_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        parts = [q.get(timeout=240) for _ in range(world)]
    finally:
        for p in procs:
            p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    x = np.empty(N, dtype=np.complex128)
    for _, off, part, kind in parts:
        assert kind == "zrec2"
        x[off:off + part.size] = part
    ref = ref256.cpu().numpy()
    err = float(np.linalg.norm(x - ref) / np.linalg.norm(ref))
    print(f"SlabPlan zrec2 in {world} processes vs oracle: {err:.3e}")
    assert err < TOL
