"""The advection-diffusion symbol on the z-slab plan, host side (no GPU): the rank's column table
of the 256^3 slab recurrence against the numpy factorisation, the new exports of both libraries,
and AdvectionDiffusionGMRES on PETSC_COMM_WORLD of several gloo ranks (host Vecs, PCNONE) against
the one-rank run."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from advdiff_cases import ELIGIBLE, apply_operator, symbol_1d, z_factors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["cfp_dist_plan_set_symbol_advdiff", "cfp_group_set_symbol_advdiff", "cfp_dist_plan_set_mid_kernel",
             "cfp_dist_plan_mid_kernel", "cfp_group_set_mid_kernel", "cfp_group_mid_kernel",
             "cfp_slab_advdiff_z_table"]


def _brev3(y2):
    return ((y2 & 1) << 2) | (y2 & 2) | (y2 >> 2)


@pytest.fixture(scope="module")
def columns():
    """name -> (beta, a, b) of all 256 x 256 columns [ky][kx], once for every P and rank"""
    out = {}
    for name in ("advdiff", "complex"):
        lam, mu = ELIGIBLE[name]
        sx, sy = symbol_1d(256, lam[0], mu[0]), symbol_1d(256, lam[1], mu[1])
        out[name] = z_factors(1 + sx[None, :] + sy[:, None], lam[2], mu[2])
    return out


@pytest.mark.parametrize("P", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("name", ["advdiff", "complex"])
def test_slab_z_table_is_the_factorisation_of_the_ranks_columns(columns, name, P):
    from circulantpreconditioner_amd.distributed import slab_advdiff_z_table
    lam, mu = ELIGIBLE[name]
    beta, a, b = columns[name]
    lane = np.arange(64)
    x, k2 = lane & 7, np.array([_brev3(int(y2)) for y2 in lane >> 3])
    u = np.arange(32 * (32 // P))
    kx = 8 * (u % 32)[:, None] + x[None, :]
    eps = np.finfo(float).eps
    for rank in range(P):
        t = slab_advdiff_z_table(P, rank, lam, mu)
        assert t.shape == (32 * (32 // P), 3, 64)
        ky = rank * 32 // P + (u // 32)[:, None] + 32 * k2[None, :]
        for e, ref in ((0, a[ky, kx]), (1, 256 / beta[ky, kx]), (2, b[ky, kx])):
            # one complex square root and one division per entry
            assert np.abs(t[:, e, :] - ref).max() <= 16 * eps * np.abs(ref).max(), (name, P, rank, e)


@pytest.mark.parametrize("P", [3, 32])
def test_slab_z_table_rejects_an_unsupported_split(P):
    from circulantpreconditioner_amd._lib import CirculantError
    from circulantpreconditioner_amd.distributed import slab_advdiff_z_table
    lam, mu = ELIGIBLE["advdiff"]
    with pytest.raises(CirculantError) as e:
        slab_advdiff_z_table(P, 0, lam, mu)
    assert e.value.code == 63  # CFP_ERR_ARG_OUTOFRANGE


def test_both_libraries_export_the_new_names():
    from circulantpreconditioner_amd import _lib, petsc_real
    names = _lib._parse_decls(os.path.join(ROOT, "include", "circulant_fft_dist.h"))
    assert set(NEW_NAMES) <= set(names)
    for path in (_lib.LIB_PATH, petsc_real.LIB_PATH):
        L = ctypes.CDLL(path)
        for n in NEW_NAMES:
            assert hasattr(L, n), (path, n)


# ---------------------------------------------------------------- the time loop on several ranks
DIMS = (8, 6, 4)
KW = dict(pc="none", device=False, a=(1.0, 0.5, 0.25), nu=0.1, dt=0.01)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, P, port, q, bc):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=P)
    try:
        import sys
        sys.path.insert(0, ROOT)
        from circulantpreconditioner_amd import diffusion as dif
        from circulantpreconditioner_amd import petsc as Pm
        comm = Pm.Comm.torch().set_world()
        res, U = dif.run(dif.config(DIMS, steps=1, bc=bc, **KW), return_field=True)
        Pm.set_comm_world(Pm.PETSC_COMM_SELF)
        comm.destroy()
        q.put((rank, {"res": res, "U": U}))
    finally:
        dist.destroy_process_group()


def _spawn(P, bc):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, P, port, q, bc)) for r in range(P)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=240) for _ in range(P))
    finally:
        for p in procs:
            p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    return res


@pytest.mark.parametrize("bc", ["wall", "periodic"])
@pytest.mark.parametrize("P", [2, 4])
def test_advdiff_gmres_on_several_ranks(P, bc):
    """AdvectionDiffusionGMRES on PETSC_COMM_WORLD of P gloo ranks (host Vecs, PCNONE): the
    iteration count of the one-rank run, the gathered field within 1e-10 of it, and the step
    solves the operator to 10 x precision."""
    from circulantpreconditioner_amd import diffusion as dif
    res = _spawn(P, bc)
    N = int(np.prod(DIMS))
    U = np.empty(N, dtype=np.complex128)
    for r in range(P):
        lo, n = res[r]["res"]["rstart"], res[r]["res"]["nlocal"]
        assert lo == sum(res[q]["res"]["nlocal"] for q in range(r))  # contiguous PETSC_DECIDE blocks
        U[lo:lo + n] = res[r]["U"]
    assert sum(res[r]["res"]["nlocal"] for r in range(P)) == N
    _, U0 = dif.run(dif.config(DIMS, steps=0, bc=bc, **KW), return_field=True)
    cfg = dif.config(DIMS, steps=1, bc=bc, **KW)
    r1, U1 = dif.run(cfg, return_field=True)
    assert r1["rstart"] == 0 and r1["nlocal"] == N
    for r in range(P):
        assert res[r]["res"]["total_its"] == r1["total_its"]
        assert res[r]["res"]["all_converged"] == 1
    d = np.linalg.norm(U - U1) / np.linalg.norm(U1)
    h = [1.0 / n for n in DIMS]
    err = np.linalg.norm(apply_operator(U, DIMS, h, cfg.dt, list(cfg.a), cfg.nu, bc == "periodic") - U0) / np.linalg.norm(U0)
    print(f"P={P} {bc}: its {r1['total_its']}  |U - U1|/|U1| {d:.3e}  |A U1 - U0|/|U0| {err:.3e}")
    assert d <= 1e-10
    assert err <= 10 * cfg.precision
