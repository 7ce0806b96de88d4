"""The advection-diffusion boundary on PETSC_COMM_WORLD of several ranks, on the GPU
(include/diffusion_equation.h).  2 and 4 fresh processes share cuda:0; PETSC_COMM_WORLD is a
communicator with torch.distributed's collectives (gloo), so the FFT matrix is backed by the z-slab
plan with the advection-diffusion symbol.  Per rank: the GMRES time loop with the diffusion
PCSHELL, setupFFTPrec3DDiffusion + applyFFT3DPrecDiffusion (own symbol, then a Diag the caller
scaled), PetscFft3DDiffusionSolver in place; the real-scalar library on 2 ranks.  Gathered results
against the oracle (1e-10) and the one-rank run."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

from advdiff_cases import apply_operator, diag as np_diag

pytestmark = pytest.mark.gpu
TOL = 1e-10
DIMS = (32, 16, 24)
A, NU, DT = (1.0, 0.5, 0.25), 0.3, 0.02
MINS, MAXS = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
SOLVER = dict(a=(1.0, 0.5, 2.0), nu=0.3, dt=0.07, h=(0.25, 0.5, 0.2))  # test_diffusion_gpu.py's numbers
RUN_KW = dict(a=(1.0, 0.5, 0.25), nu=0.5, dt=0.01, pc="fft", steps=1)


def numbers(dims, a, nu, dt, h):
    return [a[d] * dt / h[d] for d in range(3)], [nu * dt / h[d] ** 2 for d in range(3)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, job, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from oracle import oracle as O
        torch.cuda.set_device(0)
        out = _real_job(O) if job == "real" else _complex_job(job, O)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def _complex_job(job, O):
    from circulantpreconditioner_amd import diffusion as dif
    from circulantpreconditioner_amd import petsc as P
    from circulantpreconditioner_amd._lib import lib
    comm = P.Comm.torch().set_world()
    out = {}
    if job[0] == "run":
        res, U = dif.run(dif.config((32, 32, 32), bc=job[1], **RUN_KW), return_field=True)
        out = {"res": res, "U": U}
    else:
        nx, ny, nz = DIMS
        N = nx * ny * nz
        b = O.c_fill_uniform(N, 31)
        ctx = dif.context(3, DT, DIMS, A, NU, MINS, MAXS)
        pc = dif.pc_shell(ctx)
        dp = ctypes.c_void_p()
        P.PetscCall(lib().MatFFTHIPGetDistPlan(ctx.FFT_MAT, ctypes.byref(dp)))
        out["dist"] = bool(dp.value)
        diag = P.Vec.borrow(ctx.Diag)
        lo, hi = diag.ownership_range()
        out["range"] = (lo, hi)
        out["diag"] = diag.array()
        tb = torch.from_numpy(b[lo:hi].copy()).cuda()
        tx = torch.zeros_like(tb)
        vb, vx = P.Vec.from_tensor_mpi(tb, N), P.Vec.from_tensor_mpi(tx, N)
        pc.apply(vb, vx)
        torch.cuda.synchronize()
        out["pc"] = tx.cpu().numpy()
        # PetscFft3DDiffusionSolver(ctx, Un, Un) on the slab-backed matrix, in place
        F = P.Mat(ctx.FFT_MAT, owned=False)
        s = SOLVER
        sc = dif.StructuredContext(nx, ny, nz, *s["a"], s["nu"], s["dt"], *s["h"], F)
        tu = torch.from_numpy(b[lo:hi].copy()).cuda()
        vu = P.Vec.from_tensor_mpi(tu, N)
        dif.PetscFft3DDiffusionSolver(sc, vu, vu)
        torch.cuda.synchronize()
        out["direct"] = tu.cpu().numpy()
        # the matrix now holds the solver's numbers: the PCSHELL apply divides by the Diag it is
        # given, here the one the caller scaled by 2
        diag.scale(2.0)
        pc.apply(vb, vx)
        torch.cuda.synchronize()
        out["pc_2diag"] = tx.cpu().numpy()
        pc.destroy()
    P.set_comm_world(P.PETSC_COMM_SELF)
    comm.destroy()
    return out


def _real_job(O):
    from circulantpreconditioner_amd import petsc_real as R
    L = R.lib()
    comm = R.Comm.torch().set_world()
    nx, ny, nz = DIMS
    N = nx * ny * nz
    b = O.c_fill_uniform(N, 47).real.copy()
    out = {}
    ctx = R.diffusion_context(3, DT, DIMS, A, NU, MINS, MAXS)
    pc = R.pc_shell(ctx)
    dp = ctypes.c_void_p()
    R.PetscCall(L.MatFFTHIPGetDistPlan(ctx.FFT_MAT, ctypes.byref(dp)))
    out["dist"] = bool(dp.value)
    diag = R.Vec.borrow(ctx.Diag)
    out["diag_range"] = diag.ownership_range()
    out["diag"] = diag.array()
    vb, vx = R.Vec.mpi(N, hip=True), R.Vec.mpi(N, hip=True)
    lo, hi = vb.ownership_range()
    out["range"] = (lo, hi)
    vb.set_array(b[lo:hi])
    R.PetscCall(L.PCApply(pc, vb.h, vx.h))
    out["pc"] = vx.array()
    s = SOLVER
    F = ctypes.c_void_p(ctx.FFT_MAT)
    sc = R.StructuredDiffusionContext(nx, ny, nz, *s["a"], s["nu"], s["dt"], *s["h"], F)
    u = R.Vec.mpi(N, hip=True).set_array(b[lo:hi])
    R.PetscCall(L.PetscFft3DDiffusionSolver(sc, u.h, u.h))
    out["direct"] = u.array()
    for v in (vb, vx, u):
        v.destroy()
    R.PetscCall(L.PCDestroy(ctypes.byref(pc)))
    R.set_comm_world(R.PETSC_COMM_SELF)
    comm.destroy()
    return out


def _spawn(world, job):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, job, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        parts = dict(q.get(timeout=240) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    return parts


def gather(parts, key, N, dtype=np.complex128, rng="range"):
    x = np.empty(N, dtype=dtype)
    for r in parts:
        lo, hi = parts[r][rng]
        x[lo:hi] = parts[r][key]
    return x


@pytest.fixture(scope="module")
def one_rank():
    """the one-rank runs of the time loop, once for both process counts: bc -> (res, U1, U0)"""
    from circulantpreconditioner_amd import diffusion as dif
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    out = {}
    for bc in ("periodic", "wall"):
        kw = dict(RUN_KW, steps=0)
        _, u0 = dif.run(dif.config((32, 32, 32), bc=bc, **kw), return_field=True)
        cfg = dif.config((32, 32, 32), bc=bc, **RUN_KW)
        res, u1 = dif.run(cfg, return_field=True)
        out[bc] = (res, u1, u0, cfg)
    return out


@pytest.mark.parametrize("bc", ["periodic", "wall"])
@pytest.mark.parametrize("world", [2, 4])
def test_time_loop_on_the_world_communicator(world, bc, one_rank):
    dims = (32, 32, 32)
    N = 32 ** 3
    parts = _spawn(world, ("run", bc))
    r1, u1, u0, cfg = one_rank[bc]
    U = np.empty(N, dtype=np.complex128)
    for r in range(world):
        res = parts[r]["res"]
        assert (res["rstart"], res["nlocal"]) == (r * N // world, N // world)
        U[res["rstart"]:res["rstart"] + res["nlocal"]] = parts[r]["U"]
        assert res["all_converged"] == 1 and res["steps"] == 1
        assert res["total_its"] == r1["total_its"]
        assert res["pc_calls"] > 0
    if bc == "periodic":  # the operator is the circulant the PCSHELL inverts
        assert r1["total_its"] == 1
    d = np.linalg.norm(U - u1) / np.linalg.norm(u1)
    h = [1.0 / n for n in dims]
    err = np.linalg.norm(apply_operator(U, dims, h, cfg.dt, list(cfg.a), cfg.nu, bc == "periodic") - u0) / np.linalg.norm(u0)
    print(f"diffusion.run {bc} on {world} ranks: its {r1['total_its']} |U - U1|/|U1| {d:.3e} |A U - U0|/|U0| {err:.3e}")
    assert d <= 1e-10
    assert err <= 10 * cfg.precision


@pytest.mark.parametrize("world", [2, 4])
def test_pcshell_and_direct_solver_on_several_ranks(world, oracle):
    parts = _spawn(world, ("pcshell",))
    nx, ny, nz = DIMS
    N = nx * ny * nz
    for r in range(world):
        assert parts[r]["dist"]
        assert parts[r]["range"] == (r * N // world, (r + 1) * N // world)  # whole z-planes
    b = oracle.c_fill_uniform(N, 31)
    h = [(MAXS[d] - MINS[d]) / DIMS[d] for d in range(3)]
    d0 = np_diag(DIMS, *numbers(DIMS, A, NU, DT, h))
    dg = gather(parts, "diag", N)
    assert np.abs(dg - d0).max() <= 1e-15 * np.abs(d0).max()
    e_pc = oracle.rel_l2(gather(parts, "pc", N), oracle.c_solve_3d(d0, b, DIMS))
    s = SOLVER
    ds = np_diag(DIMS, *numbers(DIMS, s["a"], s["nu"], s["dt"], s["h"]))
    e_dir = oracle.rel_l2(gather(parts, "direct", N), oracle.c_solve_3d(ds, b, DIMS))
    e_2 = oracle.rel_l2(gather(parts, "pc_2diag", N), 0.5 * oracle.c_solve_3d(d0, b, DIMS))
    print(f"diffusion PCSHELL on {world} ranks: pc {e_pc:.3e} direct in place {e_dir:.3e} scaled Diag {e_2:.3e}")
    assert e_pc < TOL
    assert e_dir < TOL
    assert e_2 < TOL


def test_real_scalar_library_on_two_ranks(oracle):
    world = 2
    parts = _spawn(world, "real")
    nx, ny, nz = DIMS
    N, M = nx * ny * nz, nx // 2 + 1
    for r in range(world):
        assert parts[r]["dist"]
        assert parts[r]["diag_range"] == (r * 2 * M * ny * nz // world, (r + 1) * 2 * M * ny * nz // world)
    b = oracle.c_fill_uniform(N, 47).real.copy()
    h = [(MAXS[d] - MINS[d]) / DIMS[d] for d in range(3)]
    d0 = np_diag(DIMS, *numbers(DIMS, A, NU, DT, h))
    half = np.ascontiguousarray(d0.reshape(nz, ny, nx)[:, :, :M]).reshape(-1).view(np.float64)
    dg = gather(parts, "diag", 2 * M * ny * nz, np.float64, "diag_range")
    assert np.abs(dg - half).max() <= 1e-15 * np.abs(half).max()
    pc = gather(parts, "pc", N, np.float64)
    e_pc = oracle.rel_l2(pc.astype(np.complex128), oracle.c_solve_3d(d0, b.astype(np.complex128), DIMS))
    s = SOLVER
    ds = np_diag(DIMS, *numbers(DIMS, s["a"], s["nu"], s["dt"], s["h"]))
    dr = gather(parts, "direct", N, np.float64)
    e_dir = oracle.rel_l2(dr.astype(np.complex128), oracle.c_solve_3d(ds, b.astype(np.complex128), DIMS))
    print(f"real diffusion boundary on 2 ranks: pc {e_pc:.3e} direct {e_dir:.3e}")
    assert e_pc < TOL
    assert e_dir < TOL
