"""The real-scalar PETSc boundary on a communicator of several ranks, on the GPU.

The reference's real branch runs on PETSC_COMM_WORLD like the complex one
(src/FftLinearSolver_3D.c:6-78,176,186,235-249; src/PCSHELLFft_3D.cxx:34-35).  Here 2 and 4 fresh
processes share cuda:0; PETSC_COMM_WORLD of libcirculant_fft_real.so is a communicator with
torch.distributed's collectives (gloo), so MatCreateFFT backs the real FFT matrix with the complex
z-slab plan.  Each rank holds its z-planes: nzl ny nx grid reals, and FFTW-MPI's r2c slab
[nzl][ny][nx/2 + 1] of the spectrum.  Checked against the oracle's solve of the same real b
(1e-10) and numpy's rfftn / irfftn:
  setupFFTPrec3D + PCApply (device and host Vecs), PetscFft3DTransportSolver(ctx, Un, Un) (two
  steps, device and host), solve_3D with a changed Diag, MatMult / MatMultTranspose,
  build_diag_mat_vec_3D on the distributed half-spectrum Diag.
"""
import ctypes
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-10


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, dims, lam, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from circulantpreconditioner_amd import petsc_real as R
        from oracle import oracle as O
        torch.cuda.set_device(0)
        L = R.lib()
        comm = R.Comm.torch().set_world()
        nx, ny, nz = dims
        N = nx * ny * nz
        M = nx // 2 + 1
        b = O.c_fill_uniform(N, 47).real.copy()
        out = {}
        # --- the PCSHELL on PETSC_COMM_WORLD (setup builds the FFT matrix there)
        ctx = R.FFTPrecTransportContext(3, nx, ny, nz, lam[0], lam[1], lam[2], None, None, None, None, None)
        pc = R.pc_shell(ctx)
        dp = ctypes.c_void_p()
        R.PetscCall(L.MatFFTHIPGetDistPlan(ctx.FFT_MAT, ctypes.byref(dp)))
        out["dist"] = bool(dp.value)
        diag = R.Vec.borrow(ctx.Diag)
        dlo, dhi = diag.ownership_range()
        out["diag_range"] = (dlo, dhi)
        out["diag"] = diag.array()
        for hip in (True, False):
            vb, vx = R.Vec.mpi(N, hip=hip), R.Vec.mpi(N, hip=hip)
            lo, hi = vb.ownership_range()
            out["range"] = (lo, hi)
            vb.set_array(b[lo:hi])
            R.PetscCall(L.PCApply(pc, vb.h, vx.h))
            out["pc_hip" if hip else "pc_host"] = vx.array()
            vb.destroy()
            vx.destroy()
        lo, hi = out["range"]
        # --- the direct solver in place, two steps (device and host)
        a, dt = (1.0, 0.5, 0.25), 0.02
        h = (1.0 / nx, 1.0 / ny, 1.0 / nz)
        F = R.mat_create_fft([nz, ny, nx])
        sc = R.StructuredTransportContext(nx, ny, nz, a[0], a[1], a[2], dt, h[0], h[1], h[2], F)
        for hip in (True, False):
            u = R.Vec.mpi(N, hip=hip).set_array(b[lo:hi])
            steps = []
            for _ in range(2):
                R.PetscCall(L.PetscFft3DTransportSolver(sc, u.h, u.h))
                steps.append(u.array())
            out["direct_hip" if hip else "direct_host"] = steps
            u.destroy()
        # --- MatMult / MatMultTranspose: r2c of the slab, c2r of a half-spectrum slab
        xg, ys, _ = R.mat_create_vecs_fftw(F)
        xg.set_array(b[lo:hi])
        R.PetscCall(L.MatMult(F, xg.h, ys.h))
        out["fwd"] = ys.array()
        out["fwd_range"] = ys.ownership_range()
        R.PetscCall(L.MatMultTranspose(F, ys.h, xg.h))
        out["bwd"] = xg.array()
        # an arbitrary (not Hermitian-consistent) half spectrum: FFTW's c2r = Re IDFT(extension)
        rng = np.random.default_rng(11)
        yr = rng.standard_normal(2 * M * ny * nz)
        slo, shi = out["fwd_range"]
        ys.set_array(yr[slo:shi])
        R.PetscCall(L.MatMultTranspose(F, ys.h, xg.h))
        out["bwd_any"] = xg.array()
        xg.destroy()
        ys.destroy()
        R.PetscCall(L.MatDestroy(ctypes.byref(F)))
        # --- solve_3D divides by the Diag it is given (a changed Diag: the explicit path)
        R.PetscCall(L.VecScale(ctypes.c_void_p(ctx.Diag), 2.0))
        vb, vx = R.Vec.mpi(N, hip=True), R.Vec.mpi(N, hip=True)
        vb.set_array(b[lo:hi])
        R.PetscCall(L.PCApply(pc, vb.h, vx.h))
        out["pc_2diag"] = vx.array()
        own, exp = ctypes.c_int64(), ctypes.c_int64()
        R.PetscCall(L.MatFFTHIPGetSolveCounts(ctypes.c_void_p(ctx.FFT_MAT), ctypes.byref(own), ctypes.byref(exp)))
        out["counts"] = (own.value, exp.value)
        # --- build_diag_mat_vec_3D on the distributed half-spectrum Diag (1-D r2c columns given)
        cols = []
        for n_d in (nx, ny, nz):
            c = np.fft.rfft(np.array([1.0, -1.0] + [0.0] * (n_d - 2))[:n_d]) if n_d > 1 else np.zeros(1, complex)
            v = R.Vec.seq(2 * (n_d // 2 + 1)).set_array(c.view(np.float64))
            cols.append(v)
        R.PetscCall(L.build_diag_mat_vec_3D(ctypes.c_void_p(ctx.Diag), cols[0].h, cols[1].h, cols[2].h, nx, ny, nz,
                                            lam[0], lam[1], lam[2]))
        out["diag_built"] = diag.array()
        for v in cols + [vb, vx]:
            v.destroy()
        R.PetscCall(L.PCDestroy(ctypes.byref(pc)))
        R.set_comm_world(R.PETSC_COMM_SELF)
        comm.destroy()
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dims,world", [((32, 16, 24), 2), ((9, 6, 8), 2), ((32, 32, 16), 4), ((64, 64, 64), 4)])
def test_real_scalar_on_several_ranks(dims, world, oracle):
    import torch.multiprocessing as mp
    lam = (0.6, 0.15, 0.02)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, dims, lam, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        parts = dict(q.get(timeout=240) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    nx, ny, nz = dims
    N = nx * ny * nz
    M = nx // 2 + 1
    NS = 2 * M * ny * nz

    def gather(key, n=N, rkey="range", idx=None):
        x = np.empty(n)
        for r in range(world):
            lo, hi = parts[r][rkey]
            x[lo:hi] = parts[r][key] if idx is None else parts[r][key][idx]
        return x

    for r in range(world):
        assert parts[r]["dist"], "several ranks: the real FFT matrix is backed by the slab plan"
        assert parts[r]["range"] == (r * N // world, (r + 1) * N // world)  # whole z-planes
        assert parts[r]["diag_range"] == (r * NS // world, (r + 1) * NS // world)
        assert parts[r]["counts"] == (2, 1)  # own symbol (device, host), then the changed Diag
    b = oracle.c_fill_uniform(N, 47).real.copy()
    d0 = oracle.c_build_diag_transport(dims, lam).reshape(nz, ny, nx)
    half = np.ascontiguousarray(d0[..., :M]).view(np.float64).reshape(-1)
    assert np.abs(gather("diag", NS, "diag_range") - half).max() < 1e-13
    assert np.abs(gather("diag_built", NS, "diag_range") - half).max() < 1e-13

    def solve(diag, rhs):
        x = oracle.c_solve_3d(diag.reshape(-1), rhs.astype(np.complex128), dims)
        return x.real

    ref = solve(d0, b)
    for key in ("pc_hip", "pc_host"):
        got = gather(key)
        assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < TOL, key
    got = gather("pc_2diag")
    ref2 = solve(2 * d0, b)
    assert np.linalg.norm(got - ref2) / np.linalg.norm(ref2) < TOL
    lam_d = (1.0 * 0.02 * nx, 0.5 * 0.02 * ny, 0.25 * 0.02 * nz)  # a dt / delta
    dd = oracle.c_build_diag_transport(dims, lam_d)
    for key in ("direct_hip", "direct_host"):
        r1 = solve(dd, b)
        r2 = solve(dd, r1)
        for k, refk in enumerate((r1, r2)):
            got = gather(key, idx=k)
            assert np.linalg.norm(got - refk) / np.linalg.norm(refk) < TOL, (key, k)
    bz = b.reshape(nz, ny, nx)
    f = np.ascontiguousarray(np.fft.rfftn(bz)).view(np.float64).reshape(-1)
    got = gather("fwd", NS, "fwd_range")
    assert np.linalg.norm(got - f) / np.linalg.norm(f) < 1e-12
    g = gather("bwd")
    assert np.linalg.norm(g - b * N) / np.linalg.norm(b * N) < 1e-12  # c2r(r2c(b)) = N b
    # an arbitrary half spectrum: FFTW's c2r semantics (Re IDFT of the Hermitian extension)
    yr = np.random.default_rng(11).standard_normal(NS).view(np.complex128).reshape(nz, ny, M)
    full = np.empty((nz, ny, nx), complex)
    full[..., :M] = yr
    for kx in range(M, nx):
        full[:, :, kx] = np.conj(yr[(-np.arange(nz)) % nz][:, (-np.arange(ny)) % ny, nx - kx])
    want = (np.fft.ifftn(full) * N).real.reshape(-1)
    got = gather("bwd_any")
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-12
