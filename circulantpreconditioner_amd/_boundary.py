"""The Python PETSc boundary, written once for both scalar builds.

The objects are the library's PETSc stand-in (include/petsc_mini.h): ``Vec`` (device VECSEQHIP /
VECMPIHIP, possibly wrapping a torch tensor's memory, or host VECSEQ / VECMPI), ``Comm``, ``Mat``
(FFT matrix, AIJ), ``PC`` (PCSHELL), ``KSP``; the functions carry the reference's names and
argument order (src/PCSHELLFft_3D.hxx, src/FftLinearSolver_3D.h).

Each class is written against a ``Binding``: the library getter, ``PetscCall``, the scalar
converter, the numpy dtype and the context structs of one build.  ``COMPLEX`` binds
``libcirculant_fft.so`` (PetscScalar = complex, ``petsc.py``) and ``REAL`` binds
``libcirculant_fft_real.so`` (PetscScalar = double, ``petsc_real.py``); a binding's classes are
subclasses that carry it as the class attribute ``B``, so ``isinstance`` and the classmethod
constructors work as on any class and nothing is defined twice.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np
import torch

from . import _lib
from ._lib import CirculantError
from ._lib_ext import AIJInfo, PetscScalar, context_structs

PETSC_COMM_WORLD, PETSC_COMM_SELF = 0, 1
PETSC_DEFAULT = -2
INSERT_VALUES, ADD_VALUES = 1, 2
NORM_1, NORM_2, NORM_INFINITY = 0, 1, 3
MATOP_MULT = 0
PC_LEFT, PC_RIGHT = 0, 1
KSP_REASONS = {0: "ITERATING", 2: "CONVERGED_RTOL", 3: "CONVERGED_ATOL", 4: "CONVERGED_ITS",
               7: "CONVERGED_HAPPY_BREAKDOWN", -3: "DIVERGED_ITS", -4: "DIVERGED_DTOL", -5: "DIVERGED_BREAKDOWN"}

# PCSHELL callbacks (setup, apply, destroy) by context struct and the upwind flag
_SHELL = {
    ("FFTPrecTransportContext", False): ("setupFFTPrec3D", "applyFFT3DPrecTransport", "destroyFFTPrec3D"),
    ("FFTPrecTransportContext", True): ("setupFFTPrec3DUpwind", "applyFFT3DPrecTransport", "destroyFFTPrec3D"),
    ("FFTPrecDiffusionContext", False): ("setupFFTPrec3DDiffusion", "applyFFT3DPrecDiffusion",
                                         "destroyFFTPrec3DDiffusion"),
    ("FFTPrecDiffusionContext", True): ("setupFFTPrec3DDiffusionUpwind", "applyFFT3DPrecDiffusion",
                                        "destroyFFTPrec3DDiffusion"),
    ("FFTPrecWaveContext", False): ("setupFFTPrec3DWave", "applyFFT3DPrecWave", "destroyFFTPrec3DWave"),
    ("FFTPrecWaveRealContext", False): ("setupFFTPrec3DWaveRealData", "applyFFT3DPrecWaveRealData",
                                        "destroyFFTPrec3DWaveRealData"),
}


class PetscError(CirculantError):
    pass


class _Object:
    """A Vec / Mat / PC / KSP handle of binding B (a c_void_p, an int, or another wrapper).  An
    owned handle is destroyed by destroy() or the finaliser; ``borrow`` wraps one that something
    else destroys (e.g. ctx.Diag, made and freed by the PCSHELL callbacks), ``release`` hands an
    owned one on to the caller."""
    B: "Binding" = None
    _destroy = ""  # the library's XDestroy(X*)

    def __init__(self, handle, owned: bool = True):
        handle = getattr(handle, "h", handle)  # another wrapper of the same object: share its handle
        self.h = handle if isinstance(handle, ctypes.c_void_p) else ctypes.c_void_p(handle)
        self.owned = owned

    @classmethod
    def borrow(cls, handle):
        return cls(handle, owned=False)

    def release(self) -> ctypes.c_void_p:
        self.owned = False
        return self.h

    def destroy(self) -> None:
        if self.owned and self.h is not None and self.h.value:
            self.B.call(getattr(self.B.lib(), self._destroy)(ctypes.byref(self.h)))
        self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Vec(_Object):
    """A PETSc Vec of the stand-in.  ``Vec.from_tensor`` wraps device memory without a copy."""
    _destroy = "VecDestroy"

    def __init__(self, handle, keep=None, owned: bool = False):
        """Wrap a Vec handle made elsewhere.  Unlike Mat / PC the bare constructor does not take
        ownership: the handles callers wrap by hand are members of a context (ctx.Diag, ctx.b_hat)
        that the library frees itself, and a finaliser on them would free twice.  The classmethod
        constructors and Mat.create_vecs return owned Vecs."""
        super().__init__(handle, owned)
        self._keep = keep  # keeps a wrapped tensor alive

    @classmethod
    def _create(cls, name: str, *args, keep=None) -> "Vec":
        h = ctypes.c_void_p()
        cls.B.call(getattr(cls.B.lib(), name)(*args, ctypes.byref(h)))
        return cls(h, keep=keep, owned=True)

    @classmethod
    def _tensor(cls, t: torch.Tensor) -> torch.Tensor:
        if t.dtype != getattr(torch, cls.B.dtype.name) or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"need a contiguous {cls.B.dtype.name} device tensor")
        return t

    @classmethod
    def from_tensor(cls, t: torch.Tensor) -> "Vec":
        return cls._create("VecCreateSeqHIPWithArray", PETSC_COMM_SELF, 1, cls._tensor(t).numel(), t.data_ptr(), keep=t)

    @classmethod
    def from_tensor_mpi(cls, t: torch.Tensor, N: int, comm: int = PETSC_COMM_WORLD) -> "Vec":
        """VecCreateMPIHIPWithArray: this rank's rows of a distributed Vec, in t's memory."""
        return cls._create("VecCreateMPIHIPWithArray", int(comm), 1, cls._tensor(t).numel(), int(N), t.data_ptr(),
                           keep=t)

    @classmethod
    def seq(cls, n: int, hip: bool = False) -> "Vec":
        """VecCreateSeq (host only: exercises the PCIe staging path) or VecCreateSeqHIP."""
        return cls._create("VecCreateSeqHIP" if hip else "VecCreateSeq", PETSC_COMM_SELF, int(n))

    @classmethod
    def mpi(cls, N: int, comm: int = PETSC_COMM_WORLD, nlocal: int = -1, hip: bool = False) -> "Vec":
        """VecCreateMPI(HIP)(comm, PETSC_DECIDE or nlocal, N): this rank's block of rows."""
        return cls._create("VecCreateMPIHIP" if hip else "VecCreateMPI", int(comm), int(nlocal), int(N))

    @classmethod
    def seq_hip(cls, n: int) -> "Vec":
        return cls.seq(n, hip=True)

    @classmethod
    def mpi_hip(cls, N: int, comm: int = PETSC_COMM_WORLD, nlocal: int = -1) -> "Vec":
        return cls.mpi(N, comm, nlocal, hip=True)

    def _int(self, name: str) -> int:
        n = ctypes.c_int64()
        self.B.call(getattr(self.B.lib(), name)(self.h, ctypes.byref(n)))
        return n.value

    @property
    def size(self) -> int:
        """Global size (VecGetSize)."""
        return self._int("VecGetSize")

    @property
    def local_size(self) -> int:
        return self._int("VecGetLocalSize")

    def state(self) -> int:
        """PetscObjectStateGet: increases on every write access."""
        return self._int("PetscObjectStateGet")

    def ownership_range(self) -> tuple:
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        self.B.call(self.B.lib().VecGetOwnershipRange(self.h, ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    def set_array(self, a) -> "Vec":
        """Write this rank's rows (local size)."""
        a = np.ascontiguousarray(np.asarray(a, dtype=self.B.dtype).reshape(-1))
        if a.size != self.local_size:
            raise ValueError("size mismatch")
        p, L = ctypes.c_void_p(), self.B.lib()
        self.B.call(L.VecGetArray(self.h, ctypes.byref(p)))
        ctypes.memmove(p, a.ctypes.data, a.nbytes)
        self.B.call(L.VecRestoreArray(self.h, ctypes.byref(p)))
        return self

    def array(self) -> np.ndarray:
        """This rank's rows (local size)."""
        out = np.empty(self.local_size, dtype=self.B.dtype)
        p, L = ctypes.c_void_p(), self.B.lib()
        self.B.call(L.VecGetArrayRead(self.h, ctypes.byref(p)))
        ctypes.memmove(out.ctypes.data, p, out.nbytes)
        self.B.call(L.VecRestoreArrayRead(self.h, ctypes.byref(p)))
        return out

    def set(self, alpha) -> "Vec":
        self.B.call(self.B.lib().VecSet(self.h, self.B.S(alpha)))
        return self

    def norm(self, kind: int = NORM_2) -> float:
        v = ctypes.c_double()
        self.B.call(self.B.lib().VecNorm(self.h, kind, ctypes.byref(v)))
        return v.value

    def dot(self, other: "Vec"):
        s = self.B.scalar()
        self.B.call(self.B.lib().VecDot(self.h, other.h, ctypes.byref(s)))
        return np.frombuffer(s, dtype=self.B.dtype)[0].item()

    def axpy(self, alpha, x: "Vec") -> "Vec":
        self.B.call(self.B.lib().VecAXPY(self.h, self.B.S(alpha), x.h))
        return self

    def scale(self, alpha) -> "Vec":
        self.B.call(self.B.lib().VecScale(self.h, self.B.S(alpha)))
        return self

    def hip_array(self):
        """Context manager: VecHIPGetArray / VecHIPRestoreArray (read-write device pointer)."""
        vec, B = self, self.B

        class _Arr:
            def __enter__(self_):
                self_.p = ctypes.c_void_p()
                B.call(B.lib().VecHIPGetArray(vec.h, ctypes.byref(self_.p)))
                return self_.p.value

            def __exit__(self_, *exc):
                B.call(B.lib().VecHIPRestoreArray(vec.h, ctypes.byref(self_.p)))
        return _Arr()

    def destroy(self) -> None:
        super().destroy()
        self._keep = None


class Comm:
    """A communicator of several ranks for the stand-in PETSc (an int handle, as MPI_Comm); each
    library has its own communicator table.

    ``Comm.torch(group)``: the collectives are torch.distributed's on `group` (under gloo the
    library stages the exchange pieces through pinned host memory) -- several processes may
    then share one GPU.  ``Comm.rccl(group)``: an RCCL communicator inside the library (one
    process per GPU), its unique id broadcast over `group`.  ``set_world()`` makes it
    PETSC_COMM_WORLD, the communicator setupFFTPrec3D builds its FFT matrix on
    (src/PCSHELLFft_3D.cxx:34-35)."""
    B: "Binding" = None

    _A2A = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
    _RED = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int64, ctypes.c_int)

    class _Ops(ctypes.Structure):
        pass

    _Ops._fields_ = [("alltoall", _A2A), ("allreduce", _RED), ("user", ctypes.c_void_p)]

    def __init__(self, handle: int | None = None, keep=()):
        """Wrap a communicator handle; without one, Comm.torch() on the default process group."""
        if handle is None:
            handle, keep = self._create_torch(None)
        self.handle = int(handle)
        if keep:
            # the ctypes callbacks of live communicators, by handle: the library calls them for as
            # long as the communicator exists, whether or not this object is still referenced
            self.B.comm_callbacks[self.handle] = keep

    @classmethod
    def torch(cls, group=None) -> "Comm":
        return cls(*cls._create_torch(group))

    @classmethod
    def _create_torch(cls, group) -> tuple:
        """PetscMiniCommCreate with torch.distributed's collectives on `group`: (handle, callbacks)."""
        import torch.distributed as dist
        size, rank = dist.get_world_size(group), dist.get_rank(group)

        def doubles(address, n):
            return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_double * n).from_address(address)))

        def alltoall(_user, send, recv, nbytes):
            try:
                n = size * nbytes // 8
                dist.all_to_all_single(doubles(recv, n), doubles(send, n).clone(), group=group)
                return 0
            except Exception:  # reported to the library as a failed collective
                return 1

        def allreduce(_user, buf, count, op):
            try:
                a = doubles(ctypes.addressof(buf.contents), count)
                t = a.clone()
                dist.all_reduce(t, op=dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM, group=group)
                a.copy_(t)
                return 0
            except Exception:
                return 1

        a2a, red = cls._A2A(alltoall), cls._RED(allreduce)
        ops = cls._Ops(a2a, red, None)
        h = ctypes.c_int()
        cls.B.call(cls.B.lib().PetscMiniCommCreate(size, rank, ctypes.byref(ops), ctypes.byref(h)))
        return h.value, (a2a, red, ops)

    @classmethod
    def rccl(cls, group=None, device: int | None = None) -> "Comm":
        import torch.distributed as dist
        B, L = cls.B, cls.B.lib()
        size, rank = dist.get_world_size(group), dist.get_rank(group)
        nbytes = L.cfp_dist_unique_id_bytes()
        uid = ctypes.create_string_buffer(nbytes)
        if rank == 0:
            B.check(L.cfp_dist_get_unique_id(uid))
        t = torch.frombuffer(bytearray(uid.raw), dtype=torch.uint8).clone()
        if dist.get_backend(group) == "nccl":
            t = t.to(f"cuda:{torch.cuda.current_device() if device is None else device}")
        dist.broadcast(t, src=0, group=group)
        uid = ctypes.create_string_buffer(bytes(t.cpu().numpy().tobytes()), nbytes)
        h = ctypes.c_int()
        B.call(L.PetscMiniCommCreateRCCL(size, rank, uid, ctypes.byref(h)))
        return cls(h.value)

    def _int(self, name: str) -> int:
        v = ctypes.c_int()
        getattr(self.B.lib(), name)(self.handle, ctypes.byref(v))
        return v.value

    @property
    def size(self) -> int:
        return self._int("MPI_Comm_size")

    @property
    def rank(self) -> int:
        return self._int("MPI_Comm_rank")

    def set_world(self) -> "Comm":
        self.B.set_comm_world(self)
        return self

    def allreduce(self, values, op: int = 0) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
        self.B.call(self.B.lib().PetscMiniAllreduce(self.handle, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                    a.size, int(op)))
        return a

    def destroy(self) -> None:
        """PetscMiniCommDestroy; refused (PetscError) while FFT matrices built on it exist.  The
        built-in PETSC_COMM_WORLD / PETSC_COMM_SELF (handles below 2) are left alone."""
        if self.handle >= 2:
            h = ctypes.c_int(self.handle)
            self.B.call(self.B.lib().PetscMiniCommDestroy(ctypes.byref(h)))
            self.B.comm_callbacks.pop(self.handle, None)
        self.handle = PETSC_COMM_SELF


class Mat(_Object):
    _destroy = "MatDestroy"

    @classmethod
    def create_fft(cls, dims: Sequence[int]) -> "Mat":
        """MatCreateFFT(PETSC_COMM_WORLD, ndim, dims = {n_z, n_y, n_x} row-major, MATFFTW, &A)."""
        d = (ctypes.c_int64 * len(dims))(*[int(v) for v in dims])
        h = ctypes.c_void_p()
        cls.B.call(cls.B.lib().MatCreateFFT(PETSC_COMM_WORLD, len(dims), d, b"fftw", ctypes.byref(h)))
        return cls(h)

    @classmethod
    def aij(cls, rowptr, col, val, shape) -> "Mat":
        """MatCreateSeqAIJWithArrays from CSR arrays (e.g. a scipy matrix' indptr, indices, data)."""
        m, n = shape
        rp = np.ascontiguousarray(rowptr, dtype=np.int64)
        cj = np.ascontiguousarray(col, dtype=np.int64)
        va = np.ascontiguousarray(val, dtype=cls.B.dtype)
        P64 = ctypes.POINTER(ctypes.c_int64)
        h = ctypes.c_void_p()
        cls.B.call(cls.B.lib().MatCreateSeqAIJWithArrays(PETSC_COMM_SELF, m, n, rp.ctypes.data_as(P64),
                                                         cj.ctypes.data_as(P64), va.ctypes.data, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def create_aij(cls, N: int, comm: int = PETSC_COMM_WORLD, nlocal: int = -1) -> "Mat":
        """MatCreateAIJ(comm, nlocal | PETSC_DECIDE, same, N, N, ...): an N x N matrix to fill with
        set_values and assemble (the reference's MatCreateAIJ on PETSC_COMM_WORLD)."""
        h = ctypes.c_void_p()
        cls.B.call(cls.B.lib().MatCreateAIJ(comm, nlocal, nlocal, N, N, 7, None, 6, None, ctypes.byref(h)))
        return cls(h)

    def set_values(self, rows, cols, vals, add: bool = False) -> "Mat":
        """MatSetValues(A, len(rows), rows, len(cols), cols, vals (row-major), mode)."""
        r = np.ascontiguousarray(rows, dtype=np.int64)
        c = np.ascontiguousarray(cols, dtype=np.int64)
        v = np.ascontiguousarray(vals, dtype=self.B.dtype).reshape(-1)
        if v.size != r.size * c.size:
            raise ValueError("vals must hold len(rows) * len(cols) values")
        P64 = ctypes.POINTER(ctypes.c_int64)
        self.B.call(self.B.lib().MatSetValues(self.h, r.size, r.ctypes.data_as(P64), c.size, c.ctypes.data_as(P64),
                                              v.ctypes.data, ADD_VALUES if add else INSERT_VALUES))
        return self

    def assemble(self) -> "Mat":
        self.B.call(self.B.lib().MatAssemblyBegin(self.h, 0))
        self.B.call(self.B.lib().MatAssemblyEnd(self.h, 0))
        return self

    def _int_pair(self, name: str) -> tuple:
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self.B.call(getattr(self.B.lib(), name)(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def ownership_range(self) -> tuple:
        return self._int_pair("MatGetOwnershipRange")

    def halo(self) -> tuple:
        """(ghost columns of this rank, the largest per-peer halo over the ranks): MATMPIAIJ."""
        return self._int_pair("PetscMiniMatMPIAIJGetHalo")

    def solve_counts(self) -> tuple:
        """(solve_3D calls that used the plan's own symbol, calls that streamed the given Diag)."""
        return self._int_pair("MatFFTHIPGetSolveCounts")

    def create_vecs(self, nvec: int = 1) -> list:
        """MatCreateVecsFFTW: the first nvec of (x, y, z); the caller owns them."""
        hs = [ctypes.c_void_p() for _ in range(3)]
        refs = [ctypes.byref(hs[i]) if i < nvec else None for i in range(3)]
        self.B.call(self.B.lib().MatCreateVecsFFTW(self.h, *refs))
        return [self.B.Vec(hs[i], owned=True) for i in range(nvec)]

    def fused_ba_count(self) -> int:
        """MatFFTHIPGetFusedBACount: the applyFFT3DPrecTransportBA calls that formed A x inside the
        apply's first sweep (the calls that ran MatMult and the apply separately do not count)."""
        n = ctypes.c_int64()
        self.B.call(self.B.lib().MatFFTHIPGetFusedBACount(self.h, ctypes.byref(n)))
        return n.value

    def mult(self, x: Vec, y: Vec) -> Vec:
        self.B.call(self.B.lib().MatMult(self.h, x.h, y.h))
        return y

    def mult_transpose(self, x: Vec, y: Vec) -> Vec:
        self.B.call(self.B.lib().MatMultTranspose(self.h, x.h, y.h))
        return y

    def aij_format(self) -> str:
        """The stand-in AIJ's device storage: 'dia' (row-class diagonal form), 'bdia' (block
        row-class form, e.g. the interleaved wave operator), 'csr', or 'none' before the first
        device MatMult."""
        f = ctypes.c_int()
        self.B.call(self.B.lib().PetscMiniMatAIJGetFormat(self.h, ctypes.byref(f)))
        return {1: "dia", 2: "bdia", 0: "csr"}.get(f.value, "none")

    def aij_info(self) -> dict:
        """PetscMiniMatAIJDescribe: the form the next device MatMult will use, chosen on the host
        (no device needed): format 'csr' / 'dia' / 'bdia', B, nd, ncls, nblk, re, lds_bytes."""
        info = AIJInfo()
        self.B.call(self.B.lib().PetscMiniMatAIJDescribe(self.h, ctypes.byref(info)))
        return info.as_dict()

    def shift(self, a) -> "Mat":
        self.B.call(self.B.lib().MatShift(self.h, self.B.S(a)))
        return self


class PC(_Object):
    _destroy = "PCDestroy"

    def __init__(self, handle: ctypes.c_void_p | None = None, owned: bool = True):
        if handle is None:
            handle = ctypes.c_void_p()
            self.B.call(self.B.lib().PCCreate(PETSC_COMM_WORLD, ctypes.byref(handle)))
        super().__init__(handle, owned)
        self.ctx = None

    @classmethod
    def shell(cls, ctx, upwind: bool = False) -> "PC":
        return cls().set_shell(ctx, upwind)

    @classmethod
    def wave_shell(cls, ctx) -> "PC":
        """PCSHELL with the block-circulant wave callbacks (include/wave_system.h)."""
        return cls().set_shell(ctx)

    def set_shell(self, ctx, upwind: bool = False) -> "PC":
        """PCSetType(pc, PCSHELL); PCShellSetContext; PCShellSetSetUp/Apply/Destroy with the
        callbacks of ctx's kind (the registration the reference never does, ToDo.md:1): a
        transport, diffusion, wave or real-data wave context.  upwind=True: the setup with the upwind symbol, for
        numbers of either sign (setupFFTPrec3DUpwind / setupFFTPrec3DDiffusionUpwind)."""
        names = _SHELL.get((type(ctx).__name__, bool(upwind)))
        if names is None:
            raise TypeError(f"no PCSHELL callbacks for {type(ctx).__name__} (upwind={bool(upwind)}); supported: "
                            + ", ".join(f"{k}{' (upwind)' if u else ''}" for k, u in _SHELL))
        return self.set_shell_callbacks(ctx, *names)

    def set_shell_callbacks(self, ctx, setup: str, apply: str, destroy: str) -> "PC":
        """The PCSHELL registration, by the names of the library's three callbacks."""
        L, call, fn = self.B.lib(), self.B.call, self.B.fn
        call(L.PCSetType(self.h, b"shell"))
        self.ctx = ctx  # the library keeps its address
        call(L.PCShellSetContext(self.h, ctypes.addressof(ctx)))
        call(L.PCShellSetSetUp(self.h, fn(setup)))
        call(L.PCShellSetApply(self.h, fn(apply)))
        call(L.PCShellSetDestroy(self.h, fn(destroy)))
        return self

    @classmethod
    def none(cls) -> "PC":
        return cls().set_none()

    def set_none(self) -> "PC":
        self.B.call(self.B.lib().PCSetType(self.h, b"none"))
        return self

    def setup(self) -> "PC":
        self.B.call(self.B.lib().PCSetUp(self.h))
        return self

    def apply(self, b: Vec, x: Vec) -> Vec:
        self.B.call(self.B.lib().PCApply(self.h, b.h, x.h))
        return x

    def set_operators(self, A: "Mat", Pm: "Mat | None" = None) -> "PC":
        self.B.call(self.B.lib().PCSetOperators(self.h, A.h, (Pm or A).h))
        return self


class KSP(_Object):
    """KSPGMRES of the stand-in (csrc/ksp_gmres.cpp): restart 30, left preconditioning, CGS,
    rtol 1e-5 / abstol 1e-50 / dtol 1e5 / maxits 10000 unless set, as PETSc's defaults."""
    _destroy = "KSPDestroy"

    def __init__(self):
        h = ctypes.c_void_p()
        self.B.call(self.B.lib().KSPCreate(PETSC_COMM_WORLD, ctypes.byref(h)))
        super().__init__(h)
        self._ops = None
        self._pc = None
        self.set_type("gmres")

    def _set(self, name: str, *args) -> "KSP":
        self.B.call(getattr(self.B.lib(), name)(self.h, *args))
        return self

    def _get(self, name: str, ctype):
        v = ctype()
        self.B.call(getattr(self.B.lib(), name)(self.h, ctypes.byref(v)))
        return v.value

    def set_type(self, t: str) -> "KSP":
        return self._set("KSPSetType", t.encode())

    def set_tolerances(self, rtol=PETSC_DEFAULT, abstol=PETSC_DEFAULT, dtol=PETSC_DEFAULT,
                       maxits=PETSC_DEFAULT) -> "KSP":
        return self._set("KSPSetTolerances", float(rtol), float(abstol), float(dtol), int(maxits))

    def set_restart(self, m: int) -> "KSP":
        return self._set("KSPGMRESSetRestart", int(m))

    def set_pc_side(self, side: int) -> "KSP":
        return self._set("KSPSetPCSide", int(side))

    def set_initial_guess_nonzero(self, flag: bool = True) -> "KSP":
        return self._set("KSPSetInitialGuessNonzero", 1 if flag else 0)

    def get_pc(self) -> PC:
        if self._pc is None:
            h = ctypes.c_void_p()
            self.B.call(self.B.lib().KSPGetPC(self.h, ctypes.byref(h)))
            self._pc = self.B.PC.borrow(h)
        return self._pc

    def set_operators(self, A: Mat, P: Mat | None = None) -> "KSP":
        self._ops = (A, P or A)
        return self._set("KSPSetOperators", A.h, (P or A).h)

    def setup(self) -> "KSP":
        return self._set("KSPSetUp")

    def solve(self, b: Vec, x: Vec) -> int:
        self._set("KSPSolve", b.h, x.h)
        return self.reason

    @property
    def reason(self) -> int:
        return self._get("KSPGetConvergedReason", ctypes.c_int)

    @property
    def its(self) -> int:
        return self._get("KSPGetIterationNumber", ctypes.c_int64)

    @property
    def rnorm(self) -> float:
        return self._get("KSPGetResidualNorm", ctypes.c_double)

    def pc_stats(self) -> tuple:
        n, s = ctypes.c_int64(), ctypes.c_double()
        self.B.call(self.B.lib().KSPMiniGetPCApplyStats(self.h, ctypes.byref(n), ctypes.byref(s)))
        return n.value, s.value

    def destroy(self) -> None:
        if self._pc is not None and self.h is not None and self.h.value:
            self._pc.h = None  # KSPDestroy frees the PC it handed out
        super().destroy()


class Binding:
    """One scalar build of the boundary: `lib` (the library getter), ``call`` (PetscCall), ``S``
    (a Python number as the build's PetscScalar argument), ``scalar`` / ``dtype`` (its ctypes and
    numpy types), the four context structs, the classes above bound to it, and the
    reference-named functions."""

    def __init__(self, lib, scalar, dtype):
        self.lib, self.scalar, self.dtype = lib, scalar, np.dtype(dtype)
        self.S = PetscScalar.of if scalar is PetscScalar else float
        self.comm_callbacks: dict = {}
        self.structs = context_structs(scalar)
        for cls in (Vec, Comm, Mat, PC, KSP):
            setattr(self, cls.__name__, type(cls.__name__, (cls,), {"B": self, "__doc__": cls.__doc__}))

    def _last_error(self) -> str:
        return self.lib().cfp_last_error().decode(errors="replace")

    def check(self, rc: int) -> None:
        """A cfp_* return code: CirculantError with the library's message."""
        if rc != 0:
            raise CirculantError(rc, self._last_error())

    def call(self, rc: int) -> None:
        """PetscCall: PetscError with PetscErrorLastMessage and the library's own last error."""
        if rc != 0:
            msg = (self.lib().PetscErrorLastMessage() or b"").decode(errors="replace")
            cfp = self._last_error()
            raise PetscError(rc, f"{msg} {('| ' + cfp) if cfp else ''}".strip())

    def fn(self, name: str) -> int:
        """Address of a library function (for PCShellSetApply & co.)."""
        return ctypes.cast(getattr(self.lib(), name), ctypes.c_void_p).value

    def set_comm_world(self, comm: "Comm | int") -> None:
        """PETSC_COMM_WORLD := comm (PETSC_COMM_SELF: back to one rank)."""
        self.call(self.lib().PetscMiniSetCommWorld(comm.handle if isinstance(comm, Comm) else int(comm)))

    # --------------------------------------------------------- reference-named functions
    def getFFTPrec3DContext(self, ndim, dt, nbCells, a_x, a_y, a_z, Xmin, Ymin, Zmin, Xmax, Ymax, Zmax):
        """src/PCSHELLFft_3D.cxx:101-151 (returns the filled context)."""
        ctx, S = self.structs.FFTPrecTransportContext(), self.S
        self.call(self.lib().getFFTPrec3DContext(int(ndim), S(dt), int(nbCells), S(a_x), S(a_y), S(a_z), S(Xmin),
                                                 S(Ymin), S(Zmin), S(Xmax), S(Ymax), S(Zmax), ctypes.byref(ctx)))
        return ctx

    def diffusion_context(self, ndim: int, dt: float, dims: Sequence[int], a: Sequence[float], nu: float, mins, maxs):
        """getFFTPrec3DDiffusionContext: the PCSHELL context with the matched numbers
        lambda_d = a_d dt / h_d, mu_d = nu dt / h_d^2."""
        ctx, S, d3 = self.structs.FFTPrecDiffusionContext(), self.S, ctypes.c_double * 3
        self.call(self.lib().getFFTPrec3DDiffusionContext(
            int(ndim), S(dt), int(dims[0]), int(dims[1]), int(dims[2]), S(a[0]), S(a[1]), S(a[2]), S(nu),
            d3(*[float(v) for v in mins]), d3(*[float(v) for v in maxs]), ctypes.byref(ctx)))
        return ctx

    def make_context(self, dims: Sequence[int], lam: Sequence, space_dim: int = 3):
        """Context with explicit n and lambda (the reference struct filled by hand)."""
        ctx = self.structs.FFTPrecTransportContext()
        ctx.spaceDim = space_dim
        ctx.n_x, ctx.n_y, ctx.n_z = (int(d) for d in dims)
        ctx.lambda_x, ctx.lambda_y, ctx.lambda_z = (self.S(v) for v in lam)
        self.call(self.lib().FFTPrecTransportContextSetRemapBack(ctypes.byref(ctx), None))  # fresh side-table entry
        return ctx

    def context_plan(self, ctx) -> int:
        """The HIP plan behind ctx.FFT_MAT after setupFFTPrec3D (MatFFTHIPGetPlan), as an int handle."""
        if not ctx.FFT_MAT:
            return 0
        h = ctypes.c_void_p()
        self.call(self.lib().MatFFTHIPGetPlan(ctypes.c_void_p(ctx.FFT_MAT), ctypes.byref(h)))
        return h.value or 0

    def context_remap_back(self, ctx) -> int:
        """This build's Cartesian -> mesh remap of ctx (side table; 0 = none)."""
        h = ctypes.c_void_p()
        self.call(self.lib().FFTPrecTransportContextGetRemapBack(ctypes.byref(ctx), ctypes.byref(h)))
        return h.value or 0

    def applyFFT3DPrecTransport(self, pc: PC, b: Vec, x: Vec) -> None:
        self.call(self.lib().applyFFT3DPrecTransport(pc.h, b.h, x.h))

    def applyFFT3DPrecTransportBA(self, pc: PC, side: int, x: Vec, y: Vec, work: Vec) -> None:
        """The PCShellSetApplyBA callback: y = B A x (PC_LEFT) or A B x (PC_RIGHT), A the PC's operator."""
        self.call(self.lib().applyFFT3DPrecTransportBA(pc.h, int(side), x.h, y.h, work.h))

    def setupFFTPrec3D(self, pc: PC) -> None:
        self.call(self.lib().setupFFTPrec3D(pc.h))

    def destroyFFTPrec3D(self, pc: PC) -> None:
        self.call(self.lib().destroyFFTPrec3D(pc.h))

    def solve_3D(self, FFT_MAT: Mat, X: Vec, Diag: Vec, b: Vec, b_hat: Vec | None, size: int) -> None:
        self.call(self.lib().solve_3D(FFT_MAT.h, X.h, Diag.h, b.h, b_hat.h if b_hat is not None else None, int(size)))

    def build_transport_col(self, c: Vec, size: int) -> None:
        self.call(self.lib().build_transport_col(c.h, int(size)))

    def build_diag_mat_vec_3D(self, Diag: Vec, c_x_hat: Vec, c_y_hat: Vec, c_z_hat: Vec, n_x, n_y, n_z, lambda_x,
                              lambda_y, lambda_z) -> None:
        S = self.S
        self.call(self.lib().build_diag_mat_vec_3D(Diag.h, c_x_hat.h, c_y_hat.h, c_z_hat.h, int(n_x), int(n_y),
                                                   int(n_z), S(lambda_x), S(lambda_y), S(lambda_z)))

    def FftTransportSolver(self, n_x, n_y, n_z, lambda_x, lambda_y, lambda_z, X: Vec, b: Vec, FFT_MAT: Mat) -> None:
        S = self.S
        self.call(self.lib().FftTransportSolver(int(n_x), int(n_y), int(n_z), S(lambda_x), S(lambda_y), S(lambda_z),
                                                X.h, b.h, FFT_MAT.h))

    def Fft3DTransportSolver(self, n_x, n_y, n_z, a_x, a_y, a_z, dt, delta_x, delta_y, delta_z, X: Vec, b: Vec,
                             FFT_MAT: Mat) -> None:
        S = self.S
        self.call(self.lib().Fft3DTransportSolver(int(n_x), int(n_y), int(n_z), S(a_x), S(a_y), S(a_z), S(dt),
                                                  S(delta_x), S(delta_y), S(delta_z), X.h, b.h, FFT_MAT.h))

    def Fft2DTransportSolver(self, n_x, n_y, a_x, a_y, dt, delta_x, delta_y, X: Vec, b: Vec, FFT_MAT: Mat) -> None:
        S = self.S
        self.call(self.lib().Fft2DTransportSolver(int(n_x), int(n_y), S(a_x), S(a_y), S(dt), S(delta_x), S(delta_y),
                                                  X.h, b.h, FFT_MAT.h))

    def Fft1DTransportSolver(self, n_x, a_x, dt, delta_x, X: Vec, b: Vec, FFT_MAT: Mat) -> None:
        S = self.S
        self.call(self.lib().Fft1DTransportSolver(int(n_x), S(a_x), S(dt), S(delta_x), X.h, b.h, FFT_MAT.h))

    def _structured(self, struct, FFT_MAT: Mat, ints: dict, scalars: dict):
        c = struct()
        for name, v in ints.items():
            setattr(c, name, int(v))
        for name, v in scalars.items():
            setattr(c, name, self.S(v))
        c.FFT_MAT = FFT_MAT.h
        return c

    def StructuredContext(self, n_x, n_y, n_z, a_x, a_y, a_z, dt, delta_x, delta_y, delta_z, FFT_MAT: Mat):
        """StructuredTransportContext (src/FftLinearSolver_3D.h:7-19), for PetscFft3DTransportSolver."""
        return self._structured(self.structs.StructuredTransportContext, FFT_MAT, dict(n_x=n_x, n_y=n_y, n_z=n_z),
                                dict(a_x=a_x, a_y=a_y, a_z=a_z, dt=dt, delta_x=delta_x, delta_y=delta_y,
                                     delta_z=delta_z))

    def structured_diffusion_context(self, n_x, n_y, n_z, a_x, a_y, a_z, nu, dt, delta_x, delta_y, delta_z,
                                     FFT_MAT: Mat):
        """StructuredDiffusionContext (include/diffusion_equation.h), for PetscFft3DDiffusionSolver."""
        return self._structured(self.structs.StructuredDiffusionContext, FFT_MAT, dict(n_x=n_x, n_y=n_y, n_z=n_z),
                                dict(a_x=a_x, a_y=a_y, a_z=a_z, nu=nu, dt=dt, delta_x=delta_x, delta_y=delta_y,
                                     delta_z=delta_z))

    def PetscFft3DTransportSolver(self, customCtx, b: Vec, x: Vec) -> None:
        self.call(self.lib().PetscFft3DTransportSolver(customCtx, b.h, x.h))

    def PetscFft3DDiffusionSolver(self, customCtx, b: Vec, x: Vec) -> None:
        self.call(self.lib().PetscFft3DDiffusionSolver(customCtx, b.h, x.h))


COMPLEX = Binding(_lib.lib, PetscScalar, np.complex128)
REAL = Binding(_lib.real_lib, ctypes.c_double, np.float64)
