"""The one Python PETSc boundary of both scalar builds, without a GPU: the signature table of
_lib_ext.py against the two built libraries and the headers, the layout of the scalar-typed
context structs, and the shared Vec / Comm / Mat classes through petsc.py and petsc_real.py."""
import ctypes
import gc
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# table entries that only the complex library holds although no complex-only header declares them
COMPLEX_ONLY_OUTSIDE_THE_DRIVER_HEADERS: list = []


@pytest.fixture(scope="module")
def ext():
    from circulantpreconditioner_amd import _lib_ext
    return _lib_ext


@pytest.fixture(scope="module")
def libs(ext):
    """{build: (library, its scalar type)}, both loaded in this process."""
    from circulantpreconditioner_amd import _lib
    return {ext.COMPLEX_BUILD: (_lib.lib(), ext.PetscScalar), ext.REAL_BUILD: (_lib.real_lib(), ctypes.c_double)}


def module(name):
    from circulantpreconditioner_amd import petsc, petsc_real
    return {"petsc": petsc, "petsc_real": petsc_real}[name]


def test_every_table_entry_resolves_exactly_where_it_is_tagged(ext, libs):
    for build, (L, S) in libs.items():
        n = 0
        for group, where, sig in ext.signatures(S):
            assert where in (ext.BOTH, ext.COMPLEX_BUILD, ext.REAL_BUILD), (group, where)
            for name, (args, res) in sig.items():
                if where in (ext.BOTH, build):
                    fn = getattr(L, name)  # AttributeError: the library lacks a name the table promises
                    assert fn.argtypes is not None and list(fn.argtypes) == args and fn.restype == res, (build, name)
                    n += 1
                else:
                    assert not hasattr(L, name), f"{name} ({group}) is tagged absent from the {build} library"
        print(f"{build}: {n} functions declared")
    names = [k for _, _, sig in ext.signatures(ctypes.c_double) for k in sig]
    assert len(names) == len(set(names)), "a function stands in two groups of the table"


def test_complex_only_tags_are_the_driver_headers(ext):
    """What the real-scalar library lacks is what transport_equation.h, wave_system.h and
    mesh_unstructured.h declare (their sources are not compiled into it), nothing else."""
    from circulantpreconditioner_amd._lib import _parse_decls
    declared = set()
    for hdr in ("transport_equation.h", "wave_system.h", "mesh_unstructured.h"):
        declared |= set(_parse_decls(os.path.join(ROOT, "include", hdr)))
    table = ext.signatures(ext.PetscScalar)
    every = {k for _, _, sig in table for k in sig}
    tagged = {k for _, where, sig in table if where == ext.COMPLEX_BUILD for k in sig}
    assert tagged == (every & declared) | set(COMPLEX_ONLY_OUTSIDE_THE_DRIVER_HEADERS)
    assert {k for _, where, sig in table if where == ext.REAL_BUILD for k in sig} == {"MatFFTHIPGetRealPlan"}


def test_context_struct_layouts(ext):
    C, R = ext.context_structs(ext.PetscScalar), ext.context_structs(ctypes.c_double)
    assert ext.context_structs(ext.PetscScalar) is C  # built once per scalar
    assert ext.FFTPrecTransportContext is C.FFTPrecTransportContext
    for name, nscalars in (("FFTPrecTransportContext", 3), ("FFTPrecDiffusionContext", 6),
                           ("StructuredTransportContext", 7), ("StructuredDiffusionContext", 8)):
        c, r = getattr(C, name), getattr(R, name)
        assert [k for k, _ in c._fields_] == [k for k, _ in r._fields_], name
        assert [k for k, t in c._fields_ if t is ext.PetscScalar] == [k for k, t in r._fields_ if t is ctypes.c_double]
        assert sum(t is ext.PetscScalar for _, t in c._fields_) == nscalars, name
        assert ctypes.sizeof(c) - ctypes.sizeof(r) == 8 * nscalars, name
    for S in (C, R):  # the 12 shared leading members the C side relies on
        assert S.FFTPrecDiffusionContext._fields_[:12] == S.FFTPrecTransportContext._fields_
        assert len(S.FFTPrecTransportContext._fields_) == 12
        for k, _ in S.FFTPrecTransportContext._fields_:
            assert getattr(S.FFTPrecDiffusionContext, k).offset == getattr(S.FFTPrecTransportContext, k).offset


@pytest.mark.parametrize("name", ["petsc", "petsc_real"])
def test_shared_vec_on_host(name):
    M = module(name)
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(101), rng.standard_normal(101)
    if name == "petsc":
        a, b = a + 1j * rng.standard_normal(101), b + 1j * rng.standard_normal(101)
    alpha = 2.5 if name == "petsc_real" else 2.5 - 0.75j
    va, vb = M.Vec.seq(101).set_array(a), M.Vec.seq(101).set_array(b)
    assert va.size == va.local_size == 101 and va.array().dtype == a.dtype
    assert np.array_equal(va.array(), a)
    assert va.norm() == pytest.approx(np.linalg.norm(a), rel=1e-14)
    assert va.dot(vb) == pytest.approx(np.vdot(b, a), rel=1e-14)  # VecDot(x, y) = y^H x
    np.testing.assert_allclose(vb.axpy(alpha, va).array(), b + alpha * a, rtol=1e-14)
    np.testing.assert_allclose(vb.scale(-0.5).array(), -0.5 * (b + alpha * a), rtol=1e-14)
    with pytest.raises(ValueError):
        va.set_array(a[:100])
    # a borrowed Vec leaves the handle to its owner
    w = M.Vec.borrow(va.h.value)
    assert not w.owned and np.array_equal(w.array(), a)
    del w
    gc.collect()
    assert va.h.value and np.array_equal(va.array(), a)
    va.destroy()
    vb.destroy()
    assert va.h is None


@pytest.mark.parametrize("name", ["petsc", "petsc_real"])
def test_comm_destroy_leaves_the_builtin_communicators(name):
    M = module(name)
    for h in (M.PETSC_COMM_SELF, M.PETSC_COMM_WORLD):
        M.Comm(h).destroy()
    c = M.Comm(M.PETSC_COMM_SELF)
    assert (c.size, c.rank) == (1, 0)
    v = M.Vec.mpi(7, comm=M.PETSC_COMM_SELF).set_array(np.arange(7.0))
    assert v.ownership_range() == (0, 7)
    v.destroy()


@pytest.mark.parametrize("bc", ["wall", "periodic"])
def test_operator_of_both_bindings_acts_alike(bc):
    from circulantpreconditioner_amd import diffusion as dif
    dims = (4, 3, 2)
    h, dt, a, nu = (0.25, 0.5, 0.2), 0.07, (1.0, 0.5, 2.0), 0.3
    n = int(np.prod(dims))
    u = np.random.default_rng(2).normal(size=n)
    out = {}
    for real in (False, True):
        A = dif.operator(dims, h, dt, a, nu, bc, real=real)
        M = module("petsc_real" if real else "petsc")
        assert isinstance(A, M.Mat)
        x, y = M.Vec.seq(n).set_array(u), M.Vec.seq(n)
        out[real] = A.mult(x, y).array()
        for o in (x, y, A):
            o.destroy()
    assert out[True].dtype == np.float64 and out[False].dtype == np.complex128
    assert np.abs(out[False].imag).max() == 0
    assert np.abs(out[False].real - out[True]).max() <= 1e-15 * np.abs(out[True]).max()


def test_both_modules_export_the_same_names():
    """petsc_real.py is petsc.py bound to the other library: every public name of the complex
    module but the complex scalar type and the wave context (wave_system.h is complex only)."""
    P, R = module("petsc"), module("petsc_real")
    public = {k for k in vars(P) if not k.startswith("_") and k not in ("annotations", "B")}
    assert public - set(vars(R)) == {"PetscScalar", "FFTPrecWaveContext"}
    assert P.B is not R.B and P.Vec is not R.Vec and P.PetscError is R.PetscError
    for M in (P, R):
        assert M.Vec.B is M.B and M.FFTPrecDiffusionContext is M.B.structs.FFTPrecDiffusionContext


def test_library_path_is_read_at_the_first_load(tmp_path, monkeypatch):
    """A tool that sets _lib.LIB_PATH before anything is loaded gets that build (tools/ab_*.py)."""
    from circulantpreconditioner_amd import _lib
    real_path = _lib.LIB_PATH
    other = str(tmp_path / "libcirculant_fft.so")
    monkeypatch.setattr(_lib.lib, "_lib", None)  # as before the first load
    monkeypatch.setattr(_lib, "LIB_PATH", other)
    with pytest.raises(ImportError, match="libcirculant_fft.so not found at " + other):
        _lib.lib()
    os.symlink(real_path, other)
    assert _lib.lib()._name == other


@pytest.mark.parametrize("name", ["petsc", "petsc_real"])
def test_wrapping_handles_by_hand(name):
    """A bare Vec(handle) borrows (the handles wrapped by hand belong to a context), a wrapper is
    accepted where a handle is, and the PCSHELL registration names what it supports."""
    M = module(name)
    v = M.Vec.seq(5).set_array(np.arange(5.0))
    w = M.Vec(ctypes.c_void_p(v.h.value))
    assert v.owned and not w.owned
    del w
    gc.collect()
    assert np.array_equal(v.array().real, np.arange(5.0))
    assert np.array_equal(M.Vec.borrow(v).array(), v.array())
    v.destroy()
    with pytest.raises(TypeError, match="FFTPrecTransportContext"):
        M.PC.shell(ctypes.c_double(1.0))
    from circulantpreconditioner_amd._lib_ext import FFTPrecWaveContext
    with pytest.raises(TypeError, match="upwind=True"):
        M.PC.shell(FFTPrecWaveContext(), upwind=True)


def test_real_helpers_take_a_mat_or_its_handle():
    from circulantpreconditioner_amd import diffusion as dif
    R = module("petsc_real")
    n, u = 24, np.arange(24.0)
    A = dif.operator((4, 3, 2), (0.25, 0.5, 0.2), 0.07, (1.0, 0.5, 2.0), 0.3, "wall", real=True)
    x, y, z = R.Vec.seq(n).set_array(u), R.Vec.seq(n), R.Vec.seq(n)
    assert np.array_equal(R.mat_mult(A, x, y).array(), R.mat_mult(A.h, x, z).array())
    R.mat_destroy(A)
    assert not A.h.value
    for v in (x, y, z):
        v.destroy()


def test_comm_without_a_handle_is_the_default_process_group(tmp_path):
    import torch.distributed as dist
    R = module("petsc_real")
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        c = R.Comm()
        assert c.handle >= 2 and (c.size, c.rank) == (1, 0) and c.handle in R.B.comm_callbacks
        h = c.handle
        c.destroy()
        assert h not in R.B.comm_callbacks and c.handle == R.PETSC_COMM_SELF
    finally:
        dist.destroy_process_group()
