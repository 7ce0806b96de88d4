"""The real-data wave plan and its PCSHELL (include/wave_system_real.h) without a GPU: the names in
both built libraries and in the signature table, the context struct, the supported-grid predicate,
the half-spectrum algorithm the kernels implement (as a numpy model against the oracle's block
solve), the PCSHELL registration in both modules and the refusal on several ranks."""
import ctypes
import os

import numpy as np
import pytest

from oracle import wave as OW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wave_system_real.h")
PETSC_ERR_SUP = 56


def module(name):
    from circulantpreconditioner_amd import petsc, petsc_real
    return {"petsc": petsc, "petsc_real": petsc_real}[name]


def test_every_name_of_the_header_is_in_both_libraries_and_in_the_table():
    from circulantpreconditioner_amd import _lib, _lib_ext as ext
    declared = _lib._parse_decls(HEADER)
    assert {"cfp_wave_rplan_supported", "cfp_wave_rplan_create", "cfp_wave_rplan_destroy", "cfp_wave_rplan_set_symbol",
            "cfp_wave_rplan_apply", "cfp_wave_rplan_apply_strided", "cfp_wave_rplan_num_passes",
            "setupFFTPrec3DWaveRealData", "applyFFT3DPrecWaveRealData", "destroyFFTPrec3DWaveRealData"} <= set(declared)
    assert set(declared) <= set(_lib.exported_symbols())  # the header is in the library's list
    group = [(where, sig) for g, where, sig in ext.signatures(ctypes.c_double) if g == "wave_system_real.h"]
    assert len(group) == 1 and group[0][0] == ext.BOTH
    assert set(group[0][1]) == set(declared)
    for L in (_lib.lib(), _lib.real_lib()):
        for name, (args, res) in group[0][1].items():
            fn = getattr(L, name)  # AttributeError: the library does not export it
            assert list(fn.argtypes) == args and fn.restype == res, name


def test_context_struct_is_one_layout():
    from circulantpreconditioner_amd import _lib_ext as ext
    P, R = module("petsc"), module("petsc_real")
    assert P.FFTPrecWaveRealContext is R.FFTPrecWaveRealContext is ext.FFTPrecWaveRealContext
    new, old = ext.FFTPrecWaveRealContext, ext.FFTPrecWaveContext
    assert [k for k, _ in new._fields_] == ["n_x", "n_y", "n_z", "kappa_x", "kappa_y", "kappa_z", "c0", "plan", "dim"]
    assert [(k, t) for k, t in new._fields_] == [(k, t) for k, t in old._fields_]
    assert [getattr(new, k).offset for k, _ in new._fields_] == [getattr(old, k).offset for k, _ in old._fields_]
    assert [getattr(new, k).offset for k, _ in new._fields_] == [8 * i for i in range(9)]
    assert ctypes.sizeof(new) == ctypes.sizeof(old) == 72


def rule(nx, ny, nz, dim):
    """include/wave_system_real.h, restated: dim = 3, or dim = 2 with nz = 1; nx even with nx/2 a
    power of two in [16, 512]; ny, nz <= 4096 and not both 1; the last axis with n > 1 (the fused
    pass, a whole column in one workgroup's LDS) at most 1024 long, the complex wave plan's limit."""
    if min(nx, ny, nz) < 1 or not (dim == 3 or (dim == 2 and nz == 1)):
        return False
    if nx not in (32, 64, 128, 256, 512, 1024):
        return False
    if max(ny, nz) > 4096 or ny == nz == 1:
        return False
    return (nz if nz > 1 else ny) <= 1024


def test_supported_agrees_with_the_rule():
    from circulantpreconditioner_amd import _lib
    from circulantpreconditioner_amd import wave as W
    n_ok = 0
    for L in (_lib.lib(), _lib.real_lib()):
        for nx in (0, 1, 16, 31, 32, 33, 48, 64, 100, 128, 256, 512, 1000, 1024, 1025, 2048):
            for ny in (0, 1, 2, 7, 24, 1024, 1025, 4096, 4097):
                for nz in (1, 2, 5, 1024, 1025, 4096, 4097):
                    for dim in (0, 1, 2, 3, 4):
                        got = L.cfp_wave_rplan_supported(nx, ny, nz, dim)
                        assert got == int(rule(nx, ny, nz, dim)), (nx, ny, nz, dim)
                        n_ok += got
    assert n_ok > 0
    S = _lib.lib().cfp_wave_rplan_supported
    # the cases the feature was specified with
    for nx in (31, 33, 16, 48, 2048):
        assert not S(nx, 6, 5, 3)
    for nx in (32, 64, 128, 256, 512, 1024):
        assert S(nx, 6, 5, 3) and S(nx, 24, 1, 2) and S(nx, 1, 5, 3) and S(nx, 5, 1, 3)
    assert not S(64, 1, 1, 1) and not S(64, 8, 1, 1) and not S(64, 8, 8, 1)   # dim = 1
    assert not S(64, 8, 2, 2)                                                   # dim = 2 with nz > 1
    assert not S(64, 1, 1, 3) and not S(64, 1, 1, 2)                            # ny = nz = 1
    assert W.real_plan_supported((32, 6, 5)) and W.real_plan_supported((32, 24), dim=2)
    assert not W.real_plan_supported((48, 6, 5)) and not W.real_plan_supported((32, 24, 2), dim=2)


def half_spectrum_solve(dims, kappa, b, dim):
    """The algorithm of the kernels: rfft along x, fftn over (z, y), the block solve on the half
    spectrum kx <= nx/2, ifftn, irfft."""
    nx, ny, nz = (tuple(dims) + (1, 1))[:3]
    B = np.fft.rfft(np.asarray(b, dtype=np.float64).reshape(nz, ny, nx, dim + 1), axis=2)
    B = np.fft.fftn(B, axes=(0, 1))
    S = OW.block_symbol(dims, kappa, dim=dim)[:, :, :nx // 2 + 1]
    X = np.linalg.solve(S, B[..., None])[..., 0]
    X = np.fft.ifftn(X, axes=(0, 1))
    return np.fft.irfft(X, n=nx, axis=2).reshape(-1)


@pytest.mark.parametrize("dims,dim", [((32, 6, 5), 3), ((64, 20, 12), 3), ((32, 24), 2)],
                         ids=["32x6x5", "64x20x12", "2d-32x24"])
def test_half_spectrum_model_equals_block_solve(dims, dim):
    kappa = (0.079, 0.05, 0.11 if dim == 3 else 0.0)
    b = np.random.default_rng(11).standard_normal((dim + 1) * int(np.prod(dims)))
    ref = OW.block_solve(dims, kappa, b, dim=dim)
    x = half_spectrum_solve(dims, kappa, b, dim)
    nrm = np.linalg.norm(ref)
    print(f"{dims}: model - block_solve {np.linalg.norm(x - ref.real) / nrm:.2e}, "
          f"|Im block_solve| {np.linalg.norm(ref.imag) / nrm:.2e}")
    assert np.linalg.norm(x - ref.real) <= 1e-13 * nrm
    assert np.linalg.norm(ref.imag) <= 1e-13 * nrm  # real b: a real solution
    # S(-k) = conj S(k): what lets the half spectrum carry everything
    S = OW.block_symbol(dims, kappa, dim=dim)
    mirror = S[np.ix_(*[(-np.arange(n)) % n for n in S.shape[:3]])]
    assert np.abs(mirror - S.conj()).max() <= 1e-12 * np.abs(S).max()


@pytest.mark.parametrize("name", ["petsc", "petsc_real"])
def test_shell_resolves_the_three_callbacks(name):
    M = module(name)
    ctx = M.FFTPrecWaveRealContext(32, 6, 5, 0.079, 0.05, 0.11, 700.0, None, 3)
    pc = M.PC.shell(ctx)
    assert pc.ctx is ctx
    for fn in ("setupFFTPrec3DWaveRealData", "applyFFT3DPrecWaveRealData", "destroyFFTPrec3DWaveRealData"):
        assert M.fn(fn)
    got = ctypes.c_void_p()
    M.PetscCall(M.lib().PCShellGetContext(pc.h, ctypes.byref(got)))
    assert got.value == ctypes.addressof(ctx)
    with pytest.raises(TypeError, match="upwind=True"):
        M.PC.shell(M.FFTPrecWaveRealContext(), upwind=True)
    pc.destroy()  # never set up: the destroy callback finds no plan
    assert not ctx.plan


@pytest.mark.parametrize("name", ["petsc", "petsc_real"])
def test_setup_on_several_ranks_is_refused(name):
    """PETSC_COMM_WORLD of two ranks: PETSC_ERR_SUP from setup, before any device call (the
    communicator's collectives are never used)."""
    M = module(name)
    ops = M.Comm._Ops(M.Comm._A2A(lambda *a: 1), M.Comm._RED(lambda *a: 1), None)
    h = ctypes.c_int()
    M.PetscCall(M.lib().PetscMiniCommCreate(2, 0, ctypes.byref(ops), ctypes.byref(h)))
    comm = M.Comm(h.value)
    assert comm.size == 2
    comm.set_world()
    try:
        ctx = M.FFTPrecWaveRealContext(32, 6, 5, 0.079, 0.05, 0.11, 700.0, None, 3)
        pc = M.PC.shell(ctx)
        with pytest.raises(M.PetscError, match="one rank") as e:
            pc.setup()
        assert e.value.code == PETSC_ERR_SUP and not ctx.plan
        pc.destroy()
    finally:
        M.set_comm_world(M.PETSC_COMM_SELF)
        comm.destroy()
