"""The generated stencils of tests/stencil_cases.py against three things that do not share their code
(no GPU): the scipy product of the CSR assembled from the description equals the int64 reference
exactly; row_class_form of that CSR gives back the offsets, x_local and every row's (mask,
coefficients); and the stand-in AIJ describes the matrix as the row-class form the case expects --
what PetscMiniMatAIJGetDia will hand the PCSHELL.  At 8 x 4 x 2 (rows of 8) and at 256 x 2 x 1 (the
row length of the fused kernels)."""
import numpy as np
import pytest

import stencil_cases as S
from circulantpreconditioner_amd.plan import row_class_form

GRIDS = [(8, 4, 2), (256, 2, 1)]


@pytest.fixture(scope="module")
def P():
    from circulantpreconditioner_amd import petsc
    petsc.lib()
    return petsc


def test_every_named_case_is_there():
    want = {"up_pos", "up_neg", "centered", "diag_only", "diag16", "no_diag", "lower_only", "upper_only", "edges",
            "per_point16", "complex_coef", "stored_zero", "cls17", "wide", "y_coupled"}
    assert set(S.NAMES) == want and len(S.NAMES) == len(want)
    fused = {n: S.make(n, (256, 2, 1)).fused for n in S.NAMES}
    assert {n for n, f in fused.items() if f} == set(S.FUSED)
    assert {n for n in S.NAMES if S.make(n, (256, 2, 1)).by_x} == set(S.BY_X)


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", S.NAMES)
def test_product_is_the_int64_reference(name, dims):
    c = S.make(name, dims)
    br, bi = S.integer_vector(c.n)
    yr, yi = c.reference_numpy(br, bi)
    A = c.scipy()
    y = A @ (br + 1j * bi)
    assert np.array_equal(y.real, yr) and np.array_equal(y.imag, yi)
    assert np.abs(y).max() > 0
    if name == "complex_coef":
        t = c.tab[c.tab != 0]
        assert np.all(t.real != 0) and np.all(t.imag != 0) and np.all(np.abs(t.real) != np.abs(t.imag))
    if name == "stored_zero":
        assert np.count_nonzero(A.data == 0) > 0 and A.nnz == len(c.csr()[2])
    if name in ("no_diag", "lower_only", "upper_only"):
        assert 0 not in c.offsets and not np.any(A.diagonal())


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", S.NAMES)
def test_row_class_form_gives_the_description_back(name, dims):
    c = S.make(name, dims)
    indptr, indices, data = c.csr()
    cls, mask, tab, offs, xl = row_class_form(indptr, indices, data, c.nx)
    assert [int(o) for o in offs] == c.offsets
    assert xl == c.x_local
    assert len(mask) == c.ncls  # up to the numbering of the classes:
    assert np.array_equal(mask[cls], c.mask[c.cls])
    assert np.array_equal(tab[cls], c.tab[c.cls])
    if dims[0] >= 256 and name in S.FULL_NCLS:
        assert c.ncls == S.FULL_NCLS[name]


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", S.NAMES)
def test_aij_describes_the_expected_form(P, name, dims):
    c = S.make(name, dims)
    indptr, indices, data = c.csr()
    M = P.Mat.aij(indptr, indices, data, (c.n, c.n))
    info = M.aij_info()
    want = c.expect_info()
    assert {k: info[k] for k in want} == want, f"{name}: {info}"
    assert M.aij_format() == "none"  # describing uploads nothing
    M.destroy()
