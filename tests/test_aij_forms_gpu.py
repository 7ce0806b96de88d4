"""Device MatMult of the stand-in AIJ in each of its storage forms (k_dia_spmv, k_bdia_spmv,
k_bdia4_spmv, the CSR kernels; csrc/cfp_blas.hip), complex and real-scalar builds, against exact
references: tests/aij_cases.py builds one matrix per form / variant, each asserted through
aij_info() to be stored as intended.

Two data sets per case.  Exact: small (Gaussian) integers, so the device product must equal the
scipy product bit for bit in any summation order -- a wrong index, mask or tail cannot hide.
Rounded: standard normals against np.longdouble with the any-order summation bound per row,
|y_r - ref_r| <= 4 (nnz_r + 2) 2^-53 (|A| |x|)_r.  The device product is also held to the host-Vec
MatMult of the same Mat, and the products are repeated after MatShift."""
import numpy as np
import pytest

import aij_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0  # y before the product: a row the kernel does not write shows


@pytest.fixture(autouse=True)
def _free_temporaries():
    yield
    C.build_of("real").free_tmp()


def _products(b, case, kind, data, errors):
    """Device and host products of one case, before and after MatShift; failures go to errors."""
    M = b.mat(case.A)
    try:
        info = b.info(M)
        if case.expect is not None:
            got = {k: info[k] for k in case.expect}
            assert got == case.expect, f"stored as {info}, wanted {case.expect}"
        m, n = case.A.shape
        draw = C.Draw(case.name + "/x", kind, data)
        x = draw.vector(n)
        xd, xh = b.vec(x), b.vec(x, hip=False)
        yd, yh = b.vec(np.full(m, SENTINEL)), b.vec(np.full(m, SENTINEL), hip=False)
        A = case.A
        for step in ("", " after MatShift"):
            if step:
                if not case.shiftable:
                    break
                a = draw.shift()
                b.shift(M, a)
                # the class forms are rebuilt at the next product; CSR values follow in place
                assert b.fmt(M) == ("csr" if info["format"] == "csr" else "none"), b.fmt(M)
                A = C.shifted(case.A, a)
                yd.set_array(np.full(m, SENTINEL))
            ref, bound = C.reference(A, x, data)
            y = b.mult(M, xd, yd)
            assert b.fmt(M) == info["format"], f"uploaded as {b.fmt(M)}, described as {info['format']}"
            C.check_product(y, ref, bound, "device vs reference" + step)
            C.check_product(y, b.mult(M, xh, yh).astype(ref.dtype), bound, "device vs host MatMult" + step)
    except (AssertionError, b.mod.PetscError) as e:  # a MatMult that returns an error is a finding too
        errors.append(f"{case.name} [{kind}, {data}]: {e}")
    finally:
        b.destroy(M)


@pytest.mark.parametrize("data", C.DATA)
@pytest.mark.parametrize("kind", C.KINDS)
def test_every_form_matches_the_reference(kind, data):
    b = C.build_of(kind)
    errors = []
    for case in C.small_cases(kind, data):
        _products(b, case, kind, data, errors)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("kind,B", [("ccx", 2), ("ccx", 3), ("real", 4)])
def test_lds_boundary_products(kind, B):
    """The largest block table the launcher's LDS limit admits, and one block more (which is
    stored otherwise).  While the builder admitted any table of up to 60 KiB of values, the
    matrices one block over the launcher's limit (919 complex 2 x 2 blocks, 423 complex 3 x 3,
    474 real 4 x 4) were stored in the block form and every device MatMult on them returned
    error 76, "aij_spmv_dev: invalid argument" (hipErrorInvalidValue; seen on an MI355X)."""
    b = C.build_of(kind)
    errors = []
    for data in C.DATA:
        for case in C.lds_cases(kind, data, B):
            _products(b, case, kind, data, errors)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("data", C.DATA)
@pytest.mark.parametrize("which", C.LARGE)
def test_grid_stride_loops(which, data):
    """One large matrix per kernel: more rows than the capped grid has threads, twice over for the
    block forms, so the grid-stride loops and the class-byte prefetch of k_bdia_spmv run."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kind, case = C.large_case(which, data, cus)
    m = case.A.shape[0]
    if which in ("dia", "csr_l1"):
        assert m > C.L1_GRID + 512
    else:
        B = case.expect["B"]
        # k_bdia_spmv: one thread per block row; k_bdia4_spmv (B = 4): one per row
        assert (m if B == 4 else m // B) > 2 * 3 * cus * 512
    errors = []
    _products(C.build_of(kind), case, kind, data, errors)
    assert not errors, "\n".join(errors)
