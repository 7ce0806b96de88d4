"""The device form the stand-in AIJ picks for a matrix (PetscMiniMatAIJDescribe, host only): every
generated case of tests/aij_cases.py lands in the form it aims at, a block table never asks for
more LDS than the launcher grants, and the host-Vec MatMult -- the second reference of the GPU
tests -- agrees with the scipy / np.longdouble product.  No GPU is used."""
import os
import re

import numpy as np
import pytest

import aij_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _free_temporaries():
    yield
    C.build_of("real").free_tmp()


def _check_info(b, M, case):
    info = b.info(M)
    if case.expect is not None:
        got = {k: info[k] for k in case.expect}
        assert got == case.expect, f"{case.name}: {info}"
    if info["format"] == "bdia":
        assert 0 < info["lds_bytes"] <= C.LDS_LIMIT, f"{case.name}: {info}"
        kind = "real" if b.real else "ccx"
        assert info["lds_bytes"] == C.lds_bytes(kind, info["B"], info["nblk"])
        assert 2 <= info["B"] <= 4 and 1 <= info["nd"] <= 16 and 1 <= info["ncls"] <= 256
    elif info["format"] == "dia":
        assert 1 <= info["nd"] <= 8 and 1 <= info["ncls"] <= 256 and info["B"] == 1
        assert info["lds_bytes"] == (8 if b.real else 16) * info["ncls"] * info["nd"] + 256
    else:
        assert info["lds_bytes"] == 0
    return info


def test_lds_limit_is_the_header_s():
    txt = open(os.path.join(ROOT, "circulantpreconditioner_amd", "csrc", "cfp_blas.h")).read()
    assert re.search(r"#define BDIA_LDS_MAX \(60 \* 1024\)", txt)
    assert re.search(r"#define BDIA_LDS_LIMIT \(BDIA_LDS_MAX \+ 2048\)", txt)
    # the table of the issue: what the launcher accepts
    assert [C.lds_boundary_nblk(k, B) for k, B in (("ccx", 2), ("ccx", 3), ("real", 2), ("real", 3), ("real", 4))] \
        == [918, 422, 1735, 821, 473]


@pytest.mark.parametrize("data", C.DATA)
@pytest.mark.parametrize("kind", C.KINDS)
def test_small_cases_land_in_their_form_and_host_product(kind, data):
    b = C.build_of(kind)
    seen = set()
    for case in C.small_cases(kind, data):
        M = b.mat(case.A)
        info = _check_info(b, M, case)
        seen.add((info["format"], info["B"], min(info["nd"], 9)))
        assert b.fmt(M) == "none"  # describing uploads nothing
        draw = C.Draw(case.name + "/x", kind, data)
        x = draw.vector(case.A.shape[1])
        ref, bound = C.reference(case.A, x, data)
        xv, yv = b.vec(x, hip=False), b.vec(np.zeros(case.A.shape[0]), hip=False)
        C.check_product(b.mult(M, xv, yv), ref, bound, f"{case.name} host")
        if case.shiftable:
            a = draw.shift()
            b.shift(M, a)
            ref, bound = C.reference(C.shifted(case.A, a), x, data)
            C.check_product(b.mult(M, xv, yv), ref, bound, f"{case.name} host, shifted")
            assert b.info(M)["format"] == info["format"]
        b.destroy(M)
    # every kernel variant has a case: dia, CSR, each block size with nd <= 8 and nd > 8
    for want in [("dia", 1, n) for n in (1, 3, 8)] + [("csr", 0, 0)] + \
            [("bdia", B, n) for B in (2, 3, 4) for n in (1, 8, 9)]:
        assert want in seen, (want, sorted(seen))


@pytest.mark.parametrize("kind,B", [("ccx", 2), ("ccx", 3), ("cre", 2), ("real", 4), ("real", 3)])
def test_lds_boundary(kind, B):
    """The largest table the shared formula admits is stored in the block form and fits the
    launcher's limit; one block more is not stored at that block size (before the builder and the
    launcher shared the formula it was, and no MatMult could run on it)."""
    b = C.build_of(kind)
    fits, over = C.lds_cases(kind, "exact", B)
    M = b.mat(fits.A)
    info = _check_info(b, M, fits)
    assert info["lds_bytes"] <= C.LDS_LIMIT < info["lds_bytes"] + C.lds_bytes(kind, B, 1) - 1024
    b.destroy(M)
    M = b.mat(over.A)
    info = _check_info(b, M, over)
    assert not (info["format"] == "bdia" and info["B"] == B), info
    b.destroy(M)


@pytest.mark.parametrize("which", C.LARGE)
def test_large_cases_land_in_their_form(which):
    kind, case = C.large_case(which, "exact")
    b = C.build_of(kind)
    M = b.mat(case.A)
    _check_info(b, M, case)
    b.destroy(M)
