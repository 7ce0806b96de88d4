"""Which middle kernel a symbol gets at 256^3 (cfp_symbol_z_route, host only: the rule the three plan
flavours share, csrc/cfp_symbol.cpp decide_z_route) against the same rule restated here on the
library's own z ratios and the two caps:

    upwind setter, Re lam_z < 0, mu_z == 0:  'zrecb' if max |b| of the mapped pair <= 1 - 2^-13, else 'fft'
    (mapped) mu_z == 0:                      'zrec'  if the transport ratio     <= 1 - 2^-13, else 'fft'
    (mapped) mu_z != 0:                      'zrec2' if max |a| and max |b|     <= 1 - 2^-7,  else 'fft'
    any grid but 256^3:                      'fft'

The symbols are the ones tests/test_upwind_gpu.py routes on live plans (LAMB, LAMC, MU_Z, `over`),
plus every sign pattern of upwind_cases.SIGNS with mu = 0 and with mu_z != 0."""
import ctypes

import numpy as np
import pytest

from upwind_cases import LAM0, MUS, SIGNS, signed

N3 = (256, 256, 256)
CAP1, CAP2 = 1 - 2.0 ** -13, 1 - 2.0 ** -7
LAMB = (0.6, 0.15, -0.6)
LAMC = (55.6, 0, -1e3 / 3)  # the reference driver's cfl against z
MU_Z = (0.2, 0.2, 2.5)
OVER = (0.0, 0.0, -1e4)
ZERO = (0, 0, 0)

# (lam, mu, upwind) -> the kernel tests/test_upwind_gpu.py::test_routing_table sees on a live plan
ROUTED = [(LAMB, ZERO, True, "zrecb"), (LAMC, ZERO, True, "zrecb"), (OVER, ZERO, True, "fft"),
          (LAMB, MU_Z, True, "zrec2"), (LAMC, (0, 0, 1e-3), True, "fft"),
          ((-0.6, -0.15, 0.6), ZERO, True, "zrec"), ((-0.6, -0.15, 0.0), ZERO, True, "zrec"),
          (LAM0, ZERO, False, "zrec"), (LAM0, MU_Z, False, "zrec2")]


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    return cp


def transport_ratio(lam):
    from circulantpreconditioner_amd._lib import check, lib
    l6 = (ctypes.c_double * 6)(*[c for v in lam for c in (complex(v).real, complex(v).imag)])
    out = ctypes.c_double()
    check(lib().cfp_transport_z_ratio(256, 256, l6, ctypes.byref(out)))
    return out.value


def rule(cp, dims, lam, mu, upwind):
    """(kind, ratios) by the docstring's rule"""
    l2, m2 = cp.upwind_to_advdiff(lam, mu) if upwind else (lam, mu)
    ra, rb = cp.advdiff_z_ratio(dims[0], dims[1], l2, m2)
    if upwind and complex(lam[2]).real < 0 and complex(mu[2]) == 0:
        kind = "zrecb" if rb <= CAP1 else "fft"
    elif complex(m2[2]) == 0:
        # mu_z == 0: max |a| is the transport ratio (beta = d); where x and y carry no mu either,
        # cfp_transport_z_ratio computes it from the transport setter's tables
        if all(complex(m) == 0 for m in m2) and tuple(dims[:2]) == (256, 256):
            assert ra == transport_ratio(l2)
        kind = "zrec" if ra <= CAP1 else "fft"
    else:
        kind = "zrec2" if ra <= CAP2 and rb <= CAP2 else "fft"
    return (kind if tuple(dims) == N3 else "fft"), (ra, rb)


@pytest.mark.parametrize("lam,mu,upwind,want", ROUTED)
def test_the_symbols_the_gpu_test_routes(cp, lam, mu, upwind, want):
    kind, ratios = cp.z_route(N3, lam, mu, upwind=upwind)
    assert (kind, ratios) == rule(cp, N3, lam, mu, upwind)
    assert kind == want


def test_every_kernel_is_reached():
    assert {w for *_, w in ROUTED} == {"fft", "zrec", "zrec2", "zrecb"}


@pytest.mark.parametrize("upwind", [False, True])
@pytest.mark.parametrize("mu", list(MUS))
@pytest.mark.parametrize("signs", SIGNS, ids=lambda s: "".join("+" if v > 0 else "-" for v in s))
def test_every_sign_pattern(cp, signs, mu, upwind):
    lam = signed(signs)
    got = cp.z_route(N3, lam, MUS[mu], upwind=upwind)
    assert got == rule(cp, N3, lam, MUS[mu], upwind)
    if upwind:  # LAM0's ratios are far under the caps: the kernel follows the z sign and mu_z alone
        assert got[0] == ("zrec2" if mu == "mu" else ("zrecb" if signs[2] < 0 else "zrec"))


def test_reference_driver_cfl_is_the_backward_kernel_and_not_the_two_sided_one(cp):
    """the two facts of test_upwind_cpu.py's last test, as routes"""
    kind, (ra, rb) = cp.z_route(N3, LAMC, upwind=True)
    assert kind == "zrecb" and ra == 0.0 and CAP2 < rb <= CAP1
    # the same numbers through the advdiff setter: over the two-sided cap, so the FFT kernel
    assert cp.z_route(N3, *cp.upwind_to_advdiff(LAMC))[0] == "fft"
    assert cp.z_route(N3, *cp.upwind_to_advdiff(LAMB))[0] == "zrec2"  # never 'zrecb' without the upwind setter


@pytest.mark.parametrize("dims", [(128, 128, 128), (256, 256, 128)])
@pytest.mark.parametrize("lam,mu,upwind,_", ROUTED)
def test_other_grids_take_the_fft_kernel(cp, dims, lam, mu, upwind, _):
    kind, ratios = cp.z_route(dims, lam, mu, upwind=upwind)
    assert kind == "fft"
    assert ratios == rule(cp, dims, lam, mu, upwind)[1]


@pytest.mark.parametrize("mu", [ZERO, MU_Z, (0.2, 0.0, 0.0)])
@pytest.mark.parametrize("lam", [LAM0, (0.6, 0.15, 0.0), (0.0, 0.15 + 0.3j, 0.4 - 1j)])
def test_upwind_without_a_negative_axis_is_the_advdiff_route(cp, lam, mu):
    assert cp.z_route(N3, lam, mu, upwind=True) == cp.z_route(N3, lam, mu, upwind=False)


def test_bad_arguments_return_the_error_codes():
    from circulantpreconditioner_amd._lib import lib
    L = lib()
    six = (ctypes.c_double * 6)(0.6, 0, 0.15, 0, 0.4, 0)
    k, r = ctypes.c_int(), (ctypes.c_double * 2)()
    assert L.cfp_symbol_z_route(256, 256, 256, six, six, 0, ctypes.byref(k), r) == 0
    for args in ((None, six, 0, ctypes.byref(k), r), (six, None, 0, ctypes.byref(k), r),
                 (six, six, 0, None, r), (six, six, 0, ctypes.byref(k), None)):
        assert L.cfp_symbol_z_route(256, 256, 256, *args) == 85  # CFP_ERR_ARG_NULL
    for dims in ((0, 256, 256), (256, 0, 256), (256, 256, -1)):
        assert L.cfp_symbol_z_route(*dims, six, six, 0, ctypes.byref(k), r) == 63  # CFP_ERR_ARG_OUTOFRANGE


@pytest.mark.parametrize("P", [2, 4])
def test_slab_tables_of_the_ranks_are_the_one_rank_table_cut_by_rows(P):
    """One table function serves every rank count: rank r's units are units [r, r + 1) 1024 / P of
    the one-rank table (its 32 / P rows of 32 x tiles), byte for byte."""
    from circulantpreconditioner_amd.distributed import slab_advdiff_z_table
    lam, mu = (0.6, 0.15 + 0.05j, 0.4), (0.2, 0.2, 2.5 - 0.1j)
    whole = slab_advdiff_z_table(1, 0, lam, mu)
    parts = np.concatenate([slab_advdiff_z_table(P, r, lam, mu) for r in range(P)])
    assert whole.shape == parts.shape == (1024, 3, 64)
    assert whole.tobytes() == parts.tobytes()
