"""The z ratio of the transport symbol (cfp_transport_z_ratio, host only): the quantity that
decides whether the 256^3 middle kernel may solve z by recurrence (k_tp_mid_rec)."""
import ctypes

import numpy as np
import pytest

ZREC_MAX = 1.0 - 2.0 ** -13  # eligible iff amax <= this (cfp_plan.hip kZrecMaxRatio)

# (lambda, expected amax or None, eligible)
CASES = [
    ((0.6, 0.15, 0.02), None, True),
    ((0.6, 0.15, 333.3), 0.9970, True),
    ((0.3 + 0.2j, 1.1, 0.7 - 0.4j), None, True),
    ((55.6, 0, 0), 0.0, True),
    ((0.6, 0.15, -0.6), 1.5, False),
]


def z_ratio(n, lam):
    from circulantpreconditioner_amd._lib import check, lib
    l6 = (ctypes.c_double * 6)(*[t for v in lam for t in (complex(v).real, complex(v).imag)])
    out = ctypes.c_double()
    check(lib().cfp_transport_z_ratio(n, n, l6, ctypes.byref(out)))
    return out.value


def z_ratio_numpy(n, lam):
    s = 1.0 - np.exp(-2j * np.pi * np.arange(n) / n)
    den = 1.0 + lam[0] * s[None, :] + lam[1] * s[:, None] + lam[2]
    return float(np.abs(lam[2] / den).max())


@pytest.mark.parametrize("lam,expect,eligible", CASES, ids=["bench", "cfl333", "complex", "xonly", "negz"])
def test_z_ratio_matches_numpy(lam, expect, eligible):
    got, ref = z_ratio(256, lam), z_ratio_numpy(256, lam)
    assert abs(got - ref) <= 1e-14 * max(1.0, ref)
    if expect is not None:
        assert abs(got - expect) < 5e-5
    assert (got <= ZREC_MAX) == eligible


def test_z_ratio_other_sizes_and_errors():
    from circulantpreconditioner_amd._lib import lib
    lam = (0.6, 0.15, 333.3)
    for n in (1, 7, 100):
        assert abs(z_ratio(n, lam) - z_ratio_numpy(n, lam)) <= 1e-14
    # a zero denominator: 1 + lam_z = 0 at kx = ky = 0
    assert z_ratio(8, (0.5, 0.5, -1.0)) == float("inf")
    assert lib().cfp_transport_z_ratio(8, 8, None, None) != 0
