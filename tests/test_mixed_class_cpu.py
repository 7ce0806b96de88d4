"""The geometry of the LDS mixed-radix pass (cfp_mixed_pass_class: the host arithmetic the launch
of k_axis_mixed itself uses, no GPU) against a Python restatement of the rule over every length
1..4096, its boundaries by name, the wave cells, and the class of every length and position that
test_mixed_axis_gpu.py and test_wave.py run -- their coverage claim, checked."""
import ctypes

import pytest

from mixed_cases import ALL_LENGTHS, MAX_LDS, POSITIONS, in_class, rule

NCOLS = (1, 2, 3, 5, 64, 1000)


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    return cp


def test_export_equals_the_restated_rule_everywhere(cp):
    worst = 0
    for n in range(1, 4097):
        for row in (True, False):
            for ncols in NCOLS:
                c = cp.mixed_pass_class(n, ncols, row)
                assert c == rule(n, ncols, row), (n, ncols, row)
                assert c["lds_bytes"] <= MAX_LDS, (n, ncols, row)
                assert 1 <= c["G"] <= min(64, ncols) and (row or c["G"] & (c["G"] - 1) == 0)
                prod = 1
                for r in c["radices"]:
                    prod *= r
                assert prod == n and all(r in (2, 3, 4, 5, 7, 8) or r > 8 for r in c["radices"])
                worst = max(worst, c["lds_bytes"])
    print(f"largest dynamic LDS request: {worst} B")
    assert worst == 2 * 4097 * 16  # 4096 in column mode


@pytest.mark.parametrize("row", [True, False], ids=["row", "col"])
def test_boundaries_by_name(cp, row):
    L = lambda n: n if row else n + 1  # noqa: E731
    c = cp.mixed_pass_class(2047, 3, row)  # 23 . 89: ping-pong by a prime, the table still fits beside two buffers
    assert c["pingpong"] and c["tw_lds"] and c["G"] == 1 and c["radices"] == [23, 89]
    assert c["lds_bytes"] == 2 * L(2047) * 16 + 2047 * 16 <= 96 * 1024
    c = cp.mixed_pass_class(2048, 3, row)  # not a register-table length: 8 . 8 . 8 . 4 in place
    assert not c["pingpong"] and c["tw_lds"] and c["G"] == 1 and c["radices"] == [8, 8, 8, 4]
    assert c["lds_bytes"] == L(2048) * 16 + 2048 * 16
    c = cp.mixed_pass_class(2049, 3, row)  # the first length whose block exceeds 2,048 points
    assert c["pingpong"] and not c["tw_lds"] and c["G"] == 1 and c["radices"] == [3, 683]
    assert c["lds_bytes"] == 2 * L(2049) * 16
    c = cp.mixed_pass_class(4096, 3, row)
    assert c["pingpong"] and not c["tw_lds"] and c["radices"] == [8, 8, 8, 8] and c["U"] == 8
    assert c["lds_bytes"] == (131072 if row else 131104)


def test_loads_in_flight_step_at_512_and_1024_points(cp):
    for n, ncols, row, pts, U in [(512, 1, True, 512, 2), (513, 1, True, 513, 4), (1024, 1, True, 1024, 4),
                                  (1025, 1, True, 1025, 8), (128, 4, False, 512, 2), (129, 4, False, 516, 4),
                                  (256, 5, False, 1024, 4), (257, 5, False, 1028, 8), (171, 3, True, 513, 4),
                                  (2, 1000, False, 128, 2), (2, 1000, True, 128, 2), (16, 1000, False, 1024, 4),
                                  (17, 1000, True, 1088, 8)]:
        c = cp.mixed_pass_class(n, ncols, row)
        assert (c["G"] * n, c["U"]) == (pts, U), (n, ncols, row, c)


@pytest.mark.parametrize("nc", [2, 3, 4])
def test_wave_cells_are_whole_and_fit(cp, nc):
    for n in range(1, 1025):
        for row in (True, False):
            for k in NCOLS:
                c = cp.mixed_pass_class(n, nc * k, row, nc)
                assert c == rule(n, nc * k, row, nc), (n, nc * k, row)
                G = c["G"]
                assert G % nc == 0 and c["lds_bytes"] <= MAX_LDS, (n, nc * k, row, c)
                if nc == 3:
                    q = G // 3
                    assert q >= 1 and q & (q - 1) == 0, (n, k, row, G)  # 3 . 2^j: the magic-number split
                # two buffers always: the solve writes the second one
                assert c["lds_bytes"] >= 2 * G * n * 16


def test_refused_shapes_return_the_launch_error(cp):
    for args in [(0, 1, True, 0), (4097, 1, True, 0), (8, 6, False, 5), (8, 7, False, 2), (8, 6, False, 1),
                 (4096, 4, False, 4)]:  # the last: 2 buffers of 4 columns of 4,097 points, 524 KB of LDS
        assert rule(*args) is None
        with pytest.raises(cp.CirculantError) as e:
            cp.mixed_pass_class(*args)
        assert e.value.code == 76, args  # CFP_ERR_LIB, as the apply reports a refused launch
    with pytest.raises(cp.CirculantError) as e:
        cp.mixed_pass_class(8, 0, True)
    assert e.value.code == 63  # CFP_ERR_ARG_OUTOFRANGE
    L = cp.lib()
    i, q = ctypes.c_int(), ctypes.c_int64()
    rad = (ctypes.c_int * 24)()
    assert L.cfp_mixed_pass_class(8, 1, 1, 0, None, i, i, i, q, i, rad) == 85  # CFP_ERR_ARG_NULL
    assert L.cfp_mixed_pass_class(8, 1, 1, 0, i, i, i, i, q, i, None) == 85


def test_both_libraries_report_the_same(cp):
    from circulantpreconditioner_amd import _lib
    R = _lib.real_lib()
    for n, ncols, row, nc in [(4096, 3, 0, 0), (1001, 5, 0, 0), (1000, 8, 0, 4), (143, 1, 1, 0)]:
        G, pp, tw, U, nst = (ctypes.c_int() for _ in range(5))
        lds, rad = ctypes.c_int64(), (ctypes.c_int * 24)()
        assert R.cfp_mixed_pass_class(n, ncols, row, nc, G, pp, tw, U, lds, nst, rad) == 0
        c = cp.mixed_pass_class(n, ncols, bool(row), nc)
        assert c == {"G": G.value, "pingpong": bool(pp.value), "tw_lds": bool(tw.value), "U": U.value,
                     "lds_bytes": lds.value, "radices": list(rad[:nst.value])}
        assert all(v == 0 for v in rad[nst.value:])


@pytest.mark.parametrize("pos", POSITIONS, ids=lambda p: p[0])
def test_every_gpu_length_lands_in_its_class(cp, pos):
    name, grid, axis, modes, ncols, row = pos
    for cls, n in ALL_LENGTHS:
        g = grid(n)
        assert g["xyz".index(axis)] == n and g[0] * g[1] * g[2] // n == ncols and g[0] * g[1] * g[2] <= 24576
        assert row == (axis == "x")
        c = cp.mixed_pass_class(n, ncols, row)
        assert in_class(cls, n, c), (name, cls, n, c)


def test_gpu_lengths_reach_every_stage_and_block_shape(cp):
    """What the list is for: every specialised radix runs in place and out of place, a direct-sum
    stage runs behind each of them, twice and three times in a row, and blocks of G > 1 columns
    end in a partial one."""
    inplace, pingpong, before_prime, primes_in_a_row, partial = set(), set(), set(), 0, 0
    for cls, n in ALL_LENGTHS:
        for name, grid, axis, modes, ncols, row in POSITIONS:
            c = cp.mixed_pass_class(n, ncols, row)
            (pingpong if c["pingpong"] else inplace).update(r for r in c["radices"] if r <= 8)
            big = [i for i, r in enumerate(c["radices"]) if r > 8]
            if big and big[0] > 0:
                before_prime.add(c["radices"][big[0] - 1])
            primes_in_a_row = max(primes_in_a_row, len(big))
            partial += c["G"] > 1 and ncols % c["G"] != 0
    assert inplace == {2, 3, 4, 5, 7, 8}
    assert pingpong == {2, 3, 4, 5, 7, 8}
    assert before_prime >= {2, 3, 4, 5, 7, 8}
    assert primes_in_a_row == 3 and partial > 50


WAVE_CASES = [  # (dim, dims, class of the fused pass): test_wave.py's mixed-pass cases
    (3, (6, 5, 22), "pingpong_prime"), (3, (22, 6, 5), "inplace"), (3, (5, 22, 6), "inplace"),
    (3, (4, 13, 3), "inplace"), (3, (2, 1, 1000), "pingpong_size"),
    # (33, 10): y = 10 is a register-pass length, which 2-D cells (3 columns each) do not get
    (2, (10, 33), "pingpong_prime"), (2, (33, 10), "refused"), (2, (3, 1000), "pingpong_size"),
    (1, (143,), "pingpong_prime"), (1, (1001,), "pingpong_prime"),
]


def wave_fused_pass(dim, dims):
    """(n, ncols) of a wave plan's fused pass: the last axis longer than 1, dim + 1 columns per cell
    (always column mode: the components are interleaved)."""
    d3 = tuple(dims) + (1,) * (3 - len(dims))
    axis = max([a for a in range(3) if d3[a] > 1], default=0)
    return d3[axis], (dim + 1) * d3[0] * d3[1] * d3[2] // d3[axis]


@pytest.mark.parametrize("dim,dims,cls", WAVE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_wave_cases_land_in_their_class(cp, dim, dims, cls):
    n, ncols = wave_fused_pass(dim, dims)
    c = cp.mixed_pass_class(n, ncols, False, dim + 1)
    assert c["G"] % (dim + 1) == 0
    assert in_class(cls, n, c), c
    if dims == (2, 1, 1000):
        assert c["G"] == 4 and c["lds_bytes"] == 128128
    if dims == (3, 1000):
        assert c["G"] == 3 and c["lds_bytes"] == 96096
    if dims == (1001,):
        assert c["G"] == 2 and c["lds_bytes"] == 80144
