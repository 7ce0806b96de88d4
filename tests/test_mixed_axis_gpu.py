"""The LDS mixed-radix axis pass (k_axis_mixed) over every class of its dispatch table: in-place
and ping-pong stages, each specialised radix and the direct-sum prime stage behind each of them,
the twiddle table in LDS and in global memory, 2 / 4 / 8 loads in flight, whole and partial
blocks, dynamic LDS from 128 B to 131 KB -- each length of mixed_cases.LENGTHS on each axis
position of mixed_cases.POSITIONS (the smallest grid that puts it there; at most 24,576 points).

Every case asserts its route (the pass under test is not the register pass and its geometry,
cfp_mixed_pass_class, is the class the list names; test_mixed_class_cpu.py proves the same
without a GPU) and its result against the CPU oracle."""
import functools

import numpy as np
import pytest
import torch

from mixed_cases import ALL_LENGTHS, POSITION, POSITIONS, in_class

pytestmark = pytest.mark.gpu
TOL = 1e-10       # the project's tolerance on the preconditioned vector (relative L2, and per point)
TOL_RES = 1e-12   # ||C x - b|| / ||b||, the circulant applied by shifts
TOL_FFT = 1e-13   # forward / backward against the oracle's DFT (test_gpu_parity's)

CASES = [pytest.param(cls, n, pos[0], id=f"{pos[0]}-{n}") for pos in POSITIONS for cls, n in ALL_LENGTHS]
DIAG_CASES = [pytest.param(cls, n, name, id=f"{name}-{n}") for name in ("x_fused", "y_fused_3") for cls, n in ALL_LENGTHS]
FFT_CASES = [pytest.param(cls, n, name, id=f"{name}-{n}") for name in ("x_fused", "y_fused_5", "z_fused")
             for cls, n in ALL_LENGTHS]


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return cp


def _dev(a, device="cuda"):
    return torch.from_numpy(np.array(a, dtype=np.complex128)).to(device)  # a copy: the shared references are read-only


def _lam(grid):
    """A complex lambda per grid, as test_random_grids_vs_oracle draws it."""
    rng = np.random.default_rng(sum(grid) * 7919 + grid[0])
    return tuple(complex(rng.uniform(0.01, 2.0), rng.uniform(-0.5, 0.5)) for _ in range(3))


@functools.lru_cache(maxsize=None)
def _reference(grid):
    """(lam, b, Diag, x = C^-1 b by the oracle) of a grid, computed once and shared (read-only)."""
    from oracle import oracle as O
    N = int(np.prod(grid))
    lam = _lam(grid)
    b = O.c_fill_uniform(N, 1000 + sum(grid))
    d = O.c_build_diag_transport(grid, lam)
    ref = O.c_solve_3d(d, b, grid)
    for a in (b, d, ref):
        a.setflags(write=False)
    return lam, b, d, ref


def _assert_route(cp, plan, cls, n, name, fused_mode="fused_sep"):
    """The passes over the position's axis are the modes it names, of n points and its column
    count, none of them the register pass, and their geometry is the class `cls`."""
    _, grid, axis, modes, ncols, row = POSITION[name]
    ps = [p for p in plan.passes() if p["axis"] == axis]
    want = [fused_mode if m == "fused" else m for m in modes]
    assert [p["mode"] for p in ps] == want, plan.passes()
    for p in ps:
        assert p["n"] == n and p["ncols"] == ncols and not p["fast"], p
    c = cp.mixed_pass_class(n, ncols, row)
    assert in_class(cls, n, c), (cls, n, c)
    return c


def _assert_solution(oracle, x, grid, lam, b, ref, what=""):
    x = x.cpu().numpy()
    rel = float(np.linalg.norm(x - ref) / np.linalg.norm(ref))
    worst = float(np.abs(x - ref).max() / np.abs(ref).max())
    res = float(np.linalg.norm(oracle.c_apply_circulant(x, grid, lam) - b) / np.linalg.norm(b))
    print(f"{what}{grid}: rel L2 {rel:.2e}  max {worst:.2e}  residual {res:.2e}")
    assert np.all(np.isfinite(x))
    assert rel < TOL and worst <= TOL and res < TOL_RES


# ------------------------------------------------------------------ a + b: route, transport symbol
@pytest.mark.parametrize("cls,n,name", CASES)
def test_apply_transport_symbol(cp, oracle, cls, n, name):
    grid = POSITION[name][1](n)
    lam, b, _, ref = _reference(grid)
    with cp.CirculantPlan(grid) as plan:
        plan.set_transport_symbol(lam)
        _assert_route(cp, plan, cls, n, name)
        x = plan.apply(_dev(b))
        _assert_solution(oracle, x, grid, lam, b, ref)
        t = _dev(b)
        plan.apply(t, out=t)  # in place
        assert torch.equal(t, x)


# ------------------------------------------------------------------ c: explicit Diag (PASS_FUSED_DIAG)
@pytest.mark.parametrize("cls,n,name", DIAG_CASES)
def test_apply_with_explicit_diag(cp, oracle, cls, n, name):
    grid = POSITION[name][1](n)
    lam, b, d, ref = _reference(grid)
    with cp.CirculantPlan(grid) as plan:
        dd = _dev(d)
        x = plan.apply_with_diag(dd, _dev(b))  # a caller-owned Diag, no symbol on the plan
        _assert_solution(oracle, x, grid, lam, b, ref, "apply_with_diag ")
        t = _dev(b)
        plan.apply_with_diag(dd, t, out=t)
        assert torch.equal(t, x)
        plan.set_diag(dd)
        _assert_route(cp, plan, cls, n, name, fused_mode="fused_diag")
        assert torch.equal(plan.apply(_dev(b)), x)


# ------------------------------------------------------------------ d: forward / backward
def _impulse_spectrum(n, p, sign):
    """W_n^{p k} (sign -1) or its conjugate, k < n, evaluated in extended precision."""
    pi = 4 * np.arctan(np.longdouble(1))
    ang = 2 * pi * ((p * np.arange(n)) % n).astype(np.longdouble) / np.longdouble(n)
    return np.cos(ang).astype(np.float64) + 1j * sign * np.sin(ang).astype(np.float64)


@pytest.mark.parametrize("cls,n,name", FFT_CASES)
def test_forward_backward(cp, oracle, cls, n, name):
    """Random data against the oracle's DFT, and an impulse at a position p coprime to n on the
    axis under test: its transform is W_n^{+-pk} along that axis and constant along the others,
    every output of modulus 1 -- compared point by point with the extended-precision value."""
    _, gridf, axis, _, ncols, row = POSITION[name]
    grid = gridf(n)
    assert in_class(cls, n, cp.mixed_pass_class(n, ncols, row))
    _, b, _, _ = _reference(grid)
    a = "xyz".index(axis)
    p = next(q for q in range(max(1, n // 3), n + 1) if np.gcd(q, n) == 1)
    imp = np.zeros(grid[::-1], dtype=np.complex128)  # [z, y, x]
    idx = [0, 0, 0]
    idx[2 - a] = p % n
    imp[tuple(idx)] = 1.0
    shape = [1, 1, 1]
    shape[2 - a] = n
    with cp.CirculantPlan(grid) as plan:
        for sign, fn in ((-1, plan.forward), (+1, plan.backward)):
            f = fn(_dev(b)).cpu().numpy()
            want = oracle.c_fft3d(b, grid, sign)
            rel = float(np.linalg.norm(f - want) / np.linalg.norm(want))
            g = fn(_dev(imp.reshape(-1))).cpu().numpy().reshape(imp.shape)
            exact = np.broadcast_to(_impulse_spectrum(n, p, sign).reshape(shape), imp.shape)
            worst = float(np.abs(g - exact).max())
            print(f"{grid} sign {sign:+d}: rel L2 {rel:.2e}  impulse at {p}: max {worst:.2e}")
            assert rel < TOL_FFT and worst <= TOL_FFT


# ------------------------------------------------------------------ e: zero-divisor rule
@pytest.mark.parametrize("cls,n,name", [("pingpong_prime", 143, "y_fused_3"), ("pingpong_size", 3000, "x_fused")])
def test_zero_divisor_rule(cp, oracle, cls, n, name):
    """A Diag with planted zeros (PETSc's VecPointwiseDivide: a zero divisor gives 0), as
    test_gpu_parity's test_zero_divisor_rule, through the ping-pong stages."""
    grid = POSITION[name][1](n)
    N = int(np.prod(grid))
    b = oracle.c_fill_uniform(N, 12)
    d = oracle.c_build_diag_transport(grid, (0.6, 0.15, 0.02))
    d[[0, 3, N - 1]] = 0
    ref = oracle.c_solve_3d(d, b, grid)
    assert np.all(np.isfinite(ref))
    with cp.CirculantPlan(grid) as plan:
        plan.set_diag(_dev(d))
        _assert_route(cp, plan, cls, n, name, fused_mode="fused_diag")
        x = plan.apply(_dev(b))
        assert bool(torch.isfinite(x).all())
        x = x.cpu().numpy()
        assert np.linalg.norm(x - ref) / np.linalg.norm(ref) < TOL
        assert np.abs(x - ref).max() <= TOL * np.abs(ref).max()


# ------------------------------------------------------------------ f: a second device of the process
def test_second_device_gets_the_large_lds_launch(cp, oracle):
    """(3000, 2, 1) asks for 96 KB of dynamic LDS, above the 64 KiB a kernel gets without the
    function attribute.  The attribute belongs to the device's function object: a plan on device 1
    must get it as the one on device 0 did, in the same process."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    grid = (3000, 2, 1)
    c = cp.mixed_pass_class(3000, 2, True)
    assert c["lds_bytes"] == 96000 and c["pingpong"] and not c["tw_lds"]
    lam, b, _, ref = _reference(grid)
    for device in (0, 1):
        with torch.cuda.device(device), cp.CirculantPlan(grid, device=device) as plan:
            plan.set_transport_symbol(lam)
            assert [p["fast"] for p in plan.passes() if p["axis"] == "x"] == [False, False]
            x = plan.apply(_dev(b, f"cuda:{device}"))
            torch.cuda.synchronize(device)
            _assert_solution(oracle, x, grid, lam, b, ref, f"device {device} ")


# ------------------------------------------------------------------ g: graph replay above 64 KiB of LDS
@pytest.mark.parametrize("cls,n,name,lds", [("pingpong_prime", 1001, "y_fused_3", 80144),
                                            ("pingpong_size", 4096, "x_fused", 131072)])
def test_graph_replay(cp, oracle, cls, n, name, lds):
    grid = POSITION[name][1](n)
    lam, b_h, _, ref = _reference(grid)
    b = _dev(b_h)
    with cp.CirculantPlan(grid) as plan:
        plan.set_transport_symbol(lam)
        assert _assert_route(cp, plan, cls, n, name)["lds_bytes"] == lds
        eager = plan.apply(b)
        plan.set_graph(True)
        x = torch.empty_like(b)
        for _ in range(3):  # miss (eager + capture), then two replays
            x.zero_()
            plan.apply(b, out=x)
            torch.cuda.synchronize()
            assert torch.equal(x, eager)
        _assert_solution(oracle, x, grid, lam, b_h, ref, "graph ")
