"""The fused Krylov step of the 256^3 apply (cfp_plan_apply_ex: A b formed in P1, the Gram-Schmidt
dots in P3) and the complex applyFFT3DPrecTransportBA, over every stencil shape the fusion admits
(tests/stencil_cases.py), against exact references.

Exact mode: the plan with the transport symbol of lambda = (0, 0, 0) has Diag = 1, so
x = IDFT(DFT(A b)) / N; with integer A and b, round(x) must equal the int64 reference at every one
of the 16 777 216 points (max |x - y| < 0.5 first).  The sweeps' own rounding is some 1e-13 here
(numpy's ifftn(fftn(y)) deviates by 9.7e-14 for such a y), so one wrong neighbour, class byte or
sign -- a change of at least 1 -- cannot hide.  Measured max |x - y| on an MI355X, per case:
    up_pos 4.3e-14, up_neg 3.6e-14, centered 5.7e-14, diag_only 2.1e-14, diag16 5.7e-14,
    no_diag 4.3e-14, lower_only 2.1e-14, upper_only 5.0e-14, edges 8.5e-14, per_point16 7.1e-14,
    complex_coef 9.9e-14, stored_zero 7.8e-14, cls17 7.1e-14, wide 8.5e-14, y_coupled 7.1e-14.
Against the separate steps (device MatMult of the same matrix, then the plain apply) at the bench
symbol and at (0.3 + 0.2j, 1.1, 0.7 - 0.4j) -- both take the z-recurrence P2 -- and at the bench
symbol given as its 1-D vectors, which takes the FFT P2: measured, the fused x is bit-equal to
the separate steps' in all 15 runs (both bounds are 1e-13), the residual against C at most 5.5e-16.
The dots, each component on its own, against np.longdouble sums of the returned x within the
any-order bound (N + 2) 2^-53 sum |v_i| |x_i|; the largest measured ratio of error to bound was
1.3e-7 (an x^H x slot; 8.6e-11 over the v_j^H x slots).
Every case asserts the route it took: `fused` of apply_ex, mid_kernel() of the plan, and
MatFFTHIPGetFusedBACount for the PCSHELL."""
import ctypes

import numpy as np
import pytest
import torch

import stencil_cases as S

pytestmark = pytest.mark.gpu

N3 = (256, 256, 256)
N = 256 ** 3
U = 2.0 ** -53
BENCH = (0.6, 0.15, 0.02)
COMPLEX = (0.3 + 0.2j, 1.1, 0.7 - 0.4j)
# (symbol, given as the 1-D vectors, the P2 that then runs).  Both transport symbols are within the z
# recurrence's reach; the bench symbol handed over as vectors is the same Diag on the FFT P2.
SYMBOLS = {"bench": (BENCH, False, "zrec"), "complex": (COMPLEX, False, "zrec"), "bench_vectors": (BENCH, True, "fft")}
ROUNDED = ("up_neg", "centered", "edges", "per_point16", "complex_coef")
BA_CASES = ("up_neg", "centered", "per_point16")


@pytest.fixture(scope="module")
def cp():
    import circulantpreconditioner_amd as cp
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return cp


@pytest.fixture(scope="module")
def P():
    from circulantpreconditioner_amd import petsc
    return petsc


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class Shared:
    """One plan per symbol, one integer b, one uniform b, the cases, their matrices and the host
    copies the dots are judged by: made on first use, kept for the module, written by no test."""

    def __init__(self, cp, dev):
        self.cp, self.dev = cp, dev
        self.plans, self.cases, self.mats, self.dot_sets = {}, {}, {}, {}
        br, bi = S.integer_vector(N)
        self.br, self.bi = torch.from_numpy(br).to(dev), torch.from_numpy(bi).to(dev)
        self.b_int = torch.complex(self.br.double(), self.bi.double())
        self.b_uni = torch.empty(N, dtype=torch.complex128, device=dev)
        cp.fill_uniform(self.b_uni, 20251019)
        rng = np.random.default_rng(7)
        self.v_host = [rng.integers(-8, 9, size=N).astype(np.float64) + 1j * rng.integers(-8, 9, size=N)
                       for _ in range(4)]
        self.v = [torch.from_numpy(v).to(dev) for v in self.v_host]

    def plan(self, key="exact"):
        if key not in self.plans:
            p = self.cp.CirculantPlan(N3, device=0)
            if key == "exact":
                p.set_transport_symbol((0, 0, 0))
            else:
                lam, vectors, _ = SYMBOLS[key]
                if vectors:
                    s = self.cp.transport_symbol_1d(256)
                    p.set_separable_symbol(s, s, s, lam)
                else:
                    p.set_transport_symbol(lam)
            assert [q["mode"] for q in p.passes()] == ["rows_fwd", "mid_fused", "rows_inv"]
            self.plans[key] = p
        return self.plans[key]

    def case(self, name):
        if name not in self.cases:
            self.cases[name] = S.make(name, N3)
        return self.cases[name]

    def reference(self, name):
        return self.case(name).reference_torch(self.br, self.bi)

    def mat(self, P, name):
        if name not in self.mats:
            c = self.case(name)
            indptr, indices, data = c.csr()
            self.mats[name] = P.Mat.aij(indptr, indices, data, (N, N))
        return self.mats[name]

    def close(self):
        for m in self.mats.values():
            m.destroy()
        for p in self.plans.values():
            p.close()


@pytest.fixture(scope="module")
def sh(cp, dev):
    s = Shared(cp, dev)
    yield s
    s.close()


def _where(bad):
    """Which columns, lanes and rows a set of wrong points lies in (P1 of the fused kernel: lane
    x mod 32 of wave x / 32, ty = (y / 8) mod 2 the half-wave)."""
    idx = torch.nonzero(bad.reshape(-1)).reshape(-1)
    x, y, z = idx % 256, (idx // 256) % 256, idx // 65536
    xs = torch.unique(x).tolist()
    return (f"{idx.numel()} points; columns x {xs[:40]}{' ...' if len(xs) > 40 else ''}; "
            f"x mod 32 {torch.unique(x % 32).tolist()}; x = 0: {0 in xs}, x = 255: {255 in xs}; "
            f"ty {torch.unique((y // 8) % 2).tolist()}; first (x, y, z) {(int(x[0]), int(y[0]), int(z[0]))}")


def check_exact(x, yr, yi, what):
    """max |x - y| < 0.5, then round(x) == y at every point.  Returns the measured maximum."""
    err = float(torch.maximum((x.real - yr.double()).abs().max(), (x.imag - yi.double()).abs().max()))
    print(f"{what}: max|x - y| = {err:.3e}")
    bad = (torch.round(x.real).to(torch.int64) != yr) | (torch.round(x.imag).to(torch.int64) != yi)
    assert err < 0.5, f"{what}: max|x - y| = {err:.3e}; {_where(bad)}"
    assert torch.equal(torch.round(x.real).to(torch.int64), yr) and \
        torch.equal(torch.round(x.imag).to(torch.int64), yi), f"{what}: {_where(bad)}"
    return err


# --------------------------------------------------------------------------- exact mode
@pytest.mark.parametrize("name", S.NAMES)
def test_exact_mode(sh, dev, name):
    """x = apply(A b) at Diag = 1 is the int64 A b, point for point; the classes per point."""
    c = sh.case(name)
    assert c.ncls == S.FULL_NCLS.get(name, c.ncls)
    plan = sh.plan()
    x = torch.empty_like(sh.b_int)
    dots, fused = plan.apply_ex(sh.b_int, x, stencil=c.stencil_dev(dev))
    torch.cuda.synchronize()
    assert dots is None and fused == c.fused
    yr, yi = sh.reference(name)
    assert int(yr.abs().max()) > 0 and int(yi.abs().max()) > 0
    check_exact(x, yr, yi, name)


@pytest.mark.parametrize("name", S.BY_X)
def test_class_source(sh, dev, name):
    """Classes by x alone: the per-point class array and the [n_x] cls_x (what the PCSHELL passes)
    feed the same kernel the same values -- bit-equal x."""
    c = sh.case(name)
    assert c.by_x
    plan = sh.plan()
    x_pt, x_cx = torch.empty_like(sh.b_int), torch.empty_like(sh.b_int)
    _, f1 = plan.apply_ex(sh.b_int, x_pt, stencil=c.stencil_dev(dev))
    _, f2 = plan.apply_ex(sh.b_int, x_cx, stencil=c.stencil_dev(dev, cls_x=True))
    torch.cuda.synchronize()
    assert f1 == f2 == c.fused
    assert torch.equal(x_pt, x_cx)


# --------------------------------------------------------------------------- against the separate steps
def _rel(a, b):
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


@pytest.mark.parametrize("sym", list(SYMBOLS))
@pytest.mark.parametrize("name", ROUNDED)
def test_against_separate_steps(sh, P, dev, name, sym):
    """Rounded data: the fused apply_ex against the device MatMult of the same matrix (its own
    kernel, pinned by test_aij_forms_gpu.py) followed by the plain apply, and against the
    circulant C it inverts."""
    from test_gpu_parity import apply_C_torch
    lam, _, mid = SYMBOLS[sym]
    c = sh.case(name)
    plan = sh.plan(sym)
    assert plan.mid_kernel() == mid
    M = sh.mat(P, name)
    y_dev = torch.empty_like(sh.b_uni)
    M.mult(P.Vec.from_tensor(sh.b_uni), P.Vec.from_tensor(y_dev))
    assert M.aij_format() == "dia"
    x_fused = torch.empty_like(sh.b_uni)
    _, fused = plan.apply_ex(sh.b_uni, x_fused, stencil=c.stencil_dev(dev, cls_x=c.by_x))
    assert fused == 1
    x_sep = plan.apply(y_dev)
    torch.cuda.synchronize()
    rel = _rel(x_fused, x_sep)
    mx = float((x_fused - x_sep).abs().max() / x_sep.abs().max())
    res = _rel(apply_C_torch(x_fused, N3, lam), y_dev)
    print(f"{name}/{sym}: rel_L2 {rel:.3e}  max {mx:.3e}  residual {res:.3e}")
    assert rel < 1e-13
    assert mx < 1e-13
    assert res < 1e-12


# --------------------------------------------------------------------------- the dots
def _long(a):
    return a.real.astype(np.longdouble), a.imag.astype(np.longdouble)


def dot_set(sh, dev, stencil):
    """x of the exact mode (with the up_neg stencil, or of the plain apply), its host copy, the
    references v_j^H x and x^H x in np.longdouble and sum |v_i| |x_i| -- once per module."""
    if stencil not in sh.dot_sets:
        plan = sh.plan()
        x = torch.empty_like(sh.b_int)
        st = sh.case("up_neg").stencil_dev(dev) if stencil else None
        _, fused = plan.apply_ex(sh.b_int, x, stencil=st) if stencil else (None, 0)
        if not stencil:
            plan.apply(sh.b_int, out=x)
        torch.cuda.synchronize()
        xh = x.cpu().numpy()
        xr, xi = _long(xh)
        ax = np.abs(xh)
        refs, mags = [], []
        for vh in sh.v_host + [xh]:
            vr, vi = _long(vh)
            refs.append((np.sum(vr * xr) + np.sum(vi * xi), np.sum(vr * xi) - np.sum(vi * xr)))  # conj(v) x
            mags.append(float(np.sum(np.abs(vh) * ax)))
        sh.dot_sets[stencil] = (x, refs, mags)
    return sh.dot_sets[stencil]


def _dot_ref(refs, mags, q, v, delta):
    """(v^H x_ret, its bound) for the returned x_ret = x_mod + delta: the module's np.longdouble
    sum with x_mod plus, where delta is not zero, the device dot with delta (q = 4, v = x_ret:
    x_ret^H x_ret = x_mod^H x_mod + 2 Re x_ret^H delta - |delta|^2, the last far below rounding)."""
    ref = complex(float(refs[q][0]), float(refs[q][1]))
    if bool(delta.any()):
        corr = complex(torch.vdot(v, delta))
        ref += 2 * corr.real if q == 4 else corr
    return ref, (N + 2) * U * mags[q]


# index into (v0, v1, v2, v3): None = x itself, "x" = the output tensor handed over as a vector
ARRANGEMENTS = {
    "v0": (0,), "self": (None,), "v0_v1": (0, 1), "self_v1": (None, 1), "v1_self": (1, None),
    "v0_v1_v2": (0, 1, 2), "v0_v1_v2_v3": (0, 1, 2, 3), "v0_self_v2_self": (0, None, 2, None),
    "v0_out": (0, "x"), "out_v3_self": ("x", 3, None),
    "nv5": (0, 1, 2, 3, None), "nv8": (3, None, 2, 1, 0, "x", 1, 2),
}


@pytest.mark.parametrize("stencil", [True, False], ids=["up_neg", "no_stencil"])
@pytest.mark.parametrize("arr", list(ARRANGEMENTS))
def test_dots_component_by_component(sh, dev, arr, stencil):
    """Every dots_with arrangement; each returned component against the host sum of the returned
    x (the module's x plus, where the returned one differs from it, the device dot of the
    difference), within (N + 2) 2^-53 sum |v_i| |x_i|: a dropped or doubled point is 1/N of that
    sum, 30 times the bound."""
    x_mod, refs, mags = dot_set(sh, dev, stencil)
    plan = sh.plan()
    sel = ARRANGEMENTS[arr]
    x = torch.empty_like(sh.b_int)
    with_ = tuple(None if j is None else (x if j == "x" else sh.v[j]) for j in sel)
    st = sh.case("up_neg").stencil_dev(dev) if stencil else None
    dots, fused = plan.apply_ex(sh.b_int, x, stencil=st, dots_with=with_)
    torch.cuda.synchronize()
    assert fused == (1 if len(sel) <= 4 else 0)
    delta = x - x_mod
    assert float(delta.abs().max()) < 1e-11  # the same apply, at most rounded differently
    got = dots.cpu().numpy()
    worst = 0.0
    for k, j in enumerate(sel):
        self_ = j is None or j == "x"
        ref, bound = _dot_ref(refs, mags, 4 if self_ else j, x if self_ else sh.v[j], delta)
        err = abs(complex(got[k]) - ref)
        worst = max(worst, err / bound)
        assert err <= bound, f"{arr}[{k}]: got {got[k]}, ref {ref}, err {err:.3e} > bound {bound:.3e}"
        if self_ and fused:  # P3 sums |x|^2 alone; the separate k_mdot forms x^H x as any dot, im within the bound
            assert got[k].imag == 0.0
    print(f"dots {arr}/{'up_neg' if stencil else 'no_stencil'}: worst err/bound {worst:.3e} (returned x {'is' if not bool(delta.any()) else 'is not'} the module's)")


def test_dots_only_in_place_is_the_plain_apply(sh, dev):
    """Dots only with out aliasing b: x bit-equal to the plain in-place apply, the dots fused."""
    plan = sh.plan()
    xa, xp = sh.b_int.clone(), sh.b_int.clone()
    dots, fused = plan.apply_ex(xa, xa, dots_with=(sh.v[0], None))
    plan.apply(xp, out=xp)
    torch.cuda.synchronize()
    assert fused == 1
    assert torch.equal(xa, xp)
    _, refs, mags = dot_set(sh, dev, False)
    got = dots.cpu().numpy()
    delta = xa - dot_set(sh, dev, False)[0]
    for k, q, v in ((0, 0, sh.v[0]), (1, 4, xa)):
        ref, bound = _dot_ref(refs, mags, q, v, delta)
        assert abs(complex(got[k]) - ref) <= bound


# --------------------------------------------------------------------------- argument rules
def test_stencil_with_b_aliasing_out_is_refused(sh, cp, dev):
    plan = sh.plan()
    for name in ("up_neg", "cls17"):  # the fused and the separate route alike
        b = sh.b_int.clone()
        with pytest.raises(cp.CirculantError):
            plan.apply_ex(b, b, stencil=sh.case(name).stencil_dev(dev))
        torch.cuda.synchronize()
        assert torch.equal(b, sh.b_int)  # refused before anything ran


def test_second_stencil_on_the_same_plan(sh, dev):
    """Nothing of a call's stencil outlives it: another stencil (other offsets, another class
    count, classes by x after classes per point) on the same plan gives that stencil's product,
    and so does the first again."""
    plan = sh.plan()
    x = torch.empty_like(sh.b_int)
    for name, cls_x in (("per_point16", False), ("up_neg", True), ("diag_only", False), ("per_point16", False)):
        c = sh.case(name)
        _, fused = plan.apply_ex(sh.b_int, x, stencil=c.stencil_dev(dev, cls_x=cls_x))
        torch.cuda.synchronize()
        assert fused == 1
        yr, yi = sh.reference(name)
        check_exact(x, yr, yi, f"{name} after another stencil")


# --------------------------------------------------------------------------- applyFFT3DPrecTransportBA (complex build)
@pytest.mark.parametrize("hip", [True, False], ids=["device", "host"])
def test_apply_ba_small_is_matmult_and_pcapply(P, oracle, hip):
    """(8, 4, 2), no fused kernels: left y = B (A x), right y = A (B x) -- exactly MatMult with the
    PC's operator and PCApply, the same kernels -- and the left side within 1e-10 of the oracle."""
    from oracle import transport as OT
    dims, lam = (8, 4, 2), (0.6, 0.15, 0.02)
    n = 64
    h = tuple(1.0 / d for d in dims)
    Acsr = OT.divergence_matrix(dims, h, 0.05, (1.0, 0.5, 0.25), sign="fixed", shift=1.0).tocsr()
    Acsr.sort_indices()
    A = P.Mat.aij(Acsr.indptr, Acsr.indices, Acsr.data, Acsr.shape)
    ctx = P.make_context(dims, lam)
    pc = P.PC.shell(ctx).setup().set_operators(A)
    F = P.Mat(ctypes.c_void_p(ctx.FFT_MAT), owned=False)
    x = oracle.c_fill_uniform(n, 47)
    new = P.Vec.seq_hip if hip else P.Vec.seq
    vx, vy, vw, vy2 = (new(n) for _ in range(4))
    vx.set_array(x)
    P.applyFFT3DPrecTransportBA(pc, P.PC_LEFT, vx, vy, vw)
    A.mult(vx, vw)
    pc.apply(vw, vy2)
    left = vy.array()
    assert np.array_equal(left, vy2.array())
    ref = oracle.c_solve_3d(oracle.c_build_diag_transport(dims, lam), Acsr @ x, dims)
    assert np.linalg.norm(left - ref) < 1e-10 * np.linalg.norm(ref)
    P.applyFFT3DPrecTransportBA(pc, P.PC_RIGHT, vx, vy, vw)
    pc.apply(vx, vw)
    A.mult(vw, vy2)
    right = vy.array()
    assert np.array_equal(right, vy2.array())
    assert not np.array_equal(left, right)  # the two sides really differ
    assert F.fused_ba_count() == 0  # nothing to fuse into at this grid
    pc.destroy()
    A.destroy()


@pytest.mark.parametrize("name", BA_CASES)
def test_apply_ba_256_routes(sh, P, dev, name):
    """256^3, device Vecs, lambda = (0, 0, 0) (Diag = 1): PC_LEFT with x != y forms A x inside the
    apply (the counter moves by one); y the same Vec as x, and PC_RIGHT, run MatMult and the apply
    apart (the counter stays).  All three give the int64 A x by rounding."""
    c = sh.case(name)
    M = sh.mat(P, name)
    ctx = P.make_context(N3, (0, 0, 0))
    pc = P.PC.shell(ctx).setup().set_operators(M)
    F = P.Mat(ctypes.c_void_p(ctx.FFT_MAT), owned=False)
    yr, yi = sh.reference(name)
    tx, ty, tw = sh.b_int.clone(), torch.zeros_like(sh.b_int), torch.zeros_like(sh.b_int)
    vx, vy, vw = (P.Vec.from_tensor(t) for t in (tx, ty, tw))
    assert F.fused_ba_count() == 0
    P.applyFFT3DPrecTransportBA(pc, P.PC_LEFT, vx, vy, vw)
    torch.cuda.synchronize()
    assert F.fused_ba_count() == 1
    assert torch.equal(tx, sh.b_int) and not bool(tw.any())  # x untouched, work unused
    check_exact(ty, yr, yi, f"BA left {name}")
    P.applyFFT3DPrecTransportBA(pc, P.PC_LEFT, vx, vy, vw)
    assert F.fused_ba_count() == 2  # exactly one per fused call
    # y the same Vec as x: through work
    P.applyFFT3DPrecTransportBA(pc, P.PC_LEFT, vx, vx, vw)
    torch.cuda.synchronize()
    assert F.fused_ba_count() == 2
    check_exact(tx, yr, yi, f"BA left in place {name}")
    check_exact(tw, yr, yi, f"BA left in place {name}, work = A x")
    # right: A (B x)
    tx.copy_(sh.b_int)
    ty.zero_()
    P.applyFFT3DPrecTransportBA(pc, P.PC_RIGHT, vx, vy, vw)
    torch.cuda.synchronize()
    assert F.fused_ba_count() == 2
    check_exact(ty, yr, yi, f"BA right {name}")
    assert float((tw - sh.b_int).abs().max()) < 1e-11  # work = B x = x at Diag = 1
    pc.destroy()
