"""The Krylov vector kernels behind the PETSc-named Vec layer (csrc/cfp_blas.hip) on device Vecs of
the complex and the real-scalar build, against exact references.

Sizes: one element, around a wave (63, 64), around a workgroup (255, 257), several workgroups
(3001), and past the grids at which the reductions start their grid-stride loops (MDOT_BLOCKS /
MAXPY_BLOCKS = 1024 workgroups: n > 262,144; RED_BLOCKS = 2048: n > 524,288); the element-wise
kernels also at one n past 16384 workgroups.  The multi-vector kernels cross their chunk seams
(MDOT_K = 8 vectors per k_mdot launch, MV_MAX = 32 per k_maxpy launch).

Exact data: (Gaussian) integers, so every dot, NORM_1 value, |y|^2 and updated vector must equal
an int64 reference bit for bit whatever the summation order.  Rounded data: standard normals
against np.longdouble, sums within the any-order bound (n + 2) 2^-53 sum |x_i| |y_i|, updates
within 4 (k + 2) 2^-53 sum_j |a_j| |x_j,i| per element."""
import ctypes
import math

import numpy as np
import pytest

import aij_cases as C

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NS = [1, 63, 64, 255, 257, 3001, 262144 + 77, 524288 + 333]
BIG = 16384 * 256 + 513
KMAX = 40
NORM_1, NORM_2, NORM_INFINITY = 0, 1, 3


# --------------------------------------------------------------------------- exact arithmetic
class Z:
    """A vector (or scalar) of Gaussian integers in int64: re, im."""

    def __init__(self, re, im=None):
        self.re = np.asarray(re, dtype=np.int64)
        self.im = np.zeros_like(self.re) if im is None else np.asarray(im, dtype=np.int64)

    def __add__(self, o):
        return Z(self.re + o.re, self.im + o.im)

    def __mul__(self, o):
        return Z(self.re * o.re - self.im * o.im, self.re * o.im + self.im * o.re)

    def conj(self):
        return Z(self.re, -self.im)

    def sum(self):
        return Z(int(self.re.sum()), int(self.im.sum()))

    def abs2(self):
        return self.re * self.re + self.im * self.im

    def np(self, real):
        return self.re.astype(np.float64) if real else self.re.astype(np.float64) + 1j * self.im.astype(np.float64)

    def value(self, real):
        return float(self.re) if real else complex(float(self.re), float(self.im))

    def same(self, arr):
        arr = np.asarray(arr)
        return np.array_equal(arr.real, self.re.astype(np.float64)) and \
            np.array_equal(arr.imag, self.im.astype(np.float64))


def zrand(rng, shape, bound, real):
    return Z(rng.integers(-bound, bound + 1, size=shape),
             None if real else rng.integers(-bound, bound + 1, size=shape))


# --------------------------------------------------------------------------- shared data
class Data:
    """Vectors of one build and size, made once: the integer set (x, y with |re|, |im| <= 4, a
    basis V of KMAX vectors with entries in {-1, 0, 1}) and the normal set, and their device Vecs,
    which no test writes."""

    def __init__(self, b, n, nbasis):
        rng = np.random.default_rng(1000 * n + (1 if b.real else 0))
        self.n, self.b = n, b
        self.zx, self.zy = zrand(rng, n, 4, b.real), zrand(rng, n, 4, b.real)
        self.zV = [zrand(rng, n, 1, b.real) for _ in range(nbasis)]

        def normal():
            v = rng.standard_normal(n)
            return v if b.real else v + 1j * rng.standard_normal(n)
        self.rx, self.ry = normal(), normal()
        self.rV = [normal() for _ in range(nbasis)]
        self.dev = {}

    def vec(self, key):
        """Device Vec of a shared array ("zx", "ry", ("zV", 3), ...), uploaded once; read only."""
        if key not in self.dev:
            a = getattr(self, key[0])[key[1]] if isinstance(key, tuple) else getattr(self, key)
            self.dev[key] = self.b.vec(a.np(self.b.real) if isinstance(a, Z) else a, keep=True)
        return self.dev[key]

    def free(self):
        for v in self.dev.values():
            v.destroy()
        self.dev = {}

    def basis(self, exact, k):
        """k basis Vecs (the KMAX shared ones, reused in turn beyond that) and their arrays."""
        name = "zV" if exact else "rV"
        idx = [j % len(getattr(self, name)) for j in range(k)]
        return [self.vec((name, j)) for j in idx], [getattr(self, name)[j] for j in idx]


@pytest.fixture(scope="module", params=[(r, n) for r in (False, True) for n in NS],
                ids=lambda p: f"{'real' if p[0] else 'complex'}-{p[1]}")
def dat(request):
    """The shared data of one build and size; module scope, so the tests of one size run together."""
    real, n = request.param
    d = Data(C.build_of("real" if real else "ccx"), n, KMAX)
    yield d
    d.free()


@pytest.fixture(autouse=True)
def _free_temporaries():
    yield
    C.build_of("real").free_tmp()


def wide(a):
    return a.astype(np.clongdouble if np.iscomplexobj(a) else np.longdouble)


def sample(n):
    """Where an updated vector of the rounded data is compared with np.longdouble: everywhere up
    to 4096 elements; beyond, the head, the tail and 4096 scattered elements (the integer data is
    compared at every element, which is what finds a wrong index; this finds a wrong rounding)."""
    if n <= 4096:
        return np.arange(n)
    rng = np.random.default_rng(n)
    return np.unique(np.concatenate([np.arange(1024), np.arange(n - 1024, n), rng.integers(0, n, 4096)]))


# the vectors whose rounded dots are compared with np.longdouble (both sides of every MDOT_K seam);
# the integer dots are compared for every vector
JS = (0, 6, 7, 8, 15, 16, 30, 31, 32, 39)


def wdot(x, y):
    """y^H x in np.longdouble, and sum |x_i| |y_i|."""
    return np.sum(wide(x) * np.conj(wide(y))), float(np.sum(np.abs(wide(x)) * np.abs(wide(y))))


# --------------------------------------------------------------------------- calls
def vdot(b, x, y):
    out = (b.S * 1)()
    b.call(b.L.VecDot(x.h, y.h, out))
    return b.values(out, 1)[0]


def vnorm(b, x, kind):
    v = ctypes.c_double()
    b.call(b.L.VecNorm(x.h, kind, ctypes.byref(v)))
    return v.value


def vmdot(b, x, vs):
    out = (b.S * len(vs))()
    b.call(b.L.VecMDot(x.h, len(vs), b.handles(vs), out))
    return b.values(out, len(vs))


def vmaxpy(b, y, coef, vs):
    b.call(b.L.VecMAXPY(y.h, len(vs), b.scalars(coef), b.handles(vs)))


def vmaxpy_norm(b, y, coef, vs, overwrite, want_norm=True):
    nrm = ctypes.c_double(-1.0)
    b.call(b.L.VecMiniMAXPYNorm(y.h, len(vs), b.scalars(coef), b.handles(vs), 1 if overwrite else 0,
                                ctypes.byref(nrm) if want_norm else None))
    return nrm.value


def vmdot_maxpy_norm(b, w, scale, vs):
    k = len(vs)
    dots, nrm = (b.S * k)(), ctypes.c_double(-1.0)
    b.call(b.L.VecMiniMDotMAXPYNorm(w.h, k, (ctypes.c_double * k)(*scale), b.handles(vs), dots, ctypes.byref(nrm)))
    return b.values(dots, k), nrm.value


def ulps(a, ref):
    return abs(a - ref) / np.spacing(abs(ref)) if ref != 0 else (0.0 if a == 0 else np.inf)


# --------------------------------------------------------------------------- reductions
def test_dot_and_norms(dat):
    d, b, real, n = dat, dat.b, dat.b.real, dat.n
    # exact
    x, y = d.vec("zx"), d.vec("zy")
    assert vdot(b, x, y) == (d.zx * d.zy.conj()).sum().value(real)  # y^H x
    assert vdot(b, y, x) == (d.zy * d.zx.conj()).sum().value(real)
    assert vnorm(b, x, NORM_1) == float(int(np.abs(d.zx.re).sum() + np.abs(d.zx.im).sum()))
    s2 = int(d.zx.abs2().sum())
    assert vnorm(b, x, NORM_2) == math.sqrt(s2)
    assert ulps(vnorm(b, x, NORM_INFINITY), math.sqrt(int(d.zx.abs2().max()))) <= 2
    # rounded
    x, y = d.vec("rx"), d.vec("ry")
    ref, mag = wdot(d.rx, d.ry)
    assert abs(np.clongdouble(vdot(b, x, y)) - ref) <= (n + 2) * U * mag
    w = wide(d.rx)
    s1 = np.sum(np.abs(w.real) + np.abs(w.imag))
    assert abs(vnorm(b, x, NORM_1) - s1) <= (n + 2) * U * s1
    r2 = np.sqrt(np.sum(np.abs(w) ** 2))
    assert abs(vnorm(b, x, NORM_2) - r2) <= ((n + 2) / 2 + 2) * U * r2  # half the bound of the sum, and the root
    assert ulps(vnorm(b, x, NORM_INFINITY), float(np.abs(w).max())) <= 2


def test_mdot(dat):
    """VecMDot across the MDOT_K = 8 seam: 1, 7, 8, 9, 16, 17, 32, 33, 40 vectors."""
    d, b, real, n = dat, dat.b, dat.b.real, dat.n
    exact = [(d.zx * v.conj()).sum().value(real) for v in d.zV]
    rounded = {j: wdot(d.rx, d.rV[j]) for j in JS}
    for k in (1, 7, 8, 9, 16, 17, 32, 33, 40):
        vs, _ = d.basis(True, k)
        got = vmdot(b, d.vec("zx"), vs)
        assert list(got) == exact[:k], f"k = {k}"
        vs, _ = d.basis(False, k)
        got = vmdot(b, d.vec("rx"), vs)
        for j in [j for j in JS if j < k]:
            ref, mag = rounded[j]
            assert abs(np.clongdouble(got[j]) - ref) <= (n + 2) * U * mag, f"k = {k}, j = {j}"


# --------------------------------------------------------------------------- updates
def _maxpy_ok(got, k, y0, coef, arrs):
    """got = y0 + sum_j coef_j arrs_j at the sampled elements, within 4 (k + 2) 2^-53 (|y0| + sum |a_j| |x_j|)."""
    idx = sample(len(got))
    ref = wide(y0[idx]) if y0 is not None else 0
    mag = np.abs(wide(y0[idx])).real if y0 is not None else 0
    for a, v in zip(coef, arrs):
        wv = wide(v[idx])
        ref = ref + (np.clongdouble(a) if np.iscomplexobj(v) else np.longdouble(a)) * wv
        mag = mag + abs(a) * np.abs(wv).real
    return bool(np.all(np.abs(wide(got[idx]) - ref) <= 4 * (k + 2) * U * mag))


def test_maxpy(dat):
    """VecMAXPY across the MV_MAX = 32 seam (1, 31, 32, 33, 65 vectors), and VecMiniMAXPYNorm with
    and without overwrite, with no vectors, and without the norm."""
    d, b, real, n = dat, dat.b, dat.b.real, dat.n
    rng = np.random.default_rng(n)
    for k in (1, 31, 32, 33, 65):
        zc = zrand(rng, k, 3, real)
        vs, zs = d.basis(True, k)
        y = b.vec(d.zy.np(real))
        vmaxpy(b, y, zc.np(real), vs)
        ref = d.zy
        for j in range(k):
            ref = ref + Z(zc.re[j], zc.im[j]) * zs[j]
        assert ref.same(y.array()), f"k = {k}"
        rc = rng.standard_normal(k) if real else rng.standard_normal(k) + 1j * rng.standard_normal(k)
        vs, rs = d.basis(False, k)
        y = b.vec(d.ry)
        vmaxpy(b, y, rc, vs)
        assert _maxpy_ok(y.array(), k, d.ry, rc, rs), f"k = {k}"
    for k in (0, 1, 33):
        for overwrite in (False, True):
            for want_norm in (True, False):
                zc = zrand(rng, k, 3, real)
                vs, zs = d.basis(True, k)
                y = b.vec(d.zy.np(real))
                nrm = vmaxpy_norm(b, y, zc.np(real), vs, overwrite, want_norm)
                ref = Z(np.zeros(n)) if overwrite else d.zy
                for j in range(k):
                    ref = ref + Z(zc.re[j], zc.im[j]) * zs[j]
                what = f"k = {k}, overwrite = {overwrite}, norm = {want_norm}"
                assert ref.same(y.array()), what
                assert nrm == (math.sqrt(int(ref.abs2().sum())) if want_norm else -1.0), what
                rc = rng.standard_normal(k) if real else rng.standard_normal(k) + 1j * rng.standard_normal(k)
                vs, rs = d.basis(False, k)
                y = b.vec(d.ry)
                nrm = vmaxpy_norm(b, y, rc, vs, overwrite, want_norm)
                y0 = None if overwrite else d.ry
                got = y.array()
                assert _maxpy_ok(got, k, y0, rc, rs), what
                if want_norm:  # the norm of the vector the kernel wrote
                    r2 = np.sqrt(np.sum(np.abs(wide(got)) ** 2))
                    assert abs(nrm - r2) <= ((n + 2) / 2 + 2) * U * r2, what


def test_mdot_maxpy_norm_one_sweep(dat):
    """VecMiniMDotMAXPYNorm (classical Gram-Schmidt in one call: k_mdot chunks, k_mdot_finish with
    fewer workgroups than MDOT_BLOCKS at the small sizes, k_maxpy_dc) for 1, 8, 9, 31, 32 vectors
    with negative scales: exact on the integer data and equal, bit for bit, to VecMDot + VecMAXPY +
    VecNorm on copies."""
    d, b, real, n = dat, dat.b, dat.b.real, dat.n
    for k in (1, 8, 9, 31, 32):
        scale = [-1.0 - (j % 2) for j in range(k)]
        # exact
        vs, zs = d.basis(True, k)
        w = b.vec(d.zx.np(real))
        dots, nrm = vmdot_maxpy_norm(b, w, scale, vs)
        zd = [(d.zx * v.conj()).sum() for v in zs]
        ref = d.zx
        for j in range(k):
            ref = ref + Z(int(scale[j]) * zd[j].re, int(scale[j]) * zd[j].im) * zs[j]
        s2 = int(ref.abs2().sum())
        assert s2 < 2 ** 53 and max(abs(int(z.re)) + abs(int(z.im)) for z in zd) * 4 * k < 2 ** 53  # the data stays exact
        assert list(dots) == [z.value(real) for z in zd], f"k = {k}"
        assert ref.same(w.array()), f"k = {k}"
        assert nrm == math.sqrt(s2), f"k = {k}"
        # the unfused operations on a copy
        w2 = b.vec(d.zx.np(real))
        dots2 = vmdot(b, w2, vs)
        vmaxpy(b, w2, [scale[j] * dots2[j] for j in range(k)], vs)
        assert list(dots2) == list(dots) and np.array_equal(w2.array(), w.array()), f"k = {k}"
        assert vnorm(b, w2, NORM_2) == nrm, f"k = {k}"
        # rounded: the dots against the reference; the update against the coefficients the call returned
        vs, rs = d.basis(False, k)
        w = b.vec(d.rx)
        dots, nrm = vmdot_maxpy_norm(b, w, scale, vs)
        for j in [j for j in JS if j < k]:
            ref, mag = wdot(d.rx, rs[j])
            assert abs(np.clongdouble(dots[j]) - ref) <= (n + 2) * U * mag, f"k = {k}, j = {j}"
        coef = [scale[j] * dots[j] for j in range(k)]
        got = w.array()
        assert _maxpy_ok(got, k, d.rx, coef, rs), f"k = {k}"
        r2 = np.sqrt(np.sum(np.abs(wide(got)) ** 2))
        assert abs(nrm - r2) <= ((n + 2) / 2 + 2) * U * r2, f"k = {k}"


def test_maxpy_norm_device_dots_from_wave_apply():
    """VecMiniMAXPYNormDeviceDots fed by the dots a wave-system apply leaves on the device
    (cfp_wave_plan_apply_dots: blas_mdot_dev, k_mdot_finish): w += sum_j scale_j dots_j V_j, |w|, and
    the dots copied back."""
    import torch
    from circulantpreconditioner_amd import petsc as P
    from circulantpreconditioner_amd import wave as W
    b = C.build_of("ccx")
    grid, k = (32, 24, 16), 5
    n = 4 * int(np.prod(grid))
    rng = np.random.default_rng(5)
    rV = [rng.standard_normal(n) + 1j * rng.standard_normal(n) for _ in range(k)]
    tV = [torch.from_numpy(v).to("cuda") for v in rV]
    rhs = torch.from_numpy(rng.standard_normal(n) + 1j * rng.standard_normal(n)).to("cuda")
    wp = W.WavePlan(grid).set_symbol((0.079, 0.05, 0.11))
    x, dots_dev, _ = wp.apply_dots(rhs, dots_with=tV)
    torch.cuda.synchronize()
    x0, dots0 = x.cpu().numpy(), dots_dev.cpu().numpy()
    for j in range(k):
        ref, mag = wdot(x0, rV[j])
        assert abs(np.clongdouble(dots0[j]) - ref) <= (n + 2) * U * mag, j
    w = P.Vec.from_tensor(x)
    vs = [P.Vec.from_tensor(t) for t in tV]
    scale = [-1.0, -0.5, -2.0, -1.0, -0.25]
    out, nrm = (b.S * k)(), ctypes.c_double(-1.0)
    b.call(b.L.VecMiniMAXPYNormDeviceDots(w.h, k, (ctypes.c_double * k)(*scale), b.handles(vs), dots_dev.data_ptr(),
                                          out, ctypes.byref(nrm)))
    got_dots = b.values(out, k)
    assert np.array_equal(got_dots, dots0)  # copied back as they are
    coef = [scale[j] * dots0[j] for j in range(k)]
    got = w.array()
    assert _maxpy_ok(got, k, x0, coef, rV)
    r2 = np.sqrt(np.sum(np.abs(wide(got)) ** 2))
    assert abs(nrm.value - r2) <= ((n + 2) / 2 + 2) * U * r2
    wp.close()


def test_elementwise_updates(dat):
    """VecAXPY, VecAYPX, VecWAXPY (also in place), VecPointwiseMult / Divide, VecShift, VecScale,
    VecCopy, VecSet; and VecAXPY followed by VecNorm, which sums the partials the AXPY left."""
    _elementwise(dat)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_elementwise_updates_past_the_grid(real):
    """The same at one n past 16384 workgroups of 256 (8192 for the complex scale and divide), where
    the element-wise kernels run their grid-stride loops."""
    d = Data(C.build_of("real" if real else "ccx"), BIG, 0)
    try:
        _elementwise(d)
    finally:
        d.free()


def _elementwise(d):
    b, L, real, n = d.b, d.b.L, d.b.real, d.n
    a_z, a_r = (Z(-3, 0) if real else Z(-3, 2)), (-0.8125 if real else -0.8125 + 1.3j)
    for exact in (True, False):
        x0, y0 = (d.zx, d.zy) if exact else (d.rx, d.ry)
        xn, yn = (x0.np(real), y0.np(real)) if exact else (x0, y0)
        a = a_z.value(real) if exact else a_r
        X, Y = d.vec("zx" if exact else "rx"), d.vec("zy" if exact else "ry")

        def check(got, zref, rref, mag, k=1, what=""):
            if exact:
                assert zref.same(got), what
            else:
                assert np.all(np.abs(wide(got[idx]) - rref) <= 4 * (k + 2) * U * mag), what

        idx = sample(n)  # where the rounded results are compared; the integer ones everywhere
        wx, wy = wide(xn[idx]), wide(yn[idx])
        ax, ay = np.abs(wx).real, np.abs(wy).real
        wa = np.clongdouble(a) if not real else np.longdouble(a)
        # y += a x, then the norm from the sweep's partials against a plain VecNorm of a copy
        y = b.vec(yn)
        b.call(L.VecAXPY(y.h, b.sc(a), X.h))
        nrm = vnorm(b, y, NORM_2)
        got = y.array()
        check(got, exact and y0 + a_z * x0, wy + wa * wx, ay + abs(a) * ax, what="axpy")
        if exact:
            assert nrm == math.sqrt(int((y0 + a_z * x0).abs2().sum())) == vnorm(b, b.vec(got), NORM_2)
        else:
            r2 = np.sqrt(np.sum(np.abs(wide(got)) ** 2))
            assert abs(nrm - r2) <= ((n + 2) / 2 + 2) * U * r2
        # y = x + a y
        y = b.vec(yn)
        b.call(L.VecAYPX(y.h, b.sc(a), X.h))
        check(y.array(), exact and x0 + a_z * y0, wx + wa * wy, ax + abs(a) * ay, what="aypx")
        # w = a x + y: into a third vector, into x, into y
        for alias in ("w", "x", "y"):
            xv, yv = (b.vec(xn) if alias == "x" else X), (b.vec(yn) if alias == "y" else Y)
            w = xv if alias == "x" else yv if alias == "y" else b.vec(np.full(n, 777.0))
            b.call(L.VecWAXPY(w.h, b.sc(a), xv.h, yv.h))
            check(w.array(), exact and a_z * x0 + y0, wa * wx + wy, abs(a) * ax + ay, what="waxpy " + alias)
        # w = x * y
        w = b.vec(np.full(n, 777.0))
        b.call(L.VecPointwiseMult(w.h, X.h, Y.h))
        check(w.array(), exact and x0 * y0, wx * wy, ax * ay, what="pointwise mult")
        # w = x / y with PETSc's rule for a zero divisor; the integer y has zeros of its own
        yz = yn.copy()
        yz[::7] = 0
        w, Yz = b.vec(np.full(n, 777.0)), b.vec(yz)
        b.call(L.VecPointwiseDivide(w.h, X.h, Yz.h))
        got, nz = w.array(), yz != 0
        assert np.all(got[~nz] == 0), "pointwise divide by zero"
        nzi = idx[nz[idx]]
        q = wide(xn[nzi]) / wide(yz[nzi])
        assert np.all(np.abs(wide(got[nzi]) - q) <= 8 * U * np.abs(q)), "pointwise divide"
        # x += a, x *= a, copy, set
        w = b.vec(xn)
        b.call(L.VecShift(w.h, b.sc(a)))
        check(w.array(), exact and x0 + Z(np.full(n, a_z.re), np.full(n, a_z.im)), wx + wa, ax + abs(a),
              what="shift")
        w = b.vec(xn)
        b.call(L.VecScale(w.h, b.sc(a)))
        check(w.array(), exact and a_z * x0, wa * wx, abs(a) * ax, what="scale")
        w = b.vec(np.full(n, 777.0))
        b.call(L.VecCopy(X.h, w.h))
        assert np.array_equal(w.array(), xn), "copy"
        b.call(L.VecSet(w.h, b.sc(a)))
        assert np.array_equal(w.array(), np.full(n, a, dtype=b.dtype)), "set"
