"""Row-class stencils that aim at one branch of the fused Krylov step each (tests/test_stencil_cases_cpu.py,
tests/test_fused_stencil_gpu.py), and the exact reference their products are held to.

A case is written down directly as (offsets, mask[ncls], tab[ncls, nd], cls[n]) on an (nx, ny, nz)
grid, x fastest: row i = x + nx (y + ny z) of class c = cls[i] holds tab[c, k] at column
i + offsets[k] where bit k of mask[c] is set.  Nothing here runs row_class_form, the library or a
scipy product: the matrix (csr()) is assembled from the description, and the reference
(reference_numpy / reference_torch) is

    y[i] = sum_k [bit k of mask[cls[i]]] tab[cls[i], k] b[i + offsets[k]]

in int64, re and im apart, from the copies of b shifted along the row (zero outside the row; an
offset of a whole row or more shifts the flat vector).  Coefficients are Gaussian integers with
|re|, |im| <= 4 and b holds |re|, |im| <= 8, so the product is exact in int64 and in float64 alike.

Each case carries what the library must make of it: `x_local` (every stored entry stays in its
row of nx points), `by_x` (the classes depend on x alone, so PetscMiniMatAIJGetDia hands the
PCSHELL a cls_x), and `fused` (cfp_plan_apply_ex runs it inside the 256^3 sweeps: x-local, at
most 3 offsets in {-1, 0, +1}, at most 16 classes)."""
from __future__ import annotations

import zlib

import numpy as np

MAX_FUSED_CLS = 16  # TP_PRE_MAX_CLS (csrc/cfp_three_pass.h)


class Stencil:
    def __init__(self, name, dims, offsets, mask, tab, cls, x_local, by_x, fused, why):
        nx, ny, nz = dims
        self.name, self.dims, self.why = name, dims, why
        self.nx, self.rows, self.n = nx, ny * nz, nx * ny * nz
        self.offsets = [int(o) for o in offsets]
        assert self.offsets == sorted(set(self.offsets))
        nd = len(self.offsets)
        mask = np.asarray(mask, dtype=np.uint8)
        tab = np.asarray(tab, dtype=np.complex128).reshape(len(mask), nd)
        cls = np.asarray(cls).reshape(-1)
        assert cls.size == self.n
        # only the classes some row uses, renumbered in order; an absent slot's coefficient is 0
        used = np.unique(cls)
        renum = np.full(len(mask), -1, dtype=np.int64)
        renum[used] = np.arange(len(used))
        self.cls = renum[cls].astype(np.uint8)
        self.mask = mask[used]
        bits = ((self.mask[:, None] >> np.arange(nd)) & 1).astype(bool)
        self.tab = np.where(bits, tab[used], 0)
        self.ncls = len(used)
        self.x_local, self.by_x, self.fused = x_local, by_x, fused
        self._check(bits)

    def _check(self, bits):
        """The description is a matrix of this shape, and says of itself what is true."""
        nx, n, nd = self.nx, self.n, len(self.offsets)
        key = np.concatenate([self.tab.view(np.float64), self.mask[:, None].astype(np.float64)], axis=1)
        assert len(np.unique(key, axis=0)) == self.ncls, "two classes hold the same row"
        assert np.abs(self.tab.real).max() <= 4 and np.abs(self.tab.imag).max() <= 4
        assert np.array_equal(self.tab, np.round(self.tab.real) + 1j * np.round(self.tab.imag))
        assert bits.any(axis=0).all(), "an offset no class stores"
        present = self.present()
        i = np.arange(n, dtype=np.int64)
        local = True
        for k, o in enumerate(self.offsets):
            col = i[present[:, k]] + o
            assert col.size == 0 or (col.min() >= 0 and col.max() < n), "an entry outside the matrix"
            if abs(o) < nx:  # the in-row shift of the reference must be the matrix's entry
                row_ok = col // nx == i[present[:, k]] // nx
                local = local and bool(row_ok.all())
                assert row_ok.all() or not self.x_local
            else:
                local = local and col.size == 0
        assert local == self.x_local
        cx = self.cls.reshape(self.rows, nx)
        assert bool((cx == cx[0]).all()) == self.by_x
        fusable = (self.x_local and 1 <= nd <= 3 and all(-1 <= o <= 1 for o in self.offsets)
                   and self.ncls <= MAX_FUSED_CLS)
        assert fusable == bool(self.fused)

    # ------------------------------------------------------------------ the matrix
    def present(self):
        """[n, nd] bool: row i stores the entry of offset k."""
        nd = len(self.offsets)
        return ((self.mask[self.cls][:, None] >> np.arange(nd)) & 1).astype(bool)

    def csr(self):
        """(indptr, indices, data): the rows in order, columns ascending, stored zeros kept."""
        present = self.present()
        indptr = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(present.sum(axis=1), out=indptr[1:])
        cols = np.arange(self.n, dtype=np.int64)[:, None] + np.asarray(self.offsets, dtype=np.int64)
        return indptr, cols[present], self.tab[self.cls][present]

    def scipy(self):
        import scipy.sparse as sp
        indptr, indices, data = self.csr()
        A = sp.csr_matrix((data, indices, indptr), shape=(self.n, self.n))
        assert A.nnz == len(data)
        return A

    @property
    def cls_x(self):
        return self.cls[:self.nx].copy() if self.by_x else None

    def expect_info(self):
        """What Mat.aij(...).aij_info() must report: every case is within 8 diagonals and 256
        classes, so all are in the row-class form."""
        return dict(format="dia", nd=len(self.offsets), ncls=self.ncls)

    # ------------------------------------------------------------------ the reference
    def _terms(self):
        for k, o in enumerate(self.offsets):
            on = ((self.mask >> k) & 1).astype(np.int64)
            yield o, (on * self.tab[:, k].real.astype(np.int64)), (on * self.tab[:, k].imag.astype(np.int64))

    def reference_numpy(self, br, bi):
        """(yr, yi) int64 from int64 (br, bi)."""
        assert br.dtype == np.int64 and bi.dtype == np.int64
        yr, yi = np.zeros(self.n, dtype=np.int64), np.zeros(self.n, dtype=np.int64)
        for o, cr, ci in self._terms():
            sr, si = _shift_np(br, o, self.nx), _shift_np(bi, o, self.nx)
            cr, ci = cr[self.cls], ci[self.cls]
            yr += cr * sr - ci * si
            yi += cr * si + ci * sr
        return yr, yi

    def reference_torch(self, br, bi):
        """The same on the device of (br, bi), int64 tensors."""
        import torch
        assert br.dtype == torch.int64 and bi.dtype == torch.int64
        cls = torch.from_numpy(self.cls.astype(np.int64)).to(br.device)
        yr, yi = torch.zeros_like(br), torch.zeros_like(bi)
        for o, cr, ci in self._terms():
            sr, si = _shift_torch(br, o, self.nx), _shift_torch(bi, o, self.nx)
            cr = torch.from_numpy(cr).to(br.device)[cls]
            ci = torch.from_numpy(ci).to(br.device)[cls]
            yr += cr * sr - ci * si
            yi += cr * si + ci * sr
        return yr, yi

    # ------------------------------------------------------------------ for cfp_plan_apply_ex
    def stencil_dev(self, dev, cls_x: bool = False):
        """The `stencil` argument of CirculantPlan.apply_ex, with the [nx] class bytes as well
        when cls_x (by_x cases only)."""
        import torch
        st = (torch.from_numpy(self.cls).to(dev), torch.from_numpy(self.mask).to(dev),
              torch.from_numpy(np.ascontiguousarray(self.tab).reshape(-1)).to(dev), list(self.offsets), self.x_local)
        if cls_x:
            assert self.by_x
            st = st + (torch.from_numpy(self.cls_x).to(dev),)
        return st


def _shift_np(v, o, nx):
    """s[i] = v[i + o]: along the row for |o| < nx (zero outside the row), else of the flat vector."""
    s = np.zeros_like(v)
    if abs(o) < nx:
        s2, v2 = s.reshape(-1, nx), v.reshape(-1, nx)
        if o >= 0:
            s2[:, :nx - o] = v2[:, o:]
        else:
            s2[:, -o:] = v2[:, :nx + o]
    elif abs(o) < v.size:
        if o >= 0:
            s[:v.size - o] = v[o:]
        else:
            s[-o:] = v[:v.size + o]
    return s


def _shift_torch(v, o, nx):
    import torch
    s = torch.zeros_like(v)
    if abs(o) < nx:
        s2, v2 = s.view(-1, nx), v.view(-1, nx)
        if o >= 0:
            s2[:, :nx - o] = v2[:, o:]
        else:
            s2[:, -o:] = v2[:, :nx + o]
    elif abs(o) < v.numel():
        if o >= 0:
            s[:v.numel() - o] = v[o:]
        else:
            s[-o:] = v[:v.numel() + o]
    return s


# --------------------------------------------------------------------------- values
def _rng(name):
    return np.random.default_rng(zlib.crc32(("stencil/" + name).encode()))


def _coefs(rng, shape, kind):
    """Gaussian integers, |re|, |im| <= 4, no entry zero.  kind 'real': im = 0; 'complex': any im;
    'strict': re != 0, im != 0 and |re| != |im|."""
    re = rng.integers(1, 5, size=shape) * rng.choice([-1, 1], size=shape)
    if kind == "real":
        return re.astype(np.complex128)
    if kind == "complex":
        return re + 1j * rng.integers(-4, 5, size=shape)
    im = rng.integers(1, 4, size=shape)           # 1..3, moved past |re|: 1..4 without |re|
    im = im + (im >= np.abs(re))
    return re + 1j * im * rng.choice([-1, 1], size=shape)


def _distinct(rng, ncls, nd, kind):
    """ncls pairwise different coefficient rows."""
    rows = np.unique(_coefs(rng, (64 * ncls + 256, nd), kind), axis=0)
    assert len(rows) >= ncls, "not enough distinct coefficient rows"
    return rows[rng.permutation(len(rows))[:ncls]]


def _bits(offsets, kept):
    return sum(1 << k for k, o in enumerate(offsets) if o in kept)


def integer_vector(n, seed=20251019):
    """(br, bi) int64 with |.| <= 8."""
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, size=n, dtype=np.int64), rng.integers(-8, 9, size=n, dtype=np.int64)


# --------------------------------------------------------------------------- the cases
def _xyz(dims):
    nx, ny, nz = dims
    i = np.arange(nx * ny * nz, dtype=np.int64)
    return i % nx, (i // nx) % ny, i // (nx * ny)


def _ends(dims, offsets, kind, rng, why, name):
    """Classes by x: the rows at x = 0 drop the negative offsets, those at x = nx - 1 the positive
    ones, the interior keeps all -- the transport operator's shape."""
    nx = dims[0]
    x, _, _ = _xyz(dims)
    tab = _distinct(rng, 3, len(offsets), kind)
    mask = [_bits(offsets, [o for o in offsets if o >= 0]), _bits(offsets, offsets),
            _bits(offsets, [o for o in offsets if o <= 0])]
    cls = np.where(x == 0, 0, np.where(x == nx - 1, 2, 1))
    if min(offsets) >= 0:
        cls = np.where(cls == 0, 1, cls)   # nothing to drop at x = 0: the interior class
    if max(offsets) <= 0:
        cls = np.where(cls == 2, 1, cls)
    return Stencil(name, dims, offsets, mask, tab, cls, True, True, 1, why)


def make(name: str, dims) -> Stencil:
    nx, ny, nz = dims
    n = nx * ny * nz
    rng = _rng(name)
    x, y, z = _xyz(dims)
    row = y + ny * z
    if name == "up_pos":
        return _ends(dims, [-1, 0], "real", rng, "the control: config 3's shape, lower neighbour only (hm)", name)
    if name == "up_neg":
        return _ends(dims, [0, 1], "real", rng, "upper neighbour only (hp): negative velocity along x", name)
    if name == "centered":
        return _ends(dims, [-1, 0, 1], "real", rng, "nd = 3: both neighbours, three classes by x", name)
    if name == "diag_only":
        return Stencil(name, dims, [0], [1], _distinct(rng, 1, 1, "real"), np.zeros(n, np.int64), True, True, 1,
                       "nd = 1, one class: no neighbour, no edge load")
    if name == "diag16":
        return Stencil(name, dims, [0], [1] * 16, _distinct(rng, 16, 1, "complex"), (x + 5 * row) % 16, True, False, 1,
                       "nd = 1, 16 classes that change with x, y and z")
    if name == "no_diag":
        return _ends(dims, [-1, 1], "complex", rng, "no main diagonal: the centre slot is empty in every class", name)
    if name == "lower_only":
        return _ends(dims, [-1], "complex", rng, "nd = 1 at offset -1: an empty row at x = 0", name)
    if name == "upper_only":
        return _ends(dims, [1], "complex", rng, "nd = 1 at offset +1: an empty row at x = nx - 1", name)
    if name == "edges":
        # columns 0, nx - 1, x = 0 and x = 31 (mod 32) -- the lanes that take their neighbour from
        # the edge slots -- hold coefficients no other column has; 12 more classes cycle over the rest
        offs = [-1, 0, 1]
        tab = _distinct(rng, 16, 3, "complex")
        mask = [_bits(offs, [0, 1]), _bits(offs, [-1, 0])] + [7] * 14
        cls = 4 + x % 12
        cls = np.where(x % 32 == 0, 2, np.where(x % 32 == 31, 3, cls))
        cls = np.where(x == 0, 0, np.where(x == nx - 1, 1, cls))
        return Stencil(name, dims, offs, mask, tab, cls, True, True, 1,
                       "16 classes by x; the wave-edge columns and the row ends have coefficients of their own")
    if name == "per_point16":
        offs = [-1, 0, 1]
        mask = np.array([7, 7, 7, 7, 6, 6, 6, 3, 3, 3, 5, 5, 2, 2, 4, 1], dtype=np.uint8)  # bit k: offs[k]
        tab = _distinct(rng, 16, 3, "complex")
        first = np.flatnonzero((mask & 1) == 0)   # classes without -1: the rows at x = 0
        last = np.flatnonzero((mask & 4) == 0)    # classes without +1: the rows at x = nx - 1
        cls = rng.integers(0, 16, size=n)
        cls = np.where(x == 0, first[rng.integers(0, len(first), size=n)], cls)
        cls = np.where(x == nx - 1, last[rng.integers(0, len(last), size=n)], cls)
        return Stencil(name, dims, offs, mask, tab, cls, True, False, 1,
                       "16 classes drawn per point; interior classes drop -1, 0 or +1")
    if name == "complex_coef":
        return _ends(dims, [-1, 0, 1], "strict", rng,
                     "every coefficient with re != 0, im != 0, |re| != |im|: the signs of the two fma chains", name)
    if name == "stored_zero":
        offs = [-1, 0, 1]
        tab = _distinct(rng, 3, 3, "complex")
        tab[1, 2] = 0   # the interior stores a zero at +1
        tab[2, 0] = 0   # the last column stores a zero at -1
        cls = np.where(x == 0, 0, np.where(x == nx - 1, 2, 1))
        return Stencil(name, dims, offs, [6, 7, 3], tab, cls, True, True, 1, "a mask bit set with coefficient 0")
    if name == "cls17":
        offs = [-1, 0, 1]
        tab = _distinct(rng, 17, 3, "complex")
        mask = [_bits(offs, [0, 1])] + [7] * 15 + [_bits(offs, [-1, 0])]
        cls = np.where(x == 0, 0, np.where(x == nx - 1, 16, 1 + (x + 7 * row) % 15))
        return Stencil(name, dims, offs, mask, tab, cls, True, False, 0, "17 classes: one more than the fused table")
    if name == "wide":
        offs = [-2, 0, 1]
        tab = _distinct(rng, 3, 3, "complex")
        cls = np.where(x < 2, 0, np.where(x == nx - 1, 2, 1))
        return Stencil(name, dims, offs, [6, 7, 3], tab, cls, True, True, 0, "offset -2: x-local, but not a neighbour")
    if name == "y_coupled":
        offs = [-1, 0, nx]
        tab = _distinct(rng, 4, 3, "complex")
        # x = 0 drops -1, the last row of the grid drops +nx
        end = (row == ny * nz - 1)
        cls = np.where(x == 0, 0, 1) + 2 * end
        return Stencil(name, dims, offs, [6, 7, 2, 3], tab, cls, False, False, 0, "an offset of nx: not x-local")
    raise KeyError(name)


FUSED = ("up_pos", "up_neg", "centered", "diag_only", "diag16", "no_diag", "lower_only", "upper_only", "edges",
         "per_point16", "complex_coef", "stored_zero")
UNFUSED = ("cls17", "wide", "y_coupled")
NAMES = FUSED + UNFUSED
# at a grid of 256 columns or more these hold as many classes as their names say
FULL_NCLS = {"diag16": 16, "edges": 16, "per_point16": 16, "cls17": 17}
# the classes depend on x alone: PetscMiniMatAIJGetDia hands the PCSHELL a cls_x for these
BY_X = ("up_pos", "up_neg", "centered", "diag_only", "no_diag", "lower_only", "upper_only", "edges", "complex_coef",
        "stored_zero", "wide")
