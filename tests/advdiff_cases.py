"""Shared numpy restatements for the advection-diffusion tests (test_advdiff_cpu.py,
test_advdiff_gpu.py, test_diffusion_gpu.py): the closed-form symbol, its z factorisation, a model
of the two-sided recurrence kernel's algorithm, and a dense operator.

Symbol, per axis d with w = e^{-2 pi i k/n}:  lam_d (1 - w) + mu_d (2 - w - conj(w)), 0 for n = 1;
Diag = 1 + the sum over the axes.  Along z, with c = 1 + s_x + s_y, p = lam_z + mu_z, q = mu_z and
d = c + p + q:  d - p e^{-i t} - q e^{i t} = beta (1 - a e^{-i t}) (1 - b e^{i t}), beta the root
of beta^2 - d beta + p q = 0 of larger modulus, a = p / beta, b = q / beta."""
import numpy as np

EPS = 2.2e-16

# (lam, mu) per axis; every one is eligible for the two-sided recurrence at 256^3
ELIGIBLE = {
    "diff_small": ((0, 0, 0), (0.05, 0.05, 0.05)),
    "diff1000": ((0, 0, 0), (0.3, 0.3, 1000)),
    "advdiff": ((0.6, 0.15, 0.6), (0.2, 0.2, 2.5)),
    "complex": ((0.3 + 0.2j, 1.1, 0.3 + 0.2j), (0.1, 0.1, 0.7 - 0.1j)),
    "downwind": ((0.6, 0.15, -0.4), (0, 0, 3.0)),
}

# one z column (c, lam_z, mu_z): the cases the recurrence model was checked on
COLUMNS = {
    "pure_diffusion": (1, 0, 0.05),
    "mu1000": (1, 0, 1000),
    "mu16000": (1, 0, 16000),
    "advdiff": (1 + 0.3j, 0.6, 2.5),
    "complex": (1.2 - 0.4j, 0.3 + 0.2j, 0.7 - 0.1j),
    "downwind": (1, -0.4, 3.0),
}


def symbol_1d(n, lam, mu):
    if n == 1:
        return np.zeros(1, dtype=np.complex128)
    w = np.exp(-2j * np.pi * np.arange(n) / n)
    return complex(lam) * (1 - w) + complex(mu) * (2 - w - np.conj(w))


def diag(dims, lam, mu):
    """Diag as a flat array, x fastest."""
    nx, ny, nz = dims
    sx, sy, sz = (symbol_1d(n, l, m) for n, l, m in zip(dims, lam, mu))
    return (1 + sx[None, None, :] + sy[None, :, None] + sz[:, None, None]).reshape(-1)


def z_factors(c, lz, mz):
    """(beta, a, b) of columns with c = 1 + s_x + s_y (array or scalar)."""
    c = np.asarray(c, dtype=np.complex128)
    p, q = complex(lz) + complex(mz), complex(mz)
    d = c + p + q
    s = np.sqrt(d * d - 4 * p * q)
    b1, b2 = (d + s) / 2, (d - s) / 2
    beta = np.where(np.abs(b1) >= np.abs(b2), b1, b2)
    return beta, p / beta, q / beta


def z_ratios(nx, ny, lam, mu):
    """Brute force over all columns: (max |a|, max |b|)."""
    sx, sy = symbol_1d(nx, lam[0], mu[0]), symbol_1d(ny, lam[1], mu[1])
    c = 1 + sx[None, :] + sy[:, None]
    _, a, b = z_factors(c, lam[2], mu[2])
    return float(np.abs(a).max()), float(np.abs(b).max())


def bound(ra, rb):
    """The recurrence's bar: 8 eps / (1 - |a|) once per scan direction."""
    return 8 * EPS / ((1 - ra) * (1 - rb))


def kernel_model(v, c, lz, mz, nblk=16):
    """The two-sided recurrence kernel's algorithm on one z column v (length nblk * 16): 16 blocks
    of 16, local forward scans, block-end carries by Horner in a^16 with the cyclic closure, then
    local backward scans, block-start carries by Horner in b^16 with its closure."""
    n = v.size
    m = n // nblk
    beta, a, b = (complex(t) for t in z_factors(c, lz, mz))
    r = n / beta
    s = v.astype(np.complex128).reshape(nblk, m).copy()
    for j in range(1, m):
        s[:, j] += a * s[:, j - 1]
    E = r * s[:, m - 1]
    A = a ** m
    t = np.empty_like(s)
    for w in range(nblk):
        acc = E[w]
        for k in range(nblk - 2, -1, -1):
            acc = acc * A + E[(w - 1 - k) % nblk]
        cin = acc / (1 - A ** nblk)
        t[w] = r * s[w] + a ** np.arange(1, m + 1) * cin
    for j in range(m - 2, -1, -1):
        t[:, j] += b * t[:, j + 1]
    F = t[:, 0].copy()
    B = b ** m
    u = np.empty_like(t)
    for w in range(nblk):
        acc = F[w]
        for k in range(nblk - 2, -1, -1):
            acc = acc * B + F[(w + 1 + k) % nblk]
        cib = acc / (1 - B ** nblk)
        u[w] = t[w] + b ** np.arange(m, 0, -1) * cib
    return u.reshape(-1)


def column_reference(v, c, lz, mz):
    """The unnormalised pair's "z DFT, divide, inverse z DFT": n * ifft(fft(v) / Diag)."""
    n = v.size
    return n * np.fft.ifft(np.fft.fft(v) / (complex(c) + symbol_1d(n, lz, mz)))


def dense_operator(dims, h, dt, a, nu, periodic, shift=0.0):
    """shift I + dt (upwind advection, conservative sign, + centred 7-point diffusion); wall: the
    border faces are skipped.  Row = cell i + nx (j + ny k)."""
    nx, ny, nz = dims
    N = nx * ny * nz
    A = np.zeros((N, N))
    stride = (1, nx, nx * ny)
    for cell in range(N):
        idx = (cell % nx, (cell // nx) % ny, cell // (nx * ny))
        A[cell, cell] += shift
        for d in range(3):
            if dims[d] == 1 and periodic:
                continue  # a periodic axis of one cell: the neighbour is the cell itself, net 0
            for s in (-1, 1):
                j = idx[d] + s
                if j < 0 or j >= dims[d]:
                    if not periodic:
                        continue
                    j %= dims[d]
                nb = cell + (j - idx[d]) * stride[d]
                un = s * a[d]
                adv = dt / h[d]
                if un > 0:
                    A[cell, cell] += adv * un
                else:
                    A[cell, nb] += adv * un
                dif = nu * dt / h[d] ** 2
                A[cell, cell] += dif
                A[cell, nb] -= dif
    return A


def apply_operator(U, dims, h, dt, a, nu, periodic):
    """(I + dt L) U without a matrix, by slices: per axis and face, the upwind advection flux
    difference (conservative sign) and the diffusion difference; wall: border faces are skipped."""
    nx, ny, nz = dims
    u = np.asarray(U).reshape(nz, ny, nx)
    y = u.copy()
    for d, ax in enumerate((2, 1, 0)):  # x is the fastest axis = the last dim
        n = dims[d]
        if n == 1:
            continue
        adv, dif = a[d] * dt / h[d], nu * dt / h[d] ** 2
        for s in (-1, 1):
            nb = np.roll(u, -s, axis=ax)  # the neighbour at index + s
            un = s * adv
            t = dif * (u - nb) + (un * u if un > 0 else un * nb)
            if not periodic:  # no face beyond the first / last cell
                sl = [slice(None)] * 3
                sl[ax] = 0 if s == -1 else n - 1
                t[tuple(sl)] = 0
            y = y + t
    return y.reshape(-1)
