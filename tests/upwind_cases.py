"""Shared numpy restatements for the upwind-symbol tests (test_upwind_cpu.py, test_upwind_gpu.py,
test_upwind_mpi_gpu.py): the upwind closed form, the mapping onto the advection-diffusion pair, the
operator models and a model of the backward recurrence kernel's algorithm.

Symbol, per axis d with w = e^{-2 pi i k/n}:
    up_d + mu_d (2 - w - conj(w)),  up_d = lam_d (1 - w) for Re lam_d >= 0, (-lam_d) (1 - conj(w)) otherwise,
0 for n = 1; Diag = 1 + the sum over the axes.  A cell is coupled to index - 1 where the velocity
is positive and to index + 1 where it is negative, as the upwind operators are.  Since
    |lam| (1 - conj w) = lam (1 - w) + (-lam) (2 - w - conj w)   for lam < 0,
the pair (lam, mu - lam) in the advection-diffusion closed form gives the same symbol."""
import numpy as np

from advdiff_cases import apply_operator, dense_operator  # noqa: F401  (the operator models, either sign of a)

EPS = 2.2e-16

SIGNS = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
LAM0 = (0.6, 0.15, 0.4)
MUS = {"mu0": (0.0, 0.0, 0.0), "mu": (0.2, 0.2, 2.5)}


def signed(signs, lam=LAM0):
    return tuple(s * l for s, l in zip(signs, lam))


def upwind_symbol_1d(n, lam, mu=0.0):
    if n == 1:
        return np.zeros(1, dtype=np.complex128)
    w = np.exp(-2j * np.pi * np.arange(n) / n)
    lam, mu = complex(lam), complex(mu)
    up = lam * (1 - w) if lam.real >= 0 else (-lam) * (1 - np.conj(w))
    return up + mu * (2 - w - np.conj(w))


def literal_symbol_1d(n, lam, mu=0.0):
    """lam (1 - w) whatever the sign: for lam < 0 the implicit downwind scheme's symbol."""
    if n == 1:
        return np.zeros(1, dtype=np.complex128)
    w = np.exp(-2j * np.pi * np.arange(n) / n)
    return complex(lam) * (1 - w) + complex(mu) * (2 - w - np.conj(w))


def diag(dims, lam, mu=(0, 0, 0), sym=upwind_symbol_1d):
    """Diag as a flat array, x fastest."""
    sx, sy, sz = (sym(n, l, m) for n, l, m in zip(dims, lam, mu))
    return (1 + sx[None, None, :] + sy[None, :, None] + sz[:, None, None]).reshape(-1)


def mapped(lam, mu=(0, 0, 0)):
    """(lam, mu') with mu'_d = mu_d - lam_d where Re lam_d < 0."""
    lam = [complex(v) for v in lam]
    mu = [complex(v) for v in mu]
    return lam, [m - l if l.real < 0 else m for l, m in zip(lam, mu)]


def back_ratio(nx, ny, lam, mu=(0, 0, 0)):
    """max over the columns of |q / (1 + s_x + s_y + q)|, q = -lam_z: the backward recurrence's ratio."""
    sx, sy = upwind_symbol_1d(nx, lam[0], mu[0]), upwind_symbol_1d(ny, lam[1], mu[1])
    q = -complex(lam[2])
    return float(np.abs(q / (1 + sx[None, :] + sy[:, None] + q)).max())


def bound(amax):
    """tests/test_zrec_gpu.py's bar: 1e-13 between two schedules, 8 eps / (1 - amax) above amax = 0.5."""
    return 1e-13 if amax <= 0.5 else 8 * EPS / (1.0 - amax)


def forward_scan_model(v, a, r, nblk=16):
    """k_tp_mid_rec's algorithm on one z column: u_z = a u_{z-1} + r v_z, cyclic.  nblk blocks of m
    points: local scans from zero, the block-end values, the carry into each block by Horner in a^m
    with the cyclic closure 1 / (1 - a^n), then u_j = r s_j + a^{j+1} carry."""
    n = v.size
    m = n // nblk
    s = v.astype(np.complex128).reshape(nblk, m).copy()
    for j in range(1, m):
        s[:, j] += a * s[:, j - 1]
    E = r * s[:, m - 1]
    A = a ** m
    u = np.empty_like(s)
    for w in range(nblk):
        acc = E[w]
        for k in range(nblk - 2, -1, -1):
            acc = acc * A + E[(w - 1 - k) % nblk]
        cin = acc / (1 - A ** nblk)
        u[w] = r * s[w] + a ** np.arange(1, m + 1) * cin
    return u.reshape(-1)


def reversed_scan_model(v, c, q, nblk=16):
    """The backward kernel: the forward algorithm on the planes in reverse order.  Solves the cyclic
    u_z = a u_{z+1} + r v_z with a = q / (c + q), r = n / (c + q) (n: the factor the unnormalised
    transform pair leaves)."""
    n = v.size
    a, r = complex(q) / (complex(c) + complex(q)), n / (complex(c) + complex(q))
    return forward_scan_model(v[::-1], a, r, nblk)[::-1]


def column_reference(v, c, q):
    """n * ifft(fft(v) / Diag) for the column symbol c + q (1 - conj(w))."""
    n = v.size
    w = np.exp(-2j * np.pi * np.arange(n) / n)
    return n * np.fft.ifft(np.fft.fft(v) / (complex(c) + complex(q) * (1 - np.conj(w))))
