"""The axis lengths and grid positions of test_mixed_axis_gpu.py, with the class of the LDS
mixed-radix pass (k_axis_mixed) each one is meant to reach, and a Python restatement of the
geometry rule of that pass.  test_mixed_class_cpu.py checks both against the library's own report
(cfp_mixed_pass_class), so the GPU file's coverage claim is proved, not assumed."""

THREADS, POINTS, MAXPTS = 256, 2048, 2048      # workgroup size, target and in-place limit of points per block
TW_LDS_LIMIT = 96 * 1024                       # buffers + twiddle table up to here: the table goes to LDS
MAX_LDS = 160 * 1024 - 1024                    # the CU's LDS less the kernel's static base tables
REGISTER_LENGTHS = (16, 32, 64, 128, 256, 512, 1024, 10, 20, 50, 100, 200)  # served by the register pass

# class -> lengths.  Every class holds for every position below (1, 3, 5 or 6 columns).
LENGTHS = {
    # in-place stages, twiddles in LDS: each specialised radix alone and stacked
    "inplace": [2, 4, 8, 6, 9, 15, 21, 35, 49, 63, 105, 125, 343, 1536, 2000, 2048],
    # register-table lengths that the fast path refuses at these column counts (ncols % T != 0)
    "refused": [64, 256, 1024],
    # ping-pong forced by a prime factor above 7 (a direct-sum stage behind each specialised radix:
    # 2.11, 3.11, 4.11, 5.11, 7.11, 8.11; two in a row: 11.11, 11.13, 7.11.13, 3.11.31, 23.89;
    # three: 11^3), the block within 2,048 points, twiddles in LDS
    "pingpong_prime": [22, 33, 44, 55, 77, 88, 121, 143, 1001, 1023, 1331, 2047],
    # ping-pong forced by the block's size (above 2,048 points), twiddles read from global memory:
    # 3.683, 3^7, 7^4, 8.8.8.5, 8.3.5^3, 5^5, 3^2.5.7.13, 8^4 and the prime 4093
    "pingpong_size": [2049, 2187, 2401, 2560, 3000, 3125, 4095, 4096, 4093],
}
ALL_LENGTHS = [(cls, n) for cls, ns in LENGTHS.items() for n in ns]

# (name, grid of length n, axis of the pass under test, its modes in plan.passes(), ncols, row mode)
POSITIONS = [
    ("x_fused", lambda n: (n, 1, 1), "x", ("fused",), 1, True),
    ("x_fwd_inv", lambda n: (n, 3, 1), "x", ("fwd", "inv"), 3, True),
    ("y_fused_3", lambda n: (3, n, 1), "y", ("fused",), 3, False),    # G = 2 where n <= 1024: a partial last block
    ("y_fused_5", lambda n: (5, n, 1), "y", ("fused",), 5, False),    # G = 4 where n <= 512: a partial last block
    ("y_fwd_inv", lambda n: (3, n, 2), "y", ("fwd", "inv"), 6, False),  # inner_n = 3
    ("z_fused", lambda n: (2, 3, n), "z", ("fused",), 6, False),
]
POSITION = {p[0]: p for p in POSITIONS}


def factorize(n):
    """The stage radices in order: 8s, then 4, 2, 3, 5, 7, then the primes above 7 ascending."""
    fac = []
    while n % 8 == 0 and n > 1:
        fac.append(8)
        n //= 8
    for r in (4, 2, 3, 5, 7):
        while n % r == 0 and n > 1:
            fac.append(r)
            n //= r
    p = 11
    while n > 1:
        while n % p == 0:
            fac.append(p)
            n //= p
        if p * p > n and n > 1:
            fac.append(n)
            n = 1
        p += 2
    return fac


def _pow2_floor(g):
    q = 1
    while q * 2 <= g:
        q *= 2
    return q


def rule(n, ncols, row, wave_ncomp=0):
    """The geometry of the mixed pass restated: the dict plan.mixed_pass_class returns, or None
    where the launch refuses the shape."""
    if not 1 <= n <= 4096:
        return None
    G = max(1, min(64, POINTS // n))
    if not row:
        G = _pow2_floor(G)
    if G > ncols:
        G = ncols if row else _pow2_floor(ncols)
    if wave_ncomp:
        if not 2 <= wave_ncomp <= 4 or ncols % wave_ncomp:
            return None
        if wave_ncomp == 3:
            q = 3
            while q * 2 <= G:
                q *= 2
            G = q
        else:
            G = max(G, wave_ncomp) & ~(wave_ncomp - 1)
    fac = factorize(n) if n > 1 else []
    L = n if row else n + 1
    pingpong = any(f > 8 for f in fac) or G * n > MAXPTS
    nbuf = 2 if pingpong or wave_ncomp else 1
    lds = nbuf * G * L * 16
    tw_lds = lds + 16 * n <= TW_LDS_LIMIT
    if tw_lds:
        lds += 16 * n
    if lds > MAX_LDS:
        return None
    pts = G * n
    return {"G": G, "pingpong": pingpong, "tw_lds": tw_lds, "U": 2 if pts <= 2 * THREADS else (4 if pts <= 4 * THREADS else 8),
            "lds_bytes": lds, "radices": fac}


def in_class(cls, n, c):
    """Whether the geometry report c of length n is the class `cls` of LENGTHS."""
    prime_stage = any(r > 8 for r in c["radices"])
    if cls == "inplace":
        return not c["pingpong"] and not prime_stage and c["tw_lds"] and n not in REGISTER_LENGTHS
    if cls == "refused":
        return not c["pingpong"] and not prime_stage and c["tw_lds"] and n in REGISTER_LENGTHS
    if cls == "pingpong_prime":
        return c["pingpong"] and prime_stage and c["tw_lds"] and c["G"] * n <= MAXPTS
    if cls == "pingpong_size":
        return c["pingpong"] and c["G"] * n > MAXPTS and not c["tw_lds"]
    raise KeyError(cls)
