#!/usr/bin/env python3
"""Timing probes of the 512^3 (and 256^3) row sweeps P1 / P3 (rows_512.hip; GPU only, measurement tool).

    python tools/kexp/run_rows_512.py     # every sweep x probe, 3 interleaved rounds, min / median

ROWS_PROBES / ROWS_SWEEPS (comma-separated numbers) select probes and sweeps, ROWS_ROUNDS the rounds;
e.g. the 256^3 sweeps without and with the next unit's prefetch, all six cases:
    ROWS_SWEEPS=2,3 ROWS_PROBES=11,21,12,22,13,23,14,24,15,25,16,26 python tools/kexp/run_rows_512.py
"""
import ctypes
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
L = ctypes.CDLL(os.path.join(HERE, "rows_512.so"))
L.rows_512.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.POINTER(ctypes.c_float)]
SWEEPS = {0: ("P1", 512), 1: ("P3", 512), 2: ("P1", 256), 3: ("P3", 256)}
PROBES = {0: "product", 1: "no loads", 2: "no stores", 3: "arithmetic + exchanges alone", 4: "memory alone",
          5: "memory + transpose", 6: "product, z-major units", 7: "memory alone, z-major units",
          8: "product, XCD unit order", 9: "memory alone, XCD unit order",
          10: "memory alone, XCD, 1 WG per CU"}
# 256^3 only, XCD unit order: the plain sweeps (11-16) beside the prefetching ones (21-26), and the
# prefetching product with 4 .. 7 slots (34-37)
SIX = ("product", "memory alone", "memory + transpose", "no loads", "no stores", "arithmetic + exchanges alone")
PROBES.update({11 + i: "XCD " + s for i, s in enumerate(SIX)})
PROBES.update({21 + i: "XCD PF " + s for i, s in enumerate(SIX)})
PROBES.update({30 + k: "XCD PF product, %d slots" % k for k in (4, 5, 6, 7)})


def ONLY_256(p):
    return p >= 11


if os.environ.get("ROWS_PROBES"):
    PROBES = {int(p): PROBES[int(p)] for p in os.environ["ROWS_PROBES"].split(",")}
if os.environ.get("ROWS_SWEEPS"):
    SWEEPS = {int(s): SWEEPS[int(s)] for s in os.environ["ROWS_SWEEPS"].split(",")}
ROUNDS = int(os.environ.get("ROWS_ROUNDS", "3"))
bufs = {}
for n in sorted({n for _, n in SWEEPS.values()}, reverse=True):
    N = n ** 3
    bufs[n] = (torch.randn(N, dtype=torch.complex128, device="cuda"), torch.empty(N, dtype=torch.complex128, device="cuda"),
               torch.from_numpy(np.exp(-2j * np.pi * np.arange(n) / n)).to("cuda"))


def run(w, iters):
    n = SWEEPS[w % 10][1]
    b, x, tw = bufs[n]
    ms = ctypes.c_float()
    rc = L.rows_512(w, b.data_ptr(), x.data_ptr(), tw.data_ptr(), iters, ctypes.byref(ms))
    assert rc == 0, (w, rc)
    return ms.value * 1e3


res = {}
for rnd in range(ROUNDS):
    for s in SWEEPS:
        for p in PROBES:
            if ONLY_256(p) and SWEEPS[s][1] != 256:
                continue
            res.setdefault(10 * p + s, []).append(run(10 * p + s, 10 if SWEEPS[s][1] == 512 else 40))
for s, (name, n) in SWEEPS.items():
    for p, pname in PROBES.items():
        if 10 * p + s not in res:
            continue
        t = sorted(res[10 * p + s])
        print(f"{name} {n}^3 {pname:36s} min {t[0]:8.1f} us  med {t[len(t) // 2]:8.1f} us  "
              f"({32 * n ** 3 / (t[0] * 1e-6) / 1e12:5.2f} TB/s on 32 N)", flush=True)
