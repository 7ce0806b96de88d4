#!/usr/bin/env python3
"""The real-data wave plan against the complex wave plan, in one process (GPU only; measurement
tool): at 128^3 and at the 2-D grid 1024^2 it times, alternating over the rounds after a warm-up,

    complex5   WavePlan on the five-pass schedule (complex b)
    complex3   WavePlan on the 3-sweep schedule (128^3 only)
    real_es1   RealWavePlan on float64 b
    real_es2   RealWavePlan on the real parts of complex b

and prints applies/s (median over the rounds) with the spread (max - min over the median) of
each, the per-launch device times of the real plan and of the complex five-pass plan (events
between the launches), the algorithmic bytes per apply and the agreement of the results.

    python tools/ab_wave_real.py [--rounds 7] [--seconds 0.4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.getcwd()
sys.path.insert(0, ROOT)
KAPPA = (0.079, 0.079, 0.079)


def rate(fn, seconds, torch):
    """applies/s of fn over a window of at least `seconds`, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, reps = 0, 16
    e0.record()
    while True:
        for _ in range(reps):
            fn()
        n += reps
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1e3 * seconds:
            return 1e3 * n / ms
        reps = min(4 * reps, 1024)


def grid(dims, dim, rounds, seconds):
    import torch
    from circulantpreconditioner_amd import wave as W
    C = dim + 1
    cells = 1
    for v in dims:
        cells *= v
    kappa = KAPPA if dim == 3 else (KAPPA[0], KAPPA[1], 0.0)
    g = torch.Generator(device="cuda").manual_seed(20251017)
    br = torch.randn(C * cells, dtype=torch.float64, device="cuda", generator=g)
    bc = br.to(torch.complex128)
    xr, xc, xc3, xs = torch.empty_like(br), torch.empty_like(bc), torch.empty_like(bc), torch.empty_like(bc)
    rp = W.RealWavePlan(dims, dim=dim).set_symbol(kappa)
    c5 = W.WavePlan(dims, dim=dim).set_symbol(kappa).set_schedule("five")
    variants = {"complex5": lambda: c5.apply(bc, out=xc),
                "real_es1": lambda: rp.apply(br, out=xr),
                "real_es2": lambda: rp.apply(bc, out=xs)}
    if dims == (128, 128, 128):
        c3 = W.WavePlan(dims, dim=dim).set_symbol(kappa).set_schedule("three")
        variants["complex3"] = lambda: c3.apply(bc, out=xc3)
    for fn in variants.values():  # warm-up: code objects, clocks
        rate(fn, 0.3, torch)
    runs = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            runs[k].append(rate(fn, seconds, torch))
    out = {"grid": list(dims), "dim": dim, "rounds": rounds, "window_s": seconds, "variants": {}}
    for k, v in runs.items():
        med = statistics.median(v)
        out["variants"][k] = {"applies_per_s": round(med, 1), "spread": round((max(v) - min(v)) / med, 4),
                              "min": round(min(v), 1), "max": round(max(v), 1)}
    # bytes the algorithm moves per apply: 80 C / 96 C per cell (real, es = 1 / 2), 160 C (complex, five passes)
    out["bytes_per_apply"] = {"real_es1": 80 * C * cells, "real_es2": 96 * C * cells, "complex5": 160 * C * cells}
    out["real_pass_ms"] = {"es1": [round(v, 5) for v in rp.time_passes(br, xr, iters=50)],
                           "es2": [round(v, 5) for v in rp.time_passes(bc, xs, iters=50)]}
    out["complex5_pass_ms"] = [round(v, 5) for v in c5.time_passes(bc, xc, iters=50)]
    nrm = torch.linalg.vector_norm(xc.real)
    out["rel_diff_real_vs_complex5"] = float(torch.linalg.vector_norm(xr - xc.real) / nrm)
    out["es2_equals_es1"] = bool(torch.equal(xs.real, xr) and not xs.imag.any())
    out["real_over_complex5"] = round(out["variants"]["real_es1"]["applies_per_s"]
                                      / out["variants"]["complex5"]["applies_per_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least 5 rounds")
    import torch
    if not torch.cuda.is_available():
        sys.exit("ab_wave_real.py needs a GPU")
    res = [grid((128, 128, 128), 3, a.rounds, a.seconds), grid((1024, 1024), 2, a.rounds, a.seconds)]
    txt = "\n".join(json.dumps(r) for r in res)
    print(txt, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
