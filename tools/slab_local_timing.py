#!/usr/bin/env python3
"""Local pass time per rank of the z-slab plan (GPU only): rank 0 of P ranks runs the kernel
steps of its step list on one stream, exchanges skipped (they are timed by bench.py --gpus N on
a real node).  For each schedule and pipeline depth K (pieces) it reports the local kernel time
split into the forward part (before the first exchange piece), the middle (z) and the backward
part, and a model of the whole apply over xGMI: one link of ~150 GB/s per peer (7 links on an
8-GPU node), each all-to-all moving 16 N/P (P-1)/P bytes out of every GPU.

  unpipelined (K = 1):  fwd + X + mid + X + bwd
  pipelined  (K > 1):   max(fwd, X) + min(fwd, X)/K + mid + max(bwd, X) + min(bwd, X)/K
                        (X: one all-to-all; the first / last piece cannot overlap)

    python tools/slab_local_timing.py [--grid 512] [--ranks 2 4 8] [--pieces 1 4 8] [--iters 20] [--lib SO]
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import circulantpreconditioner_amd as cp  # noqa: E402
from circulantpreconditioner_amd._lib import check, lib  # noqa: E402
from circulantpreconditioner_amd.distributed import STEP_KEYS, slab_layout  # noqa: E402

LINK_GBS = 150.0


def steps_of(h):
    n = ctypes.c_int()
    check(lib().cfp_dist_plan_num_steps(h, ctypes.byref(n)))
    out = []
    for i in range(n.value):
        d = (ctypes.c_int64 * len(STEP_KEYS))()
        check(lib().cfp_dist_plan_step(h, i, d))
        out.append(dict(zip(STEP_KEYS, list(d))))
    return out


def mid_ab(a, lam, mu):
    """--mid: the 3-sweep middle sweep (segment 1, one piece: the z-pencil block is x) of rank 0 of
    P with each middle kernel in turn, alternating over --rounds; one JSON line per P with the
    kernel each mode launched and its time per round in us."""
    import json
    if mu is None:
        sys.exit("--mid needs --mu (the recurrence serves the advection-diffusion symbol)")
    n = a.grid
    modes = {"auto": 0, "fft": 1, "rec": 2}
    for P in a.ranks:
        loc = slab_layout((n, n, n), P, 0)["local_size"]
        x = torch.empty(loc, dtype=torch.complex128, device="cuda")
        w, w2 = torch.empty_like(x), torch.empty_like(x)
        h = ctypes.c_void_p()
        check(lib().cfp_dist_plan_create_external(ctypes.byref(h), n, n, n, P, 0, 0))
        check(lib().cfp_dist_plan_set_work_buffers(h, w.data_ptr(), w2.data_ptr()))
        check(lib().cfp_dist_plan_set_schedule(h, 2))
        check(lib().cfp_dist_plan_set_pieces(h, 1))
        check(lib().cfp_dist_plan_set_symbol_advdiff(h, lam, mu))
        idx = [i for i, d in enumerate(steps_of(h)) if d["kind"] != 1 and d["seg"] == 1]
        s = torch.cuda.current_stream()
        kinds, us = {}, {m: [] for m in a.mid}
        for _ in range(a.rounds):
            for m in a.mid:
                check(lib().cfp_dist_plan_set_mid_kernel(h, modes[m]))
                k = ctypes.c_int()
                check(lib().cfp_dist_plan_mid_kernel(h, ctypes.byref(k)))
                kinds[m] = "zrec2" if k.value == 2 else "fft"

                def run():
                    for i in idx:
                        check(lib().cfp_dist_plan_run_step(h, i, x.data_ptr(), x.data_ptr(),
                                                           ctypes.c_void_p(s.cuda_stream)))
                cp.fill_uniform(x, 3)  # (the sweep is in place and unnormalised: fresh values per block)
                for _ in range(3):
                    run()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    run()
                e1.record()
                torch.cuda.synchronize()
                us[m].append(round(e0.elapsed_time(e1) / a.iters * 1e3, 2))
        print(json.dumps({"grid": n, "P": P, "lam": list(a.lam), "mu": list(a.mu), "iters": a.iters,
                          "kernel": kinds, "mid_us": us}), flush=True)
        check(lib().cfp_dist_plan_destroy(h))
        del x, w, w2
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--ranks", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--pieces", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of libcirculant_fft.so (A/B of two builds)")
    ap.add_argument("--lam", type=float, nargs=3, default=[0.6, 0.15, 0.02], help="lambda per axis")
    ap.add_argument("--mu", type=float, nargs=3, default=None,
                    help="mu per axis: the advection-diffusion symbol instead of the transport one")
    ap.add_argument("--mid", nargs="+", choices=["auto", "fft", "rec"], default=None,
                    help="A/B of the 3-sweep middle kernel (needs --mu): the kinds alternate over --rounds")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.lib:
        import circulantpreconditioner_amd._lib as Lib
        Lib.LIB_PATH = os.path.abspath(a.lib)
    n = a.grid
    lam = (ctypes.c_double * 6)(*[v for t in a.lam for v in (t, 0.0)])
    mu = (ctypes.c_double * 6)(*[v for t in a.mu for v in (t, 0.0)]) if a.mu else None
    if a.mid:
        mid_ab(a, lam, mu)
        return
    for P in a.ranks:
        L = slab_layout((n, n, n), P, 0)
        loc = L["local_size"]
        b = torch.empty(loc, dtype=torch.complex128, device="cuda")
        cp.fill_uniform(b, 3)
        x = torch.empty_like(b)
        w, w2 = torch.empty_like(b), torch.empty_like(b)
        h = ctypes.c_void_p()
        check(lib().cfp_dist_plan_create_external(ctypes.byref(h), n, n, n, P, 0, 0))
        check(lib().cfp_dist_plan_set_work_buffers(h, w.data_ptr(), w2.data_ptr()))
        if mu is not None:
            check(lib().cfp_dist_plan_set_symbol_advdiff(h, lam, mu))
        else:
            check(lib().cfp_dist_plan_set_symbol_transport(h, lam))
        links = max(1, min(P - 1, 7))
        x_us = 16 * loc * (P - 1) / P / (links * LINK_GBS * 1e9) * 1e6  # one all-to-all
        for name, sched in (("three", 2), ("five", 1)):
            if lib().cfp_dist_plan_set_schedule(h, sched) != 0:
                continue
            for K in a.pieces:
                if lib().cfp_dist_plan_set_pieces(h, K) != 0:
                    continue
                st = steps_of(h)
                s = torch.cuda.current_stream()
                seg_t = []
                for seg in (0, 1, 2):
                    idx = [i for i, d in enumerate(st) if d["kind"] != 1 and d["seg"] == seg]

                    def run():
                        for i in idx:
                            check(lib().cfp_dist_plan_run_step(h, i, b.data_ptr(), x.data_ptr(),
                                                               ctypes.c_void_p(s.cuda_stream)))
                    for _ in range(3):
                        run()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        run()
                    e1.record()
                    torch.cuda.synchronize()
                    seg_t.append(e0.elapsed_time(e1) / a.iters * 1e3)
                fwd, mid, bwd = seg_t
                if K == 1:
                    model = fwd + x_us + mid + x_us + bwd
                else:
                    model = max(fwd, x_us) + min(fwd, x_us) / K + mid + max(bwd, x_us) + min(bwd, x_us) / K
                print(f"{n}^3 P={P} {name} K={K}: local kernels fwd {fwd:.1f} + mid {mid:.1f} + bwd {bwd:.1f} = "
                      f"{fwd + mid + bwd:.1f} us; all-to-all model {x_us:.1f} us ({links} x {LINK_GBS:.0f} GB/s); "
                      f"apply model {model:.1f} us = {1e6 / model:.0f} PCApply/s", flush=True)
        check(lib().cfp_dist_plan_destroy(h))
        del b, x, w, w2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
