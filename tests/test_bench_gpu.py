"""bench.py's N > 1 launch on the GPU box: `bench.py --gpus 2` without a
launcher starts its two ranks itself and both drive the card (CFP_BENCH_SHARE_DEVICE=1, gloo
process group).  RCCL cannot put two ranks on one GPU, so the line carries the labelled
torch-fallback exchange; the apply's output check still runs on the device."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_gpus_2_self_launched_rehearsal():
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CFP_BENCH_SELF_LAUNCHED")}
    env.update({"CFP_BENCH_SHARE_DEVICE": "1", "CFP_BENCH_BACKEND": "gloo"})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--grid", "64", "--full",
                        "--scaling-grid", "0", "--no-configs", "--no-real", "--no-cpu-baseline", "--steps", "5",
                        "--warmup", "2", "--settle-ms", "0"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0, p.stderr[-4000:]
    assert len(lines) == 1
    ln = lines[0]
    assert ln["n_gpus"] == 2 and ln["status"] == "ok" and ln["launcher"] == "self (torch.distributed.run)"
    assert ln["check"]["ok"] and ln["check"]["residual"] < 1e-10
    assert ln["exchange"] in ("rccl", "torch-fallback") and "rccl" in ln["rccl"]["lib"]


def _plain(args, timeout=300):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CFP_BENCH_SELF_LAUNCHED")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return lines[0]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_apply(tmp_path, oracle):
    """A plain run times the headline and nothing else, and --dump-outputs writes the x of its last
    timed apply: float64 (re, im) pairs, the whole vector at this size, equal to the oracle's
    solve of the same seeded b to the suite's parity bar (1e-10)."""
    import numpy as np
    import bench

    n = (48, 40, 36)  # no axis a power of two: the mixed-radix passes
    d = tmp_path / "out"
    ln = _plain(["--gpus", "1", "--grid"] + [str(v) for v in n] +
                ["--steps", "3", "--warmup", "1", "--settle-ms", "0", "--dump-outputs", str(d)])
    assert ln["status"] == "ok" and ln["full"] is False and ln["steps"] == 3 and ln["warmup"] == 1
    assert ln["unit"] == "PCApply/s" and ln["higher_is_better"] is True and ln["dtype"].startswith("c128")
    assert ln["ms_per_step"] > 0 and ln["value"] == pytest.approx(1e3 / ln["ms_per_step"], rel=1e-3)
    # nothing beyond the headline ran
    assert ln["check"]["ok"] is None and ln["roofline"] is None and ln["cpu_baseline"] is None
    for key in ("real_variant", "other_configs", "scaling_512", "passes"):
        assert key not in ln
    assert sorted(os.listdir(d)) == ["x.npy"]
    x = np.load(d / "x.npy")
    N = n[0] * n[1] * n[2]
    assert x.dtype == np.float64 and x.shape == (N, 2)
    ref = oracle.c_solve_3d(oracle.c_build_diag_transport(n, bench.LAM), oracle.c_fill_uniform(N, bench.SEED), n)
    assert oracle.rel_l2(x[:, 0] + 1j * x[:, 1], ref) < 1e-10
