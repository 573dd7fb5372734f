"""bench.py's N > 1 path end to end on one GPU: ``--gpus 2 --same-gpu``
starts two ranks itself, both on device 0 (gloo + same-device xGMI mappings), and must print one
JSON line with ``n_gpus: 2``, the MNIST xGMI Adam step replica-verified, and the data-parallel
ResNet-50 step (ShardedMasterSGD, hipGraph) replica-verified as ``dp2``."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_two_ranks_same_gpu_end_to_end():
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env["PYTHONPATH"] = REPO
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--full", "--gpus", "2", "--same-gpu",
           "--steps", "60", "--warmup", "20", "--verify-every", "20",
           "--resnet-batch", "16", "--resnet-steps", "4", "--resnet-verify-every", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-4000:]
    (line,) = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert line["n_gpus"] == 2 and line["config"]["parallelism"] == "dp2", line
    assert line["config"]["launch"] == "bench.py" and "emulated" in line, line
    assert "comm=xgmi" in line["config"]["exec"], line
    assert line["replicas_verified"] > 0, line
    assert "resnet50_error" not in line, line
    rc = line["resnet50_config"]
    assert rc["parallelism"] == "dp2" and rc["replicas_verified"] > 0, line
    assert rc["comm"].startswith("xgmi-sharded-sgd"), line
    # north-star #2 rows: xGMI timed at every size, RCCL marked skipped under gloo
    ccl = line["ccl"]
    assert ccl["xgmi"]["form"] == "pull", ccl
    assert all(v == "ok" for v in ccl["xgmi"]["selftest"].values()), ccl
    assert {"allreduce_oneshot", "allreduce_twoshot", "adam", "sgd_bf16", "sgd_f32",
            "broadcast_direct", "allgather"} <= set(ccl["xgmi"]["selftest"]), ccl
    ops = [r["op"] for r in ccl["rows"]]
    assert ops.count("allreduce") == 5 and "sharded_sgd_bf16_bucket" in ops, ccl
    assert all("xgmi_us" in r and "rccl_us" not in r and "gloo" in r["rccl"]
               for r in ccl["rows"]), ccl


def test_bench_failed_resnet_fails_the_run():
    """A ResNet-50 failure at N > 1 is reported in the line AND exits non-zero."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env.update(PYTHONPATH=REPO, ARENA_BENCH_FAIL_RESNET="1")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--full", "--gpus", "2", "--same-gpu",
           "--steps", "20", "--warmup", "10", "--ccl", "0"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0, r.stdout[-2000:]
    (line,) = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert line["failed"] == ["resnet50"] and "injected" in line["resnet50_error"], line


def _plain_run(steps, out):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env["PYTHONPATH"] = REPO
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", "5", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-4000:]
    (line,) = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    import numpy as np
    return line, {p.stem: np.load(p) for p in out.glob("*.npy")}


def test_plain_bench_is_lean_and_dumps_outputs(tmp_path):
    """A plain run times only the MNIST headline (no ResNet-50 / collective keys without
    ``--full``) and reports ``ms_per_step`` for exactly ``--steps`` timed steps.
    ``--dump-outputs`` writes one step from the seeded start state as finite float32 ``.npy``
    arrays, the same whatever was timed before it: a second run with another step count agrees
    to within one step's float-atomic rounding (logits: 32 partial sums of magnitude <= 10 in any
    order, 32 * 2^-24 * 10 = 2e-5; hidden layer: no atomics; first Adam step: gradients follow
    the logits' 1e-6 relative error, m = 0.1 g, v = 0.001 g^2; where g is within its own noise,
    at most 2e-5 * 0.25 / 100 = 5e-8 per dz entry times a dim pixel's 0.02 = 1e-9, the update
    lr * g / (|g| + eps) moves by up to lr * 1e-9 / 1e-8 = 1e-4, a tenth of a step)."""
    import numpy as np
    line, arrays = _plain_run(20, tmp_path / "a")
    assert line["metric"] == "mnist_mlp_train_throughput" and line["steps"] == 20, line
    assert line["ms_per_step"] > 0 and "20/20 graph-replayed" in line["config"]["exec"], line
    assert not [k for k in line if k.startswith(("resnet50", "ccl"))], line
    assert {"params", "adam_m", "adam_v", "hidden", "logits", "loss", "correct"} == set(arrays)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["params"].shape == arrays["adam_m"].shape == (397512,)
    assert arrays["logits"].shape == (100, 10) and arrays["logits"].any()
    # the Adam step touched the moments of every weight whose input pixel is lit in the batch
    assert np.count_nonzero(arrays["adam_v"]) > 50000
    assert 0 < float(arrays["loss"][0]) < 10
    line2, again = _plain_run(40, tmp_path / "b")
    assert line2["steps"] == 40 and "40/40 graph-replayed" in line2["config"]["exec"], line2
    tol = {"hidden": (0, 1e-6), "logits": (0, 2e-5), "loss": (1e-5, 0), "correct": (0, 0),
           "adam_m": (1e-4, 1e-7), "adam_v": (1e-3, 1e-10), "params": (0, 1e-4)}
    for name, (rtol, atol) in tol.items():
        np.testing.assert_allclose(again[name], arrays[name], rtol=rtol, atol=atol, err_msg=name)
