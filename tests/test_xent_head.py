"""Cross-entropy head semantics on the CPU (the stock-op path of ``ops.pool.cross_entropy``, which
is also the reference of the HIP kernels): ignore_index, label smoothing, invalid labels, top-k
counts, and the cnn_bench flags built on them.

The top-k rule is ``tf.nn.in_top_k``'s: a row is top-k correct iff fewer than k classes have a
logit strictly greater than the label's (ties at the boundary count as correct).
"""
from __future__ import annotations

import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(rows=12, classes=37, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, classes, generator=g) * 3
    y = torch.randint(0, classes, (rows,), generator=g)
    return x, y


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("ignore_index", [-100, 7])
def test_fallback_matches_torch(eps, ignore_index):
    from arena_amd.ops.pool import cross_entropy
    x, y = _data()
    y[::3] = ignore_index           # a third of the rows
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    loss = cross_entropy(x1, y, ignore_index=ignore_index, label_smoothing=eps)
    ref = F.cross_entropy(x2, y, ignore_index=ignore_index, label_smoothing=eps)
    assert loss.dtype == torch.float32 and loss.shape == ()
    torch.testing.assert_close(loss, ref, rtol=1e-6, atol=1e-6)
    (loss * 0.75).backward()
    (ref * 0.75).backward()
    torch.testing.assert_close(x1.grad, x2.grad, rtol=1e-6, atol=1e-7)
    assert torch.equal(x1.grad[::3], torch.zeros_like(x1.grad[::3]))


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_all_rows_ignored_gives_nan_loss_and_zero_gradient(eps):
    from arena_amd.ops.pool import cross_entropy
    x, _ = _data()
    y = torch.full((x.shape[0],), -100)
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    stats = torch.zeros(4, dtype=torch.int64)
    loss = cross_entropy(x1, y, ignore_index=-100, label_smoothing=eps, stats=stats)
    ref = F.cross_entropy(x2, y, ignore_index=-100, label_smoothing=eps)
    assert torch.isnan(ref) and torch.isnan(loss)     # torch's own behaviour, checked here
    loss.backward()
    ref.backward()
    assert torch.equal(x2.grad, torch.zeros_like(x))
    assert torch.equal(x1.grad, torch.zeros_like(x))
    assert stats.tolist() == [0, 0, 0, 0]


def test_stats_follow_the_rank_rule():
    from arena_amd.ops.pool import cross_entropy
    x, y = _data(rows=40, classes=16, seed=3)
    x = x.bfloat16().float().round()       # few distinct values: many ties with the label's logit
    order = x.argsort(1, descending=True)
    y = order[torch.arange(40), torch.arange(40) % 8]
    y[5] = -100
    stats = torch.tensor([10, 20, 30, 40])
    cross_entropy(x, y, ignore_index=-100, stats=stats)
    keep = y != -100
    rank = (x > x.gather(1, y.clamp(min=0)[:, None])).sum(1)
    top1, top5 = int((keep & (rank < 1)).sum()), int((keep & (rank < 5)).sum())
    assert 0 < top1 < top5 < 39
    assert stats.tolist() == [10 + 39, 20 + top1, 30 + top5, 40]
    cross_entropy(x, y, ignore_index=-100, stats=stats)     # accumulates
    assert stats.tolist() == [10 + 78, 20 + 2 * top1, 30 + 2 * top5, 40]


def test_tied_maxima_count_as_top1():
    from arena_amd.ops.pool import cross_entropy
    x = torch.zeros(1, 10)
    x[0, 2:8] = 4.0                       # six equal maxima, the label among them
    stats = torch.zeros(4, dtype=torch.int64)
    cross_entropy(x, torch.tensor([5]), stats=stats)
    assert stats.tolist() == [1, 1, 1, 0]


def test_invalid_labels_are_masked_and_counted():
    from arena_amd.ops.pool import cross_entropy
    x, y = _data()
    classes = x.shape[1]
    bad = {1: classes, 4: classes + 1, 6: -1, 9: -2}
    yb = y.clone()
    for r, v in bad.items():
        yb[r] = v
    yb[2] = -100
    y_ref = yb.clone()
    y_ref[list(bad)] = -100
    x1 = x.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True)
    stats = torch.zeros(4, dtype=torch.int64)
    loss = cross_entropy(x1, yb, ignore_index=-100, label_smoothing=0.1, stats=stats)
    ref = F.cross_entropy(x2, y_ref, ignore_index=-100, label_smoothing=0.1)
    torch.testing.assert_close(loss, ref, rtol=1e-6, atol=1e-6)
    loss.backward()
    ref.backward()
    torch.testing.assert_close(x1.grad, x2.grad, rtol=1e-6, atol=1e-7)
    assert stats[0] == x.shape[0] - 5 and stats[3] == 4
    # without an ignore_index every out-of-range label is invalid, -100 included
    stats.zero_()
    loss2 = cross_entropy(x, yb, stats=stats)
    torch.testing.assert_close(loss2, F.cross_entropy(x, y_ref), rtol=1e-6, atol=1e-6)
    assert stats[0] == x.shape[0] - 5 and stats[3] == 5


@pytest.mark.parametrize("eps", [-0.01, 1.5, float("nan")])
def test_label_smoothing_out_of_range_raises(eps):
    from arena_amd.ops.pool import cross_entropy
    x, y = _data()
    with pytest.raises(ValueError):
        cross_entropy(x, y, label_smoothing=eps)


def test_bad_stats_tensor_raises():
    from arena_amd.ops.pool import cross_entropy
    x, y = _data()
    with pytest.raises(ValueError):
        cross_entropy(x, y, stats=torch.zeros(4))
    with pytest.raises(ValueError):
        cross_entropy(x, y, stats=torch.zeros(5, dtype=torch.int64))


def test_cnn_bench_parse_accepts_the_new_flags():
    from arena_amd.examples import cnn_bench
    a = cnn_bench.parse([])
    assert a.label_smoothing == 0.0 and not a.print_training_accuracy and not a.eval
    a = cnn_bench.parse(["--label_smoothing", "0.1", "--print_training_accuracy", "--eval"])
    assert a.label_smoothing == 0.1 and a.print_training_accuracy and a.eval
    with pytest.raises(SystemExit):
        cnn_bench.parse(["--label_smoothing", "1.5"])


def test_train_step_head_keyword():
    """``head=None`` is the plain loss; a head dict routes through the extended loss and counts."""
    import types
    from arena_amd.examples import cnn_bench
    args = types.SimpleNamespace(model="resnet_tiny", data_format="NHWC", batch_size=4,
                                 image_size=32, num_classes=10, width=8, learning_rate=0.05,
                                 momentum=0.9, weight_decay=1e-3, bucket_mb=0.01, comm="auto")
    model, opt, x, y = cnn_bench.build(args, torch.device("cpu"), 1)
    model2, opt2, _, _ = cnn_bench.build(args, torch.device("cpu"), 1)
    stats = torch.zeros(4, dtype=torch.int64)
    l1 = cnn_bench.train_step(model, opt, x, y, None)
    l2 = cnn_bench.train_step(model2, opt2, x, y, None,
                              head={"label_smoothing": 0.0, "stats": stats})
    torch.testing.assert_close(l1, l2, rtol=1e-6, atol=1e-6)
    assert stats[0] == 4 and stats[3] == 0 and 0 <= stats[1] <= stats[2] <= 4


def test_cnn_bench_eval_run_prints_accuracy(tmp_path):
    env = {k: v for k, v in os.environ.items()   # a world of one, whatever earlier tests set
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["ARENA_HEARTBEAT_FILE"] = str(tmp_path / "hb")
    r = subprocess.run([sys.executable, "-m", "arena_amd.examples.cnn_bench", "--model",
                        "resnet_tiny", "--width", "8", "--image_size", "32", "--num_classes",
                        "10", "--batch_size", "4", "--num_batches", "3", "--num_warmup_batches",
                        "1", "--display_every", "2", "--device", "cpu", "--dtype", "fp32",
                        "--eval"], capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "images/sec:" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Accuracy @ 1 = ")]
    assert len(line) == 1 and line[0].endswith("[12 examples]"), r.stdout
    assert " Accuracy @ 5 = " in line[0]
