"""Extended cross-entropy head kernels (ignore_index, label smoothing, label checks, top-k counts)
against ``F.cross_entropy`` on the fp32-upcast logits and the rank rule in torch (MI355X).

Tolerances are those of ``test_fused_cross_entropy_matches_torch``: loss rtol = atol = 1e-5;
gradient 1e-2 (bf16) / 1e-5 (fp32) with atol = tol * 1e-2. Counts are exact: the rank compares
the stored logits in fp32 (``tf.nn.in_top_k``'s rule, ties at the boundary count as correct).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(5, 37),       # partial block, partial lane tail
          (33, 64),      # exactly one element per lane
          (4, 1024),     # last width of the register form
          (6, 1030),     # first widths of the three-pass form
          (1, 8),        # smallest
          (128, 1000)]   # the workload's own
TOPK_SHAPES = [s for s in SHAPES if s[0] >= 8 and s[1] >= 8]
DTYPES = [torch.bfloat16, torch.float32]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(rows, classes, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(rows + classes + seed)
    x = (torch.randn(rows, classes, device="cuda", generator=g) * 3).to(dtype)
    y = torch.randint(0, classes, (rows,), device="cuda", generator=g)
    return x, y


def _run(x, y, upstream=0.75, **kw):
    """(loss, gradient) of the op under test for upstream gradient ``upstream``."""
    from arena_amd.ops.pool import cross_entropy
    x = x.detach().clone().requires_grad_(True)
    loss = cross_entropy(x, y, **kw)
    (loss * upstream).backward()
    return loss.detach(), x.grad


def _ref(x, y, ignore_index, eps, upstream=0.75):
    x = x.detach().clone().requires_grad_(True)
    loss = F.cross_entropy(x.float(), y, ignore_index=ignore_index, label_smoothing=eps)
    (loss * upstream).backward()
    return loss.detach(), x.grad


def _ref_counts(x, y, ignore_index):
    classes = x.shape[1]
    valid = (y >= 0) & (y < classes)
    ignored = y == ignore_index if ignore_index is not None else torch.zeros_like(valid)
    keep = valid & ~ignored
    xf = x.float()
    rank = (xf > xf.gather(1, y.clamp(0, classes - 1)[:, None])).sum(1)
    return [int(keep.sum()), int((keep & (rank < 1)).sum()), int((keep & (rank < 5)).sum()),
            int((~valid & ~ignored).sum())]


def _close(loss, grad, ref_loss, ref_grad, dtype):
    assert loss.dtype == torch.float32 and loss.shape == () and grad.dtype == dtype
    print(f"loss {float(loss):.8f} ref {float(ref_loss):.8f}  max |dgrad| "
          f"{float((grad.float() - ref_grad.float()).abs().max()):.3e}")
    assert torch.allclose(loss, ref_loss, rtol=1e-5, atol=1e-5), (float(loss), float(ref_loss))
    tol = 1e-2 if dtype == torch.bfloat16 else 1e-5
    assert torch.allclose(grad.float(), ref_grad.float(), rtol=tol, atol=tol * 1e-2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,classes", SHAPES)
@pytest.mark.parametrize("ignore_index", [-100, 7])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_loss_and_gradient_match_torch(dtype, rows, classes, ignore_index, eps):
    x, y = _data(rows, classes, dtype)
    y[2::3] = ignore_index          # every third row (the single row of the 1 x 8 case is kept)
    loss, grad = _run(x, y, ignore_index=ignore_index, label_smoothing=eps)
    ref_loss, ref_grad = _ref(x, y, ignore_index, eps)
    _close(loss, grad, ref_loss, ref_grad, dtype)
    assert torch.equal(grad[2::3], torch.zeros_like(grad[2::3]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,classes", SHAPES)
def test_all_rows_ignored(dtype, rows, classes):
    x, _ = _data(rows, classes, dtype)
    y = torch.full((rows,), -100, device="cuda")
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    loss, grad = _run(x, y, ignore_index=-100, label_smoothing=0.1, stats=stats)
    assert torch.isnan(loss)
    assert torch.equal(grad, torch.zeros_like(grad))
    assert stats.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,classes", [s for s in SHAPES if s[0] >= 3])
def test_invalid_labels_are_dropped_and_counted(dtype, rows, classes):
    """Out-of-range labels in interior rows only (as many of the four values as there are interior
    rows): even an unchecked index would stay inside the logits tensor."""
    x, y = _data(rows, classes, dtype)
    bad = dict(zip(range(1, rows - 1), [classes, classes + 1, -1, -2]))
    n = len(bad)
    assert n == min(4, rows - 2) and 0 not in bad and rows - 1 not in bad
    for r, v in bad.items():
        y[r] = v
    y_ref = y.clone()
    y_ref[list(bad)] = -100
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    loss, grad = _run(x, y, ignore_index=-100, label_smoothing=0.1, stats=stats)
    ref_loss, ref_grad = _ref(x, y_ref, -100, 0.1)
    assert int(stats[3]) == n and int(stats[0]) == rows - n
    _close(loss, grad, ref_loss, ref_grad, dtype)
    assert torch.equal(grad[list(bad)], torch.zeros_like(grad[list(bad)]))
    # no ignore_index: the same rows are invalid, nothing else is dropped
    stats.zero_()
    loss2, grad2 = _run(x, y, label_smoothing=0.1, stats=stats)
    assert int(stats[3]) == n and int(stats[0]) == rows - n
    _close(loss2, grad2, ref_loss, ref_grad, dtype)


def _topk_case(rows, classes):
    """bf16 logits; row i's label is the class at descending-sorted position i % 8; row 0 is
    hand-built: six equal maxima, the label among them (rank 0)."""
    x, _ = _data(rows, classes, torch.bfloat16, seed=1)
    y = x.float().argsort(1, descending=True)[torch.arange(rows), torch.arange(rows) % 8]
    x[0] = 0
    x[0, 1:7] = 5.0
    y[0] = 4
    return x, y


@pytest.mark.parametrize("rows,classes", TOPK_SHAPES)
def test_top_k_counts_follow_the_rank_rule(rows, classes):
    from arena_amd.ops.pool import cross_entropy
    x, y = _topk_case(rows, classes)
    y[3] = -100
    ref = _ref_counts(x, y, -100)
    kept, top1, top5, _ = ref
    assert kept == rows - 1 and 0 < top1 < top5 < kept, ref
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    cross_entropy(x, y, ignore_index=-100, stats=stats)
    assert stats.tolist() == ref
    one = torch.zeros(4, dtype=torch.int64, device="cuda")
    cross_entropy(x[:1], y[:1], stats=one)       # the tied row alone counts for top-1
    assert one.tolist() == [1, 1, 1, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_stats_accumulate_and_graph_replay(dtype):
    rows, classes = 33, 64
    xa, ya = _topk_case(rows, classes)
    xa = xa.to(dtype)
    xb, yb = _data(rows, classes, dtype, seed=2)
    yb[1] = -100
    yb[4] = classes
    ra, rb = _ref_counts(xa, ya, -100), _ref_counts(xb, yb, -100)
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    kw = dict(ignore_index=-100, label_smoothing=0.1, stats=stats)
    _run(xa, ya, **kw)
    loss_e, grad_e = _run(xb, yb, **kw)
    assert stats.tolist() == [a + b for a, b in zip(ra, rb)]

    # forward + backward captured on a single stream, replayed three times
    from arena_amd.ops.pool import cross_entropy
    stats.zero_()
    xs = xb.detach().clone().requires_grad_(True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss_g = cross_entropy(xs, yb, **kw)
        (grad_g,) = torch.autograd.grad(loss_g * 0.75, xs)
    assert stats.tolist() == [0, 0, 0, 0]        # capture executes nothing
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert stats.tolist() == [3 * b for b in rb]
    assert torch.equal(loss_g, loss_e) and torch.equal(grad_g, grad_e)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,classes", [(128, 1000), (6, 1030)])
def test_new_path_is_deterministic(dtype, rows, classes):
    x, y = _data(rows, classes, dtype)
    y[2::3] = -100
    out = []
    for _ in range(2):
        stats = torch.zeros(4, dtype=torch.int64, device="cuda")
        loss, grad = _run(x, y, ignore_index=-100, label_smoothing=0.1, stats=stats)
        out.append((loss, grad, stats))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert not torch.isnan(out[0][0])            # (NaN would compare unequal above anyway)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,classes", SHAPES)
def test_legacy_path_unchanged(dtype, rows, classes):
    x, y = _data(rows, classes, dtype)
    loss, grad = _run(x, y)
    loss_d, grad_d = _run(x, y, ignore_index=None, label_smoothing=0.0, stats=None)
    assert torch.equal(loss, loss_d) and torch.equal(grad, grad_d)
    # the new kernels with nothing ignored and no smoothing compute the same function
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    loss_n, grad_n = _run(x, y, ignore_index=-100, stats=stats)
    _close(loss_n, grad_n, loss, grad, dtype)
    assert int(stats[0]) == rows and int(stats[3]) == 0


def _cnn_bench(tmp_path, *flags):
    env = {k: v for k, v in os.environ.items()   # a world of one, whatever earlier tests set
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MIOPEN_FIND_MODE="FAST", ARENA_HEARTBEAT_FILE=str(tmp_path / "hb"))
    r = subprocess.run([sys.executable, "-m", "arena_amd.examples.cnn_bench", "--model",
                        "resnet_tiny", "--width", "16", "--image_size", "64", "--num_classes",
                        "10", "--batch_size", "16", "--num_batches", "6",
                        "--num_warmup_batches", "2", "--display_every", "3", *flags],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_cnn_bench_label_smoothing_and_training_accuracy(tmp_path):
    out = _cnn_bench(tmp_path, "--label_smoothing", "0.1", "--print_training_accuracy", "--json")
    res = json.loads(out.strip().splitlines()[-1])
    assert res["exec"] == "hipgraph"
    assert 0 <= res["top_1_accuracy"] <= res["top_5_accuracy"] <= 1
    assert res["invalid_labels"] == 0
    lines = [ln for ln in out.splitlines() if "images/sec:" in ln and "total" not in ln]
    assert len(lines) == 2 and all("top_1_accuracy: " in ln and "top_5_accuracy: " in ln
                                   for ln in lines)


def test_cnn_bench_eval(tmp_path):
    out = _cnn_bench(tmp_path, "--eval")
    line = [ln for ln in out.splitlines() if ln.startswith("Accuracy @ 1 = ")]
    assert len(line) == 1 and " Accuracy @ 5 = " in line[0], out
    assert line[0].endswith("[96 examples]")
