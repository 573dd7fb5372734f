"""The image batch kernel (``csrc/ops/data_kernels.hip``) on the GPU against its CPU reference, bit
for bit; 64-bit dataset offsets; hipGraph replay; the model's space-to-depth entry; ``cnn_bench``
on a resident dataset end to end.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest
import torch

from arena_amd.ops.data import DeviceImageLoader

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OUTS = {"s2d": ("s2d", torch.bfloat16), "nhwc_bf16": ("nhwc", torch.bfloat16),
        "nhwc_fp32": ("nhwc", torch.float32)}


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(gpu: DeviceImageLoader, cpu: DeviceImageLoader, rows=None):
    assert gpu.out.shape == cpu.out.shape and gpu.out.stride() == cpu.out.stride()
    assert torch.equal(_bits(gpu.out), _bits(cpu.out))
    assert torch.equal(gpu.labels_out.cpu(), cpu.labels_out)
    assert torch.equal(gpu.rows_out.cpu(), cpu.rows_out if rows is None else rows)
    assert torch.equal(gpu.crop_out.cpu(), cpu.crop_out)


def _pair(x, y, batch, crop, dev, **kw):
    """the same loader on the GPU and on the CPU, with the GPU's permutation"""
    g = DeviceImageLoader(x.to(dev), y.to(dev), batch, crop, mean=MEAN, std=STD, **kw)
    c = DeviceImageLoader(x, y, batch, crop, mean=MEAN, std=STD, **kw)
    c.set_permutation(g.perm.cpu())
    return g, c


_SETS = {}


def _dataset(n, size):
    if (n, size) not in _SETS:
        g = torch.Generator().manual_seed(n * 1000 + size)
        _SETS[n, size] = (torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8,
                                        generator=g),
                          torch.randint(0, 1000, (n,), generator=g))
    return _SETS[n, size]


# (n, S, crop, B): odd offsets and a wrap past L; no room (y0 = x0 = 0 always); an odd stored size;
# a one-pixel z per image with more rows than one block has threads; the workload's geometry
CASES = [(37, 20, 16, 5), (8, 16, 16, 8), (50, 33, 24, 7), (300, 7, 2, 300), (64, 256, 224, 32)]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("out", sorted(OUTS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_S%d_c%d_B%d" % c)
def test_kernel_equals_reference(cuda, case, out, train):
    n, size, crop, batch = case
    layout, dtype = OUTS[out]
    x, y = _dataset(n, size)
    g, c = _pair(x, y, batch, crop, cuda, train=train, seed=17, stream=3, layout=layout,
                 dtype=dtype)
    start = max(n // batch - 1, 0)      # the steps around the end of the data: wrap / padding
    g.cursor.fill_(start)
    c.cursor.fill_(start)
    for _ in range(3):
        g.next()
        c.next()
        _same(g, c)
    assert int(g.cursor) == start + 3
    if not train:
        assert int(g.rows_out[-1]) == -1 and int(g.labels_out[-1]) == -100
    if crop == size:
        assert bool((g.crop_out[:, :2] == 0).all())


def test_rows_past_two_gigabytes(cuda):
    """22000 images of 256^2 are 4.3 GB: rows 10923, 21845 and 21999 start past 2^31, 2^32 and
    near the end. The reference runs on those four rows alone (the draws depend on the position,
    not on the row)."""
    n, size, crop = 22000, 256, 224
    rows = torch.tensor([0, 10923, 21845, 21999], dtype=torch.int32)
    big = torch.empty((n, size, size, 3), dtype=torch.uint8, device=cuda)
    small, _ = _dataset(4, size)
    for k, r in enumerate(rows.tolist()):
        big[r].copy_(small[k])
    labels = torch.arange(n, device=cuda)
    for layout in ("s2d", "nhwc"):
        g = DeviceImageLoader(big, labels, 4, crop, train=True, seed=5, mean=MEAN, std=STD,
                              layout=layout)
        g.set_permutation(rows)
        c = DeviceImageLoader(small, rows.to(torch.int64), 4, crop, train=True, seed=5,
                              mean=MEAN, std=STD, layout=layout)
        c.set_permutation(torch.arange(4))
        for _ in range(2):
            g.next()
            c.next()
            _same(g, c, rows=rows)
    del big


def test_graph_replay_advances(cuda):
    x, y = _dataset(50, 33)
    g, c = _pair(x, y, 7, 24, cuda, train=True, seed=9, layout="s2d")
    g.next()                                # warm-up (loads the extension), then rewind
    g.cursor.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lab = g.next()
    assert out is g.out and lab is g.labels_out
    for k in range(4):
        graph.replay()                      # batch k: nothing reads the cursor on the host
        c.next()
        _same(g, c)
    assert int(g.cursor) == 4


def _tiny(cuda):
    from arena_amd.models.resnet import resnet
    torch.manual_seed(3)
    model = resnet("resnet_tiny", num_classes=10, width=64).to(cuda)
    return model.to(memory_format=torch.channels_last)


def _two_layouts(cuda):
    x, y = _dataset(16, 72)
    kw = dict(train=True, seed=2, mean=MEAN, std=STD, dtype=torch.bfloat16)
    a = DeviceImageLoader(x.to(cuda), y.to(cuda), 8, 64, layout="s2d", **kw)
    b = DeviceImageLoader(x.to(cuda), y.to(cuda), 8, 64, layout="nhwc", **kw)
    b.set_permutation(a.perm)
    return a.next()[0], b.next()[0]


def test_model_takes_z(cuda):
    model = _tiny(cuda)
    assert model.takes_s2d(cuda, torch.bfloat16)
    assert not model.takes_s2d(cuda, torch.float32)
    assert not model.takes_s2d(torch.device("cpu"), torch.bfloat16)
    z, xb = _two_layouts(cuda)
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        lz = model(z, s2d=True)
        lx = model(xb)
    assert lz.shape == (8, 10) and bool(torch.isfinite(lz.float()).all())
    assert torch.equal(_bits(lz), _bits(lx))


def test_stem_output_from_z_in_training(cuda):
    """Full-model logits are not compared in training mode (the statistics accumulate with
    atomics); the stem convolution's output is."""
    model = _tiny(cuda).train()
    z, xb = _two_layouts(cuda)
    with torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
        yz, _ = model.stem[0].forward_s2d(z)
        yx, _ = model.stem[0].forward_stats(xb)
    assert yz.shape == (8, 64, 32, 32) and yz.requires_grad
    assert torch.equal(_bits(yz.detach()), _bits(yx.detach()))


def test_cnn_bench_on_a_resident_dataset(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MIOPEN_FIND_MODE="FAST", ARENA_HEARTBEAT_FILE=str(tmp_path / "hb"))
    r = subprocess.run([sys.executable, "-m", "arena_amd.examples.cnn_bench", "--synth_images",
                        "256", "--stored_size", "72", "--image_size", "64", "--model",
                        "resnet_tiny", "--width", "64", "--num_classes", "4", "--batch_size",
                        "16", "--num_epochs", "3", "--num_warmup_batches", "3", "--dtype", "bf16",
                        "--graph", "1",
                        "--print_training_accuracy", "--json"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    head = [ln for ln in r.stdout.splitlines() if ln.startswith("Model: ")]
    assert len(head) == 1 and "Data: synthetic-images (256 images, 72 -> 64)" in head[0], head
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["exec"] == "hipgraph" and res["layout"] == "s2d"
    assert res["steps_per_epoch"] == 16 and res["epochs"] == 3
    assert res["kept"] == 3 * 16 * 16          # steps x batch: every replay fed a full batch
    assert res["invalid_labels"] == 0
