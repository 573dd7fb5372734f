"""The random-resized-crop kernel (``image_batch_resized_kernel``, ``csrc/ops/data_kernels.hip``)
on the GPU against its CPU reference, bit for bit; the identity box against the fixed-crop kernel;
hipGraph replay; padding rows; ``cnn_bench --distortions`` end to end.
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


def _same(gpu: DeviceImageLoader, cpu: DeviceImageLoader):
    assert gpu.out.shape == cpu.out.shape and gpu.out.stride() == cpu.out.stride()
    assert torch.equal(_bits(gpu.out), _bits(cpu.out))
    assert torch.equal(gpu.labels_out.cpu(), cpu.labels_out)
    assert torch.equal(gpu.rows_out.cpu(), cpu.rows_out)
    assert torch.equal(gpu.crop_out.cpu(), cpu.crop_out)
    if cpu.box_out is not None:
        assert torch.equal(gpu.box_out.cpu(), cpu.box_out)


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


# (n, S, crop, B, distort): boxes from 4 to 20 around a crop of 16 (up- and down-scaling), odd
# offsets and a wrap past L; an odd stored size; one quad per image and more rows than a block has
# threads; the whole image as the only box; the workload's geometry at a small batch
WHOLE = {"area": (1.0, 1.0), "aspect": (1.0, 1.0)}
CASES = [(37, 20, 16, 5, True), (50, 33, 24, 7, True), (300, 7, 2, 300, True),
         (8, 16, 16, 8, WHOLE), (16, 256, 224, 8, True)]


@pytest.mark.parametrize("out", sorted(OUTS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_S%d_c%d_B%d" % c[:4])
def test_kernel_equals_reference(cuda, case, out):
    n, size, crop, batch, distort = case
    layout, dtype = OUTS[out]
    x, y = _dataset(n, size)
    g, c = _pair(x, y, batch, crop, cuda, train=True, seed=17, stream=3, layout=layout,
                 dtype=dtype, distort=distort)
    assert torch.equal(g.boxes.cpu(), c.boxes)
    if distort is WHOLE:
        assert set(map(tuple, c.boxes.tolist())) == {(size, size)}
    start = max(n // batch - 1, 0)      # one step before the wrap past L
    g.cursor.fill_(start)
    c.cursor.fill_(start)
    seen = set()
    for _ in range(3):
        g.next()
        c.next()
        _same(g, c)
        seen |= set(map(tuple, g.box_out.tolist()))
    assert int(g.cursor) == start + 3
    if (n, size) == (37, 20):           # the case is meant to scale both ways
        assert any(h < crop for h, _ in seen) and any(h > crop for h, _ in seen)


@pytest.mark.parametrize("out", sorted(OUTS))
def test_identity_box_equals_the_fixed_crop_kernel(cuda, out):
    layout, dtype = OUTS[out]
    x, y = _dataset(50, 33)
    kw = dict(train=True, seed=4, stream=1, mean=MEAN, std=STD, layout=layout, dtype=dtype)
    a = DeviceImageLoader(x.to(cuda), y.to(cuda), 7, 24, **kw)
    b = DeviceImageLoader(x.to(cuda), y.to(cuda), 7, 24, distort=True, **kw)
    b.set_permutation(a.perm)
    b.set_boxes(torch.tensor([[24, 24]]))
    for _ in range(3):
        a.next()
        b.next()
        assert torch.equal(_bits(b.out), _bits(a.out))
        assert torch.equal(b.labels_out, a.labels_out) and torch.equal(b.rows_out, a.rows_out)
        assert torch.equal(b.crop_out, a.crop_out)
        assert b.box_out.tolist() == [[24, 24]] * 7


def test_graph_replay_advances(cuda):
    x, y = _dataset(50, 33)
    g, c = _pair(x, y, 7, 24, cuda, train=True, seed=9, layout="s2d", distort=True)
    g.next()                                # warm-up (loads the extension), then rewind
    g.cursor.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lab = g.next()
    assert out is g.out and lab is g.labels_out
    boxes = []
    for k in range(4):
        graph.replay()                      # batch k: nothing reads the cursor on the host
        c.next()
        _same(g, c)
        boxes.append(g.box_out.cpu().clone())
    assert int(g.cursor) == 4
    assert any(not torch.equal(boxes[0], b) for b in boxes[1:])


def test_a_stray_permutation_entry_is_a_padding_row(cuda):
    x, y = _dataset(37, 20)
    g, c = _pair(x, y, 5, 16, cuda, train=True, seed=2, layout="nhwc", distort=True)
    for ld in (g, c):                       # written past set_permutation's check
        ld.perm[1] = 37
        ld.perm[3] = -2
    g.next()
    c.next()
    _same(g, c)
    assert g.rows_out.tolist()[1::2] == [-1, -1] and g.labels_out.tolist()[1::2] == [-100, -100]
    assert bool((g.out[1::2] == 0).all()) and bool((g.out[0::2] != 0).any())
    assert min(g.rows_out.tolist()[0::2]) >= 0


def test_cnn_bench_with_distortions(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MIOPEN_FIND_MODE="FAST", ARENA_HEARTBEAT_FILE=str(tmp_path / "hb"))
    r = subprocess.run([sys.executable, "-m", "arena_amd.examples.cnn_bench", "--synth_images",
                        "512", "--stored_size", "72", "--image_size", "64", "--model",
                        "resnet_tiny", "--distortions", "--num_batches", "6",
                        "--num_warmup_batches", "2", "--json"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    head = [ln for ln in r.stdout.splitlines() if ln.startswith("Model: ")]
    assert len(head) == 1 and "distorted" in head[0], head
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["exec"] == "hipgraph"
    assert res["distortions"] is True and res["crop_boxes"] > 0
