"""The colour distortion of the resized batch kernel (``image_batch_resized_kernel`` in its
IMAGE_SUMS and IMAGE_COLOR modes, ``csrc/ops/data_kernels.hip``) on the GPU against its CPU
reference, bit for bit; the identity and mean-only ranges against the colourless kernel; hipGraph
replay; padding rows; ``cnn_bench --distort_color`` end to end.
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
COLOR = {"color": True}
IDENTITY = {"brightness": 0.0, "saturation": (1.0, 1.0), "hue": 0.0, "contrast": (1.0, 1.0)}


def _bits(t):
    return t.cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(gpu: DeviceImageLoader, cpu: DeviceImageLoader):
    assert gpu.out.shape == cpu.out.shape and gpu.out.stride() == cpu.out.stride()
    assert torch.equal(gpu.color_out.cpu(), cpu.color_out)
    assert torch.equal(gpu.color_sums.cpu(), cpu.color_sums)
    assert torch.equal(_bits(gpu.out), _bits(cpu.out))
    assert torch.equal(gpu.labels_out.cpu(), cpu.labels_out)
    assert torch.equal(gpu.rows_out.cpu(), cpu.rows_out)
    assert torch.equal(gpu.crop_out.cpu(), cpu.crop_out)
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


# (n, S, crop, B): scaling both ways with a wrap past L; 144 quads, a partial block with a partial
# wave; one quad per image (N = 4) and more rows than a block has threads; 49 blocks per image, so
# the sums cross blocks
CASES = [(37, 20, 16, 5), (50, 33, 24, 7), (300, 7, 2, 300), (16, 256, 224, 8)]


@pytest.mark.parametrize("out", sorted(OUTS))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_S%d_c%d_B%d" % c)
def test_kernel_equals_reference(cuda, case, out):
    n, size, crop, batch = case
    layout, dtype = OUTS[out]
    x, y = _dataset(n, size)
    g, c = _pair(x, y, batch, crop, cuda, train=True, seed=17, stream=3, layout=layout,
                 dtype=dtype, distort=COLOR)
    assert torch.equal(g.color_table.cpu(), c.color_table)
    assert g.color_sums.shape[1] == -(-(crop // 2) ** 2 // 256)
    start = max(n // batch - 1, 0)      # one step before the wrap past L
    g.cursor.fill_(start)
    c.cursor.fill_(start)
    for _ in range(3):
        g.next()
        c.next()
        _same(g, c)
    assert int(g.cursor) == start + 3


@pytest.mark.parametrize("out", sorted(OUTS))
def test_identity_ranges_equal_the_colourless_kernel(cuda, out):
    layout, dtype = OUTS[out]
    x, y = _dataset(50, 33)
    kw = dict(train=True, seed=4, stream=1, mean=MEAN, std=STD, layout=layout, dtype=dtype)
    a = DeviceImageLoader(x.to(cuda), y.to(cuda), 7, 24, distort=True, **kw)
    b = DeviceImageLoader(x.to(cuda), y.to(cuda), 7, 24, distort={"color": IDENTITY}, **kw)
    b.set_permutation(a.perm)
    for _ in range(3):
        a.next()
        b.next()
        assert torch.equal(_bits(b.out), _bits(a.out))
        assert torch.equal(b.labels_out, a.labels_out) and torch.equal(b.rows_out, a.rows_out)
        assert torch.equal(b.crop_out, a.crop_out) and torch.equal(b.box_out, a.box_out)
        assert b.color_out[:, 1:].tolist() == [[256, 0]] * 7


@pytest.mark.parametrize("out", sorted(OUTS))
@pytest.mark.parametrize("size,crop", [(33, 24), (256, 224)])
def test_contrast_zero_writes_the_rounded_channel_mean(cuda, size, crop, out):
    """Every pixel of image b, channel c is table[c][floor(s_c / N + 1/2)], with s_c summed by
    torch over the colourless kernel's bytes (read through mean 0, std 1 in fp32): a check of the
    two-launch reduction that does not go through the reference."""
    layout, dtype = OUTS[out]
    x, y = _dataset(16 if size == 256 else 50, size)
    B, N = 6, crop * crop
    xs, ys = x.to(cuda), y.to(cuda)
    col = DeviceImageLoader(xs, ys, B, crop, train=True, seed=8, mean=MEAN, std=STD, layout=layout,
                            dtype=dtype, distort={"color": dict(IDENTITY, contrast=(0.0, 0.0))})
    flat = DeviceImageLoader(xs, ys, B, crop, train=True, seed=8, mean=(0.0, 0.0, 0.0),
                             std=(1.0, 1.0, 1.0), layout="nhwc", dtype=torch.float32, distort=True)
    flat.set_permutation(col.perm)
    for _ in range(2):
        got, _ = col.next()
        u = (flat.next()[0] * 255.0).round().to(torch.int64)                # [B, 3, H, W]
        s = u.sum((2, 3))
        mean = (2 * s + N) // (2 * N)                                       # [B, 3]
        want = col.table[torch.arange(3, device=cuda).view(1, 3), mean]     # [B, 3]
        if layout == "nhwc":
            assert torch.equal(_bits(got), _bits(want.view(B, 3, 1, 1).expand_as(got)))
        else:
            z = torch.cat([want.repeat(1, 4), torch.zeros_like(want[:, :1]).expand(B, 4)], 1)
            assert torch.equal(_bits(got), _bits(z.view(B, 16, 1, 1).expand_as(got)))


def test_graph_replay_advances(cuda):
    x, y = _dataset(50, 33)
    g, c = _pair(x, y, 7, 24, cuda, train=True, seed=9, layout="s2d", distort=COLOR)
    g.next()                                # warm-up (loads the extension), then rewind
    g.cursor.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lab = g.next()
    assert out is g.out and lab is g.labels_out
    draws = []
    for k in range(4):
        graph.replay()                      # batch k: nothing reads the cursor on the host
        c.next()
        _same(g, c)
        draws.append(g.color_out.cpu().clone())
    assert int(g.cursor) == 4
    assert all(not torch.equal(draws[0], d) for d in draws[1:])


def test_a_stray_permutation_entry_is_a_padding_row(cuda):
    x, y = _dataset(37, 20)
    g, c = _pair(x, y, 5, 16, cuda, train=True, seed=2, layout="nhwc", distort=COLOR)
    for ld in (g, c):                       # written past set_permutation's check
        ld.perm[1] = 37
        ld.perm[3] = -2
    g.next()
    c.next()
    _same(g, c)
    assert g.rows_out.tolist()[1::2] == [-1, -1] and g.labels_out.tolist()[1::2] == [-100, -100]
    assert bool((g.out[1::2] == 0).all()) and bool((g.out[0::2] != 0).any())
    assert bool((g.color_sums[1::2] == 0).all()) and min(g.rows_out.tolist()[0::2]) >= 0


def test_cnn_bench_with_distort_color(tmp_path):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MIOPEN_FIND_MODE="FAST", ARENA_HEARTBEAT_FILE=str(tmp_path / "hb"))
    r = subprocess.run([sys.executable, "-m", "arena_amd.examples.cnn_bench", "--synth_images",
                        "512", "--stored_size", "72", "--image_size", "64", "--model",
                        "resnet_tiny", "--distortions", "--distort_color", "--num_batches", "6",
                        "--num_warmup_batches", "2", "--json"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    head = [ln for ln in r.stdout.splitlines() if ln.startswith("Model: ")]
    assert len(head) == 1 and "distorted+color" in head[0], head
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["exec"] == "hipgraph"
    assert res["distortions"] is True and res["distort_color"] is True
