"""Colour distortion of the device image loader on the CPU: the reference semantics
(``reference.image_batch_color`` through ``DeviceImageLoader(distort={"color": ...})``) against a
plain fp64 form of tf_cnn_benchmarks' ``distort_color`` (YIQ), the identity and mean-only ranges,
the draws, validation and state, and ``cnn_bench --distort_color``.
"""
from __future__ import annotations

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from arena_amd.ops import reference
from arena_amd.ops.data import DeviceImageLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = {"brightness": 0.0, "saturation": (1.0, 1.0), "hue": 0.0, "contrast": (1.0, 1.0)}
MEAN_ONLY = dict(IDENTITY, contrast=(0.0, 0.0))
OUTS = {"s2d": ("s2d", torch.bfloat16), "nhwc_bf16": ("nhwc", torch.bfloat16),
        "nhwc_fp32": ("nhwc", torch.float32)}


def _random_set(n, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g),
            torch.randint(0, 7, (n,), generator=g))


def _byte_loader(x, y, batch, crop, color, **kw):
    """fp32 nhwc with mean 0 and std 1: the output is byte / 255, so ``_bytes`` reads the byte"""
    distort = True if color is None else {"color": color}
    return DeviceImageLoader(x, y, batch, crop, train=True, mean=(0.0, 0.0, 0.0),
                             std=(1.0, 1.0, 1.0), layout="nhwc", dtype=torch.float32,
                             distort=distort, **kw)


def _bytes(out):
    """[B, 3, H, W] of byte / 255 -> int64 [B, H, W, 3]"""
    return (out * 255.0).round().to(torch.int64).permute(0, 2, 3, 1).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------- 1. against tf's chain in fp64
YIQ = np.array([[0.299, 0.587, 0.114], [0.5959, -0.2746, -0.3213], [0.2115, -0.5227, 0.3112]])


def _matrix(m, saturation, hue):
    """the real-valued map of table row m: the grid point's saturation and angle (the table is
    row-major over 32 saturation steps x 32 hue steps, each at the middle of its step)"""
    i, j = divmod(int(m), 32)
    s = saturation[0] + (saturation[1] - saturation[0]) * (i + 0.5) / 32
    t = -hue + 2.0 * hue * (j + 0.5) / 32
    R = np.array([[1.0, 0.0, 0.0], [0.0, s * math.cos(t), -s * math.sin(t)],
                  [0.0, s * math.sin(t), s * math.cos(t)]])
    return np.linalg.inv(YIQ) @ R @ YIQ


def _tf_distort_color(x, M, k, d, order):
    """tf_cnn_benchmarks' distort_color on one image x [H, W, 3] in [0, 1]: brightness, then
    saturation / hue (one YIQ map) and contrast in the order of the batch position's parity"""
    def contrast(v):
        mu = v.reshape(-1, 3).mean(0)
        return (v - mu) * k + mu
    x = x + d
    x = contrast(x @ M.T) if order == 0 else contrast(x) @ M.T
    return np.clip(x, 0.0, 1.0)


def test_the_yiq_rows_that_make_both_orders_one_map():
    assert abs(YIQ[1].sum()) < 1e-15 and abs(YIQ[2].sum()) < 1e-15
    assert np.abs(_matrix(777, (0.5, 1.5), 0.2 * math.pi) @ np.ones(3) - 1.0).max() < 1e-12
    assert tuple(map(tuple, YIQ)) == reference.RGB_TO_YIQ


@pytest.mark.parametrize("n,S,crop,B", [(40, 7, 2, 40), (30, 9, 4, 15), (24, 20, 16, 8),
                                        (12, 33, 24, 6)])
def test_reference_matches_tf_chain_in_fp64(n, S, crop, B):
    """Every byte within 1 of tf's chain evaluated in fp64 on the dequantised draws, in both
    orders: quantising M to 2^-12 moves a byte by at most 3 * 255 * 2^-13 * 1.5 = 0.14, the floor
    in b by less than 2^-20, and one rounding boundary accounts for the rest."""
    x, y = _random_set(n, S, seed=S)
    x[: n // 2] = (x[: n // 2] // 4) + 150          # bright, flat images: they clip at the top
    col = _byte_loader(x, y, B, crop, True, seed=3, stream=1)
    plain = _byte_loader(x, y, B, crop, None, seed=3, stream=1)
    sat, hue = reference.COLOR_SATURATION, reference.COLOR_HUE
    worst, differing, total, clipped = 0, 0, 0, 0
    for _ in range(3):
        got = _bytes(col.next()[0]).numpy()
        src = _bytes(plain.next()[0]).numpy() / 255.0
        for b in range(B):
            m, kq, dq = col.color_out[b].tolist()
            M = _matrix(m, sat, hue)
            f0 = _tf_distort_color(src[b], M, kq / 256.0, dq / 255.0, 0)
            f1 = _tf_distort_color(src[b], M, kq / 256.0, dq / 255.0, 1)
            assert np.abs(f0 - f1).max() < 1e-12
            for f in (f0, f1):
                diff = np.abs(got[b] - np.rint(f * 255.0))
                worst = max(worst, int(diff.max()))
                differing += int((diff > 0).sum())
                total += diff.size
            clipped += int(((f0 == 0.0) | (f0 == 1.0)).sum())
    print(f"worst byte difference {worst}, share differing {differing / total:.4f}, "
          f"clipped values {clipped}")
    assert worst <= 1
    assert clipped > 0


# --------------------------------------------------------------------------- 2. identity ranges
@pytest.mark.parametrize("out", sorted(OUTS))
def test_identity_ranges_equal_the_colourless_loader(out):
    layout, dtype = OUTS[out]
    x, y = _random_set(23, 13, seed=6)
    kw = dict(train=True, seed=5, stream=2, layout=layout, dtype=dtype)
    a = DeviceImageLoader(x, y, 6, 8, distort=True, **kw)
    b = DeviceImageLoader(x, y, 6, 8, distort={"color": IDENTITY}, **kw)
    assert torch.equal(a.perm, b.perm)
    assert set(map(tuple, b.color_table.tolist())) == {(4096, 0, 0, 0, 4096, 0, 0, 0, 4096)}
    for _ in range(5):                              # wraps past L = 23
        oa, la = a.next()
        ob, lb = b.next()
        assert torch.equal(_bits(oa), _bits(ob))
        assert torch.equal(la, lb) and torch.equal(a.rows_out, b.rows_out)
        assert torch.equal(a.crop_out, b.crop_out) and torch.equal(a.box_out, b.box_out)
        assert b.color_out[:, 1:].tolist() == [[256, 0]] * 6


# ---------------------------------------------------------------- 3. contrast 0: the mean alone
@pytest.mark.parametrize("S,crop", [(13, 8), (40, 34)])      # 34: 289 quads, two blocks of sums
def test_contrast_zero_writes_the_rounded_channel_mean(S, crop):
    x, y = _random_set(11, S, seed=2)
    col = _byte_loader(x, y, 4, crop, MEAN_ONLY, seed=8)
    plain = _byte_loader(x, y, 4, crop, None, seed=8)
    N = crop * crop
    for _ in range(3):
        got = _bytes(col.next()[0])
        s = _bytes(plain.next()[0]).sum((1, 2))                             # [B, 3]
        assert torch.equal(col.color_sums.to(torch.int64).sum(1), s)
        want = (2 * s + N) // (2 * N)                                       # floor(s / N + 1/2)
        assert torch.equal(got, want.view(4, 1, 1, 3).expand(4, crop, crop, 3))


# ------------------------------------------------------------------------------------ 4. clamp
def test_both_clamps_are_reached():
    x, y = _random_set(16, 12, seed=1)
    ld = _byte_loader(x, y, 8, 8, {"contrast": (1.5, 1.5), "brightness": 32.0 / 255.0}, seed=0)
    lo = hi = False
    for _ in range(2):
        v = _bytes(ld.next()[0])
        assert int(v.min()) >= 0 and int(v.max()) <= 255
        lo, hi = lo or bool((v == 0).any()), hi or bool((v == 255).any())
    assert lo and hi


# ------------------------------------------------------------------------------------ 5. draws
def _run_draws(color, seed=5, stream=0, steps=4, start=0):
    x, y = _random_set(16, 12, seed=4)
    ld = _byte_loader(x, y, 8, 4, color, seed=seed, stream=stream)
    ld.cursor.fill_(start)
    geo, col = [], []
    for _ in range(steps):
        ld.next()
        geo.append(torch.cat([ld.crop_out, ld.box_out, ld.rows_out.view(-1, 1)], 1).clone())
        col.append(None if ld.color_out is None else ld.color_out.clone())
    return torch.cat(geo), (None if col[0] is None else torch.cat(col))


def test_geometry_draws_do_not_depend_on_colour():
    g0, c0 = _run_draws(None)
    g1, c1 = _run_draws(True)
    assert c0 is None and torch.equal(g0, g1)


def test_colour_draws_depend_on_seed_stream_and_position_alone():
    _, c = _run_draws(True)
    assert torch.equal(c, _run_draws(True)[1])
    assert torch.equal(c[16:], _run_draws(True, steps=2, start=2)[1])       # a rewound cursor
    assert not torch.equal(c, _run_draws(True, stream=1)[1])
    assert not torch.equal(c, _run_draws(True, seed=6)[1])
    # ... and they are reference.image_color_draws of the position
    m, k, d = reference.image_color_draws(torch.arange(32), 1024, 128, 384, 32, 5, 0)
    assert torch.equal(c.to(torch.int64), torch.stack([m, k, d], 1))


def test_colour_draws_cover_their_ranges():
    # 60000 positions: a value of the largest range (1024 matrices) is missed with probability
    # 1024 (1 - 1/1024)^60000 < 1e-22
    m, k, d = reference.image_color_draws(torch.arange(60000), 1024, 128, 384, 32, 99, 3)
    assert sorted(set(m.tolist())) == list(range(1024))
    assert sorted(set(k.tolist())) == list(range(128, 385))
    assert sorted(set(d.tolist())) == list(range(-32, 33))


# ----------------------------------------------------------------------- 6. the table, checking
def test_color_matrix_table():
    t = reference.color_matrix_table()
    assert t.dtype == torch.int32 and tuple(t.shape) == (1024, 9)
    # each row is the rounded real matrix of its grid point
    for m in (0, 31, 500, 1023):
        want = np.floor(_matrix(m, reference.COLOR_SATURATION, reference.COLOR_HUE) * 4096 + 0.5)
        assert t[m].tolist() == want.reshape(9).astype(np.int64).tolist()
    assert reference.color_coefficient_bound(t, 128, 384, 32) <= 2 ** 31 - 1
    for kw in (dict(saturation=(1.5, 0.5)), dict(saturation=(-0.1, 1.0)), dict(hue=-0.1),
               dict(hue=4.0), dict(saturation=(0.5, math.inf))):
        with pytest.raises(ValueError):
            reference.color_matrix_table(**kw)


@pytest.mark.parametrize("color", [
    {"contrast": (1.5, 0.5)}, {"contrast": (-0.1, 1.0)}, {"contrast": (0.5, 17.0)},
    {"brightness": -0.1}, {"brightness": 1.5}, {"saturation": (2.0, 1.0)}, {"hue": 4.0},
    {"tint": 1.0}, "yes", 1,
    {"contrast": (0.5, 16.0)},                      # legal ranges that pass 2^31 per pixel
    {"saturation": (0.0, 40.0)},
])
def test_bad_colour_ranges_raise(color):
    x, y = _random_set(8, 18)
    with pytest.raises(ValueError):
        DeviceImageLoader(x, y, 4, 8, distort={"color": color})


def test_colour_needs_training_and_false_means_off():
    x, y = _random_set(8, 18)
    with pytest.raises(ValueError):
        DeviceImageLoader(x, y, 4, 8, train=False, distort={"color": True})
    off = DeviceImageLoader(x, y, 4, 8, distort={"color": False})
    assert off.distort == {"area": [0.05, 1.0], "aspect": [0.75, 1.33]}
    assert off.color_table is None and off.color_out is None


def test_argument_forms():
    x, y = _random_set(8, 18)
    a = DeviceImageLoader(x, y, 4, 8, distort={"color": True})
    assert a.distort["color"] == {"brightness": 32.0 / 255.0, "saturation": [0.5, 1.5],
                                  "hue": 0.2 * math.pi, "contrast": [0.5, 1.5]}
    assert a.color_q == (128, 384, 32) and tuple(a.color_out.shape) == (4, 3)
    assert torch.equal(a.color_table, reference.color_matrix_table())
    b = DeviceImageLoader(x, y, 4, 8, distort={"area": (0.3, 0.6), "color": {"contrast": (0, 2)}})
    assert b.distort["area"] == [0.3, 0.6] and b.color_q == (0, 512, 32)


def test_set_color_table_checks_and_writes_in_place():
    x, y = _random_set(8, 18)
    ld = _byte_loader(x, y, 4, 8, True)
    buf = ld.color_table
    flipped = reference.color_matrix_table().flip(0)
    ld.set_color_table(flipped)
    assert ld.color_table is buf and torch.equal(buf, flipped)   # a captured next() reads this
    eye = torch.tensor([[4096, 0, 0, 0, 4096, 0, 0, 0, 4096]])
    ld.set_color_table(eye)
    assert ld.color_table.dtype == torch.int32 and ld.color_table.shape == (1, 9)
    ld.next()
    assert ld.color_out[:, 0].tolist() == [0] * 4
    for bad in (eye.view(3, 3), eye.float(), torch.zeros(0, 9, dtype=torch.int32),
                eye.expand(4097, 9), eye * 200):     # 200 I: 384 * 819200 * 255 passes 2^31
        with pytest.raises(ValueError):
            ld.set_color_table(bad)
    with pytest.raises(ValueError):
        _byte_loader(x, y, 4, 8, None).set_color_table(eye)


def test_state_dict_round_trip_and_mismatch():
    x, y = _random_set(20, 12, seed=8)
    kw = dict(train=True, seed=4, stream=2, dtype=torch.float32)
    a = DeviceImageLoader(x, y, 6, 8, distort={"color": True}, **kw)
    a.next()
    a.new_epoch()
    a.next()
    sd = a.state_dict()
    assert sd["distort"]["color"] == a.distort["color"]
    b = DeviceImageLoader(x, y, 6, 8, distort={"color": True}, **kw)
    b.load_state_dict(sd)
    for _ in range(3):
        oa, la = a.next()
        ob, lb = b.next()
        assert torch.equal(oa, ob) and torch.equal(la, lb)
        assert torch.equal(a.color_out, b.color_out) and torch.equal(a.box_out, b.box_out)
    plain = DeviceImageLoader(x, y, 6, 8, distort=True, **kw)
    assert "color" not in plain.state_dict()["distort"]
    with pytest.raises(ValueError, match="distort"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="distort"):
        b.load_state_dict(plain.state_dict())
    other = DeviceImageLoader(x, y, 6, 8, distort={"color": {"contrast": (0.8, 1.2)}}, **kw)
    with pytest.raises(ValueError, match="distort"):
        other.load_state_dict(sd)


# --------------------------------------------------------------------------------- 7. cnn_bench
BENCH = ["--device", "cpu", "--synth_images", "256", "--stored_size", "36", "--image_size", "32",
         "--model", "resnet_tiny", "--width", "8", "--num_classes", "4", "--batch_size", "16",
         "--dtype", "fp32", "--graph", "0", "--json"]


def _run(tmp_path, argv):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(ARENA_HEARTBEAT_FILE=str(tmp_path / "hb"))
    return subprocess.run([sys.executable, "-m", "arena_amd.examples.cnn_bench", *argv],
                          capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)


def test_cnn_bench_with_distort_color(tmp_path):
    r = _run(tmp_path, [*BENCH, "--distortions", "--distort_color", "--num_batches", "3",
                        "--num_warmup_batches", "0"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    head = [ln for ln in r.stdout.splitlines() if ln.startswith("Model: ")]
    assert len(head) == 1 and "(256 images, 36 -> 32 distorted+color)" in head[0], head
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["distortions"] is True and res["distort_color"] is True
    assert res["crop_boxes"] == 1815


@pytest.mark.parametrize("argv,msg", [
    (["--synth_images", "64", "--distort_color"], "--distort_color needs --distortions"),
    (["--synth_images", "64", "--distortions", "--distort_color", "--eval"],
     "does not apply to --eval"),
    (["--synth_images", "64", "--distort_color", "--eval"], "--distort_color does not apply"),
])
def test_cnn_bench_flag_errors(tmp_path, argv, msg):
    r = _run(tmp_path, ["--device", "cpu", *argv])
    assert r.returncode == 2 and msg in r.stderr, r.stderr[-1000:]
