"""Image-classification datasets for the ResNet path: a directory of uint8 ``.npy`` shards that is
loaded whole into the GPU's memory, and a deterministic synthetic stand-in with no files.

The reference's user guide trains from a mounted ``--data`` directory
(``docs/userguide/4-tfjob-distributed-data.md``). Here the data stays *resident*: 288 GB of HBM
hold 1.28 M images of 128x128 (63 GB) or 500 k of 256x256 (98 GB) as uint8, and the input
pipeline is one kernel per step (``arena_amd.ops.data.DeviceImageLoader``). Decoding JPEG and
streaming from the host are out of scope: convert once, offline, with ``write_images``.

Directory format
    ``{split}_images_{k:05d}.npy``  uint8 ``[n_k, S, S, 3]`` (NHWC, one stored size S per dir)
    ``{split}_labels_{k:05d}.npy``  int64 or int32 ``[n_k]``
    ``meta.json`` (optional)        ``{"num_classes": C, "mean": [r, g, b], "std": [r, g, b]}``
with ``split`` in ``train`` / ``val`` and ``k`` = 0, 1, .... Mean and std are in 0..1 units and
default to ImageNet's; ``num_classes`` defaults to ``max(label) + 1``.

    python -m arena_amd.data.images --out DIR --synthetic N --size S --classes C
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ..ops.data import IMAGENET_MEAN, IMAGENET_STD
from ..ops.reference import hash4

SPLITS = ("train", "val")
CHUNK_BYTES = 64 << 20      # host staging per copy: the loader's peak host memory


def _shard_paths(data_dir: str, split: str, k: int) -> Tuple[str, str]:
    return (os.path.join(data_dir, f"{split}_images_{k:05d}.npy"),
            os.path.join(data_dir, f"{split}_labels_{k:05d}.npy"))


def _open_shards(data_dir: str, split: str):
    """Memory-mapped (images, labels) per shard, validated; raises ValueError naming the file."""
    if split not in SPLITS:
        raise ValueError(f"split must be one of {SPLITS}, got {split!r}")
    shards, size = [], None
    k = 0
    while True:
        ip, lp = _shard_paths(data_dir, split, k)
        if not os.path.exists(ip):
            break
        if not os.path.exists(lp):
            raise ValueError(f"{ip} has no label shard {lp}")
        im = np.load(ip, mmap_mode="r")
        lb = np.load(lp, mmap_mode="r")
        if im.dtype != np.uint8:
            raise ValueError(f"{ip}: images must be uint8, found {im.dtype}")
        if im.ndim != 4 or im.shape[3] != 3 or im.shape[1] != im.shape[2]:
            raise ValueError(f"{ip}: images must be [n, S, S, 3], found shape {tuple(im.shape)}")
        if size is None:
            size = im.shape[1]
        if im.shape[1] != size:
            raise ValueError(f"{ip}: stored size {im.shape[1]} differs from the directory's {size}")
        if lb.dtype not in (np.int64, np.int32) or lb.ndim != 1:
            raise ValueError(f"{lp}: labels must be int64 or int32 [n], found {lb.dtype} "
                             f"{tuple(lb.shape)}")
        if lb.shape[0] != im.shape[0]:
            raise ValueError(f"{lp}: {lb.shape[0]} labels for the {im.shape[0]} images of {ip}")
        shards.append((im, lb))
        k += 1
    if not shards:
        raise ValueError(f"no {split}_images_00000.npy in {data_dir}")
    return shards, size


def read_meta(data_dir: str) -> dict:
    meta = {"mean": list(IMAGENET_MEAN), "std": list(IMAGENET_STD)}
    path = os.path.join(data_dir, "meta.json")
    if os.path.exists(path):
        with open(path) as f:
            got = json.load(f)
        for key in ("mean", "std"):
            if key in got:
                v = [float(x) for x in got[key]]
                if len(v) != 3 or (key == "std" and min(v) <= 0):
                    raise ValueError(f"{path}: {key} must be three floats (std positive)")
                meta[key] = v
        if "num_classes" in got:
            meta["num_classes"] = int(got["num_classes"])
    return meta


def check_fits(nbytes: int, device: torch.device, reserve_gb: float) -> None:
    """Refuse a dataset that would not leave ``reserve_gb`` of the device's free memory."""
    if device.type != "cuda":
        return
    free, _ = torch.cuda.mem_get_info(device)
    need = nbytes + int(reserve_gb * (1 << 30))
    if need > free:
        raise MemoryError(
            f"the dataset shard needs {nbytes / 2**30:.1f} GiB on {device} plus {reserve_gb:g} GiB "
            f"to train, but only {free / 2**30:.1f} GiB are free; store smaller images, use more "
            "ranks (each holds 1/world of the rows), or lower reserve_gb (datasets are resident: "
            "there is no streaming from the host)")


def load_images(data_dir: str, split: str, device, rank: int = 0, world: int = 1, *,
                reserve_gb: float = 16.0):
    """(images uint8 ``[L, S, S, 3]``, labels int64 ``[L]``, meta) on ``device``: the rows with
    ``global_index % world == rank`` of the split, copied shard by shard through one host chunk.
    meta: ``num_classes``, ``mean``, ``std``, ``size`` and ``n`` (rows of the whole split)."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside world {world}")
    device = torch.device(device)
    shards, size = _open_shards(data_dir, split)
    meta = read_meta(data_dir)
    total = sum(im.shape[0] for im, _ in shards)
    mine = len(range(rank, total, world))
    if mine == 0:
        raise ValueError(f"{data_dir}: rank {rank} of {world} gets no {split} rows ({total} in all)")
    row_bytes = size * size * 3
    check_fits(mine * row_bytes, device, reserve_gb)
    images = torch.empty((mine, size, size, 3), dtype=torch.uint8, device=device)
    labels = torch.empty(mine, dtype=torch.int64, device=device)
    step = max(1, CHUNK_BYTES // row_bytes)
    g0 = done = 0
    max_label = -1
    for im, lb in shards:
        first = (rank - g0) % world             # this rank's first row inside the shard
        idx = np.arange(first, im.shape[0], world)
        for a in range(0, idx.size, step):
            sel = idx[a:a + step]
            if world == 1:
                chunk = np.array(im[sel[0]:sel[-1] + 1])
            else:
                chunk = np.array(im[sel])
            images[done:done + sel.size].copy_(torch.from_numpy(chunk))
            lab = torch.from_numpy(np.array(lb[sel], dtype=np.int64))
            max_label = max(max_label, int(lab.max()))
            labels[done:done + sel.size].copy_(lab)
            done += sel.size
        g0 += im.shape[0]
    assert done == mine
    if "num_classes" not in meta:
        # every rank must agree: the maximum over the whole split, not over this rank's rows
        meta["num_classes"] = max(int(np.asarray(lb).max()) for _, lb in shards) + 1
    elif max_label >= meta["num_classes"]:
        raise ValueError(f"{data_dir}: label {max_label} but meta.json says "
                         f"num_classes = {meta['num_classes']}")
    meta["size"], meta["n"] = size, total
    return images, labels, meta


def write_images(out_dir: str, split: str, images, labels, shard: int = 4096,
                 meta: Optional[dict] = None) -> int:
    """Write ``images`` (uint8 ``[n, S, S, 3]``) and ``labels`` (``[n]``) as shards of ``shard``
    rows (or, with a sequence of ints, of exactly those lengths); ``meta`` goes to meta.json.
    Returns the number of shards."""
    if split not in SPLITS:
        raise ValueError(f"split must be one of {SPLITS}, got {split!r}")
    im = images.cpu().numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
    lb = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if im.dtype != np.uint8 or im.ndim != 4 or im.shape[3] != 3 or im.shape[1] != im.shape[2]:
        raise ValueError("images must be uint8 [n, S, S, 3]")
    if lb.ndim != 1 or lb.shape[0] != im.shape[0] or lb.dtype.kind not in "iu":
        raise ValueError("labels must be integers [n]")
    n = im.shape[0]
    lens = [int(s) for s in shard] if isinstance(shard, (list, tuple)) else None
    if lens is None:
        if shard < 1:
            raise ValueError("shard must be positive")
        lens = [min(shard, n - a) for a in range(0, n, shard)]
    if sum(lens) != n or min(lens, default=0) < 1:
        raise ValueError(f"shard lengths {lens} do not add up to {n} rows")
    os.makedirs(out_dir, exist_ok=True)
    a = 0
    for k, m in enumerate(lens):
        ip, lp = _shard_paths(out_dir, split, k)
        np.save(ip, im[a:a + m])
        np.save(lp, lb[a:a + m].astype(np.int32 if lb.dtype == np.int32 else np.int64))
        a += m
    if meta is not None:
        with open(os.path.join(out_dir, "meta.json"), "w") as f:
            json.dump({k: meta[k] for k in ("num_classes", "mean", "std") if k in meta}, f)
    return len(lens)


def synthetic_images(n: int, size: int, num_classes: int, seed: int = 0, *, draw: int = 0,
                     device="cpu", noise: int = 24) -> Tuple[torch.Tensor, torch.Tensor]:
    """A deterministic, learnable dataset: (uint8 ``[n, size, size, 3]``, int64 ``[n]``).

    Each class owns a colour and a low-frequency texture (a seeded 4x4 grid, bilinearly enlarged);
    sample i of draw ``draw`` is its class's pattern rolled by up to size/8 pixels each way plus
    uniform pixel noise of +-``noise``, all from the counter hash of ``(seed, draw, i)``, so the
    same arguments give the same bytes on any device. ``draw`` separates splits that share the
    classes (0: train, 1: val)."""
    if n < 1 or size < 2 or num_classes < 1:
        raise ValueError("synthetic_images: n >= 1, size >= 2, num_classes >= 1")
    device = torch.device(device)
    g = torch.Generator().manual_seed(seed)
    colour = torch.rand(num_classes, 3, 1, 1, generator=g) * 150.0 + 50.0
    grid = (torch.rand(num_classes, 3, 4, 4, generator=g) - 0.5) * 90.0
    labels = torch.empty(n, dtype=torch.int64, device=device)
    images = torch.empty((n, size, size, 3), dtype=torch.uint8, device=device)
    pats = torch.empty((num_classes, size, size, 3), dtype=torch.uint8, device=device)
    for a in range(0, num_classes, 64):     # the enlargement always runs on the host: same bytes
        tex = torch.nn.functional.interpolate(grid[a:a + 64], size=(size, size), mode="bilinear",
                                              align_corners=True)
        pats[a:a + 64] = (colour[a:a + 64] + tex).clamp(0, 255).round().to(torch.uint8) \
            .permute(0, 2, 3, 1).to(device)
    span = 2 * (size // 8) + 1
    ar = torch.arange(size, dtype=torch.int64, device=device)
    pix = torch.arange(size * size * 3, dtype=torch.int64, device=device).view(1, -1)
    step = max(1, (32 << 20) // (size * size * 3))
    for a in range(0, n, step):
        i = torch.arange(a, min(a + step, n), dtype=torch.int64, device=device)
        m = i.numel()
        zero = torch.zeros_like(i)
        lab = (hash4(seed, 4 * draw, i, zero) * num_classes) >> 32
        dy = ((hash4(seed, 4 * draw + 1, i, zero) * span) >> 32) - size // 8
        dx = ((hash4(seed, 4 * draw + 2, i, zero) * span) >> 32) - size // 8
        ys = (ar.view(1, size) + dy.view(m, 1)) % size
        xs = (ar.view(1, size) + dx.view(m, 1)) % size
        img = pats[lab.view(m, 1, 1), ys.view(m, size, 1), xs.view(m, 1, size)].to(torch.int16)
        h = hash4(seed, 4 * draw + 3, i.view(m, 1), pix)           # one byte of noise per value
        nz = (((h & 0xFFFF) * (2 * noise + 1)) >> 16) - noise
        images[a:a + m] = (img + nz.view(m, size, size, 3).to(torch.int16)).clamp(0, 255) \
            .to(torch.uint8)
        labels[a:a + m] = lab
    return images, labels


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(description="write a synthetic image dataset in the shard format")
    ap.add_argument("--out", required=True)
    ap.add_argument("--synthetic", type=int, required=True, metavar="N", help="training images")
    ap.add_argument("--val", type=int, default=None, help="validation images (default N // 10)")
    ap.add_argument("--size", type=int, default=256, help="stored size S")
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--shard", type=int, default=4096, help="rows per shard file")
    args = ap.parse_args(argv)
    meta = {"num_classes": args.classes, "mean": list(IMAGENET_MEAN), "std": list(IMAGENET_STD)}
    n_val = max(1, args.synthetic // 10) if args.val is None else args.val
    for split, n, draw in (("train", args.synthetic, 0), ("val", n_val, 1)):
        if n < 1:
            continue
        x, y = synthetic_images(n, args.size, args.classes, args.seed, draw=draw)
        k = write_images(args.out, split, x, y, shard=args.shard, meta=meta)
        print(f"{split}: {n} images of {args.size}x{args.size} in {k} shards -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
