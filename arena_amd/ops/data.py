"""Device-resident image loader: the dataset stays in HBM as uint8, a device permutation and a
device cursor select the rows, and one HIP kernel (``csrc/ops/data_kernels.hip``) writes the
cropped, flipped, normalised batch -- in the stem's space-to-depth layout when the model takes it.
No host work per step: ``next()`` is one launch that a captured graph replays, batch k, k+1, ....

GPU tensors go to the extension (raises if it is missing), CPU tensors to the bit-compatible
reference (``ops/reference.py image_batch``).
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import _ext, reference

Tensor = torch.Tensor

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
LAYOUTS = {"s2d": 0, "nhwc": 1}


def _impl(t: Tensor):
    return _ext.load() if t.is_cuda else reference


class DeviceImageLoader:
    """Batches of ``images`` (uint8 ``[n, S, S, 3]``) / ``labels`` (``[n]``) on their device.

    ``train=True``: rows in a shuffled order that wraps (``steps_per_epoch = L // B``; call
    ``new_epoch()`` between epochs), a random ``crop`` x ``crop`` window and a random horizontal
    flip per image, drawn from ``(seed, stream, position)`` alone. ``train=False``: rows in order,
    centre crop, ``ceil(L / B)`` batches whose tail is padded with label -100 (``cross_entropy``'s
    ``ignore_index``). ``stream`` separates the draws of data-parallel ranks.

    ``layout="s2d"`` yields ``z`` bf16 ``[B, 16, crop/2, crop/2]`` (``ResNet.forward(z,
    s2d=True)``), ``"nhwc"`` yields ``x`` ``[B, 3, crop, crop]`` in ``dtype``; both channels_last.
    ``next()`` returns the loader's static buffers: the same tensors every call, so a captured
    step reads them in place.
    """

    def __init__(self, images: Tensor, labels: Tensor, batch: int, crop: int, *, train: bool = True,
                 seed: int = 0, stream: int = 0, mean: Sequence[float] = IMAGENET_MEAN,
                 std: Sequence[float] = IMAGENET_STD, layout: str = "nhwc",
                 dtype: torch.dtype = torch.bfloat16):
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 \
                or images.shape[1] != images.shape[2]:
            raise ValueError("images must be uint8 [n, S, S, 3]")
        if labels.dim() != 1 or labels.shape[0] != images.shape[0] or labels.device != images.device:
            raise ValueError("labels must be [n] on the images' device")
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(LAYOUTS)}")
        if layout == "s2d" and dtype != torch.bfloat16:
            raise ValueError("the space-to-depth layout is bf16")
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("dtype must be bfloat16 or float32")
        n, S = images.shape[0], images.shape[1]
        crop = int(crop)
        if crop < 2 or crop % 2 or crop > S:
            raise ValueError(f"crop must be even and in [2, {S}] (stored size), got {crop}")
        if batch < 1 or n < 1:
            raise ValueError("empty batch or dataset")
        dev = images.device
        self.images = images.contiguous()
        self.labels = labels.to(torch.int64).contiguous()
        self.batch, self.crop, self.train = int(batch), crop, bool(train)
        self.seed, self.stream, self.layout = int(seed), int(stream), layout
        self.L = n
        self.steps_per_epoch = n // self.batch if train else -(-n // self.batch)
        self.table = reference.image_table(mean, std, dtype).to(dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.perm = torch.arange(n, dtype=torch.int32, device=dev)
        shape = (batch, 16, crop // 2, crop // 2) if layout == "s2d" else (batch, 3, crop, crop)
        self.out = torch.empty(shape, dtype=dtype, device=dev,
                               memory_format=torch.channels_last).zero_()
        self.labels_out = torch.zeros(batch, dtype=torch.int64, device=dev)
        self.rows_out = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.crop_out = torch.zeros(batch, 3, dtype=torch.int32, device=dev)
        self.epoch = 0
        self._gen = torch.Generator(device=dev).manual_seed(self.seed * 7919 + self.stream)
        if self.train:
            self._shuffle()

    def _shuffle(self) -> None:
        # drawn on the device (no host sync); a permutation of range(L), so every entry is a row
        self.perm.copy_(torch.randperm(self.L, generator=self._gen, device=self.perm.device))

    def next(self, advance: bool = True) -> Tuple[Tensor, Tensor]:
        """Write the batch at the cursor into the static buffers and (``advance``) move the
        cursor on, all on the device. Returns ``(x or z, labels)``."""
        _impl(self.images).image_batch(
            self.images, self.labels, self.perm, self.cursor, self.table, self.out,
            self.labels_out, self.rows_out, self.crop_out, self.crop, self.crop, self.train,
            self.seed, self.stream, LAYOUTS[self.layout], bool(advance))
        return self.out, self.labels_out

    def new_epoch(self) -> None:
        """A new shuffled order (training) and the cursor back to 0; enqueued on the device, so it
        may sit between two replays of a graph that holds ``next()``."""
        self.epoch += 1
        if self.train:
            self._shuffle()
        self.cursor.zero_()

    def set_permutation(self, perm: Tensor) -> None:
        """Replace the row order (any length >= 1); every entry must be a dataset row."""
        perm = perm.to(device=self.perm.device, dtype=torch.int32).reshape(-1).contiguous()
        if perm.numel() < 1 or int(perm.min()) < 0 or int(perm.max()) >= self.images.shape[0]:
            raise ValueError("permutation entries must be dataset rows")
        if perm.numel() == self.perm.numel():
            self.perm.copy_(perm)      # in place: a captured next() keeps reading this buffer
        else:
            self.perm = perm
        self.L = perm.numel()
        self.steps_per_epoch = self.L // self.batch if self.train else -(-self.L // self.batch)

    def state_dict(self) -> dict:
        return {"perm": self.perm.detach().cpu().clone(), "cursor": int(self.cursor.item()),
                "epoch": self.epoch, "rng": self._gen.get_state().clone(),
                "seed": self.seed, "stream": self.stream}

    def load_state_dict(self, sd: dict) -> None:
        if (sd["seed"], sd["stream"]) != (self.seed, self.stream):
            raise ValueError("loader state belongs to another seed / stream")
        self.set_permutation(sd["perm"])
        self.cursor.fill_(int(sd["cursor"]))
        self.epoch = int(sd["epoch"])
        self._gen.set_state(sd["rng"])
