"""Device-resident image loader: the dataset stays in HBM as uint8, a device permutation and a
device cursor select the rows, and one HIP kernel (``csrc/ops/data_kernels.hip``) writes the
cropped, flipped, normalised batch -- in the stem's space-to-depth layout when the model takes it.
No host work per step: ``next()`` is one launch that a captured graph replays, batch k, k+1, ....
With ``distort`` the window is a random box of random area and aspect ratio, resized to the crop by
a second kernel of the same file (random resized crop); with its ``"color"`` key that kernel also
applies tf_cnn_benchmarks' colour distortion (YIQ form), after a launch that sums each crop's
channels for the contrast step.

GPU tensors go to the extension (raises if it is missing), CPU tensors to the bit-compatible
reference (``ops/reference.py image_batch`` / ``image_batch_resized`` / ``image_batch_color``).
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _ext, reference

Tensor = torch.Tensor

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
LAYOUTS = {"s2d": 0, "nhwc": 1}


def _impl(t: Tensor):
    return _ext.load() if t.is_cuda else reference


def color_ranges(color) -> Optional[dict]:
    """``color`` (None / False, True or a dict with any of ``brightness`` (largest |delta| in
    [0, 1]), ``saturation`` (lo, hi), ``hue`` (largest |angle| in radians) and ``contrast``
    (lo, hi)) -> the four ranges, or None."""
    if color is None or color is False:
        return None
    if color is True:
        color = {}
    if not isinstance(color, dict) or set(color) - {"brightness", "saturation", "hue", "contrast"}:
        raise ValueError("distort['color'] must be True or a dict with 'brightness', "
                         "'saturation', 'hue' and / or 'contrast'")
    return {"brightness": float(color.get("brightness", reference.COLOR_BRIGHTNESS)),
            "saturation": [float(v) for v in color.get("saturation", reference.COLOR_SATURATION)],
            "hue": float(color.get("hue", reference.COLOR_HUE)),
            "contrast": [float(v) for v in color.get("contrast", reference.COLOR_CONTRAST)]}


def distort_ranges(distort) -> Optional[dict]:
    """``distort`` (None / False, True or ``{"area": (lo, hi), "aspect": (lo, hi), "color":
    ...}``) -> the two ranges as lists, plus the colour ranges (``color_ranges``) when the colour
    distortion is on; or None."""
    if distort is None or distort is False:
        return None
    if distort is True:
        distort = {}
    if not isinstance(distort, dict) or set(distort) - {"area", "aspect", "color"}:
        raise ValueError("distort must be None, True or a dict with 'area', 'aspect' and / or "
                         "'color'")
    out = {"area": [float(v) for v in distort.get("area", reference.CROP_AREA)],
           "aspect": [float(v) for v in distort.get("aspect", reference.CROP_ASPECT)]}
    color = color_ranges(distort.get("color"))
    if color is not None:
        out["color"] = color
    return out


class DeviceImageLoader:
    """Batches of ``images`` (uint8 ``[n, S, S, 3]``) / ``labels`` (``[n]``) on their device.

    ``train=True``: rows in a shuffled order that wraps (``steps_per_epoch = L // B``; call
    ``new_epoch()`` between epochs), a random ``crop`` x ``crop`` window and a random horizontal
    flip per image, drawn from ``(seed, stream, position)`` alone. ``train=False``: rows in order,
    centre crop, ``ceil(L / B)`` batches whose tail is padded with label -100 (``cross_entropy``'s
    ``ignore_index``). ``stream`` separates the draws of data-parallel ranks.

    ``distort`` (training only): ``True`` or ``{"area": (lo, hi), "aspect": (lo, hi)}`` takes a
    random box of that share of the area and that width / height instead of the fixed window and
    resizes it to the crop (``box_out`` int32 ``[B, 2]``: the drawn ``(h, w)``). Its key
    ``"color"`` (``True`` for tf_cnn_benchmarks' ranges, or a dict: ``color_ranges``) adds a random
    brightness, saturation, hue and contrast per image, clipped to the byte range (``color_out``
    int32 ``[B, 3]``: matrix index, contrast in 1/256ths, brightness in bytes).

    ``layout="s2d"`` yields ``z`` bf16 ``[B, 16, crop/2, crop/2]`` (``ResNet.forward(z,
    s2d=True)``), ``"nhwc"`` yields ``x`` ``[B, 3, crop, crop]`` in ``dtype``; both channels_last.
    ``next()`` returns the loader's static buffers: the same tensors every call, so a captured
    step reads them in place.
    """

    def __init__(self, images: Tensor, labels: Tensor, batch: int, crop: int, *, train: bool = True,
                 seed: int = 0, stream: int = 0, mean: Sequence[float] = IMAGENET_MEAN,
                 std: Sequence[float] = IMAGENET_STD, layout: str = "nhwc",
                 dtype: torch.dtype = torch.bfloat16, distort=None):
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
        self.distort = distort_ranges(distort)
        if self.distort is not None and not train:
            raise ValueError("distort applies to training; evaluation takes the centre crop")
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
        self.boxes = self.box_out = None
        if self.distort is not None:
            self.box_out = torch.zeros(batch, 2, dtype=torch.int32, device=dev)
            self.set_boxes(reference.crop_box_table(S, self.distort["area"],
                                                    self.distort["aspect"]))
        self.color_table = self.color_out = self.color_sums = self.color_q = None
        if self.distort is not None and "color" in self.distort:
            col = self.distort["color"]
            self.color_q = reference.color_quantised_ranges(col["brightness"], col["contrast"])
            self.color_out = torch.zeros(batch, 3, dtype=torch.int32, device=dev)
            self.color_sums = torch.zeros(batch, reference.image_sum_blocks(crop, crop), 3,
                                          dtype=torch.int32, device=dev)
            self.set_color_table(reference.color_matrix_table(col["saturation"], col["hue"]))
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
        if self.boxes is None:
            _impl(self.images).image_batch(
                self.images, self.labels, self.perm, self.cursor, self.table, self.out,
                self.labels_out, self.rows_out, self.crop_out, self.crop, self.crop, self.train,
                self.seed, self.stream, LAYOUTS[self.layout], bool(advance))
        elif self.color_table is not None:
            _impl(self.images).image_batch_color(
                self.images, self.labels, self.perm, self.cursor, self.table, self.out,
                self.labels_out, self.rows_out, self.crop_out, self.boxes, self.box_out,
                self.color_table, self.color_sums, self.color_out, self.crop, self.crop,
                self.train, self.seed, self.stream, *self.color_q, LAYOUTS[self.layout],
                bool(advance))
        else:
            _impl(self.images).image_batch_resized(
                self.images, self.labels, self.perm, self.cursor, self.table, self.out,
                self.labels_out, self.rows_out, self.crop_out, self.boxes, self.box_out,
                self.crop, self.crop, self.train, self.seed, self.stream, LAYOUTS[self.layout],
                bool(advance))
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

    def set_boxes(self, boxes: Tensor) -> None:
        """Replace the candidate ``(h, w)`` boxes of a distorting loader (int ``[T, 2]``, ``1 <= T
        <= 4096``); every entry must lie in ``[2, S]``."""
        if self.distort is None:
            raise ValueError("set_boxes needs a loader built with distort")
        S = self.images.shape[1]
        if boxes.dim() != 2 or boxes.shape[1] != 2 or boxes.dtype.is_floating_point \
                or not 1 <= boxes.shape[0] <= reference.MAX_CROP_BOXES:
            raise ValueError(f"boxes must be integer [T, 2] with 1 <= T <= "
                             f"{reference.MAX_CROP_BOXES}")
        if int(boxes.min()) < 2 or int(boxes.max()) > S:
            raise ValueError(f"box sides must lie in [2, {S}] (stored size)")
        boxes = boxes.to(device=self.images.device, dtype=torch.int32).contiguous()
        if self.boxes is not None and boxes.shape == self.boxes.shape:
            self.boxes.copy_(boxes)    # in place: a captured next() keeps reading this buffer
        else:
            self.boxes = boxes.clone()

    def set_color_table(self, matrices: Tensor) -> None:
        """Replace the candidate colour matrices of a loader built with ``distort["color"]`` (int
        ``[T, 9]``: row-major 3 x 3 in 1/4096ths, ``1 <= T <= 4096``). With the loader's contrast
        and brightness ranges every pixel's sum must stay inside 32 bits
        (``reference.color_coefficient_bound``)."""
        if self.color_q is None:
            raise ValueError("set_color_table needs a loader built with distort['color']")
        if matrices.dim() != 2 or matrices.shape[1] != 9 or matrices.dtype.is_floating_point \
                or not 1 <= matrices.shape[0] <= reference.MAX_COLOR_MATRICES:
            raise ValueError(f"matrices must be integer [T, 9] with 1 <= T <= "
                             f"{reference.MAX_COLOR_MATRICES}")
        if reference.color_coefficient_bound(matrices, *self.color_q) > 2 ** 31 - 1:
            raise ValueError("these colour matrices with the loader's contrast and brightness "
                             "ranges overflow the kernel's 32-bit pixel arithmetic")
        matrices = matrices.to(device=self.images.device, dtype=torch.int32).contiguous()
        if self.color_table is not None and matrices.shape == self.color_table.shape:
            self.color_table.copy_(matrices)   # in place: a captured next() keeps reading it
        else:
            self.color_table = matrices.clone()

    def state_dict(self) -> dict:
        return {"perm": self.perm.detach().cpu().clone(), "cursor": int(self.cursor.item()),
                "epoch": self.epoch, "rng": self._gen.get_state().clone(),
                "seed": self.seed, "stream": self.stream, "distort": distort_ranges(self.distort)}

    def load_state_dict(self, sd: dict) -> None:
        if (sd["seed"], sd["stream"]) != (self.seed, self.stream):
            raise ValueError("loader state belongs to another seed / stream")
        if "distort" in sd and distort_ranges(sd["distort"]) != self.distort:
            raise ValueError("loader state belongs to another distort setting")
        self.set_permutation(sd["perm"])
        self.cursor.fill_(int(sd["cursor"]))
        self.epoch = int(sd["epoch"])
        self._gen.set_state(sd["rng"])
