"""Learning-rate schedules that advance on the device, inside a captured training step.

A captured hipGraph bakes a ``float`` kernel argument in, so a schedule cannot reach the update
kernels as a host value. Here the learning rate is one fp32 value in device memory
(:class:`DeviceLR`): a one-lane kernel (``arena_lr_schedule`` in ``csrc/ops/optim_kernels.hip``)
at the head of every step evaluates the schedule at the device step counter, writes the value and
counts the step; every SGD update kernel reads it through its ``lr_ptr`` argument.

A schedule is a list of at most ``MAX_SEGMENTS`` segments ``(begin, end, lr0, lr1)``. ``t`` is the
number of completed optimizer steps (0-based); segments are contiguous, start at 0, and the last
one is open-ended (``end`` is None). Inside a segment the value is ``lr0`` when ``lr1 == lr0``,
else ``float32(lr0 + (lr1 - lr0) * ((t - begin) / (end - begin)))``: ``lr0`` / ``lr1`` are fp64,
every operation is an fp64 operation rounded on its own (no fused multiply-add), and the result
is rounded once to fp32. The open-ended segment holds its ``lr1``. :func:`reference_lr` is that
definition; the kernel matches it bit for bit.

The builders follow tf_cnn_benchmarks (``--piecewise_learning_rate_schedule``,
``--num_learning_rate_warmup_epochs``, ``--init_learning_rate`` / ``--num_epochs_per_decay`` /
``--learning_rate_decay_factor`` / ``--minimum_learning_rate``); epochs become steps by
``int(epochs * steps_per_epoch)``.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import fused

Tensor = torch.Tensor
Segment = Tuple[int, Optional[int], float, float]
MAX_SEGMENTS = 64


def validate(segments: Sequence) -> List[Segment]:
    """The segments as a list of ``(int, int | None, float, float)``; ValueError if they are not
    a schedule."""
    segs: List[Segment] = []
    for s in segments:
        if len(s) != 4:
            raise ValueError(f"a segment is (begin, end, lr0, lr1), got {s!r}")
        b, e, lr0, lr1 = s
        segs.append((int(b), None if e is None else int(e), float(lr0), float(lr1)))
    if not segs:
        raise ValueError("a schedule needs at least one segment")
    if len(segs) > MAX_SEGMENTS:
        raise ValueError(f"a schedule holds at most {MAX_SEGMENTS} segments, got {len(segs)}")
    if segs[0][0] != 0:
        raise ValueError(f"the first segment must begin at step 0, not {segs[0][0]}")
    for i, (b, e, lr0, lr1) in enumerate(segs):
        for v in (lr0, lr1):
            if not math.isfinite(v) or v < 0.0:
                raise ValueError(f"segment {i}: learning rate {v!r} must be finite and >= 0")
        last = i == len(segs) - 1
        if last:
            if e is not None:
                raise ValueError("the last segment is open-ended (end None)")
        else:
            if e is None or e <= b:
                raise ValueError(f"segment {i}: boundaries must increase (begin {b}, end {e})")
            if segs[i + 1][0] != e:
                raise ValueError(f"segment {i + 1} must begin where segment {i} ends ({e})")
    return segs


def reference_lr(segments: Sequence, t: int) -> np.float32:
    """The schedule's value after ``t`` completed steps (the definition the kernel matches)."""
    t = int(t)
    k = 0
    for i in range(1, len(segments)):
        if t >= segments[i][0]:
            k = i
    b, e, lr0, lr1 = segments[k]
    lr0, lr1 = float(lr0), float(lr1)
    if k == len(segments) - 1:
        v = lr1
    elif lr1 == lr0:
        v = lr0
    else:
        frac = float(t - b) / float(e - b)     # Python floats: fp64, one rounding per operation
        rise = (lr1 - lr0) * frac
        v = lr0 + rise
    return np.float32(v)


# ----------------------------------------------------------------------------------- builders
def constant(lr: float) -> List[Segment]:
    return validate([(0, None, lr, lr)])


def _from_values(values: Sequence[float], bounds: Sequence[int]) -> List[Segment]:
    """Value i holds for bounds[i-1] <= t < bounds[i] (bounds[-1] = 0)."""
    begins = [0] + [int(b) for b in bounds]
    segs = []
    for i, v in enumerate(values):
        end = begins[i + 1] if i + 1 < len(begins) else None
        segs.append((begins[i], end, v, v))
    return validate(segs)


def piecewise(spec: str, steps_per_epoch: float) -> List[Segment]:
    """tf_cnn_benchmarks' ``LR0;E1;LR1;...;En;LRn``: LRi from epoch Ei (E0 = 0) on."""
    parts = [p.strip() for p in str(spec).split(";")]
    if len(parts) % 2 == 0 or any(not p for p in parts):
        raise ValueError("a piecewise schedule is 'LR0;E1;LR1;...;En;LRn' (an odd number of "
                         f"fields), got {spec!r}")
    try:
        values = [float(p) for p in parts[0::2]]
        epochs = [float(p) for p in parts[1::2]]
    except ValueError:
        raise ValueError(f"piecewise schedule {spec!r}: every field must be a number") from None
    if len(values) > MAX_SEGMENTS:
        raise ValueError(f"a schedule holds at most {MAX_SEGMENTS} segments, got {len(values)}")
    return _from_values(values, [int(e * steps_per_epoch) for e in epochs])


def exponential(init_lr: float, epochs_per_decay: float, factor: float, min_lr: float,
                steps_per_epoch: float, total_steps: int) -> List[Segment]:
    """Staircase decay: ``max(init_lr * factor ** floor(t / decay_steps), min_lr)`` with
    ``decay_steps = int(epochs_per_decay * steps_per_epoch)``, laid out up to ``total_steps`` (or
    up to the stair that reaches ``min_lr``, whichever comes first)."""
    decay_steps = int(epochs_per_decay * steps_per_epoch)
    if decay_steps < 1:
        raise ValueError(f"{epochs_per_decay} epochs per decay at {steps_per_epoch} steps per "
                         "epoch is less than one step")
    if not 0.0 < factor <= 1.0:
        raise ValueError(f"the decay factor must lie in (0, 1], got {factor}")
    values, bounds = [], []
    k = 0
    while True:
        v = max(float(init_lr) * float(factor) ** k, float(min_lr))
        values.append(v)
        k += 1
        if v <= min_lr or factor == 1.0 or k * decay_steps >= max(int(total_steps), 1):
            break
        if len(values) >= MAX_SEGMENTS:
            raise ValueError(f"the staircase needs more than {MAX_SEGMENTS} segments over "
                             f"{total_steps} steps (decay every {decay_steps} steps)")
        bounds.append(k * decay_steps)
    return _from_values(values, bounds)


def with_warmup(segments: Sequence, warmup_epochs: float, steps_per_epoch: float) -> List[Segment]:
    """Linear warm-up over the first ``W = int(warmup_epochs * steps_per_epoch)`` steps:
    ``lr = base_lr0 * t / W`` for ``t < W`` (whatever the base schedule says there), the base
    schedule from ``W`` on."""
    base = validate(segments)
    W = int(warmup_epochs * steps_per_epoch)
    if W < 1:
        return base
    out: List[Segment] = [(0, W, 0.0, base[0][2])]
    for b, e, lr0, lr1 in base:
        if e is not None and e <= W:
            continue
        if b < W:
            if lr0 != lr1 and e is not None:
                raise ValueError("the warm-up must not end inside a ramp of the base schedule")
            b = W
        out.append((b, e, lr0, lr1))
    return validate(out)


# ------------------------------------------------------------------------------- device table
def encode(segments: Sequence, device) -> Tensor:
    """The segment table the kernel reads: int64 [n, 4] rows (begin, end or -1, lr0, lr1), the
    fp64 values stored as their bit patterns."""
    rows = []
    for b, e, lr0, lr1 in segments:
        bits = torch.tensor([lr0, lr1], dtype=torch.float64).view(torch.int64).tolist()
        rows.append([b, -1 if e is None else e] + bits)
    return torch.tensor(rows, dtype=torch.int64).to(device)


def decode(table: Tensor) -> List[Segment]:
    segs = []
    for b, e, x0, x1 in table.cpu().tolist():
        lr0, lr1 = torch.tensor([x0, x1], dtype=torch.int64).view(torch.float64).tolist()
        segs.append((b, None if e < 0 else e, lr0, lr1))
    return segs


class DeviceLR:
    """A schedule with its state where the update kernels read it.

    ``lr`` (fp32 [1]) and ``step`` (int64 [1]) live on ``device`` next to the segment table.
    :meth:`advance` enqueues ONE launch on the current stream: ``lr[0] = reference_lr(segments,
    step[0])``, then ``step[0] += 1``. Call it at the head of every training step, before the
    backward whose updates read ``lr``; captured into a hipGraph it moves the schedule on at
    every replay. On CPU tensors the reference runs instead."""

    def __init__(self, segments: Sequence, device="cpu"):
        self.segments = validate(segments)
        self.device = torch.device(device)
        self.lr = torch.full((1,), float(reference_lr(self.segments, 0)), dtype=torch.float32,
                             device=self.device)
        self.step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._table = encode(self.segments, self.device)

    def advance(self) -> None:
        fused.lr_schedule(self._table, self.step, self.lr)

    def reset(self, step: int = 0) -> None:
        """Continue from ``step`` completed steps (one fill, not captured: between replays)."""
        self.step.fill_(int(step))

    def value(self) -> float:
        """The current learning rate (a host read: synchronises)."""
        return float(self.lr.item())

    def steps(self) -> int:
        return int(self.step.item())

    def state_dict(self) -> dict:
        return {"step": self.steps(), "segments": [list(s) for s in self.segments]}

    def load_state_dict(self, state: dict) -> None:
        segs = validate(state["segments"])
        table = encode(segs, self.device)
        if table.shape == self._table.shape:
            self._table.copy_(table)     # in place: a captured advance() keeps reading it
        else:
            self._table = table
        self.segments = segs
        t = int(state["step"])
        self.step.fill_(t)
        self.lr.fill_(float(reference_lr(segs, max(t - 1, 0))))


def attach_state(state: dict, lr) -> dict:
    """Add a :class:`DeviceLR`'s state to an optimizer's ``state_dict`` (floats add nothing)."""
    if isinstance(lr, DeviceLR):
        state["lr_schedule"] = lr.state_dict()
    return state


def restore_state(state: dict, lr) -> None:
    """Load what :func:`attach_state` stored; a checkpoint without it leaves the schedule at
    step 0."""
    if isinstance(lr, DeviceLR):
        if "lr_schedule" in state:
            lr.load_state_dict(state["lr_schedule"])
        else:
            lr.reset(0)
            lr.lr.fill_(float(reference_lr(lr.segments, 0)))
