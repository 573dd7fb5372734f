"""Mixed-precision optimizers over the native multi-tensor kernels.

:class:`MasterSGD` keeps conv/linear weights as bf16 parameters (views into one flat bf16 buffer)
and their fp32 master copies + momentum in flat fp32 buffers. The bf16 weights feed the MFMA
convolutions directly, so a bf16-autocast step has no per-weight fp32->bf16 cast in the forward
and no bf16->fp32 gradient cast in the backward; the update is one multi-tensor kernel
(``mt_sgd_master`` in ``csrc/ops/optim_kernels.hip``). The reference trains through TF inside its
Horovod image (``charts/tf-horovod/values.yaml``); tf_cnn_benchmarks' fp16 mode keeps fp32
master variables the same way.

:class:`MultiTensorSGD32` is the same one-launch update for the fp32 parameters next to them
(BatchNorm scales / shifts, biases). Both take ``lr`` as a float or as a
:class:`arena_amd.ops.schedule.DeviceLR`, whose device value the kernels read at every launch, so
a schedule keeps moving under hipGraph replay (the caller advances it at the head of the step).

:class:`MasterRMSprop` / :class:`MultiTensorRMSprop32` and :class:`MasterAdam` /
:class:`MultiTensorAdam32` are the same two designs with TF1's RMSProp and Adam (the forms
tf_cnn_benchmarks' ``--optimizer`` defaults assume; :mod:`arena_amd.ops.reference` defines them).
Adam's bias correction depends on the step count, which a captured graph would bake in, so it
lives on the device in an :class:`AdamClock` that one one-lane kernel advances per step.

:class:`MasterLARS` is :class:`MasterSGD` with LARS's per-tensor trust ratio: the two L2 norms it
needs are reduced on the device (per-block partials, then a fixed-order sum inside the update
kernel), so the captured step has no host read. Its BN / bias group is :class:`MultiTensorSGD32`.

:class:`TFRMSprop`, :class:`TFAdam` and :class:`TFLars` are the same formulas as
``torch.optim.Optimizer`` subclasses in plain tensor ops, for the paths without a fused kernel
(CPU, fp32 weights, data parallel under ``hvd.DistributedOptimizer``).
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import torch

from . import fused
from .schedule import DeviceLR, attach_state, restore_state

Tensor = torch.Tensor


def _lr_args(lr) -> dict:
    """``lr=`` / ``lr_t=`` keyword arguments of the update kernels for a float or a DeviceLR."""
    if isinstance(lr, DeviceLR):
        return {"lr": 0.0, "lr_t": lr.lr}
    return {"lr": float(lr)}


def _take_lr(lr, device) -> Union[float, DeviceLR]:
    if isinstance(lr, DeviceLR):
        if lr.device != device:
            raise ValueError(f"the DeviceLR lives on {lr.device}, the parameters on {device}")
        return lr
    return float(lr)


def _unit_interval(name: str, v: float) -> float:
    v = float(v)
    if not 0.0 <= v < 1.0:
        raise ValueError(f"{name} must lie in [0, 1), got {v}")
    return v


def _positive(name: str, v: float) -> float:
    v = float(v)
    if not v > 0.0:
        raise ValueError(f"{name} must be > 0, got {v}")
    return v


class AdamClock:
    """Adam's step-dependent state where the update kernels read it.

    ``step`` (int64 [1]), ``pow`` (fp64 [2]: ``b1^t`` and ``b2^t`` as running products that start
    at 1.0) and ``corr`` (fp32 [1]) live on ``device``. :meth:`tick` enqueues ONE launch
    (``arena_adam_tick``): ``pow *= (b1, b2)``, ``corr = float32(sqrt(1 - b2^t) / (1 - b1^t))``,
    ``step += 1``: :func:`arena_amd.ops.reference.reference_adam_corr`, bit for bit. Captured into
    a hipGraph it keeps correcting the bias at every replay. One clock serves every Adam optimizer
    of a training step: the one that created it ticks it, the others only read ``corr``."""

    def __init__(self, betas: Sequence[float] = (0.9, 0.999), device="cpu"):
        self.b1 = _unit_interval("beta1", betas[0])
        self.b2 = _unit_interval("beta2", betas[1])
        self.device = torch.device(device)
        self.step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.pow = torch.ones(2, dtype=torch.float64, device=self.device)
        self.corr = torch.ones(1, dtype=torch.float32, device=self.device)

    @property
    def betas(self) -> Tuple[float, float]:
        return self.b1, self.b2

    def tick(self) -> None:
        fused.adam_tick(self.step, self.pow, self.corr, self.b1, self.b2)

    def steps(self) -> int:
        """Completed ticks (a host read: synchronises)."""
        return int(self.step.item())

    def state_dict(self) -> dict:
        return {"step": self.steps(), "pow": self.pow.tolist(), "betas": [self.b1, self.b2]}

    def load_state_dict(self, state: dict) -> None:
        p1, p2 = (float(v) for v in state["pow"])
        self.b1 = _unit_interval("beta1", state["betas"][0])
        self.b2 = _unit_interval("beta2", state["betas"][1])
        self.step.fill_(int(state["step"]))            # in place: a captured tick keeps its buffers
        self.pow.copy_(torch.tensor([p1, p2], dtype=torch.float64))
        self.corr.fill_(math.sqrt(1.0 - p2) / (1.0 - p1) if int(state["step"]) > 0 else 1.0)


class _FlatOptimizer:
    """What the flat-buffer optimizers share: parameters as views into one flat buffer at
    ``offsets``, fp32 state buffers next to it, ``lr`` as a float or a DeviceLR, and a state in
    logical layout. Subclasses name their state buffers and hyper-parameters:

    ``_STATE``: ``(attribute, state_dict key, initial value)`` per flat fp32 state buffer;
    ``_HYPER``: the float attributes saved with the state;
    ``_GRAD``: the gradient dtype the update kernel takes."""

    _STATE: Tuple[Tuple[str, str, float], ...] = ()
    _HYPER: Tuple[str, ...] = ()
    _GRAD = torch.float32

    params: List[Tensor]
    offsets: List[int]
    lr: Union[float, DeviceLR]

    @property
    def _name(self) -> str:
        return type(self).__name__

    def _take_params(self, params: Iterable[Tensor], lr) -> torch.device:
        self.params = list(params)
        if not self.params:
            raise ValueError(f"{self._name} needs at least one parameter")
        dev = self.params[0].device
        self.lr = _take_lr(lr, dev)
        self.offsets = []
        return dev

    def _make_state(self, total: int, dev) -> None:
        for attr, _, init in self._STATE:
            setattr(self, attr, torch.full((total,), float(init), dtype=torch.float32, device=dev))

    def _views(self, flat: Tensor):
        return [flat.as_strided(p.shape, p.stride(), off) for p, off in zip(self.params,
                                                                            self.offsets)]

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _check_grad(self, p: Tensor, g: Tensor) -> None:
        if g.dtype != self._GRAD or not _same_memory_order(g, p):
            kind = "bf16" if self._GRAD == torch.bfloat16 else "fp32"
            raise RuntimeError(f"{self._name}: gradient must be {kind} with the parameter's "
                               f"strides (param {tuple(p.shape)} strides {p.stride()}, grad "
                               f"{g.dtype} strides {g.stride()})")

    def _state_of(self, extra: dict) -> dict:
        """``extra`` + the state buffers in logical layout + shapes, lr and hyper-parameters."""
        scheduled = isinstance(self.lr, DeviceLR)
        state = dict(extra)
        for attr, key, _ in self._STATE:
            state[key] = [m.contiguous() for m in self._views(getattr(self, attr))]
        state["shapes"] = [tuple(p.shape) for p in self.params]
        state["lr"] = self.lr.value() if scheduled else self.lr
        for h in self._HYPER:
            state[h] = getattr(self, h)
        return attach_state(state, self.lr)

    def _check_lists(self, lists: dict) -> None:
        """ValueError unless every list of ``lists`` holds one tensor of each parameter's shape."""
        n = len(self.params)
        if any(len(v) != n for v in lists.values()):
            held = " / ".join(f"{len(v)} {k}" for k, v in lists.items())
            raise ValueError(f"{self._name} state holds {held} for {n} parameters")
        for i, p in enumerate(self.params):
            shapes = [tuple(v[i].shape) for v in lists.values()]
            if any(s != tuple(p.shape) for s in shapes):
                raise ValueError(f"{self._name} state: parameter {i} has shape {tuple(p.shape)}, "
                                 f"state has {' / '.join(str(s) for s in shapes)}")

    def _load_state(self, state: dict) -> None:
        """The state buffers (already checked), lr and hyper-parameters of ``state``."""
        for attr, key, _ in self._STATE:
            for m, b in zip(self._views(getattr(self, attr)), state[key]):
                m.copy_(b)
        if isinstance(self.lr, DeviceLR):
            restore_state(state, self.lr)
        else:
            self.lr = float(state["lr"])
        for h in self._HYPER:
            setattr(self, h, float(state.get(h, getattr(self, h))))


class _MasterOptimizer(_FlatOptimizer):
    """bf16 parameters as views into the flat ``wbf`` with fp32 masters in ``master``: the part of
    :class:`MasterSGD` that does not depend on the update rule. Subclasses implement
    ``_update(grads, offsets)``."""

    _GRAD = torch.bfloat16

    def _init_master(self, params: Iterable[Tensor], lr) -> None:
        dev = self._take_params(params, lr)
        total = 0
        for p in self.params:
            if not (p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)):
                raise ValueError(f"{self._name} parameters must be contiguous or channels_last")
            if p.numel() % 4:
                raise ValueError(f"{self._name} needs numel % 4 == 0 (got {tuple(p.shape)})")
            self.offsets.append(total)
            total += p.numel()
        self.master = torch.empty(total, dtype=torch.float32, device=dev)
        self._make_state(total, dev)
        self.wbf = torch.empty(total, dtype=torch.bfloat16, device=dev)
        with torch.no_grad():
            for p, off in zip(self.params, self.offsets):
                self.master.as_strided(p.shape, p.stride(), off).copy_(p)
                v = self.wbf.as_strided(p.shape, p.stride(), off)
                v.copy_(p)
                p.data = v
                p.grad = None

    @torch.no_grad()
    def step(self) -> None:
        grads, offs = [], []
        for p, off in zip(self.params, self.offsets):
            g = p.grad
            if g is None:
                continue
            self._check_grad(p, g)
            grads.append(g)
            offs.append(off)
        self._before_update()
        if grads:
            self._update(grads, offs)

    def _before_update(self) -> None:
        pass

    def _update(self, grads, offs) -> None:
        raise NotImplementedError

    @torch.no_grad()
    def sync_from_params(self) -> None:
        """Re-derive the fp32 masters from the current (bf16) parameter values.

        Call this after ``model.load_state_dict(...)`` on a model whose optimizer already exists:
        otherwise the next :meth:`step` overwrites the loaded weights with the stale masters.
        (The optimizer's state buffers are left as they are; load the optimizer state too to
        restore them.)"""
        for p, m, w in zip(self.params, self._views(self.master), self._views(self.wbf)):
            if p.data_ptr() != w.data_ptr():
                # the parameter's data was re-bound (``p.data = t``): adopt its values and
                # make it a view into the flat bf16 buffer again. (``load_state_dict(...,
                # assign=True)`` replaces the Parameter objects themselves; like any torch
                # optimizer, this one must then be rebuilt.)
                w.copy_(p)
                p.data = w
            m.copy_(p)

    def master_params(self) -> List[Tensor]:
        """fp32 master weights, one tensor per parameter in logical (contiguous) layout."""
        return [m.contiguous() for m in self._views(self.master)]

    def state_dict(self) -> dict:
        """fp32 masters + state buffers, one tensor per parameter in LOGICAL layout (independent
        of channels_last strides), so a checkpoint moves between NHWC and NCHW runs and CPU/GPU."""
        return self._state_of({"master": self.master_params()})

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        lists = {"masters": state["master"]}
        for _, key, _ in self._STATE:
            lists[_LIST_NAMES.get(key, key)] = state[key]
        if any(isinstance(v, Tensor) for v in lists.values()):
            raise ValueError(f"{self._name} state is in the old flat format (memory-order "
                             "dependent); re-save it with this version")
        self._check_lists(lists)
        for m, a in zip(self._views(self.master), state["master"]):
            m.copy_(a)
        self._load_state(state)
        self.wbf.copy_(self.master)   # bf16 weights are views into wbf


class _Flat32Optimizer(_FlatOptimizer):
    """fp32 parameters as views into the flat ``w`` (16-byte aligned slots, so the kernels take
    their vector path; values and strides unchanged): the part of :class:`MultiTensorSGD32` that
    does not depend on the update rule. Subclasses implement ``_update(grads, offsets)``."""

    def _init_flat32(self, params: Iterable[Tensor], lr) -> None:
        dev = self._take_params(params, lr)
        total = 0
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError(f"{self._name} takes fp32 parameters on one device")
            if not (p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)):
                raise ValueError(f"{self._name} parameters must be contiguous or channels_last")
            self.offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.w = torch.zeros(total, dtype=torch.float32, device=dev)
        self._make_state(total, dev)
        with torch.no_grad():
            for p, v in zip(self.params, self._views(self.w)):
                v.copy_(p)
                p.data = v
                p.grad = None

    @torch.no_grad()
    def step(self) -> None:
        grads, offs = [], []
        for p, off, v in zip(self.params, self.offsets, self._views(self.w)):
            g = p.grad
            if g is None:
                continue
            if p.data_ptr() != v.data_ptr():
                raise RuntimeError(f"{self._name}: a parameter's data was re-bound; call "
                                   "sync_from_params() after loading weights")
            self._check_grad(p, g)
            grads.append(g)
            offs.append(off)
        self._before_update()
        if grads:
            self._update(grads, offs)

    def _before_update(self) -> None:
        pass

    def _update(self, grads, offs) -> None:
        raise NotImplementedError

    @torch.no_grad()
    def sync_from_params(self) -> None:
        """Adopt the values of parameters whose data was re-bound (``p.data = t``) and make them
        views into the flat buffer again."""
        for p, v in zip(self.params, self._views(self.w)):
            if p.data_ptr() != v.data_ptr():
                v.copy_(p)
                p.data = v

    def state_dict(self) -> dict:
        """The state buffers per parameter in logical layout (the weights are the model's own
        state)."""
        return self._state_of({})

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        self._check_lists({_LIST_NAMES.get(key, key): state[key] for _, key, _ in self._STATE})
        self._load_state(state)


# how a state list is called in an error message
_LIST_NAMES = {"momentum_buffer": "momentum buffers"}


class _NesterovFlag:
    """``nesterov=True`` of the momentum-SGD optimizers (:mod:`arena_amd.ops.reference` defines
    the rule). The momentum buffer means what it means under the plain rule; a state dict carries
    ``nesterov: True`` only with the flag, and loading a state whose flag differs raises."""

    nesterov = False

    def _take_nesterov(self, nesterov: bool, momentum: float) -> None:
        self.nesterov = bool(nesterov)
        if self.nesterov and not float(momentum) > 0.0:   # before any parameter is re-bound
            raise ValueError(f"{type(self).__name__}(nesterov=True) needs momentum > 0, got "
                             f"{momentum}")

    def state_dict(self) -> dict:
        state = super().state_dict()
        if self.nesterov:
            state["nesterov"] = True
        return state

    def load_state_dict(self, state: dict) -> None:
        if bool(state.get("nesterov", False)) != self.nesterov:
            raise ValueError(f"{type(self).__name__}(nesterov={self.nesterov}) cannot load a state "
                             f"saved with nesterov={bool(state.get('nesterov', False))}")
        super().load_state_dict(state)
        if self.nesterov and not self.momentum > 0.0:
            raise ValueError(f"{type(self).__name__}(nesterov=True) needs momentum > 0, the "
                             f"loaded state has {self.momentum}")


class MasterSGD(_NesterovFlag, _MasterOptimizer):
    """Momentum SGD (torch.optim.SGD semantics, dampening 0) with fp32 master weights.

    Converts every parameter in ``params`` to bf16 in place (``p.data`` becomes a view into the
    flat bf16 buffer with the parameter's own strides, so channels_last weights stay
    channels_last). ``lr``: a float, or a :class:`DeviceLR` on the parameters' device.
    ``nesterov``: Nesterov momentum (torch's ``nesterov=True``, TF's ``use_nesterov=True``)."""

    _STATE = (("mom", "momentum_buffer", 0.0),)
    _HYPER = ("momentum", "weight_decay")

    def __init__(self, params: Iterable[Tensor], lr: Union[float, DeviceLR], momentum: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False):
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        self._take_nesterov(nesterov, momentum)
        self._init_master(params, lr)

    def _update(self, grads, offs) -> None:
        fused.mt_sgd_master(grads, offs, self.master, self.mom, self.wbf,
                            momentum=self.momentum, weight_decay=self.weight_decay,
                            nesterov=self.nesterov, **_lr_args(self.lr))


class MultiTensorSGD32(_NesterovFlag, _Flat32Optimizer):
    """Momentum SGD (torch.optim.SGD semantics, dampening 0) over fp32 parameters with fp32
    gradients, one ``mt_sgd_f32`` launch per 48 tensors: the BN / bias group next to
    :class:`MasterSGD`.

    The parameters become views into one flat fp32 buffer (16-byte aligned slots, so the kernel
    takes its vector path; values and strides unchanged), momentum lives in a second one.
    ``lr``: a float, or a :class:`DeviceLR` on the parameters' device. ``scale`` multiplies the
    gradients (1 / world for summed gradients). ``nesterov``: Nesterov momentum, as
    :class:`MasterSGD`'s."""

    _STATE = (("mom", "momentum_buffer", 0.0),)
    _HYPER = ("momentum", "weight_decay", "scale")

    def __init__(self, params: Iterable[Tensor], lr: Union[float, DeviceLR], momentum: float = 0.0,
                 weight_decay: float = 0.0, scale: float = 1.0, nesterov: bool = False):
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        self.scale = float(scale)
        self._take_nesterov(nesterov, momentum)
        self._init_flat32(params, lr)

    def _update(self, grads, offs) -> None:
        fused.mt_sgd_f32(grads, offs, self.w, self.mom, momentum=self.momentum,
                         weight_decay=self.weight_decay, scale=self.scale,
                         nesterov=self.nesterov, **_lr_args(self.lr))


# ---------------------------------------------------------------------------------------- LARS
def _non_negative(name: str, v: float) -> float:
    v = float(v)
    if not v >= 0.0:
        raise ValueError(f"{name} must be >= 0, got {v}")
    return v


class MasterLARS(_MasterOptimizer):
    """LARS (tf.contrib's ``LARSOptimizer``, the MLPerf ResNet form;
    :mod:`arena_amd.ops.reference` defines it) with fp32 master weights: :class:`MasterSGD`'s
    design with the step ``lr * trust``, ``trust = eeta * |w| / (|g| + weight_decay * |w| + eps)``
    per tensor (1.0 when a norm is 0). The norms, the ratio and the update run on the device in
    two ``mt_lars_master`` launches per 48 tensors, without atomics, so a captured step replays
    it. ``trust`` (fp32, one entry per parameter, 1.0 until the parameter's first update) holds
    the ratios of the last step; it is derived, not state. The BN / bias group next to it is
    :class:`MultiTensorSGD32` (LARS's skip list: plain momentum SGD, no weight decay)."""

    _STATE = (("mom", "momentum_buffer", 0.0),)
    _HYPER = ("momentum", "weight_decay", "eeta", "eps")

    def __init__(self, params: Iterable[Tensor], lr: Union[float, DeviceLR], momentum: float = 0.9,
                 weight_decay: float = 0.0, eeta: float = 0.001, eps: float = 0.0):
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        self.eeta, self.eps = _positive("eeta", eeta), _non_negative("eps", eps)
        self._init_master(params, lr)
        dev = self.master.device
        self.trust = torch.ones(len(self.params), dtype=torch.float32, device=dev)
        self.workspace = torch.empty(
            fused.mt_lars_workspace_floats([p.numel() for p in self.params]),
            dtype=torch.float32, device=dev)
        self._slot = {off: i for i, off in enumerate(self.offsets)}

    def _update(self, grads, offs) -> None:
        fused.mt_lars_master(grads, offs, self.master, self.mom, self.wbf, self.trust,
                             [self._slot[o] for o in offs], self.workspace,
                             momentum=self.momentum, weight_decay=self.weight_decay,
                             eeta=self.eeta, eps=self.eps, **_lr_args(self.lr))


# ------------------------------------------------------------------------------------- RMSProp
class _RMSpropHyper:
    """TF1's non-centred RMSProp: ``ms`` starts at 1.0 as TF's slot does, ``mom`` at 0."""

    _STATE = (("ms", "mean_square", 1.0), ("mom", "momentum_buffer", 0.0))

    def _take_hyper(self, decay, momentum, eps, weight_decay) -> None:
        self.decay = _unit_interval("decay", decay)
        self.momentum = _unit_interval("momentum", momentum)
        self.eps = _positive("eps", eps)
        self.weight_decay = float(weight_decay)

    def _hyper(self) -> dict:
        return {"decay": self.decay, "momentum": self.momentum, "eps": self.eps,
                "weight_decay": self.weight_decay}


class MasterRMSprop(_RMSpropHyper, _MasterOptimizer):
    """TF1 RMSProp with fp32 master weights: :class:`MasterSGD`'s design (bf16 parameters as
    views into one flat buffer, ``lr`` a float or a :class:`DeviceLR`) with the update
    ``ms = decay * ms + (1 - decay) * d * d; mom = momentum * mom + lr * d / sqrt(ms + eps);
    w -= mom`` over ``d = g + weight_decay * w``, one ``mt_rmsprop_master`` launch per 48
    tensors."""

    _HYPER = ("decay", "momentum", "eps", "weight_decay")

    def __init__(self, params: Iterable[Tensor], lr: Union[float, DeviceLR], decay: float = 0.9,
                 momentum: float = 0.9, eps: float = 1.0, weight_decay: float = 0.0):
        self._take_hyper(decay, momentum, eps, weight_decay)
        self._init_master(params, lr)

    def _update(self, grads, offs) -> None:
        fused.mt_rmsprop_master(grads, offs, self.master, self.ms, self.mom, self.wbf,
                                **self._hyper(), **_lr_args(self.lr))


class MultiTensorRMSprop32(_RMSpropHyper, _Flat32Optimizer):
    """TF1 RMSProp over fp32 parameters with fp32 gradients (the BN / bias group next to
    :class:`MasterRMSprop`), one ``mt_rmsprop_f32`` launch per 48 tensors. ``scale`` multiplies
    the gradients."""

    _HYPER = ("decay", "momentum", "eps", "weight_decay", "scale")

    def __init__(self, params: Iterable[Tensor], lr: Union[float, DeviceLR], decay: float = 0.9,
                 momentum: float = 0.9, eps: float = 1.0, weight_decay: float = 0.0,
                 scale: float = 1.0):
        self._take_hyper(decay, momentum, eps, weight_decay)
        self.scale = float(scale)
        self._init_flat32(params, lr)

    def _update(self, grads, offs) -> None:
        fused.mt_rmsprop_f32(grads, offs, self.w, self.ms, self.mom, scale=self.scale,
                             **self._hyper(), **_lr_args(self.lr))


# ---------------------------------------------------------------------------------------- Adam
class _AdamHyper:
    """TF1's Adam: ``m`` and ``v`` start at 0; the bias correction comes from an
    :class:`AdamClock`. The optimizer that created its clock ticks it at the head of ``step()``;
    one that was handed a clock only reads it (one tick per training step)."""

    _STATE = (("m", "exp_avg", 0.0), ("v", "exp_avg_sq", 0.0))

    def _take_hyper(self, betas, eps, weight_decay, clock: Optional[AdamClock]) -> None:
        self.eps = _positive("eps", eps)
        self.weight_decay = float(weight_decay)
        self._owns_clock = clock is None
        self._betas = (float(betas[0]), float(betas[1]))
        if clock is not None and clock.betas != self._betas:   # before any parameter is re-bound
            raise ValueError(f"betas {self._betas} differ from the shared AdamClock's "
                             f"{clock.betas}")
        self.clock = clock

    def _take_clock(self, dev) -> None:
        if self.clock is None:
            self.clock = AdamClock(self._betas, dev)
        elif self.clock.device != dev:
            raise ValueError(f"the AdamClock lives on {self.clock.device}, the parameters on "
                             f"{dev}")

    def _before_update(self) -> None:
        if self._owns_clock:
            self.clock.tick()

    def _hyper(self) -> dict:
        return {"betas": self.clock.betas, "eps": self.eps, "weight_decay": self.weight_decay}

    def state_dict(self) -> dict:
        state = super().state_dict()
        state["clock"] = self.clock.state_dict()
        return state

    def load_state_dict(self, state: dict) -> None:
        super().load_state_dict(state)
        self.clock.load_state_dict(state["clock"])


class MasterAdam(_AdamHyper, _MasterOptimizer):
    """TF1 Adam with fp32 master weights: :class:`MasterSGD`'s design with the update
    ``m = b1 * m + (1 - b1) * d; v = b2 * v + (1 - b2) * d * d; w -= lr * corr * m / (sqrt(v) +
    eps)`` over ``d = g + weight_decay * w``, one ``mt_adam_master`` launch per 48 tensors.
    ``clock``: an :class:`AdamClock` to read; None creates one, ticked at the head of every
    :meth:`step`."""

    _HYPER = ("eps", "weight_decay")

    def __init__(self, params: Iterable[Tensor], lr: Union[float, DeviceLR],
                 betas: Sequence[float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, clock: Optional[AdamClock] = None):
        self._take_hyper(betas, eps, weight_decay, clock)
        self._init_master(params, lr)
        self._take_clock(self.master.device)

    def _update(self, grads, offs) -> None:
        fused.mt_adam_master(grads, offs, self.master, self.m, self.v, self.wbf, self.clock.corr,
                             **self._hyper(), **_lr_args(self.lr))


class MultiTensorAdam32(_AdamHyper, _Flat32Optimizer):
    """TF1 Adam over fp32 parameters with fp32 gradients (the BN / bias group next to
    :class:`MasterAdam`), one ``mt_adam_f32`` launch per 48 tensors. Pass :class:`MasterAdam`'s
    ``clock`` so the step has one tick; ``scale`` multiplies the gradients."""

    _HYPER = ("eps", "weight_decay", "scale")

    def __init__(self, params: Iterable[Tensor], lr: Union[float, DeviceLR],
                 betas: Sequence[float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, scale: float = 1.0,
                 clock: Optional[AdamClock] = None):
        self._take_hyper(betas, eps, weight_decay, clock)
        self.scale = float(scale)
        self._init_flat32(params, lr)
        self._take_clock(self.w.device)

    def _update(self, grads, offs) -> None:
        fused.mt_adam_f32(grads, offs, self.w, self.m, self.v, self.clock.corr, scale=self.scale,
                          **self._hyper(), **_lr_args(self.lr))


def _same_memory_order(g: Tensor, p: Tensor) -> bool:
    """True if ``g`` is dense and walks memory in the same element order as ``p``.

    Strides of size-1 dims are irrelevant (autograd's AccumulateGrad keeps such gradients as they
    come: a channels_last gradient of a [Cout, Cin, 1, 1] weight is contiguous in both senses)."""
    if g.shape != p.shape:
        return False
    if not (g.is_contiguous() or g.is_contiguous(memory_format=torch.channels_last)):
        return False
    return all(gs == ps for gs, ps, n in zip(g.stride(), p.stride(), p.shape) if n > 1)


class OptimizerGroup:
    """Steps several optimizers as one (e.g. MasterSGD for weights + torch SGD for BN/bias)."""

    def __init__(self, *opts):
        self.opts = opts

    def zero_grad(self, set_to_none: bool = True) -> None:
        for o in self.opts:
            o.zero_grad(set_to_none=set_to_none)

    def step(self) -> None:
        for o in self.opts:
            o.step()

    def state_dict(self) -> dict:
        return {"opts": [o.state_dict() for o in self.opts]}

    def load_state_dict(self, state: dict) -> None:
        if len(state["opts"]) != len(self.opts):
            raise ValueError(f"OptimizerGroup state holds {len(state['opts'])} optimizers, "
                             f"this group has {len(self.opts)}")
        for o, st in zip(self.opts, state["opts"]):
            o.load_state_dict(st)


# --------------------------------------------------------- the same formulas in plain tensor ops
class TFRMSprop(torch.optim.Optimizer):
    """TF1's non-centred RMSProp (:mod:`arena_amd.ops.reference`'s form) in plain tensor ops on
    any device, for the paths without a fused kernel. ``ms`` starts at 1.0, ``epsilon`` sits
    inside the square root, weight decay is coupled (``d = g + weight_decay * w``). Nothing that
    changes per step lives on the host, so a captured step replays correctly; ``lr`` is read from
    ``param_groups`` at every (eager) step."""

    def __init__(self, params, lr: float, decay: float = 0.9, momentum: float = 0.9,
                 eps: float = 1.0, weight_decay: float = 0.0):
        super().__init__(params, dict(lr=float(lr), decay=_unit_interval("decay", decay),
                                      momentum=_unit_interval("momentum", momentum),
                                      eps=_positive("eps", eps),
                                      weight_decay=float(weight_decay)))
        for group in self.param_groups:    # now, not at the first step: that one may be captured
            for p in group["params"]:
                self._init_state(p)

    def _init_state(self, p: Tensor) -> dict:
        st = self.state[p]
        st["ms"] = torch.ones_like(p, memory_format=torch.preserve_format)
        st["mom"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, rho, mu = group["lr"], group["decay"], group["momentum"]
            eps, wd = group["eps"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p] or self._init_state(p)
                ms, mom = st["ms"], st["mom"]
                d = p.grad.to(p.dtype) + wd * p
                ms.mul_(rho).add_((1.0 - rho) * (d * d))
                mom.mul_(mu).add_(lr * d / torch.sqrt(ms + eps))
                p.sub_(mom)
        return loss


class TFAdam(torch.optim.Optimizer):
    """TF1's Adam (:mod:`arena_amd.ops.reference`'s form) in plain tensor ops on any device:
    ``w -= lr * corr * m / (sqrt(v) + eps)`` with coupled weight decay. The bias correction's
    state (``step`` int64 [1], ``pow`` fp64 [2] holding ``b1^t`` / ``b2^t``, ``corr`` fp32 [1]) is
    tensors on the parameters' device updated by tensor ops, as :class:`AdamClock` keeps it, so
    a captured step keeps correcting the bias on replay. One ``betas`` pair for all groups."""

    def __init__(self, params, lr: float, betas: Sequence[float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 0.0):
        self.betas = (_unit_interval("beta1", betas[0]), _unit_interval("beta2", betas[1]))
        super().__init__(params, dict(lr=float(lr), eps=_positive("eps", eps),
                                      weight_decay=float(weight_decay)))
        dev = self.param_groups[0]["params"][0].device
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.pow = torch.ones(2, dtype=torch.float64, device=dev)
        self.corr = torch.ones(1, dtype=torch.float32, device=dev)
        self._betas_t = torch.tensor(self.betas, dtype=torch.float64, device=dev)
        for group in self.param_groups:    # now, not at the first step: that one may be captured
            for p in group["params"]:
                self._init_state(p)

    def _init_state(self, p: Tensor) -> dict:
        st = self.state[p]
        st["m"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["v"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        b1, b2 = self.betas
        self.pow.mul_(self._betas_t)
        self.corr.copy_(torch.sqrt(1.0 - self.pow[1:2]) / (1.0 - self.pow[0:1]))
        self.step_count.add_(1)
        for group in self.param_groups:
            eps, wd = group["eps"], group["weight_decay"]
            size = group["lr"] * self.corr.reshape(())    # fp32 scalar: lr * corr, rounded once
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p] or self._init_state(p)
                m, v = st["m"], st["v"]
                d = p.grad.to(p.dtype) + wd * p
                m.mul_(b1).add_((1.0 - b1) * d)
                v.mul_(b2).add_((1.0 - b2) * (d * d))
                p.sub_(size * m / (torch.sqrt(v) + eps))
        return loss

    def state_dict(self) -> dict:
        state = super().state_dict()
        state["clock"] = {"step": int(self.step_count.item()), "pow": self.pow.tolist(),
                          "betas": list(self.betas)}
        return state

    def load_state_dict(self, state: dict) -> None:
        state = dict(state)
        clock = state.pop("clock")
        super().load_state_dict(state)
        self.betas = (_unit_interval("beta1", clock["betas"][0]),
                      _unit_interval("beta2", clock["betas"][1]))
        self._betas_t.copy_(torch.tensor(self.betas, dtype=torch.float64))
        self.step_count.fill_(int(clock["step"]))
        self.pow.copy_(torch.tensor(clock["pow"], dtype=torch.float64))


class TFLars(torch.optim.Optimizer):
    """LARS (:mod:`arena_amd.ops.reference`'s form) in plain tensor ops on any device, for the
    paths without the fused kernel: momentum SGD whose step is ``lr * trust`` with ``trust = eeta
    * |w| / (|g| + weight_decay * |w| + eps)`` per tensor, 1.0 when a norm is 0. Param groups
    carry ``lars: bool``; a group with ``lars=False`` (BN scales / shifts, biases: LARS's skip
    list) takes plain momentum SGD with its own ``weight_decay``. The norms and the guard stay on
    the device (no host read), so a captured step replays correctly; ``lr`` is read from
    ``param_groups`` at every (eager) step."""

    def __init__(self, params, lr: float, momentum: float = 0.9, eeta: float = 0.001,
                 eps: float = 0.0, weight_decay: float = 0.0):
        super().__init__(params, dict(lr=float(lr), momentum=_unit_interval("momentum", momentum),
                                      eeta=_positive("eeta", eeta), eps=_non_negative("eps", eps),
                                      weight_decay=float(weight_decay), lars=True))
        for group in self.param_groups:    # now, not at the first step: that one may be captured
            for p in group["params"]:
                self._init_state(p)

    def _init_state(self, p: Tensor) -> dict:
        st = self.state[p]
        st["mom"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, mu, wd = group["lr"], group["momentum"], group["weight_decay"]
            eeta, eps = group["eeta"], group["eps"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                mom = (self.state[p] or self._init_state(p))["mom"]
                g = p.grad.to(p.dtype)
                step = lr
                if group["lars"]:
                    wn = torch.linalg.vector_norm(p)
                    gn = torch.linalg.vector_norm(g)
                    trust = torch.where((wn > 0) & (gn > 0), eeta * wn / (gn + wd * wn + eps),
                                        torch.ones_like(wn))
                    step = lr * trust
                mom.mul_(mu).add_(g + wd * p)
                p.sub_(step * mom)
        return loss
