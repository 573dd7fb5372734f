"""Functional API over the native kernels with device dispatch.

GPU tensors -> HIP kernels in ``arena_amd._C`` (raises if the extension is missing: no silent
fallback); CPU tensors -> the bit-compatible PyTorch reference in :mod:`arena_amd.ops.reference`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _ext, reference

Tensor = torch.Tensor


def _impl(t: Tensor):
    return _ext.load() if t.is_cuda else reference


def linear_fwd(x: Tensor, W: Tensor, Y: Tensor, bias: Optional[Tensor] = None, *,
               x_scale: float = 1.0, idx: Optional[Tensor] = None,
               cursor: Optional[Tensor] = None, batch: int = 0, act: int = 1,
               keep_prob: float = 1.0, seed: int = 0, step: Optional[Tensor] = None) -> Tensor:
    """Y = dropout(act(gather(x)·scale @ W + bias)). ``act``: 0 identity, 1 ReLU."""
    _impl(W).linear_fwd(x, float(x_scale), idx, cursor, int(batch), W, bias, Y, int(act),
                        float(keep_prob), int(seed), step)
    return Y


def xent_head(H: Tensor, W2: Tensor, b2: Optional[Tensor], labels: Tensor, *,
              loss_acc: Tensor, correct_acc: Tensor, idx: Optional[Tensor] = None,
              cursor: Optional[Tensor] = None, batch: int = 0,
              dlogits: Optional[Tensor] = None, dZ: Optional[Tensor] = None,
              keep_prob: float = 1.0, relu_mask: bool = True, loss_scale: float = 1.0,
              hist_step: Optional[Tensor] = None, ctr_dst: Optional[Tensor] = None,
              ctr_src: Optional[Tensor] = None, ctr_add: int = 0) -> None:
    _impl(H).xent_head(H, W2, b2, labels, idx, cursor, int(batch), dlogits, dZ, float(keep_prob),
                       bool(relu_mask), float(loss_scale), loss_acc, correct_acc, hist_step,
                       ctr_dst, ctr_src, int(ctr_add))


def mlp_fwd_logits(x: Tensor, W1: Tensor, b1: Tensor, H: Tensor, W2: Tensor, logits2: Tensor, *,
                   W2_copy: Optional[Tensor] = None, xb: Optional[Tensor] = None,
                   labels: Optional[Tensor] = None, yb: Optional[Tensor] = None,
                   x_scale: float = 1.0,
                   idx: Optional[Tensor] = None, cursor: Optional[Tensor] = None, batch: int = 0,
                   keep_prob: float = 1.0, seed: int = 0, step: Optional[Tensor] = None,
                   ctr_dst: Optional[Tensor] = None, ctr_src: Optional[Tensor] = None,
                   ctr_add: int = 0, xa: Optional[Tensor] = None, xa_parity: int = -1) -> None:
    """H = dropout(relu(x·W1ᵀ+b1)) and logits2[step & 1] += H·W2ᵀ in ONE launch.

    ``logits2`` is [2, M, C]; the consuming wgrad (head mode) zeroes the other buffer each step.
    With ``xb``/``labels``/``yb`` the gathered u8 batch rows and their labels are published for the
    backward kernel (so it skips the cursor -> permutation -> row dependency chain).
    ``xa`` (uint8 [2, M, K], instead of ``idx``/``cursor`` and ``xb``/``yb``): this step's batch
    sits in ``xa[step & 1]``, where the previous ``wgrad_grouped`` published it (``next_xa``), so
    the kernel loads its X rows from an address known at launch. ``xa_parity`` 0/1 names the half
    at launch (it must equal the step counter's parity); -1 takes it from ``step`` in-kernel.
    Training-step kernel only: uint8 ``x`` (for its shape), K <= 1024, ``ctr_src is step``.
    """
    _impl(H).mlp_fwd_logits(x, float(x_scale), idx, cursor, int(batch), W1, b1, H,
                            float(keep_prob), int(seed), step, W2, W2_copy, logits2, xb, labels, yb,
                            ctr_dst, ctr_src, int(ctr_add), xa, int(xa_parity))


def wgrad_grouped(xs: Sequence[Tensor], dzs: Sequence[Optional[Tensor]], outW: Sequence[Tensor],
                  outB: Sequence[Optional[Tensor]], *, x_scales: Sequence[float],
                  gather: Sequence[bool], idx: Optional[Tensor] = None,
                  cursor: Optional[Tensor] = None, cursor_off: int = 0, batch: int = 0,
                  head_modes: Optional[Sequence[int]] = None, head_w2=None, head_h=None,
                  head_keep_prob: float = 1.0, head_logits2: Optional[Tensor] = None,
                  head_step: Optional[Tensor] = None, head_step_off: int = 0,
                  head_b2: Optional[Tensor] = None, head_labels: Optional[Tensor] = None,
                  head_loss_scale: float = 1.0, head_loss_acc: Optional[Tensor] = None,
                  head_correct_acc: Optional[Tensor] = None,
                  mode: int = 0, mW=None, vW=None, mB=None, vB=None, lr: float = 1e-3,
                  lr_t: Optional[Tensor] = None, betas=(0.9, 0.999), eps: float = 1e-8,
                  weight_decay: float = 0.0, t_step: Optional[Tensor] = None,
                  grad_scale: float = 1.0, tf_style: bool = False,
                  ctr_dst: Optional[Tensor] = None, ctr_src: Optional[Tensor] = None,
                  ctr_add: int = 0, head_parity: int = -1, next_x: Optional[Tensor] = None,
                  next_labels: Optional[Tensor] = None, next_perm: Optional[Tensor] = None,
                  next_xa: Optional[Tensor] = None, next_ya: Optional[Tensor] = None) -> None:
    """dW_i = dz_iᵀ·gather(x_i), db_i = Σ_rows dz_i for up to 2 layers in one launch.

    Head modes (fused MLP step): every workgroup recomputes softmax-xent from ``head_logits2``
    (+ ``head_b2``, ``head_labels``); ``head_modes[i]`` 1 -> dz = dlogits (output layer),
    2 -> dz = (dlogits·head_w2[i]) ⊙ (head_h[i] > 0) / head_keep_prob (hidden layer).
    ``head_parity`` 0/1 names this step's logits buffer at launch (it must equal the counter's
    parity); -1 derives it from ``head_step`` in-kernel.
    Batch ahead: with ``next_xa`` (uint8 [2, M, K]) / ``next_ya`` (int32 [2, M]) extra workgroups
    copy the NEXT step's batch -- rows ``next_x[p]``, labels ``next_labels[p]`` for ``p =
    next_perm[((step + 1) * M + r) % len]`` -- into half ``(step + 1) & 1``. A 3-D ``xs[i]``
    [2, M, K] and 2-D ``head_labels`` [2, M] are such pairs: this step reads half ``step & 1``.
    mode 0 writes ``grad_scale * dW`` into ``outW`` (e.g. views of the flat all-reduce bucket);
    mode 1 applies Adam in place to parameters ``outW``/``outB`` with state ``mW,vW,mB,vB``.
    """
    n = len(xs)
    none = [None] * n
    hm = list(head_modes) if head_modes is not None else [0] * n
    _impl(outW[0]).wgrad_grouped(
        list(xs), [float(s) for s in x_scales], [bool(g) for g in gather], idx, cursor,
        int(cursor_off), int(batch), list(dzs), [int(m) for m in hm], list(head_w2 or none),
        list(head_h or none), float(head_keep_prob), head_logits2, head_step, int(head_step_off),
        head_b2, head_labels, float(head_loss_scale), head_loss_acc, head_correct_acc, int(mode),
        list(outW), list(outB), list(mW or none), list(vW or none), list(mB or none),
        list(vB or none), float(lr), lr_t, float(betas[0]), float(betas[1]), float(eps),
        float(weight_decay), t_step, float(grad_scale), bool(tf_style), ctr_dst, ctr_src,
        int(ctr_add), next_xa, next_ya, int(head_parity), next_x, next_labels, next_perm)


def adam_flat(P: Tensor, M: Tensor, V: Tensor, G: Tensor, *, lr: float = 1e-3,
              lr_t: Optional[Tensor] = None, betas=(0.9, 0.999), eps: float = 1e-8,
              weight_decay: float = 0.0, t_step: Optional[Tensor] = None,
              grad_scale: float = 1.0, tf_style: bool = False,
              ctr_dst: Optional[Tensor] = None, ctr_src: Optional[Tensor] = None,
              ctr_add: int = 0) -> None:
    _impl(P).adam_flat(P, M, V, G, float(lr), lr_t, float(betas[0]), float(betas[1]), float(eps),
                       float(weight_decay), t_step, float(grad_scale), bool(tf_style), ctr_dst,
                       ctr_src, int(ctr_add))


def sgd_flat(P: Tensor, G: Tensor, *, lr: float, lr_t: Optional[Tensor] = None,
             grad_scale: float = 1.0) -> None:
    _impl(P).sgd_flat(P, G, float(lr), lr_t, float(grad_scale))


def softmax_xent(logits: Tensor, labels: Tensor, grad_scale: float = 1.0,
                 need_grad: bool = True):
    """Per-row cross-entropy loss and (optionally) dlogits = (softmax - onehot) * grad_scale."""
    out = _impl(logits).softmax_xent(logits, labels, float(grad_scale), bool(need_grad))
    return tuple(out)


def flatten_into(tensors: Sequence[Tensor], offsets: Sequence[int], flat: Tensor,
                 scale: float = 1.0) -> None:
    """flat[off_i : off_i+n_i] = t_i * scale (one multi-tensor launch per 48 tensors)."""
    _impl(flat).mt_copy_scale(list(tensors), [int(o) for o in offsets], flat, float(scale), 0)


def unflatten_from(tensors: Sequence[Tensor], offsets: Sequence[int], flat: Tensor,
                   scale: float = 1.0) -> None:
    """t_i = flat[off_i : off_i+n_i] * scale."""
    _impl(flat).mt_copy_scale(list(tensors), [int(o) for o in offsets], flat, float(scale), 1)


def _check_lr_t(lr_t: Optional[Tensor], like: Tensor) -> Optional[Tensor]:
    """A device learning rate is one fp32 value on the updated tensors' device."""
    if lr_t is not None and (lr_t.dtype != torch.float32 or lr_t.numel() != 1
                             or lr_t.device != like.device):
        raise ValueError(f"lr_t must be a float32 [1] tensor on {like.device} (got {lr_t.dtype} "
                         f"{tuple(lr_t.shape)} on {lr_t.device})")
    return lr_t


def mt_sgd_master(grads: Sequence[Tensor], offsets: Sequence[int], master: Tensor, mom: Tensor,
                  wbf: Tensor, *, lr: float, momentum: float, weight_decay: float,
                  lr_t: Optional[Tensor] = None, nesterov: bool = False) -> None:
    """One launch (per 48 tensors) of momentum SGD over bf16 grads with fp32 master weights;
    also writes the rounded bf16 weights into ``wbf`` (``mt_master_kernel<SgdRule>`` in
    ``csrc/ops/optim_kernels.hip``). ``lr_t`` (optional, fp32 [1]) is read by the kernel instead
    of ``lr``: a schedule under graph replay. ``nesterov``: Nesterov momentum (``NesterovRule``:
    w -= lr * (d + momentum * mom) after the same d and mom; needs momentum > 0)."""
    _impl(master).mt_sgd_master(list(grads), [int(o) for o in offsets], master, mom, wbf,
                                float(lr), float(momentum), float(weight_decay),
                                lr_t=_check_lr_t(lr_t, master), **_nesterov_kw(nesterov, momentum))


def _nesterov_kw(nesterov: bool, momentum: float) -> dict:
    """The ``nesterov=`` keyword of the momentum-SGD updates: passed only when set, and only with
    a momentum above 0 (:mod:`arena_amd.ops.reference` defines the rule)."""
    if not nesterov:
        return {}
    if not float(momentum) > 0.0:
        raise ValueError(f"Nesterov momentum needs momentum > 0, got {momentum}")
    return {"nesterov": True}


def mt_sgd_f32(grads: Sequence[Tensor], offsets: Sequence[int], w: Tensor, mom: Tensor, *,
               lr: float, momentum: float, weight_decay: float = 0.0, scale: float = 1.0,
               lr_t: Optional[Tensor] = None, nesterov: bool = False) -> None:
    """Momentum SGD over fp32 tensors (BN scales/shifts, biases), one launch per 48 tensors:
    gradient i updates ``w`` / ``mom`` at ``[offsets[i], offsets[i] + numel_i)`` in place, any
    sizes; d = g * scale + wd * w; mom = momentum * mom + d; w -= lr * mom, or with ``nesterov``
    w -= lr * (d + momentum * mom)."""
    _impl(w).mt_sgd_f32(list(grads), [int(o) for o in offsets], w, mom, float(lr), float(momentum),
                        float(weight_decay), float(scale), lr_t=_check_lr_t(lr_t, w),
                        **_nesterov_kw(nesterov, momentum))


def shard_sgd(grad: Tensor, w32: Tensor, mom: Tensor, wbf: Optional[Tensor] = None, *, lr: float,
              momentum: float, weight_decay: float, scale: float,
              lr_t: Optional[Tensor] = None, nesterov: bool = False) -> None:
    """Momentum SGD over one flat range (a rank's shard of a reduce-scattered bucket):
    d = grad * scale + wd * w32; mom = momentum * mom + d; w32 -= lr * mom; with bf16 ``grad``
    the fp32 ``w32`` are masters and ``wbf`` receives the rounded bf16 weights. An fp32 ``grad``
    with ``wbf`` is the wide layout (a reduce-scatter that summed in fp32 over fp32 masters of
    bf16 weights), which the ``shard_update`` kernel runs. ``nesterov``: w32 -= lr * (d +
    momentum * mom); every layout then goes through ``shard_update``."""
    if nesterov:
        _nesterov_kw(nesterov, momentum)
        _impl(w32).shard_update(rule=reference.OPT_NESTEROV, grad=grad, w32=w32, st0=mom, wbf=wbf,
                                lr=float(lr), a=0.0, oma=0.0, b=float(momentum), omb=0.0, eps=0.0,
                                weight_decay=float(weight_decay), scale=float(scale),
                                lr_t=_check_lr_t(lr_t, w32))
        return
    if w32.is_cuda and wbf is not None and grad.dtype == torch.float32:
        _ext.load().shard_update(rule=reference.OPT_SGD, grad=grad, w32=w32, st0=mom, wbf=wbf,
                                 lr=float(lr), a=0.0, oma=0.0, b=float(momentum), omb=0.0, eps=0.0,
                                 weight_decay=float(weight_decay), scale=float(scale),
                                 lr_t=_check_lr_t(lr_t, w32))
        return
    _impl(w32).shard_sgd(grad, w32, mom, wbf, float(lr), float(momentum), float(weight_decay),
                         float(scale), lr_t=_check_lr_t(lr_t, w32))


def lr_schedule(table: Tensor, step: Tensor, lr: Tensor) -> None:
    """``lr[0] = schedule(step[0])``, then ``step[0] += 1``, in one launch (``table``: the segment
    table of :func:`arena_amd.ops.schedule.encode`)."""
    _impl(lr).lr_schedule(table, step, lr)


def _one_minus(x: float) -> float:
    """``1 - x`` in fp64 (the kernels receive it rounded once to fp32: the fp32 difference
    ``1 - float32(0.999)`` is 4.7e-5 off in relative terms)."""
    return 1.0 - float(x)


def mt_rmsprop_master(grads: Sequence[Tensor], offsets: Sequence[int], master: Tensor, ms: Tensor,
                      mom: Tensor, wbf: Tensor, *, lr: float, decay: float = 0.9,
                      momentum: float = 0.9, eps: float = 1.0, weight_decay: float = 0.0,
                      lr_t: Optional[Tensor] = None) -> None:
    """TF1 RMSProp over bf16 grads with fp32 masters, one launch per 48 tensors (the layout of
    :func:`mt_sgd_master` with two state buffers): d = g + wd * w; ms = decay * ms + (1 - decay)
    * d * d; mom = momentum * mom + lr * d / sqrt(ms + eps); w -= mom; ``wbf`` gets the rounded
    bf16 weights. Semantics: :mod:`arena_amd.ops.reference`."""
    _impl(master).mt_rmsprop_master(list(grads), [int(o) for o in offsets], master, ms, mom, wbf,
                                    float(lr), float(decay), _one_minus(decay), float(momentum),
                                    float(eps), float(weight_decay),
                                    lr_t=_check_lr_t(lr_t, master))


def mt_rmsprop_f32(grads: Sequence[Tensor], offsets: Sequence[int], w: Tensor, ms: Tensor,
                   mom: Tensor, *, lr: float, decay: float = 0.9, momentum: float = 0.9,
                   eps: float = 1.0, weight_decay: float = 0.0, scale: float = 1.0,
                   lr_t: Optional[Tensor] = None) -> None:
    """TF1 RMSProp over fp32 tensors with fp32 gradients (any sizes and offsets, as
    :func:`mt_sgd_f32`); d = g * scale + wd * w."""
    _impl(w).mt_rmsprop_f32(list(grads), [int(o) for o in offsets], w, ms, mom, float(lr),
                            float(decay), _one_minus(decay), float(momentum), float(eps),
                            float(weight_decay), float(scale), lr_t=_check_lr_t(lr_t, w))


def _check_corr(corr: Tensor, like: Tensor) -> Tensor:
    """The Adam clock's bias correction is one fp32 value on the updated tensors' device."""
    if corr.dtype != torch.float32 or corr.numel() != 1 or corr.device != like.device:
        raise ValueError(f"corr must be a float32 [1] tensor on {like.device} (got {corr.dtype} "
                         f"{tuple(corr.shape)} on {corr.device})")
    return corr


def mt_adam_master(grads: Sequence[Tensor], offsets: Sequence[int], master: Tensor, m: Tensor,
                   v: Tensor, wbf: Tensor, corr: Tensor, *, lr: float, betas=(0.9, 0.999),
                   eps: float = 1e-8, weight_decay: float = 0.0,
                   lr_t: Optional[Tensor] = None) -> None:
    """TF1 Adam over bf16 grads with fp32 masters, one launch per 48 tensors: d = g + wd * w;
    m = b1 * m + (1 - b1) * d; v = b2 * v + (1 - b2) * d * d; w -= (lr * corr) * m / (sqrt(v) +
    eps); ``wbf`` gets the rounded bf16 weights. ``corr`` (fp32 [1]) is the bias correction of
    this step, kept on the device by :func:`adam_tick`."""
    b1, b2 = float(betas[0]), float(betas[1])
    _impl(master).mt_adam_master(list(grads), [int(o) for o in offsets], master, m, v, wbf,
                                 _check_corr(corr, master), float(lr), b1, _one_minus(b1), b2,
                                 _one_minus(b2), float(eps), float(weight_decay),
                                 lr_t=_check_lr_t(lr_t, master))


def mt_adam_f32(grads: Sequence[Tensor], offsets: Sequence[int], w: Tensor, m: Tensor, v: Tensor,
                corr: Tensor, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                weight_decay: float = 0.0, scale: float = 1.0,
                lr_t: Optional[Tensor] = None) -> None:
    """TF1 Adam over fp32 tensors with fp32 gradients (any sizes and offsets, as
    :func:`mt_sgd_f32`); d = g * scale + wd * w."""
    b1, b2 = float(betas[0]), float(betas[1])
    _impl(w).mt_adam_f32(list(grads), [int(o) for o in offsets], w, m, v, _check_corr(corr, w),
                         float(lr), b1, _one_minus(b1), b2, _one_minus(b2), float(eps),
                         float(weight_decay), float(scale), lr_t=_check_lr_t(lr_t, w))


def mt_lars_workspace_floats(numels: Sequence[int]) -> int:
    """fp32 elements of :func:`mt_lars_master`'s ``workspace`` for tensors of these sizes: one
    (sum w^2, sum g^2) pair per 1024-element block."""
    return 2 * sum((int(n) + 1023) // 1024 for n in numels)


def mt_lars_master(grads: Sequence[Tensor], offsets: Sequence[int], master: Tensor, mom: Tensor,
                   wbf: Tensor, trust: Tensor, slots: Sequence[int], workspace: Tensor, *,
                   lr: float, momentum: float, weight_decay: float = 0.0, eeta: float = 0.001,
                   eps: float = 0.0, lr_t: Optional[Tensor] = None) -> None:
    """LARS over bf16 grads with fp32 masters (the layout of :func:`mt_sgd_master`), two launches
    per 48 tensors: per-block partial sums of w^2 and g^2 into ``workspace``, then the update,
    which reduces them per tensor on the device: trust = eeta * |w| / (|g| + wd * |w| + eps) (1.0
    when a norm is 0); m = momentum * m + (g + wd * w); w -= (lr * trust) * m; ``wbf`` gets the
    rounded bf16 weights. ``trust`` (fp32) receives tensor i's ratio at ``slots[i]``; the other
    entries keep their values. ``workspace``: fp32, at least
    :func:`mt_lars_workspace_floats` elements, contents irrelevant. Deterministic: no atomics.
    Semantics: :mod:`arena_amd.ops.reference`."""
    _impl(master).mt_lars_master(list(grads), [int(o) for o in offsets], master, mom, wbf, trust,
                                 [int(s) for s in slots], workspace, float(lr), float(momentum),
                                 float(weight_decay), float(eeta), float(eps),
                                 lr_t=_check_lr_t(lr_t, master))


def shard_rmsprop(grad: Tensor, w32: Tensor, ms: Tensor, mom: Tensor,
                  wbf: Optional[Tensor] = None, *, lr: float, decay: float = 0.9,
                  momentum: float = 0.9, eps: float = 1.0, weight_decay: float = 0.0,
                  scale: float = 1.0, lr_t: Optional[Tensor] = None) -> None:
    """TF1 RMSProp over one flat range (a rank's shard of a reduce-scattered bucket), d = grad *
    scale + wd * w32, in :func:`shard_sgd`'s three layouts: bf16 ``grad`` with ``wbf`` (fp32
    masters, rounded bf16 weights written), fp32 ``grad`` without (the fp32 weights are their own
    masters), fp32 ``grad`` with ``wbf`` (wide)."""
    _impl(w32).shard_update(rule=reference.OPT_RMSPROP, grad=grad, w32=w32, st0=ms, st1=mom,
                            wbf=wbf, lr=float(lr), a=float(decay), oma=_one_minus(decay),
                            b=float(momentum), omb=0.0, eps=float(eps),
                            weight_decay=float(weight_decay), scale=float(scale),
                            lr_t=_check_lr_t(lr_t, w32))


def shard_adam(grad: Tensor, w32: Tensor, m: Tensor, v: Tensor, corr: Tensor,
               wbf: Optional[Tensor] = None, *, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
               weight_decay: float = 0.0, scale: float = 1.0,
               lr_t: Optional[Tensor] = None) -> None:
    """TF1 Adam over one flat range, the layouts of :func:`shard_rmsprop`; ``corr`` (fp32 [1]) is
    the bias correction of this step, kept on the device by :func:`adam_tick`."""
    b1, b2 = float(betas[0]), float(betas[1])
    _impl(w32).shard_update(rule=reference.OPT_ADAM, grad=grad, w32=w32, st0=m, st1=v, wbf=wbf,
                            corr=_check_corr(corr, w32), lr=float(lr), a=b1, oma=_one_minus(b1),
                            b=b2, omb=_one_minus(b2), eps=float(eps),
                            weight_decay=float(weight_decay), scale=float(scale),
                            lr_t=_check_lr_t(lr_t, w32))


def shard_lars_norms(grad: Tensor, master: Tensor, goffs: Sequence[int], moffs: Sequence[int],
                     ns: Sequence[int], slots: Sequence[int], sums: Tensor, workspace: Tensor, *,
                     scale: float) -> None:
    """Sharded LARS, first half. ``grad``: a rank's shard of a summed (bf16 or fp32) gradient;
    piece i is ``ns[i]`` elements at ``grad[goffs[i]:]`` and ``master[moffs[i]:]`` of tensor
    ``slots[i]``. ``sums`` (fp64, two entries per tensor of the sub-range) receives the sums of
    w^2 and (g * scale)^2 over this rank's piece of each tensor, 0.0 without one. The caller
    all-reduces ``sums`` before :func:`shard_lars_update`. ``workspace``: fp32, at least
    ``mt_lars_workspace_floats(ns)`` elements. Deterministic: no atomics."""
    _impl(master).shard_lars_norms(grad, master, [int(o) for o in goffs], [int(o) for o in moffs],
                                   [int(n) for n in ns], [int(s) for s in slots], sums, workspace,
                                   float(scale))


def shard_lars_update(grad: Tensor, master: Tensor, mom: Tensor, wbf: Tensor,
                      goffs: Sequence[int], moffs: Sequence[int], ns: Sequence[int],
                      slots: Sequence[int], sums: Tensor, trust: Tensor, *, lr: float,
                      momentum: float, weight_decay: float = 0.0, eeta: float = 0.001,
                      eps: float = 0.0, scale: float = 1.0,
                      lr_t: Optional[Tensor] = None) -> None:
    """Sharded LARS, second half: ``trust[s]`` for every tensor of the sub-range from the reduced
    ``sums`` (1.0 when a norm is 0), then d = g * scale + wd * w; m = momentum * m + d; w -= (lr *
    trust) * m over this rank's pieces, rounded bf16 weights to ``wbf``. ``master`` / ``mom`` /
    ``wbf``: the flat buffers ``moffs`` index."""
    _impl(master).shard_lars_update(grad, master, mom, wbf, [int(o) for o in goffs],
                                    [int(o) for o in moffs], [int(n) for n in ns],
                                    [int(s) for s in slots], sums, trust, float(lr),
                                    float(momentum), float(weight_decay), float(eeta), float(eps),
                                    float(scale), lr_t=_check_lr_t(lr_t, master))


def adam_tick(step: Tensor, pow: Tensor, corr: Tensor, b1: float, b2: float) -> None:
    """One tick of Adam's device clock, in one launch: ``pow *= (b1, b2)`` (fp64 running products
    ``b1^t``, ``b2^t``), ``corr[0] = float32(sqrt(1 - pow[1]) / (1 - pow[0]))``, ``step[0] += 1``
    (:func:`arena_amd.ops.reference.reference_adam_corr`)."""
    _impl(corr).adam_tick(step, pow, corr, float(b1), float(b2))
