"""Plain-PyTorch fp32 reference implementations of every arena_amd HIP kernel.

Used (a) as the numerics oracle in tests and (b) as the implementation for CPU tensors (the
multi-process gloo paths that run without a GPU). Semantics match csrc/ops/mlp_kernels.hip
and csrc/ops/optim_kernels.hip exactly, including the counter-hash dropout mask, the device step
counters and the gather.
"""
from __future__ import annotations

import math

import numpy as np
import torch

_M32 = 0xFFFFFFFF


def _mul32(h: torch.Tensor, c: int) -> torch.Tensor:
    """(h * c) mod 2**32 for int64 tensors holding uint32 values, without int64 overflow."""
    lo = h & 0xFFFF
    hi = h >> 16
    return ((lo * c) + (((hi * c) & 0xFFFF) << 16)) & _M32


def _mix32(h: torch.Tensor) -> torch.Tensor:
    h = h ^ (h >> 16)
    h = _mul32(h, 0x7FEB352D)
    h = h ^ (h >> 15)
    h = _mul32(h, 0x846CA68B)
    h = h ^ (h >> 16)
    return h


def hash4(seed: int, step: int, rows: torch.Tensor, cols: torch.Tensor) -> torch.Tensor:
    """uint32 hash of (seed, step, row, col) -- bit-identical to arena::hash4 (common.h)."""
    h = torch.full_like(rows, (seed & _M32) ^ 0x9E3779B9, dtype=torch.int64)
    h = _mix32(h)
    h = _mix32(h ^ _mul32(torch.full_like(h, step & _M32), 0x85EBCA77))
    h = _mix32(h ^ _mul32(rows.to(torch.int64) & _M32, 0xC2B2AE3D))
    h = _mix32(h ^ _mul32(cols.to(torch.int64) & _M32, 0x27D4EB2F))
    return h


def keep_threshold(keep_prob: float) -> int:
    return 0xFFFFFFFF if keep_prob >= 1.0 else int(keep_prob * 4294967296.0)


def dropout_keep_mask(M: int, N: int, keep_prob: float, seed: int, step: int,
                      device=None) -> torch.Tensor:
    """Boolean [M, N] keep-mask used by linear_fwd's fused dropout."""
    if keep_prob >= 1.0:
        return torch.ones(M, N, dtype=torch.bool, device=device)
    rows = torch.arange(M, device=device, dtype=torch.int64).unsqueeze(1).expand(M, N)
    cols = torch.arange(N, device=device, dtype=torch.int64).unsqueeze(0).expand(M, N)
    return hash4(seed, step, rows, cols) < keep_threshold(keep_prob)


def _cursor_val(cursor: torch.Tensor | None, off: int) -> int:
    return (int(cursor.reshape(-1)[0].item()) if cursor is not None else 0) + off


def gather_rows(x: torch.Tensor, idx: torch.Tensor | None, cursor: torch.Tensor | None,
                batch: int, M: int, cursor_off: int = 0) -> torch.Tensor:
    if idx is None:
        return x[:M]
    cur = _cursor_val(cursor, cursor_off)
    pos = (cur * batch + torch.arange(M, dtype=torch.int64, device=x.device)) % idx.numel()
    return x[idx.to(torch.int64)[pos]]


def linear_fwd(x, x_scale, idx, cursor, batch, W, bias, Y, act, keep_prob, seed, step):
    M = Y.shape[0]
    xr = gather_rows(x, idx, cursor, batch, M).to(torch.float32) * x_scale
    z = xr @ W.t()  # W is [out, in]
    if bias is not None:
        z = z + bias
    if act == 1:
        z = torch.relu(z)
    if keep_prob < 1.0:
        st = int(step.reshape(-1)[0].item()) & _M32 if step is not None else 0
        mask = dropout_keep_mask(M, W.shape[0], keep_prob, seed, st, device=z.device)
        z = torch.where(mask, z * (1.0 / keep_prob), torch.zeros_like(z))
    Y.copy_(z)


def xent_head(H, W2, b2, labels, idx, cursor, batch, dlogits, dZ, keep_prob, relu_mask,
              loss_scale, loss_acc, correct_acc, hist_step, ctr_dst, ctr_src, ctr_add):
    M = H.shape[0]
    hs = int(hist_step.reshape(-1)[0].item()) if hist_step is not None else 0
    L = loss_acc.numel()
    slot = hs % L if L > 1 else 0
    if L > 1:
        loss_acc[(hs + 1) % L] = 0.0
        correct_acc[(hs + 1) % L] = 0
    logits = H @ W2.t()  # W2 is [classes, hidden]
    if b2 is not None:
        logits = logits + b2
    y = gather_rows(labels, idx, cursor, batch, M).to(torch.int64)
    lse = torch.logsumexp(logits, dim=1)
    loss = lse - logits.gather(1, y.unsqueeze(1)).squeeze(1)
    loss_acc[slot] += (loss * loss_scale).sum()
    correct_acc[slot] += (logits.argmax(dim=1) == y).sum().to(correct_acc.dtype)
    if ctr_dst is not None:
        src = int(ctr_src.reshape(-1)[0].item()) if ctr_src is not None else 0
        ctr_dst.fill_(src + ctr_add)
    if dlogits is None:
        return
    g = (torch.softmax(logits, dim=1) - torch.nn.functional.one_hot(y, W2.shape[0]).to(H.dtype))
    g = g * loss_scale
    dlogits.view(M, -1).copy_(g)
    if dZ is None:
        return
    dz = g @ W2
    if relu_mask:
        inv_keep = 1.0 / keep_prob if keep_prob < 1.0 else 1.0
        dz = torch.where(H > 0, dz * inv_keep, torch.zeros_like(dz))
    dZ.view(M, -1).copy_(dz)


def adam_update(p, m, v, g, lr, b1, b2, eps, wd, t, grad_scale, tf_style):
    """In-place Adam on tensors (fp32), same formula as adam_apply in csrc/ops/adam.h."""
    g = g * grad_scale + wd * p
    m.mul_(b1).add_(g, alpha=1.0 - b1)
    v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    if tf_style:
        step_size = lr * math.sqrt(bc2) / bc1
        p.sub_(step_size * m / (v.sqrt() + eps))
    else:
        p.sub_((lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps))


def head_dz(dl, w2, h, keep_prob):
    """dz = (dlogits · W2) ⊙ (h > 0) / keep -- ReLU + dropout backward through the head."""
    dz = dl @ w2
    inv_keep = 1.0 / keep_prob
    return torch.where(h > 0, dz * inv_keep, torch.zeros_like(dz))


def mlp_fwd_logits(x, x_scale, idx, cursor, batch, W1, b1, H, keep_prob, seed, step, W2, W2_copy,
                   logits2, xb, labels, yb, ctr_dst, ctr_src, ctr_add, xa=None, xa_parity=-1):
    """Reference for the logits-emitting forward: H and logits2[step & 1] += H·W2ᵀ.
    ``xa`` [2, M, K]: the batch is ``xa[step & 1]`` (published by the previous ``wgrad_grouped``);
    a launch-time ``xa_parity`` must name that half (kernel contract, checked here)."""
    if xa is not None:
        st = int(step.reshape(-1)[0].item())
        if xa_parity >= 0 and (st & 1) != xa_parity:
            raise AssertionError(f"xa parity {xa_parity} does not match step {st}")
        if idx is not None or xb is not None:
            raise AssertionError("xa replaces the idx/cursor gather and the xb/yb publication")
        x = xa[st & 1]
    if ctr_dst is not None:
        src = int(ctr_src.reshape(-1)[0].item()) if ctr_src is not None else 0
        ctr_new = src + ctr_add
    linear_fwd(x, x_scale, idx, cursor, batch, W1, b1, H, 1, keep_prob, seed, step)
    if xb is not None:
        M = H.shape[0]
        xb.copy_(gather_rows(x, idx, cursor, batch, M))
        yb.copy_(gather_rows(labels, idx, cursor, batch, M).to(yb.dtype))
    if W2_copy is not None:
        W2_copy.view_as(W2).copy_(W2)
    st = int(step.reshape(-1)[0].item()) if step is not None else 0
    logits2[st & 1] += H @ W2.t()
    if ctr_dst is not None:
        ctr_dst.fill_(ctr_new)


def _head_dlogits(logits2, hd_step, hd_step_off, b2, labels, idx, cursor, cursor_off, batch,
                  gather_any, loss_scale, loss_acc, correct_acc):
    hstep = int(hd_step.reshape(-1)[0].item()) + hd_step_off
    lg = logits2[hstep & 1].clone()
    M, C = lg.shape
    if b2 is not None:
        lg = lg + b2
    y = (gather_rows(labels, idx, cursor, batch, M, cursor_off) if gather_any
         else labels[:M]).to(torch.int64)
    lse = torch.logsumexp(lg, dim=1)
    loss = lse - lg.gather(1, y.unsqueeze(1)).squeeze(1)
    L = loss_acc.numel()
    loss_acc[(hstep + 1) & (L - 1)] = 0.0
    correct_acc[(hstep + 1) & (L - 1)] = 0
    loss_acc[hstep & (L - 1)] += (loss * loss_scale).sum()
    correct_acc[hstep & (L - 1)] += (lg.argmax(dim=1) == y).sum().to(correct_acc.dtype)
    dl = (torch.softmax(lg, dim=1) - torch.nn.functional.one_hot(y, C).to(lg.dtype)) * loss_scale
    logits2[(hstep + 1) & 1].zero_()
    return dl


def wgrad_grouped(xs, x_scales, gather, idx, cursor, cursor_off, batch, dzs, hd_modes, hd_w2, hd_h,
                  hd_keep_prob, hd_logits2, hd_step, hd_step_off, hd_b2, hd_labels, hd_loss_scale,
                  hd_loss_acc, hd_correct_acc, mode, outW, outB, mW, vW, mB, vB, lr, lr_t, b1, b2,
                  eps, wd, t_step, grad_scale, tf_style, ctr_dst, ctr_src, ctr_add, next_xa=None,
                  next_ya=None, hd_parity=-1, next_x=None, next_labels=None, next_perm=None):
    if hd_parity >= 0:  # the launch-time parity must name the counter's buffer (kernel contract)
        hs = int(hd_step.reshape(-1)[0].item()) + hd_step_off
        if (hs & 1) != hd_parity:
            raise AssertionError(f"head parity {hd_parity} does not match step {hs}")
    t = int(t_step.reshape(-1)[0].item()) if t_step is not None else 1
    lr_v = float(lr_t.reshape(-1)[0].item()) if lr_t is not None else lr
    dl = None
    if any(m != 0 for m in hd_modes):  # step-parity pairs: this step reads half (step & 1)
        par = (int(hd_step.reshape(-1)[0].item()) + hd_step_off) & 1
        xs = [x[par] if (x.dim() == 3 and m != 0) else x for x, m in zip(xs, hd_modes)]
        if hd_labels.dim() == 2:
            hd_labels = hd_labels[par]
    if next_xa is not None:  # publish the next step's batch into the other half
        st = int(hd_step.reshape(-1)[0].item()) + hd_step_off + 1
        n, L = next_xa.shape[1], next_perm.numel()
        pos = (st * n + torch.arange(n, device=next_perm.device)) % L
        rows = next_perm.reshape(-1)[pos].to(torch.int64)
        next_xa[st & 1].copy_(next_x[rows])
        next_ya[st & 1].copy_(next_labels[rows].to(next_ya.dtype))
    if any(m != 0 for m in hd_modes):
        dl = _head_dlogits(hd_logits2, hd_step, hd_step_off, hd_b2, hd_labels, idx, cursor,
                           cursor_off, batch, any(gather), hd_loss_scale, hd_loss_acc,
                           hd_correct_acc)
    pending = []
    for i in range(len(xs)):
        if hd_modes[i] == 0:
            dz = dzs[i]
        elif hd_modes[i] == 1:
            dz = dl
        else:
            dz = head_dz(dl, hd_w2[i], hd_h[i], hd_keep_prob)
        M = dz.shape[0]
        if gather[i]:
            xr = gather_rows(xs[i], idx, cursor, batch, M, cursor_off)
        else:
            xr = xs[i][:M]
        xr = xr.to(torch.float32) * x_scales[i]
        gw = dz.t() @ xr  # [N, K] = [out, in]
        gb = dz.sum(dim=0)
        pending.append((i, gw, gb))
    for i, gw, gb in pending:
        if mode == 0:
            outW[i].view_as(gw).copy_(gw * grad_scale)
            if outB[i] is not None:
                outB[i].copy_(gb * grad_scale)
        else:
            adam_update(outW[i].view_as(gw), mW[i].view_as(gw), vW[i].view_as(gw), gw, lr_v, b1,
                        b2, eps, wd, t, grad_scale, tf_style)
            if outB[i] is not None:
                adam_update(outB[i], mB[i], vB[i], gb, lr_v, b1, b2, eps, wd, t, grad_scale,
                            tf_style)
    if ctr_dst is not None:
        src = int(ctr_src.reshape(-1)[0].item()) if ctr_src is not None else 0
        ctr_dst.fill_(src + ctr_add)


def adam_flat(P, M, V, G, lr, lr_t, b1, b2, eps, wd, t_step, grad_scale, tf_style, ctr_dst,
              ctr_src, ctr_add):
    t = int(t_step.reshape(-1)[0].item()) if t_step is not None else 1
    lr_v = float(lr_t.reshape(-1)[0].item()) if lr_t is not None else lr
    adam_update(P, M, V, G, lr_v, b1, b2, eps, wd, t, grad_scale, tf_style)
    if ctr_dst is not None:
        src = int(ctr_src.reshape(-1)[0].item()) if ctr_src is not None else 0
        ctr_dst.fill_(src + ctr_add)


def sgd_flat(P, G, lr, lr_t, grad_scale):
    lr_v = float(lr_t.reshape(-1)[0].item()) if lr_t is not None else lr
    P.sub_(G * (lr_v * grad_scale))


def softmax_xent(logits, labels, grad_scale, need_grad):
    lse = torch.logsumexp(logits, dim=1)
    loss = lse - logits.gather(1, labels.unsqueeze(1)).squeeze(1)
    if not need_grad:
        return [loss]
    d = torch.softmax(logits, dim=1)
    d[torch.arange(labels.numel()), labels] -= 1.0
    return [loss, d * grad_scale]


def mt_copy_scale(tensors, offsets, flat, scale, direction):
    for t, off in zip(tensors, offsets):
        n = t.numel()
        if direction == 0:
            flat[off:off + n].copy_(t.reshape(-1) * scale)
        else:
            t.view(-1).copy_(flat[off:off + n] * scale)


def _storage_flat(t):
    """A dense tensor's elements in memory order (channels_last weights included)."""
    return t.as_strided((t.numel(),), (1,), t.storage_offset())


def _lr_value(lr, lr_t):
    return float(lr_t.reshape(-1)[0].item()) if lr_t is not None else lr


def mt_sgd_master(grads, offsets, master, mom, wbf, lr, momentum, weight_decay, lr_t=None,
                  nesterov=False):
    lr = _lr_value(lr, lr_t)
    for g, off in zip(grads, offsets):
        n = g.numel()
        w, m = master[off:off + n], mom[off:off + n]
        if nesterov:
            _nesterov(_storage_flat(g).float(), w, m, lr, momentum, weight_decay, None)
        else:
            m.mul_(momentum).add_(_storage_flat(g).float() + weight_decay * w)
            w.sub_(lr * m)
        wbf[off:off + n].copy_(w)


def mt_sgd_f32(grads, offsets, w, mom, lr, momentum, weight_decay, scale, lr_t=None,
               nesterov=False):
    """CPU reference of the HIP ``mt_sgd_f32`` kernel (same operation order as ``shard_sgd``)."""
    lr = _lr_value(lr, lr_t)
    for g, off in zip(grads, offsets):
        n = g.numel()
        ws, m = w[off:off + n], mom[off:off + n]
        if nesterov:
            _nesterov(_storage_flat(g), ws, m, lr, momentum, weight_decay, scale)
            continue
        d = _storage_flat(g) * scale + weight_decay * ws
        m.mul_(momentum).add_(d)
        ws.sub_(lr * m)


# ------------------------------------------------------------------------------------------------
# RMSProp and Adam, TF1's forms (tf_cnn_benchmarks' defaults assume them: --rmsprop_epsilon 1.0
# sits inside the square root). Defined once, here; the HIP kernels (``RmspropRule`` / ``AdamRule``
# in csrc/ops/optim_kernels.hip), ``TFRMSprop`` / ``TFAdam`` and the tests follow it. Both take the
# coupled gradient of the SGD kernels, ``d = g * scale + wd * w`` (``scale`` only on the fp32
# group), and every operation below is an fp32 operation in the order written:
#
#   RMSProp (non-centred; ms starts at 1.0 as TF's slot does, mom at 0):
#       ms  = rho * ms + omr * (d * d)
#       mom = mu * mom + lr * d / sqrt(ms + eps)
#       w   = w - mom
#   Adam (m and v start at 0):
#       m = b1 * m + omb1 * d
#       v = b2 * v + omb2 * (d * d)
#       w = w - (lr * corr) * m / (sqrt(v) + eps)
#
# ``omr = 1 - rho``, ``omb1 = 1 - b1`` and ``omb2 = 1 - b2`` are formed by the caller in fp64 and
# rounded to fp32 once (``1 - float32(0.999)`` is 4.7e-5 off in relative terms). ``corr`` is the
# bias correction ``sqrt(1 - b2^t) / (1 - b1^t)`` of step t = 1, 2, ...:
# :func:`reference_adam_corr`, kept on the device by the ``arena_adam_tick`` kernel
# (:func:`adam_tick` here).
# ------------------------------------------------------------------------------------------------
def reference_adam_corr(b1: float, b2: float, t: int) -> np.float32:
    """Adam's bias correction at step ``t`` >= 1 (the definition ``arena_adam_tick`` matches bit
    for bit): ``b1^t`` and ``b2^t`` as running products of Python floats (fp64, one rounding per
    operation), ``float32(sqrt(1 - b2^t) / (1 - b1^t))``."""
    t = int(t)
    if t < 1:
        raise ValueError(f"Adam's bias correction is defined from step 1 on, got t = {t}")
    b1, b2 = float(b1), float(b2)
    p1 = p2 = 1.0
    for _ in range(t):
        p1 *= b1
        p2 *= b2
    return np.float32(math.sqrt(1.0 - p2) / (1.0 - p1))


def adam_tick(step, pow, corr, b1, b2):
    """CPU form of the ``arena_adam_tick`` kernel: one step of the running products."""
    p1 = float(pow[0].item()) * float(b1)
    p2 = float(pow[1].item()) * float(b2)
    pow[0], pow[1] = p1, p2
    corr.fill_(float(np.float32(math.sqrt(1.0 - p2) / (1.0 - p1))))
    step.add_(1)


def _f32(v) -> torch.Tensor:
    """A Python number rounded once to fp32, as the kernels receive their arguments."""
    return torch.tensor(float(v), dtype=torch.float32)


def _rmsprop(g, w, ms, mom, lr, rho, omr, mu, eps, wd, scale):
    d = g * _f32(scale) + _f32(wd) * w
    ms.copy_(_f32(rho) * ms + _f32(omr) * (d * d))
    mom.copy_(_f32(mu) * mom + _f32(lr) * d / torch.sqrt(ms + _f32(eps)))
    w.sub_(mom)


def _adam(g, w, m, v, step, b1, omb1, b2, omb2, eps, wd, scale):
    d = g * _f32(scale) + _f32(wd) * w
    m.copy_(_f32(b1) * m + _f32(omb1) * d)
    v.copy_(_f32(b2) * v + _f32(omb2) * (d * d))
    w.sub_(step * m / (torch.sqrt(v) + _f32(eps)))


# ------------------------------------------------------------------------------------------------
# Nesterov momentum: TF's ``MomentumOptimizer(use_nesterov=True)`` (what tf_cnn_benchmarks'
# ``--optimizer momentum`` builds), which is also ``torch.optim.SGD(nesterov=True)`` with dampening
# 0. Defined once, here; the HIP kernels (``NesterovRule`` / ``NesterovScaledRule`` in
# csrc/ops/optim_kernels.hip, ``sgd1_nesterov`` in csrc/ccl/xgmi_ccl.hip), the optimizers'
# ``nesterov=True`` and the tests follow it. Every operation is an fp32 operation, in the order
# written:
#
#       d = g * scale + wd * w        (master layout: d = g + wd * w, no scale, as the plain rule)
#       m = mu * m + d                (m starts at 0)
#       w = w - step * (d + mu * m)   (step: the float lr, or the DeviceLR value)
#
# One state: the momentum buffer means what it means under the plain rule, so the two rules'
# states have the same keys. The rule requires ``mu > 0``.
# ------------------------------------------------------------------------------------------------
def _nesterov(g, w, m, step, mu, wd, scale):
    """One Nesterov step in place; ``scale`` None: the master layout's unscaled ``d``."""
    if not float(mu) > 0.0:
        raise ValueError(f"Nesterov momentum needs momentum > 0, got {mu}")
    d = (g if scale is None else g * _f32(scale)) + _f32(wd) * w
    m.copy_(_f32(mu) * m + d)
    w.sub_(_f32(step) * (d + _f32(mu) * m))


def mt_rmsprop_master(grads, offsets, master, ms, mom, wbf, lr, rho, omr, momentum, eps,
                      weight_decay, lr_t=None):
    """CPU reference of the HIP ``mt_rmsprop_master`` kernel."""
    lr = _lr_value(lr, lr_t)
    for g, off in zip(grads, offsets):
        s = slice(off, off + g.numel())
        _rmsprop(_storage_flat(g).float(), master[s], ms[s], mom[s], lr, rho, omr, momentum, eps,
                 weight_decay, 1.0)
        wbf[s].copy_(master[s])


def mt_rmsprop_f32(grads, offsets, w, ms, mom, lr, rho, omr, momentum, eps, weight_decay, scale,
                   lr_t=None):
    """CPU reference of the HIP ``mt_rmsprop_f32`` kernel."""
    lr = _lr_value(lr, lr_t)
    for g, off in zip(grads, offsets):
        s = slice(off, off + g.numel())
        _rmsprop(_storage_flat(g), w[s], ms[s], mom[s], lr, rho, omr, momentum, eps, weight_decay,
                 scale)


def mt_adam_master(grads, offsets, master, m, v, wbf, corr, lr, b1, omb1, b2, omb2, eps,
                   weight_decay, lr_t=None):
    """CPU reference of the HIP ``mt_adam_master`` kernel (``corr``: the clock's fp32 [1])."""
    step = _f32(_lr_value(lr, lr_t)) * corr.reshape(())
    for g, off in zip(grads, offsets):
        s = slice(off, off + g.numel())
        _adam(_storage_flat(g).float(), master[s], m[s], v[s], step, b1, omb1, b2, omb2, eps,
              weight_decay, 1.0)
        wbf[s].copy_(master[s])


def mt_adam_f32(grads, offsets, w, m, v, corr, lr, b1, omb1, b2, omb2, eps, weight_decay, scale,
                lr_t=None):
    """CPU reference of the HIP ``mt_adam_f32`` kernel."""
    step = _f32(_lr_value(lr, lr_t)) * corr.reshape(())
    for g, off in zip(grads, offsets):
        s = slice(off, off + g.numel())
        _adam(_storage_flat(g), w[s], m[s], v[s], step, b1, omb1, b2, omb2, eps, weight_decay,
              scale)


# ------------------------------------------------------------------------------------------------
# LARS (layer-wise adaptive rate scaling), tf.contrib's LARSOptimizer as the MLPerf ResNet
# reference uses it: momentum SGD whose learning rate is scaled per tensor. Defined once, here; the
# HIP kernels (``mt_lars_*_kernel`` in csrc/ops/optim_kernels.hip), ``MasterLARS`` / ``TFLars`` and
# the tests follow it. For a tensor with fp32 master w, bf16 gradient g and momentum m:
#
#       wn = ||w||2            gn = ||g||2
#       trust = eeta * wn / (gn + wd * wn + eps)    if wn > 0 and gn > 0, else 1.0
#       step  = lr * trust
#       m = mu * m + (g + wd * w)
#       w = w - step * m                            wbf = bf16(w)
#
# The norms are fp64 sums over the squares of the fp32 values in memory order (the bf16 gradient
# widens to fp32 exactly), ``wn`` and ``gn`` are ``float32(sqrt(sum))``, ``trust`` and ``step``
# are fp32 operations in the order written, and the last two lines are ``mt_sgd_master``'s. A
# kernel may sum in any fixed order, in fp32 or wider. BatchNorm scales / shifts and biases are on
# LARS's skip list: they keep plain momentum SGD without weight decay (``mt_sgd_f32``).
# ------------------------------------------------------------------------------------------------
def _sum_squares(v: torch.Tensor) -> float:
    """The fp64 sum of the squares of ``v``'s fp32 values, in memory order."""
    if v.numel() == 0:
        return 0.0
    d = v.double()
    return float(torch.cumsum(d * d, 0)[-1])


def reference_lars_trust(w, g, eeta, weight_decay, eps) -> torch.Tensor:
    """LARS's trust ratio of one tensor (flat fp32 ``w`` and ``g``) as an fp32 scalar tensor."""
    return lars_trust_of_sums(_sum_squares(w), _sum_squares(g), eeta, weight_decay, eps)


def lars_trust_of_sums(sw: float, sg: float, eeta, weight_decay, eps) -> torch.Tensor:
    """The trust ratio from the two fp64 sums of squares (sharded LARS all-reduces them)."""
    wn = _f32(math.sqrt(float(sw)))
    gn = _f32(math.sqrt(float(sg)))
    if not (wn > 0 and gn > 0):
        return _f32(1.0)
    return _f32(eeta) * wn / (gn + _f32(weight_decay) * wn + _f32(eps))


def mt_lars_master(grads, offsets, master, mom, wbf, trust, slots, workspace, lr, momentum,
                   weight_decay, eeta, eps, lr_t=None):
    """CPU reference of the HIP ``mt_lars_master`` kernels (``workspace`` is not used)."""
    lr = _f32(_lr_value(lr, lr_t))
    for g, off, slot in zip(grads, offsets, slots):
        n = g.numel()
        if n == 0:
            continue
        w, m = master[off:off + n], mom[off:off + n]
        g32 = _storage_flat(g).float()
        t = reference_lars_trust(w, g32, eeta, weight_decay, eps)
        trust[slot] = t
        step = lr * t
        m.mul_(momentum).add_(g32 + weight_decay * w)
        w.sub_(step * m)
        wbf[off:off + n].copy_(w)


def lr_schedule(table, step, lr):
    """CPU form of the ``arena_lr_schedule`` kernel: decodes the device table and evaluates
    :func:`arena_amd.ops.schedule.reference_lr`."""
    from . import schedule
    t = int(step.reshape(-1)[0].item())
    lr.fill_(float(schedule.reference_lr(schedule.decode(table), t)))
    step.add_(1)


def shard_sgd(grad, w32, mom, wbf, lr, momentum, weight_decay, scale, lr_t=None):
    """CPU reference of the HIP ``shard_sgd`` kernel (same operation order)."""
    lr = _lr_value(lr, lr_t)
    d = grad.float() * scale + weight_decay * w32
    mom.mul_(momentum).add_(d)
    w32.sub_(lr * mom)
    if wbf is not None:
        wbf.copy_(w32)


OPT_SGD, OPT_RMSPROP, OPT_ADAM, OPT_NESTEROV = 0, 1, 2, 3      # csrc/ops/abi.h ARENA_OPT_*


def shard_update(rule, grad, w32, st0, st1=None, wbf=None, corr=None, *, lr, a, oma, b, omb, eps,
                 weight_decay, scale, lr_t=None):
    """CPU reference of the HIP ``shard_update`` kernels: ``rule`` over one flat range, ``a`` /
    ``oma`` / ``b`` / ``omb`` as ``ArenaOptHyper`` names them (RMSProp: rho, 1 - rho, momentum, -;
    Adam: b1, 1 - b1, b2, 1 - b2; SGD and Nesterov SGD: -, -, momentum, -). ``st0`` / ``st1``:
    RMSProp's ms / mom, Adam's m / v, SGD's and Nesterov SGD's mom. With ``wbf`` the fp32 ``w32``
    are masters and ``wbf`` receives the rounded bf16 weights."""
    if rule == OPT_SGD:
        shard_sgd(grad, w32, st0, wbf, lr, b, weight_decay, scale, lr_t=lr_t)
        return
    g = grad.float()
    if rule == OPT_NESTEROV:
        _nesterov(g, w32, st0, _lr_value(lr, lr_t), b, weight_decay, scale)
    elif rule == OPT_RMSPROP:
        _rmsprop(g, w32, st0, st1, _lr_value(lr, lr_t), a, oma, b, eps, weight_decay, scale)
    elif rule == OPT_ADAM:
        step = _f32(_lr_value(lr, lr_t)) * corr.reshape(())
        _adam(g, w32, st0, st1, step, a, oma, b, omb, eps, weight_decay, scale)
    else:
        raise ValueError(f"shard_update: unknown rule {rule}")
    if wbf is not None:
        wbf.copy_(w32)


# ------------------------------------------------------------------------------------------------
# Sharded LARS (``ShardedMasterSGD(rule="lars")``): the definition above on the AVERAGED gradient
# of data-parallel ranks, each of which holds a shard of the summed gradient after the
# reduce-scatter. With ``scale = 1 / world`` and g the summed gradient:
#
#       d = g * scale (an fp32 product)       wn = ||w||2       gn = ||d||2
#       trust, step as above
#       m = mu * m + (d + wd * w)             w = w - step * m          wbf = bf16(w)
#
# A shard intersects several tensors; each intersection is a piece. ``shard_lars_norms`` gives the
# fp64 sums of w^2 and d^2 over each piece of this rank (0.0 for tensors without one), the ranks
# all-reduce the sums (every rank then holds the same bits, so the same trust), and
# ``shard_lars_update`` forms ``wn`` / ``gn`` = ``float32(sqrt(sum))`` and steps its pieces.
# ------------------------------------------------------------------------------------------------
def shard_lars_norms(grad, master, goffs, moffs, ns, slots, sums, workspace, scale):
    """CPU reference of the HIP ``shard_lars_norms`` kernels (``workspace`` is not used)."""
    sums.zero_()
    for go, mo, n, slot in zip(goffs, moffs, ns, slots):
        sums[2 * slot] = _sum_squares(master[mo:mo + n])
        sums[2 * slot + 1] = _sum_squares(grad[go:go + n].float() * _f32(scale))


def shard_lars_update(grad, master, mom, wbf, goffs, moffs, ns, slots, sums, trust, lr, momentum,
                      weight_decay, eeta, eps, scale, lr_t=None):
    """CPU reference of the HIP ``shard_lars_update`` kernels: ``trust[s]`` for every tensor of the
    sub-range from the (reduced) ``sums``, then ``shard_sgd``'s lines over the pieces with the
    step ``lr * trust``."""
    lr = _f32(_lr_value(lr, lr_t))
    for s in range(trust.numel()):
        trust[s] = lars_trust_of_sums(sums[2 * s], sums[2 * s + 1], eeta, weight_decay, eps)
    for go, mo, n, slot in zip(goffs, moffs, ns, slots):
        w, m = master[mo:mo + n], mom[mo:mo + n]
        d = grad[go:go + n].float() * scale + weight_decay * w
        m.mul_(momentum).add_(d)
        w.sub_((lr * trust[slot]) * m)
        wbf[mo:mo + n].copy_(w)


# ------------------------------------------------------------------------------------------------
# Device-resident image pipeline (csrc/ops/data_kernels.hip). Everything the kernel and this
# reference must agree on is defined once, here:
#
# * rows: ``pos = cursor * B + r``; training takes ``perm[pos % L]``; evaluation takes
#   ``perm[pos]`` while ``pos < L`` and pads the rest (zero image, label IMAGE_PAD_LABEL, row -1).
#   A permutation entry outside ``[0, n)`` is padding too.
# * the hash: ``image_hash(seed, stream, pos, k) = hash4(seed, stream * 4 + k, pos & 0xFFFFFFFF,
#   pos >> 32)`` for draw k (0: y0, 1: x0, 2: flip) -- a function of (seed, stream, pos) alone.
# * uniform to range: ``uniform_below(h, m) = (h * m) >> 32`` (the high word of the product), so
#   ``y0 = uniform_below(h0, S - Hc + 1)``, ``x0 = uniform_below(h1, S - Wc + 1)``, ``flip = h2 >>
#   31``. Evaluation: the centre crop ``((S - Hc) // 2, (S - Wc) // 2)``, no flip.
# * the table: ``image_table(mean, std, dtype)[c][u] = ((u / 255 - mean[c]) / std[c])`` computed
#   in fp32 on the host and rounded once to ``dtype``; both sides only look values up.
# * the space-to-depth channel: ``s2d_channel(dy, dx, c) = (dy * 2 + dx) * 3 + c``, channels
#   12..15 zero, ``z[n][ch][i][j] = x[n][c][2i + dy][2j + dx]`` (the order of ``s2d_stem``).
# ------------------------------------------------------------------------------------------------
IMAGE_PAD_LABEL = -100


def image_hash(seed: int, stream: int, pos: torch.Tensor, k: int) -> torch.Tensor:
    pos = pos.to(torch.int64)
    return hash4(seed, (stream * 4 + k) & _M32, pos & _M32, (pos >> 32) & _M32)


def uniform_below(h: torch.Tensor, m: int) -> torch.Tensor:
    """uint32 hash -> integer in [0, m), m <= 2**16 (the product stays inside int64)."""
    return (h * m) >> 32


def image_crop_draws(pos: torch.Tensor, S: int, Hc: int, Wc: int, train: bool, seed: int,
                     stream: int):
    """(y0, x0, flip) int64 tensors for batch positions ``pos``."""
    if not train:
        one = torch.ones_like(pos, dtype=torch.int64)
        return one * ((S - Hc) // 2), one * ((S - Wc) // 2), one * 0
    return (uniform_below(image_hash(seed, stream, pos, 0), S - Hc + 1),
            uniform_below(image_hash(seed, stream, pos, 1), S - Wc + 1),
            image_hash(seed, stream, pos, 2) >> 31)


def image_table(mean, std, dtype=torch.float32) -> torch.Tensor:
    """[3, 256] lookup table of ``(u / 255 - mean[c]) / std[c]`` (fp32 arithmetic, one rounding)."""
    m = torch.tensor([float(v) for v in mean], dtype=torch.float32).view(3, 1)
    s = torch.tensor([float(v) for v in std], dtype=torch.float32).view(3, 1)
    u = torch.arange(256, dtype=torch.float32).view(1, 256)
    return ((u / 255.0 - m) / s).to(dtype).contiguous()


def s2d_channel(dy: int, dx: int, c: int) -> int:
    return (dy * 2 + dx) * 3 + c


def image_batch(images, labels, perm, cursor, table, out, labels_out, rows_out, crop_out, crop_h,
                crop_w, train, seed, stream, layout, advance):
    """CPU twin of ``arena_image_batch`` (same arguments as the extension's ``image_batch``)."""
    n, S = images.shape[0], images.shape[1]
    B, L, Hc, Wc = out.shape[0], perm.numel(), int(crop_h), int(crop_w)
    if Hc % 2 or Wc % 2 or not (2 <= Hc <= S and 2 <= Wc <= S):
        raise ValueError("image_batch: the crop must be even and at most the stored size")
    if table.dtype != out.dtype or tuple(table.shape) != (3, 256):
        raise ValueError("image_batch: table must be [3, 256] in out's dtype")
    pos = _cursor_val(cursor, 0) * B + torch.arange(B, dtype=torch.int64)
    p64 = perm.to(torch.int64)
    if train:
        row = p64[pos % L]
    else:
        row = torch.where(pos < L, p64[pos.clamp(max=L - 1)], torch.full_like(pos, -1))
    valid = (row >= 0) & (row < n)
    row = torch.where(valid, row, torch.full_like(row, -1))
    y0, x0, flip = image_crop_draws(pos, S, Hc, Wc, bool(train), int(seed) & _M32, int(stream))
    xo = torch.arange(Wc, dtype=torch.int64).view(1, Wc)
    ys = y0.view(B, 1) + torch.arange(Hc, dtype=torch.int64).view(1, Hc)
    xs = x0.view(B, 1) + torch.where(flip.view(B, 1) != 0, Wc - 1 - xo, xo)
    px = images[row.clamp(min=0).view(B, 1, 1), ys.view(B, Hc, 1), xs.view(B, 1, Wc)]
    val = table[torch.arange(3).view(1, 1, 1, 3), px.to(torch.int64)]       # [B, Hc, Wc, 3]
    val = torch.where(valid.view(B, 1, 1, 1), val, torch.zeros_like(val))
    _image_store(out, val, layout)
    labels_out.copy_(torch.where(valid, labels.to(torch.int64)[row.clamp(min=0)],
                                 torch.full_like(row, IMAGE_PAD_LABEL)))
    rows_out.copy_(row)
    crop_out.view(B, 3).copy_(torch.stack([y0, x0, flip], dim=1))
    if advance:
        cursor.add_(1)


def _image_store(out, val, layout):
    """``val`` [B, Hc, Wc, 3] -> ``out``: x (layout 1) or its space-to-depth z (layout 0)."""
    B, Hc, Wc = val.shape[:3]
    if layout == 1:
        out.copy_(val.permute(0, 3, 1, 2))
    else:
        z = torch.zeros(B, Hc // 2, Wc // 2, 16, dtype=val.dtype)
        for dy in range(2):
            for dx in range(2):
                ch = s2d_channel(dy, dx, 0)
                z[..., ch:ch + 3] = val[:, dy::2, dx::2, :]
        out.copy_(z.permute(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------
# Random resized crop (image_batch_resized_kernel). On top of the definitions above:
#
# * the candidates: ``crop_box_table(S, area, aspect)`` lists the (h, w) boxes of a 64 x 32 grid
#   of (area fraction, aspect ratio) that fit the stored image; draw 3 picks one uniformly, so the
#   device needs neither a rejection loop nor a transcendental function.
# * the draws: ``box = uniform_below(h3, T)``, ``(h, w) = boxes[box]`` (clamped to [2, S]), ``y0 =
#   uniform_below(h0, S - h + 1)``, ``x0 = uniform_below(h1, S - w + 1)``, ``flip = h2 >> 31``.
# * the resampling: bilinear, half-pixel centres, 8-bit weights, integers only. ``resize_taps``
#   gives (i0, i1, f) per output index; the byte of a pixel is ``((256-fx)(256-fy) p00 + fx
#   (256-fy) p01 + (256-fx) fy p10 + fx fy p11 + 32768) >> 16`` and goes through the same table.
#   With (h, w) == (Hc, Wc) every f is 0 and i0 is the output index: the fixed crop, exactly.
# ------------------------------------------------------------------------------------------------
CROP_AREA = (0.05, 1.0)       # tf_cnn_benchmarks' area_range
CROP_ASPECT = (0.75, 1.33)    # ... and aspect_ratio_range
CROP_BOX_GRID = (64, 32)      # area steps x aspect steps
MAX_CROP_BOXES = 4096         # the launcher's bound on the table length


def crop_box_table(S: int, area=CROP_AREA, aspect=CROP_ASPECT) -> torch.Tensor:
    """int32 [T, 2] candidate (h, w) boxes in source pixels, row-major in (area, aspect) step."""
    S = int(S)
    lo, hi = (float(v) for v in area)
    rlo, rhi = (float(v) for v in aspect)
    if not (0.0 < lo <= hi <= 1.0):
        raise ValueError(f"crop_box_table: area range {area} must satisfy 0 < lo <= hi <= 1")
    if not (0.0 < rlo <= rhi < math.inf):
        raise ValueError(f"crop_box_table: aspect range {aspect} must satisfy 0 < lo <= hi < inf")
    na, nr = CROP_BOX_GRID
    rows = []
    for i in range(na):
        a = lo + (hi - lo) * (i + 0.5) / na
        for j in range(nr):
            r = math.exp(math.log(rlo) + (math.log(rhi) - math.log(rlo)) * (j + 0.5) / nr)
            w = math.floor(math.sqrt(a * S * S * r) + 0.5)
            h = math.floor(math.sqrt(a * S * S / r) + 0.5)
            if 2 <= h <= S and 2 <= w <= S:
                rows.append((h, w))
    if not rows:
        raise ValueError(f"crop_box_table: no box of area {area} and aspect {aspect} fits "
                         f"a {S} x {S} image")
    return torch.tensor(rows, dtype=torch.int32)


def resize_taps(n_out: int, extent: torch.Tensor):
    """(i0, i1, f) int64 [B, n_out]: output index o of ``n_out`` reads source indices i0 and i1 of
    ``extent`` [B] with weights 256 - f and f."""
    e = extent.to(torch.int64).view(-1, 1)
    o = torch.arange(n_out, dtype=torch.int64).view(1, n_out)
    num = ((2 * o + 1) * e - n_out).clamp(min=0)      # num < 0: i0 = 0 and f = 0
    den = 2 * n_out
    i0 = num // den
    f = ((num % den) * 256) // den
    return i0, torch.minimum(i0 + 1, e - 1), f


def image_box_draws(pos: torch.Tensor, S: int, boxes: torch.Tensor, seed: int, stream: int):
    """(h, w, y0, x0, flip) int64 tensors for batch positions ``pos``."""
    T = boxes.shape[0]
    hw = boxes.to(torch.int64)[uniform_below(image_hash(seed, stream, pos, 3), T)].clamp(2, S)
    h, w = hw[:, 0], hw[:, 1]
    return (h, w, (image_hash(seed, stream, pos, 0) * (S - h + 1)) >> 32,
            (image_hash(seed, stream, pos, 1) * (S - w + 1)) >> 32,
            image_hash(seed, stream, pos, 2) >> 31)


def image_batch_resized(images, labels, perm, cursor, table, out, labels_out, rows_out, crop_out,
                        boxes, box_out, crop_h, crop_w, train, seed, stream, layout, advance):
    """CPU twin of ``arena_image_batch_resized`` (same arguments as the extension's
    ``image_batch_resized``)."""
    _image_batch_resized(images, labels, perm, cursor, table, out, labels_out, rows_out, crop_out,
                         boxes, box_out, crop_h, crop_w, train, seed, stream, layout, advance,
                         None)


def _image_batch_resized(images, labels, perm, cursor, table, out, labels_out, rows_out, crop_out,
                         boxes, box_out, crop_h, crop_w, train, seed, stream, layout, advance,
                         color):
    """``color``: None, or the function of (u [B, Hc, Wc, 3] int64, zero in padding rows; pos) that
    distorts the resampled bytes (``image_batch_color``, below)."""
    n, S = images.shape[0], images.shape[1]
    B, L, Hc, Wc = out.shape[0], perm.numel(), int(crop_h), int(crop_w)
    if not train:
        raise ValueError("image_batch_resized: training only")
    if Hc % 2 or Wc % 2 or not (2 <= Hc <= S and 2 <= Wc <= S):
        raise ValueError("image_batch_resized: the crop must be even and at most the stored size")
    if table.dtype != out.dtype or tuple(table.shape) != (3, 256):
        raise ValueError("image_batch_resized: table must be [3, 256] in out's dtype")
    if boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 2 \
            or not 1 <= boxes.shape[0] <= MAX_CROP_BOXES:
        raise ValueError(f"image_batch_resized: boxes must be int32 [T, 2], 1 <= T <= "
                         f"{MAX_CROP_BOXES}")
    if box_out.dtype != torch.int32 or box_out.numel() != 2 * B:
        raise ValueError("image_batch_resized: box_out must be int32 [B, 2]")
    pos = _cursor_val(cursor, 0) * B + torch.arange(B, dtype=torch.int64)
    row = perm.to(torch.int64)[pos % L]
    valid = (row >= 0) & (row < n)
    row = torch.where(valid, row, torch.full_like(row, -1))
    h, w, y0, x0, flip = image_box_draws(pos, S, boxes, int(seed) & _M32, int(stream))
    i0, i1, fy = resize_taps(Hc, h)                                         # [B, Hc]
    xo = torch.arange(Wc, dtype=torch.int64).view(1, Wc)
    xs = torch.where(flip.view(B, 1) != 0, Wc - 1 - xo, xo)
    j0, j1, fx = (t.gather(1, xs) for t in resize_taps(Wc, w))              # [B, Wc]
    img = images[row.clamp(min=0)]                                          # [B, S, S, 3]
    bi = torch.arange(B).view(B, 1, 1)

    def tap(i, j):
        return img[bi, (y0.view(B, 1) + i).view(B, Hc, 1),
                   (x0.view(B, 1) + j).view(B, 1, Wc)].to(torch.int64)      # [B, Hc, Wc, 3]

    fy, fx = fy.view(B, Hc, 1, 1), fx.view(B, 1, Wc, 1)
    u = ((256 - fx) * (256 - fy) * tap(i0, j0) + fx * (256 - fy) * tap(i0, j1)
         + (256 - fx) * fy * tap(i1, j0) + fx * fy * tap(i1, j1) + 32768) >> 16
    if color is not None:
        u = color(torch.where(valid.view(B, 1, 1, 1), u, torch.zeros_like(u)), pos)
    val = table[torch.arange(3).view(1, 1, 1, 3), u]
    val = torch.where(valid.view(B, 1, 1, 1), val, torch.zeros_like(val))
    _image_store(out, val, layout)
    labels_out.copy_(torch.where(valid, labels.to(torch.int64)[row.clamp(min=0)],
                                 torch.full_like(row, IMAGE_PAD_LABEL)))
    rows_out.copy_(row)
    crop_out.view(B, 3).copy_(torch.stack([y0, x0, flip], dim=1))
    box_out.view(B, 2).copy_(torch.stack([h, w], dim=1))
    if advance:
        cursor.add_(1)


# ------------------------------------------------------------------------------------------------
# Colour distortion (image_batch_color_kernel): tf_cnn_benchmarks' distort_color in its YIQ form,
# between the resampled byte ``u`` above and the table lookup. In [0, 1] it is brightness (add d),
# saturation s and hue rotation t as one linear map ``M = Y^-1 diag(1, s R(t)) Y`` (Y: RGB -> YIQ),
# contrast ``(x - mu) k + mu`` about the per-channel mean mu of the image, and a clip to [0, 1].
# The I and Q rows of Y sum to 0, so ``M (1, 1, 1) = (1, 1, 1)`` and either order of contrast
# against saturation / hue (tf alternates them with the batch position's parity) is the same map,
# ``clip(k M x + (1 - k) M mu + d)``. In bytes and integers, on top of the definitions above:
#
# * the candidates: ``color_matrix_table(saturation, hue)`` is int32 [T, 9]: ``round(M * 2^12)``,
#   row-major, over a 32 x 32 grid of (saturation, hue angle) steps, built on the host with cos /
#   sin. Saturation (1, 1) with hue 0 is exactly ``4096 I``.
# * the draws: ``color_hash(seed, stream, pos, k) = image_hash(seed ^ COLOR_SEED_SALT, stream,
#   pos, k)``. ``stream * 4 + k`` of draws 0..3 already fills the 32-bit word, so the colour draws
#   get a domain of their own through the seed, and draws 0..3 stay what they were. ``m =
#   uniform_below(c0, T)``, ``k_q = k_lo + uniform_below(c1, k_hi - k_lo + 1)`` (contrast in
#   1/256ths), ``d_q = uniform_below(c2, 2 D + 1) - D`` (brightness in bytes, ``D = round(255
#   max_delta)``); ``color_out`` receives (m, k_q, d_q).
# * per image: ``s_c`` = the sum of u over the ``N = Hc Wc`` resampled, flipped crop pixels (exact
#   integers: any order of summation gives the same bits), ``A = k_q M_q`` (Q20) and ``b_c = d_q
#   2^20 + floor((256 - k_q) (sum_c' M_q[c][c'] s_c') / N)``, the product in 64 bits (N <= 2^28 for
#   S <= 16384 and |256 - k_q| r 255 < 2^31 under the bound below: less than 2^59).
# * per pixel: ``v_c = clamp((sum_c' A[c][c'] u_c' + b_c + 2^19) >> 20, 0, 255)``, then
#   ``table[c][v_c]``. A padding row stays a zero image.
# * rounding: both the division in b_c and the shift in v_c round towards minus infinity (Python's
#   ``//`` and ``>>``). In C++ ``>>`` of a negative int does so too, ``/`` truncates: the kernel
#   corrects its quotient when the remainder is negative.
# * widths: with r the largest sum over a row of |M_q|, |sum A u| <= k_hi r 255 and |b_c| <= D 2^20
#   + max|256 - k_q| r 255 + 1. Their sum is ``M_q w + d_q 2^20`` (less the floor's fraction) with
#   ``w = k_q u + (256 - k_q) s / N``, and every channel of w lies in [0, 256 * 255] for k_q <= 256
#   and in [-(k_q - 256) 255, k_q 255] above, so it is at most ``r 255 max(256, k_hi) + D 2^20 +
#   1`` in size. ``color_coefficient_bound`` is the larger of the bound on b_c and of that one plus
#   2^19; the loader refuses ranges for which it passes 2^31 - 1, so a pixel is 32-bit work. tf's
#   ranges give r = 13319 (3.25) and 1.34e9.
# ------------------------------------------------------------------------------------------------
COLOR_BRIGHTNESS = 32.0 / 255.0     # tf_cnn_benchmarks' max_delta
COLOR_SATURATION = (0.5, 1.5)
COLOR_HUE = 0.2 * math.pi           # the largest |angle| of the rotation in the IQ plane
COLOR_CONTRAST = (0.5, 1.5)
COLOR_MATRIX_GRID = (32, 32)        # saturation steps x hue steps
MAX_COLOR_MATRICES = 4096           # the launcher's bound on the table length
MAX_COLOR_CONTRAST_Q = 4096         # ... and on k_q (16.0)
COLOR_SEED_SALT = 0x636F6C72
RGB_TO_YIQ = ((0.299, 0.587, 0.114), (0.5959, -0.2746, -0.3213), (0.2115, -0.5227, 0.3112))


def color_matrix_table(saturation=COLOR_SATURATION, hue=COLOR_HUE) -> torch.Tensor:
    """int32 [T, 9] candidate matrices ``round(M * 4096)``, row-major in (saturation, hue) step;
    ``hue`` is the largest |angle| in radians."""
    slo, shi = (float(v) for v in saturation)
    hue = float(hue)
    if not (0.0 <= slo <= shi < math.inf):
        raise ValueError(f"color_matrix_table: saturation range {saturation} must satisfy "
                         f"0 <= lo <= hi < inf")
    if not (0.0 <= hue <= math.pi):
        raise ValueError(f"color_matrix_table: hue {hue} must lie in [0, pi]")
    Y = torch.tensor(RGB_TO_YIQ, dtype=torch.float64)
    Yi = torch.linalg.inv(Y)
    ns, nh = COLOR_MATRIX_GRID
    rows = []
    for i in range(ns):
        s = slo + (shi - slo) * (i + 0.5) / ns
        for j in range(nh):
            t = -hue + 2.0 * hue * (j + 0.5) / nh
            c, d = s * math.cos(t), s * math.sin(t)
            R = torch.tensor([[1.0, 0.0, 0.0], [0.0, c, -d], [0.0, d, c]], dtype=torch.float64)
            rows.append(torch.floor((Yi @ R @ Y) * 4096.0 + 0.5).reshape(9))
    return torch.stack(rows).to(torch.int32)


def color_quantised_ranges(brightness=COLOR_BRIGHTNESS, contrast=COLOR_CONTRAST):
    """(k_lo, k_hi, D): contrast in 1/256ths and the largest |brightness| in bytes."""
    clo, chi = (float(v) for v in contrast)
    brightness = float(brightness)
    if not (0.0 <= clo <= chi) or math.floor(chi * 256.0 + 0.5) > MAX_COLOR_CONTRAST_Q:
        raise ValueError(f"color: contrast range {contrast} must satisfy 0 <= lo <= hi <= "
                         f"{MAX_COLOR_CONTRAST_Q // 256}")
    if not (0.0 <= brightness <= 1.0):
        raise ValueError(f"color: brightness {brightness} must lie in [0, 1]")
    return (math.floor(clo * 256.0 + 0.5), math.floor(chi * 256.0 + 0.5),
            math.floor(brightness * 255.0 + 0.5))


def color_coefficient_bound(matrices: torch.Tensor, k_lo: int, k_hi: int, delta: int) -> int:
    """The largest |sum A u + b + 2^19| a pixel can reach (see the contract above)."""
    r = int(matrices.to(torch.int64).abs().view(-1, 3, 3).sum(2).max())
    b = (delta << 20) + max(abs(256 - k_lo), abs(256 - k_hi)) * r * 255 + 1
    return max(b, r * 255 * max(256, k_hi) + (delta << 20) + 1 + (1 << 19))


def color_hash(seed: int, stream: int, pos: torch.Tensor, k: int) -> torch.Tensor:
    return image_hash((seed ^ COLOR_SEED_SALT) & _M32, stream, pos, k)


def image_color_draws(pos: torch.Tensor, T: int, k_lo: int, k_hi: int, delta: int, seed: int,
                      stream: int):
    """(m, k_q, d_q) int64 tensors for batch positions ``pos``."""
    return (uniform_below(color_hash(seed, stream, pos, 0), T),
            k_lo + uniform_below(color_hash(seed, stream, pos, 1), k_hi - k_lo + 1),
            uniform_below(color_hash(seed, stream, pos, 2), 2 * delta + 1) - delta)


IMAGE_BLOCK_QUADS = 256             # 2 x 2 pixel quads per block of the batch kernels


def image_sum_blocks(crop_h: int, crop_w: int) -> int:
    """Blocks per image: the length of an image's row of partial channel sums."""
    return -(-((crop_h // 2) * (crop_w // 2)) // IMAGE_BLOCK_QUADS)


def image_batch_color(images, labels, perm, cursor, table, out, labels_out, rows_out, crop_out,
                      boxes, box_out, matrices, sums, color_out, crop_h, crop_w, train, seed,
                      stream, k_lo, k_hi, delta, layout, advance):
    """CPU twin of ``arena_image_batch_color`` (same arguments as the extension's
    ``image_batch_color``): ``image_batch_resized`` with the colour distortion above. ``matrices``
    int32 [T, 9]; ``sums`` int32 [B, image_sum_blocks, 3] receives the channel sums of each block's
    quads (quad q = i * (Wc / 2) + j belongs to block q // 256), ``color_out`` int32 [B, 3] the
    draws."""
    B, Hc, Wc = out.shape[0], int(crop_h), int(crop_w)
    k_lo, k_hi, delta = int(k_lo), int(k_hi), int(delta)
    T, nblk = matrices.shape[0], image_sum_blocks(Hc, Wc)
    if matrices.dtype != torch.int32 or matrices.dim() != 2 or matrices.shape[1] != 9 \
            or not 1 <= T <= MAX_COLOR_MATRICES:
        raise ValueError(f"image_batch_color: matrices must be int32 [T, 9], 1 <= T <= "
                         f"{MAX_COLOR_MATRICES}")
    if not (0 <= k_lo <= k_hi <= MAX_COLOR_CONTRAST_Q and 0 <= delta <= 255):
        raise ValueError("image_batch_color: contrast or brightness out of range")
    if sums.dtype != torch.int32 or sums.numel() != B * nblk * 3:
        raise ValueError("image_batch_color: sums must be int32 [B, blocks per image, 3]")
    if color_out.dtype != torch.int32 or color_out.numel() != 3 * B:
        raise ValueError("image_batch_color: color_out must be int32 [B, 3]")

    def color(u, pos):
        m, kq, dq = image_color_draws(pos, T, k_lo, k_hi, delta, int(seed) & _M32, int(stream))
        color_out.view(B, 3).copy_(torch.stack([m, kq, dq], dim=1))
        quads = u.view(B, Hc // 2, 2, Wc // 2, 2, 3).sum((2, 4)).view(B, -1, 3)
        part = torch.zeros(B, nblk * IMAGE_BLOCK_QUADS, 3, dtype=torch.int64)
        part[:, :quads.shape[1]] = quads
        part = part.view(B, nblk, IMAGE_BLOCK_QUADS, 3).sum(2)
        sums.view(B, nblk, 3).copy_(part)
        s = part.sum(1)                                                     # [B, 3]
        Mq = matrices.to(torch.int64)[m].view(B, 3, 3)
        A = kq.view(B, 1, 1) * Mq
        b = (dq << 20).view(B, 1) + torch.div(
            (256 - kq).view(B, 1) * (Mq * s.view(B, 1, 3)).sum(2), Hc * Wc, rounding_mode="floor")
        acc = (A.view(B, 1, 1, 3, 3) * u.view(B, Hc, Wc, 1, 3)).sum(4) + b.view(B, 1, 1, 3)
        return ((acc + (1 << 19)) >> 20).clamp(0, 255)

    _image_batch_resized(images, labels, perm, cursor, table, out, labels_out, rows_out, crop_out,
                         boxes, box_out, crop_h, crop_w, train, seed, stream, layout, advance,
                         color)
