"""The shard kernels of the optimizer family on the GPU: ``shard_update`` (RMSProp, Adam in three
layouts, SGD in the wide one) and the two halves of sharded LARS against the CPU reference, the
bindings' refusals, and ``ShardedMasterSGD(rule=...)`` on two ranks time-sharing GPU 0."""
from __future__ import annotations

import hashlib
import os
import queue
import socket
import traceback

import pytest
import torch
import torch.multiprocessing as mp

from arena_amd.ops import fused, reference, schedule
from arena_amd.ops.optim import AdamClock
from arena_amd.ops.schedule import DeviceLR, reference_lr

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _bits64(t):
    return t.contiguous().view(torch.int64)


BF16, F32 = torch.bfloat16, torch.float32
TOL = dict(rtol=1e-5, atol=1e-6)          # tests/test_optim_family_gpu.py's
SENTINEL = 96.0                           # exact in bf16 too
SIZES = [4, 1024, 1028, 4096 * 1024 + 1024]   # the last: the grid-stride loop past the block cap
LAYOUTS = ["master", "f32", "wide"]       # bf16 grad + wbf; fp32 grad, no wbf; fp32 grad + wbf
LR, WD, SCALE = 0.01, 4e-5, 0.5


# --------------------------------------------------------------------------------- shard_update
def _run_shard(rule, layout, n, dev, lr_form):
    """Three steps over a range of n elements; every buffer carries 8 sentinels behind it."""
    g = torch.Generator().manual_seed(7 + n % 1000)
    pad = n + 8

    def buf(t, dtype=F32):
        out = torch.full((pad,), SENTINEL, dtype=dtype)
        out[:n] = t.to(dtype)
        return out.to(dev)

    w = buf(torch.randn(n, generator=g) * 0.1)
    st0 = buf(torch.ones(n) if rule == "rmsprop" else torch.zeros(n))
    st1 = buf(torch.zeros(n))
    wbf = None if layout == "f32" else buf(torch.zeros(n), BF16)
    gdt = BF16 if layout == "master" else F32
    clock = AdamClock((0.9, 0.999), dev)
    lr_t = torch.tensor([LR], dtype=F32, device=dev)
    kw = {"lr": LR} if lr_form == "float" else {"lr": 123.0, "lr_t": lr_t}
    for _ in range(3):
        grad = buf(torch.randn(n, generator=g) * 0.1, gdt)
        wb = None if wbf is None else wbf[:n]
        if rule == "rmsprop":
            fused.shard_rmsprop(grad[:n], w[:n], st0[:n], st1[:n], wb, decay=0.9, momentum=0.9,
                                eps=1.0, weight_decay=WD, scale=SCALE, **kw)
        elif rule == "adam":
            clock.tick()
            fused.shard_adam(grad[:n], w[:n], st0[:n], st1[:n], clock.corr, wb,
                             betas=(0.9, 0.999), eps=1e-8, weight_decay=WD, scale=SCALE, **kw)
        else:
            fused.shard_sgd(grad[:n], w[:n], st0[:n], wb, momentum=0.9, weight_decay=WD,
                            scale=SCALE, **kw)
        assert grad[n:].tolist() == [SENTINEL] * 8
    out = [w.cpu(), st0.cpu(), st1.cpu()]
    if wbf is not None:
        out.append(wbf.cpu())
    return out


_REF = {}


def _ref(rule, layout, n):
    """The CPU reference of a case, computed once and shared by both lr forms."""
    key = (rule, layout, n)
    if key not in _REF:
        _REF[key] = _run_shard(rule, layout, n, torch.device("cpu"), "float")
    return _REF[key]


def _check(got, want, n):
    for a, b in zip(got, want):
        assert a[n:].tolist() == [SENTINEL] * 8                   # nothing written past the range
        assert bool(torch.isfinite(b[:n].float()).all())
        if a.dtype != BF16:
            torch.testing.assert_close(a[:n], b[:n], **TOL)
    if len(got) == 4:
        # wbf = bf16(master) bit for bit (a master within TOL of the reference may round to the
        # neighbouring bf16, so wbf is held to its own master, not to the reference's)
        assert torch.equal(got[3][:n], got[0][:n].to(BF16))
        assert torch.equal(want[3][:n], want[0][:n].to(BF16))


@pytest.mark.parametrize("lr_form", ["float", "lr_t"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rule", ["rmsprop", "adam"])
def test_shard_update_matches_cpu_reference(cuda, rule, layout, n, lr_form):
    want = _ref(rule, layout, n)
    assert not torch.equal(want[1][:n], torch.ones(n) if rule == "rmsprop" else torch.zeros(n))
    _check(_run_shard(rule, layout, n, cuda, lr_form), want, n)


@pytest.mark.parametrize("lr_form", ["float", "lr_t"])
@pytest.mark.parametrize("n", SIZES)
def test_wide_shard_sgd_matches_cpu_reference(cuda, n, lr_form):
    """fp32 gradient, fp32 master, bf16 weight out: what ``rccl_reduce_fp32`` hands the update of
    bf16 weights. The binding of ``shard_sgd`` refuses it; the wrapper takes the wide kernel."""
    _check(_run_shard("sgd", "wide", n, cuda, lr_form), _ref("sgd", "wide", n), n)


# ----------------------------------------------------------------------------------------- LARS
BIG = 40 * 1024
ZERO_G, ZERO_W = 6, 7                     # small tensors with a zero gradient / zero weights
EETA, EPS_L = 0.001, 1e-9


def _lars_layout():
    """A sub-range of 54 tensors in 8-element slots: a 40-block + 4 tensor, 50 small ones (4 to
    1028 elements), a 40-block tensor, and two tensors that lie wholly on another rank. The shard
    begins inside the first and ends inside the 40-block one: 52 pieces, two launch groups."""
    ns = [BIG + 4] + [4 * (1 + i % 5) for i in range(48)] + [1028, 1024] + [BIG, 64, 8]
    offs, total = [], 0
    for k in ns:
        offs.append(total)
        total += (k + 7) // 8 * 8
    lo, hi = 10 * 1024 + 8, offs[51] + 17 * 1024 + 8
    goffs, moffs, pn, slots = [], [], [], []
    for s, (o, k) in enumerate(zip(offs, ns)):
        a, b = max(o, lo), min(o + k, hi)
        if a < b:
            goffs.append(a - lo)
            moffs.append(a)
            pn.append(b - a)
            slots.append(s)
    assert len(pn) == 52 and 45000 < hi - lo < 55000 and pn[0] < ns[0] and pn[-1] < ns[51]
    return ns, offs, total, lo, hi, (goffs, moffs, pn, slots)


def _lars_data(wide):
    ns, offs, total, lo, hi, pieces = _lars_layout()
    g = torch.Generator().manual_seed(23)
    master = torch.randn(total + 8, generator=g) * 0.1
    mom = torch.rand(total + 8, generator=g) * 0.01
    for t in (master, mom):
        t[offs[1 + ZERO_W]:offs[1 + ZERO_W] + ns[1 + ZERO_W]] = 0.0
        t[total:] = SENTINEL
    grads = []
    for _ in range(3):
        gr = torch.full((hi - lo + 8,), SENTINEL)
        gr[:hi - lo] = torch.randn(hi - lo, generator=g) * 0.1
        o = offs[1 + ZERO_G] - lo
        gr[o:o + ns[1 + ZERO_G]] = 0.0
        grads.append(gr.to(F32 if wide else BF16))
    # what the other ranks' pieces add to the all-reduced sums: the rest of the two cut tensors,
    # and the two tensors this rank holds nothing of (the last one: zero weights elsewhere too)
    other = torch.zeros(2 * len(ns), dtype=torch.float64)
    other[0:2] = torch.tensor([101.25, 1.5])
    other[2 * 51:2 * 51 + 2] = torch.tensor([230.5, 2.25])
    other[2 * 52:2 * 52 + 2] = torch.tensor([0.75, 0.125])
    return master, mom, grads, other


def _run_lars(dev, wide, sums_from=None):
    """Three steps. Returns the sums this rank formed at every step, and master, mom, wbf and trust
    after the last. ``sums_from``: per step, the sums the update takes instead (the reference's)."""
    ns, offs, total, lo, hi, (goffs, moffs, pn, slots) = _lars_layout()
    master, mom, grads, other = _lars_data(wide)
    master, mom = master.to(dev), mom.to(dev)
    wbf = torch.full((total + 8,), SENTINEL, dtype=BF16, device=dev)
    sums = torch.full((2 * len(ns) + 2,), SENTINEL, dtype=torch.float64, device=dev)
    trust = torch.full((len(ns) + 2,), SENTINEL, dtype=F32, device=dev)
    work = torch.full((fused.mt_lars_workspace_floats(pn) + 4,), SENTINEL, dtype=F32, device=dev)
    seen, trusts = [], []
    for t, gr in enumerate(grads):
        gr = gr.to(dev)
        fused.shard_lars_norms(gr[:hi - lo], master[:total], goffs, moffs, pn, slots,
                               sums[:-2], work[:-4], scale=SCALE)
        seen.append(sums.cpu().clone())
        red = (seen[-1] if sums_from is None else sums_from[t]).clone()
        red[:-2] += other                                  # the "all-reduce"
        fused.shard_lars_update(gr[:hi - lo], master[:total], mom[:total], wbf[:total], goffs,
                                moffs, pn, slots, red[:-2].to(dev), trust[:-2], lr=0.5,
                                momentum=0.9, weight_decay=WD, eeta=EETA, eps=EPS_L, scale=SCALE)
        trusts.append(trust.cpu().clone())
    assert work[-4:].tolist() == [SENTINEL] * 4
    return seen, master.cpu(), mom.cpu(), wbf.cpu(), torch.stack(trusts)


_LARS_REF = {}


def _lars_ref(wide):
    if wide not in _LARS_REF:
        _LARS_REF[wide] = _run_lars(torch.device("cpu"), wide)
    return _LARS_REF[wide]


@pytest.mark.parametrize("wide", [False, True])
def test_shard_lars_matches_cpu_reference(cuda, wide):
    """The sums at rtol 1e-5, as tests/test_lars_gpu.py derives it: a piece has at most 41 K
    non-negative fp32 terms, each the square of a value with at most one rounding more than there
    (d = g * scale), summed as 16 serial per lane + a 64-lane tree per chunk (25 fp32 roundings on
    any term's path), then at most 41 partials in fp64: within 50 * 2^-24 = 3e-6 of the fp64 sum.
    The update takes the REFERENCE's sums, so its tolerance is the element-wise one."""
    ns, offs, total, lo, hi, (goffs, moffs, pn, slots) = _lars_layout()
    rsums, rw, rm, rwbf, rtrust = _lars_ref(wide)
    sums, w, m, wbf, trust = _run_lars(cuda, wide, sums_from=rsums)
    for a, b in zip(sums, rsums):
        assert a[-2:].tolist() == [SENTINEL] * 2
        assert a[2 * 52:2 * 54].tolist() == [0.0] * 4               # no piece here: written, 0.0
        assert a[2 * (1 + ZERO_G) + 1].item() == 0.0 and b[2 * (1 + ZERO_G) + 1].item() == 0.0
        torch.testing.assert_close(a[:-2], b[:-2], rtol=1e-5, atol=0.0)
    assert trust[:, -2:].tolist() == [[SENTINEL] * 2] * 3
    torch.testing.assert_close(trust[:, :-2], rtrust[:, :-2], **TOL)
    for t in (trust, rtrust):
        assert t[:, 1 + ZERO_G].tolist() == [1.0] * 3       # all-zero gradient: every step
        assert t[0, 1 + ZERO_W].item() == 1.0               # all-zero weights: the first step
        assert t[:, 53].tolist() == [1.0] * 3               # no piece anywhere: both sums 0.0
        assert bool((t[:, 52] != 1.0).all())                # wholly on another rank: still written
        assert int((t[:, :-2] == 1.0).sum()) == 7           # the zero cases and nothing else
    init = _lars_data(wide)[0]
    assert not torch.equal(rw[lo:hi], init[lo:hi])
    for a, b in ((w, rw), (m, rm)):
        torch.testing.assert_close(a, b, **TOL)
        assert a[total:].tolist() == [SENTINEL] * 8
    assert torch.equal(w[:lo], init[:lo]) and torch.equal(w[hi:], init[hi:])   # the shard only
    inside = torch.zeros(total + 8, dtype=torch.bool)
    for o, k in zip(moffs, pn):
        inside[o:o + k] = True
    assert torch.equal(wbf[inside], w[inside].to(BF16))
    assert bool((wbf[~inside] == SENTINEL).all())


def test_shard_lars_is_deterministic_and_takes_an_empty_shard(cuda):
    a = _run_lars(cuda, False)
    b = _run_lars(cuda, False)
    for x, y in zip(a[0], b[0]):
        assert torch.equal(_bits64(x), _bits64(y))
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(_bits(x), _bits(y))
    # a shard of padding only: no piece, every sum 0.0, every trust from the given sums
    sums = torch.full((6,), SENTINEL, dtype=torch.float64, device=cuda)
    trust = torch.full((3,), SENTINEL, dtype=F32, device=cuda)
    master = torch.full((16,), SENTINEL, dtype=F32, device=cuda)
    wbf = torch.full((16,), SENTINEL, dtype=BF16, device=cuda)
    grad = torch.zeros(8, dtype=BF16, device=cuda)
    work = torch.empty(4, dtype=F32, device=cuda)
    fused.shard_lars_norms(grad, master, [], [], [], [], sums, work, scale=SCALE)
    assert sums.tolist() == [0.0] * 6
    red = torch.tensor([4.0, 1.0, 0.0, 1.0, 9.0, 0.0], dtype=torch.float64, device=cuda)
    fused.shard_lars_update(grad, master, master.clone(), wbf, [], [], [], [], red, trust, lr=0.5,
                            momentum=0.9, weight_decay=0.0, eeta=0.25, eps=0.0, scale=SCALE)
    assert trust.tolist() == [0.5, 1.0, 1.0]         # 0.25 * 2 / 1; a zero norm; a zero norm
    assert master.tolist() == [SENTINEL] * 16 and wbf.float().tolist() == [SENTINEL] * 16


# ----------------------------------------------------------------------------- binding refusals
def test_bindings_refuse_bad_arguments(cuda):
    from arena_amd.ops import _ext
    ext = _ext.load()
    n = 16
    w, ms, mom, g = (torch.zeros(n + 4, device=cuda) for _ in range(4))
    wbf = torch.zeros(n + 4, dtype=BF16, device=cuda)
    corr = torch.ones(1, device=cuda)
    with pytest.raises(RuntimeError, match="misaligned"):
        fused.shard_rmsprop(g[:n], w[1:n + 1], ms[:n], mom[:n], lr=LR)
    with pytest.raises(RuntimeError, match="misaligned"):
        fused.shard_adam(g[2:n + 2], w[:n], ms[:n], mom[:n], corr, lr=LR)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        fused.shard_rmsprop(g[:6], w[:6], ms[:6], mom[:6], lr=LR)
    hyper = dict(lr=LR, a=0.9, oma=0.1, b=0.9, omb=0.001, eps=1.0, weight_decay=0.0, scale=1.0)
    with pytest.raises(RuntimeError, match="second state"):
        ext.shard_update(rule=reference.OPT_RMSPROP, grad=g[:n], w32=w[:n], st0=ms[:n], **hyper)
    with pytest.raises(RuntimeError, match="corr"):
        ext.shard_update(rule=reference.OPT_ADAM, grad=g[:n], w32=w[:n], st0=ms[:n],
                         st1=mom[:n], **hyper)
    with pytest.raises(RuntimeError, match="wide layout only"):
        ext.shard_update(rule=reference.OPT_SGD, grad=g[:n], w32=w[:n], st0=ms[:n], **hyper)
    with pytest.raises(RuntimeError, match="need the bf16 weight range"):
        fused.shard_rmsprop(g[:n].to(BF16), w[:n], ms[:n], mom[:n], lr=LR)
    with pytest.raises(ValueError, match="corr must be"):
        fused.shard_adam(g[:n], w[:n], ms[:n], mom[:n], corr.cpu(), lr=LR)
    with pytest.raises(ValueError, match="lr_t must be"):
        fused.shard_rmsprop(g[:n], w[:n], ms[:n], mom[:n], lr=LR, lr_t=corr.double())
    sums = torch.zeros(4, dtype=torch.float64, device=cuda)
    trust = torch.zeros(2, device=cuda)
    work = torch.zeros(8, device=cuda)
    gb = g.to(BF16)
    lars = dict(lr=0.5, momentum=0.9, weight_decay=0.0, eps=0.0, scale=1.0)
    with pytest.raises(RuntimeError, match="out of range"):
        fused.shard_lars_norms(gb[:n], w[:n], [0], [0], [8], [2], sums, work, scale=1.0)
    with pytest.raises(RuntimeError, match="out of range"):
        fused.shard_lars_update(gb[:n], w[:n], mom[:n], wbf[:n], [0], [0], [8], [-1], sums, trust,
                                eeta=0.001, **lars)
    with pytest.raises(RuntimeError, match="two pieces"):
        fused.shard_lars_norms(gb[:n], w[:n], [0, 8], [0, 8], [8, 8], [1, 1], sums, work,
                               scale=1.0)
    with pytest.raises(RuntimeError, match="misaligned or out of bounds"):
        fused.shard_lars_norms(gb[:n], w[:n], [0], [2], [8], [0], sums, work, scale=1.0)
    with pytest.raises(RuntimeError, match="misaligned or out of bounds"):
        fused.shard_lars_norms(gb[:n], w[:n], [12], [0], [8], [0], sums, work, scale=1.0)
    with pytest.raises(RuntimeError, match="workspace holds"):
        fused.shard_lars_norms(gb[:n], w[:n], [0], [0], [8], [0], sums, work[:0], scale=1.0)
    with pytest.raises(RuntimeError, match="eeta must be > 0"):
        fused.shard_lars_update(gb[:n], w[:n], mom[:n], wbf[:n], [0], [0], [8], [0], sums, trust,
                                eeta=0.0, **lars)
    torch.cuda.synchronize()
    assert float(w.abs().sum()) == 0.0 and float(trust.abs().sum()) == 0.0   # nothing ran


# -------------------------------------------------------------------------------- data parallel
# the spawn pattern, schedule and shapes of tests/test_lr_schedule_gpu.py
def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(fn, world, *args, timeout=150):
    """Run ``fn(rank, world, port, q, *args)`` in ``world`` spawned processes and collect one
    result per rank; the first failure (or a rank that does not answer in time) takes the whole
    gang down."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=fn, args=(r, world, port, q) + args) for r in range(world)]
    for p in procs:
        p.start()
    out, err = {}, None
    try:
        for _ in range(world):
            try:
                r, res, e = q.get(timeout=timeout)
            except queue.Empty:
                err = f"no answer from a rank within {timeout} s (got {sorted(out)})"
                break
            if e is not None:
                err = f"rank {r} failed:\n{e}"
                break
            out[r] = res
    finally:
        for p in procs:
            if err is not None and p.is_alive():
                p.terminate()
        for p in procs:
            p.join(20)
            if p.is_alive():
                p.kill()
                p.join(10)
    assert err is None, err
    return out


DP_SEGS = schedule.with_warmup(schedule.piecewise("0.3;4;0.03", 1), 2, 1)
DP_SHAPES = [((16, 8, 3, 3), "bf16"), ((16,), "fp32"), ((32, 16), "bf16"), ((7,), "fp32"),
             ((64, 32, 1, 1), "bf16"), ((33,), "fp32")]


def _dp_worker(rank, world, port, q, rule):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world), LOCAL_RANK="0", LOCAL_WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        import torch.distributed as dist
        dist.init_process_group("gloo")      # two ranks share GPU 0: RCCL takes one rank per GPU
        from arena_amd.parallel.zero import ShardedMasterSGD
        dev = torch.device("cuda", 0)

        def run(reduce_fp32, scheduled):
            g = torch.Generator().manual_seed(42)
            params = []
            for shp, kind in DP_SHAPES:
                t = torch.randn(shp, generator=g)
                if len(shp) == 4:
                    t = t.contiguous(memory_format=torch.channels_last)
                params.append((torch.nn.Parameter(t.to(dev)), kind))
            start = [p.detach().float().cpu().clone() for p, _ in params]
            sched = DeviceLR(DP_SEGS, dev) if scheduled else None
            opt = ShardedMasterSGD(
                [{"params": [p for p, k in params if k == "bf16"], "weight_decay": 1e-3},
                 {"params": [p for p, k in params if k == "fp32"], "weight_decay": 0.0,
                  "weights": "fp32"}],
                lr=sched if scheduled else 1.0, momentum=0.9, bucket_mb=0.004,
                last_bucket_mb=0.001, backend="rccl", order=[p for p, _ in params],
                timeout_s=30.0, rccl_reduce_fp32=reduce_fp32, rule=rule)
            for t in range(4):
                if scheduled:
                    sched.advance()          # main stream, head of the step
                else:
                    for grp in opt.param_groups:
                        grp["lr"] = float(reference_lr(DP_SEGS, t))
                gg = torch.Generator().manual_seed(1000 * t + rank)
                for p, _ in params:
                    gr = (torch.randn(p.shape, generator=gg) * 0.1).to(p.dtype)
                    if p.dim() == 4:
                        gr = gr.contiguous(memory_format=torch.channels_last)
                    p.grad = gr.to(dev)
                opt.step()
                opt.zero_grad()
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for p, _ in params:
                h.update(_bits(p).numpy().tobytes())
            weights = h.hexdigest()
            sd = opt.state_dict()            # collective: the shards of every rank, assembled
            for key in ("master", "momentum_buffer", "mean_square", "exp_avg_sq"):
                for t_ in sd.get(key, []):
                    h.update(_bits(t_).numpy().tobytes())
            if rule == "lars":
                h.update(_bits(opt.trust).numpy().tobytes())
            res = {"weights": weights, "state": h.hexdigest(), "backend": opt.backend,
                   "nbuckets": len(opt.buckets),
                   "mixed": sum(1 for b in opt.buckets if len(b.ranges) == 2),
                   "finite": all(bool(torch.isfinite(p).all()) for p, _ in params),
                   "moved": all(not torch.equal(p.detach().float().cpu(), s)
                                for (p, _), s in zip(params, start)),
                   "clock": opt.clock.steps() if rule == "adam" else None,
                   "trust": opt.trust.tolist() if rule == "lars" else None}
            opt.close()
            return res

        res = {(red, form): run(red, form == "sched")
               for red in (False, True) for form in ("float", "sched")}
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res, None))
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("rule", ["rmsprop", "adam", "lars", "sgd"])
def test_sharded_rules_on_two_ranks(rule):
    """W = 2 ranks time-sharing GPU 0 over gloo, 4 steps across the end of the warm-up, three
    buckets of which one is mixed, bf16 and fp32 reduce-scatter sums: both ranks end with
    bit-identical weights and states, bit-identical under a float lr and a DeviceLR. ``sgd`` with
    fp32 sums steps bf16 weights through the wide kernel (it used to raise on a GPU)."""
    out = _spawn(_dp_worker, 2, rule)
    for red in (False, True):
        for form in ("float", "sched"):
            a, b = out[0][(red, form)], out[1][(red, form)]
            assert a["backend"] == "rccl" and a["nbuckets"] > 1 and a["mixed"] >= 1, a
            assert a["finite"] and a["moved"] and b["finite"] and b["moved"], (a, b)
            assert a["weights"] == b["weights"] and a["state"] == b["state"], (red, form, a, b)
            if rule == "adam":
                assert a["clock"] == b["clock"] == 4, (a, b)        # one tick per step
            if rule == "lars":
                assert a["trust"] == b["trust"] and len(a["trust"]) == 3, (a, b)
                assert all(0.0 < t < 1.0 for t in a["trust"]), a
        for r in (0, 1):
            assert out[r][(red, "float")]["state"] == out[r][(red, "sched")]["state"], (red, out)


def test_xgmi_backend_refuses_the_other_rules(cuda):
    """Before any communicator (or process group) is touched."""
    from arena_amd.parallel.zero import ShardedMasterSGD
    p = torch.nn.Parameter(torch.randn(8, 8, device=cuda))
    with pytest.raises(ValueError, match="xgmi.*momentum SGD only"):
        ShardedMasterSGD([p], lr=0.1, backend="xgmi", rule="adam")
    assert p.dtype == F32                   # untouched
