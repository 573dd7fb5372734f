"""The device learning rate on the GPU: the ``arena_lr_schedule`` kernel bit for bit against
``reference_lr``, the ``lr_ptr`` form of every SGD update kernel bit for bit against its float
form, the new ``mt_sgd_f32`` kernel, a captured step whose learning rate moves from replay to
replay, two data-parallel ranks on the xGMI and the RCCL backend, and ``cnn_bench`` end to end."""
from __future__ import annotations

import hashlib
import json
import os
import queue
import re
import socket
import subprocess
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from arena_amd.ops import schedule
from arena_amd.ops.schedule import DeviceLR, reference_lr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def test_schedule_kernel_matches_reference_bit_for_bit(cuda):
    """40 launches over a 7-step warm-up (not a power of two) to 0.3, boundaries at 12 and 25, with
    values fp32 cannot hold exactly; the last 15 steps lie past the last boundary."""
    segs = schedule.with_warmup(schedule.piecewise("0.3;12;0.1;25;0.03", 1), 7, 1)
    assert [s[0] for s in segs] == [0, 7, 12, 25]
    s = DeviceLR(segs, cuda)
    seen = torch.zeros(40, dtype=torch.float32, device=cuda)
    for t in range(40):
        s.advance()
        seen[t:t + 1].copy_(s.lr)
    want = np.array([reference_lr(segs, t) for t in range(40)], dtype=np.float32)
    got = seen.cpu().numpy()
    assert got.view(np.int32).tolist() == want.view(np.int32).tolist(), (got, want)
    assert s.steps() == 40 and s.step.dtype == torch.int64
    assert len(set(got[:8].tolist())) == 8          # the ramp did ramp


def _master_set(cuda):
    """50 tensors of 8 elements (a second chunk of the 48-tensor launches), one just above a
    1024-element block and one below."""
    g = torch.Generator().manual_seed(11)
    ns = [8] * 50 + [1028, 32]
    offs = [sum(ns[:i]) for i in range(len(ns))]
    total = sum(ns)
    grads = [(torch.randn(n, generator=g) * 0.1).to(BF16).to(cuda) for n in ns]
    master = torch.randn(total, generator=g).to(cuda)
    mom = (torch.randn(total, generator=g) * 0.01).to(cuda)
    return grads, offs, master, mom, torch.zeros(total, dtype=BF16, device=cuda)


def test_mt_sgd_master_lr_t_equals_float_lr(cuda):
    from arena_amd.ops import fused
    x = 0.1
    grads, offs, m1, v1, w1 = _master_set(cuda)
    _, _, m2, v2, w2 = _master_set(cuda)
    before = m1.clone()
    for _ in range(2):
        fused.mt_sgd_master(grads, offs, m1, v1, w1, lr=x, momentum=0.9, weight_decay=4e-5)
        fused.mt_sgd_master(grads, offs, m2, v2, w2, lr=123.0, momentum=0.9, weight_decay=4e-5,
                            lr_t=torch.tensor([x], dtype=torch.float32, device=cuda))
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and torch.equal(w1, w2)
    assert not torch.equal(m1, before) and torch.equal(w1, m1.to(BF16))
    with pytest.raises((ValueError, RuntimeError), match="lr_t"):
        fused.mt_sgd_master(grads, offs, m1, v1, w1, lr=x, momentum=0.9, weight_decay=0.0,
                            lr_t=torch.tensor([x], dtype=torch.float32))        # on the host
    with pytest.raises((ValueError, RuntimeError), match="lr_t"):
        fused.mt_sgd_master(grads, offs, m1, v1, w1, lr=x, momentum=0.9, weight_decay=0.0,
                            lr_t=torch.zeros(2, device=cuda))


@pytest.mark.parametrize("dtype", [BF16, torch.float32])
def test_shard_sgd_lr_t_equals_float_lr(cuda, dtype):
    from arena_amd.ops import fused
    n, x = 4096 + 12, 0.3
    g = torch.Generator().manual_seed(5)
    grad = (torch.randn(n, generator=g) * 0.1).to(dtype).to(cuda)
    w = torch.randn(n, generator=g).to(cuda)
    m = (torch.randn(n, generator=g) * 0.01).to(cuda)
    w2, m2 = w.clone(), m.clone()
    wb = torch.zeros(n, dtype=BF16, device=cuda) if dtype == BF16 else None
    wb2 = wb.clone() if wb is not None else None
    kw = dict(momentum=0.9, weight_decay=1e-3, scale=1.0 / 3)
    fused.shard_sgd(grad, w, m, wb, lr=x, **kw)
    fused.shard_sgd(grad, w2, m2, wb2, lr=0.0, lr_t=torch.tensor([x], device=cuda), **kw)
    assert torch.equal(w, w2) and torch.equal(m, m2)
    assert wb is None or (torch.equal(wb, wb2) and torch.equal(wb, w.to(BF16)))


GUARD = 77.0


def _f32_set(dev):
    """50 tensors of 4 elements, then numel 1, 3, 10, 64, 1000, 1025, 2049, laid out in flat
    buffers with 5 guard values after each tensor: offsets 9 i for the small ones (one in four
    16-byte aligned), and every other gradient a view one element into its storage, so both the
    vector path and the element path run, whole blocks and tails."""
    g = torch.Generator().manual_seed(21)
    ns = [4] * 50 + [1, 3, 10, 64, 1000, 1025, 2049]
    offs, total = [], 0
    for n in ns:
        offs.append(total)
        total += n + 5
    w = torch.full((total,), GUARD)
    m = torch.full((total,), GUARD)
    live = torch.zeros(total, dtype=torch.bool)
    grads = []
    for i, (n, o) in enumerate(zip(ns, offs)):
        w[o:o + n] = torch.randn(n, generator=g)
        m[o:o + n] = torch.randn(n, generator=g) * 0.01
        live[o:o + n] = True
        store = (torch.randn(n + 1, generator=g) * 0.1).to(dev)
        grads.append(store[1:] if i % 2 else store[:n])
    return grads, offs, w.to(dev), m.to(dev), live


@pytest.mark.parametrize("hp", [(2.0 ** -4, 0.5, 2.0 ** -10, 0.25, True),
                                (0.05, 0.9, 1e-3, 1.0 / 3, False)])
def test_mt_sgd_f32_kernel_matches_reference(cuda, hp):
    """Bit-equal with exact hyperparameters (every product exact, each result rounds once whatever
    FMAs the compiler forms: the argument of test_shard_sgd_kernel_matches_reference), within
    4 * 2^-23 * max|w| with real ones; the guard values between the tensors stay."""
    from arena_amd.ops import fused
    lr, mu, wd, sc, exact = hp
    gr, offs, wr, mr, live = _f32_set("cpu")
    gg, offs_g, wg, mg, _ = _f32_set(cuda)
    assert offs == offs_g and all(torch.equal(a, b.cpu()) for a, b in zip(gr, gg))
    assert any(o % 4 == 0 for o in offs[:50]) and any(o % 4 for o in offs[:50])
    w0 = wr.clone()
    fused.mt_sgd_f32(gr, offs, wr, mr, lr=lr, momentum=mu, weight_decay=wd, scale=sc)
    fused.mt_sgd_f32(gg, offs, wg, mg, lr=lr, momentum=mu, weight_decay=wd, scale=sc)
    wg, mg = wg.cpu(), mg.cpu()
    assert not torch.equal(wr[live], w0[live])
    for ref in (wr, mr):
        assert bool((ref[~live] == GUARD).all())
    assert bool((wg[~live] == GUARD).all()) and bool((mg[~live] == GUARD).all())
    if exact:
        assert torch.equal(wg, wr) and torch.equal(mg, mr)
    else:
        assert float((wg - wr)[live].abs().max()) <= 4 * 2.0 ** -23 * float(wr[live].abs().max())
        assert float((mg - mr)[live].abs().max()) <= 4 * 2.0 ** -23 * float(mr[live].abs().max())
    # the lr_ptr form is the float form
    _, _, w2, m2, _ = _f32_set(cuda)
    fused.mt_sgd_f32(gg, offs, w2, m2, lr=9.0, momentum=mu, weight_decay=wd, scale=sc,
                     lr_t=torch.tensor([lr], dtype=torch.float32, device=cuda))
    assert torch.equal(w2.cpu(), wg) and torch.equal(m2.cpu(), mg)


# ------------------------------------------------------------------------------- graph replay
def _param_sets(cuda):
    g = torch.Generator().manual_seed(7)
    bf = []
    for i, shp in enumerate([(16, 8, 3, 3), (32, 16, 1, 1), (10, 32), (8, 4)]):
        t = torch.randn(shp, generator=g) * 0.05
        if len(shp) == 4 and i % 2 == 0:
            t = t.contiguous(memory_format=torch.channels_last)
        bf.append(torch.nn.Parameter(t.to(cuda)))
    f32 = [torch.nn.Parameter(torch.randn(n, generator=g).to(cuda)) for n in (16, 7, 1, 33, 10)]
    gb = []
    for p in bf:
        t = (torch.randn(p.shape, generator=g) * 0.1).to(BF16)
        if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
            t = t.contiguous(memory_format=torch.channels_last)
        gb.append(t.to(cuda))
    gf = [(torch.randn(p.shape, generator=g) * 0.1).to(cuda) for p in f32]
    return bf, f32, gb, gf


def test_captured_step_follows_the_schedule(cuda):
    """One graph holding advance(), MasterSGD.step(), MultiTensorSGD32.step(), replayed 12 times
    across a 4-step warm-up and a boundary at step 8, against the same parameters stepped eagerly
    with float lr = reference_lr(t): bit-identical weights and momentum. (A float lr would be
    baked into the graph at capture: every replay would repeat one value.)"""
    from arena_amd.ops.optim import MasterSGD, MultiTensorSGD32
    segs = schedule.with_warmup(schedule.piecewise("0.1;8;0.01", 1), 4, 1)
    mu, wd = 0.9, 4e-5

    def build(lr):
        bf, f32, gb, gf = _param_sets(cuda)
        a = MasterSGD(bf, lr=lr, momentum=mu, weight_decay=wd)
        b = MultiTensorSGD32(f32, lr=lr, momentum=mu)
        for p, gr in zip(bf + f32, gb + gf):
            p.grad = gr
        return a, b

    # load every kernel's code object before the capture (on a throw-away set)
    s0 = DeviceLR(segs, cuda)
    a0, b0 = build(s0)
    s0.advance(), a0.step(), b0.step()
    torch.cuda.synchronize()

    sched = DeviceLR(segs, cuda)
    a, b = build(sched)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        sched.advance()
        a.step()
        b.step()
    assert sched.steps() == 0          # the capture ran nothing
    for _ in range(12):
        graph.replay()
    torch.cuda.synchronize()

    ea, eb = build(1.0)
    for t in range(12):
        ea.lr = eb.lr = float(reference_lr(segs, t))
        ea.step()
        eb.step()
    torch.cuda.synchronize()
    assert torch.equal(a.master, ea.master) and torch.equal(a.mom, ea.mom)
    assert torch.equal(a.wbf, ea.wbf)
    assert torch.equal(b.w, eb.w) and torch.equal(b.mom, eb.mom)
    assert _bits(sched.lr).item() == np.float32(reference_lr(segs, 11)).view(np.int32)
    assert sched.steps() == 12
    for p, v in zip(b.params, b._views(b.w)):        # the parameters are the updated buffer
        assert p.data_ptr() == v.data_ptr()


# ------------------------------------------------------------------------------ data parallel
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


DP_SEGS = schedule.with_warmup(schedule.piecewise("0.3;4;0.03", 1), 2, 1)   # 6 steps cross both
DP_SHAPES = [((16, 8, 3, 3), "bf16"), ((16,), "fp32"), ((32, 16), "bf16"), ((7,), "fp32"),
             ((64, 32, 1, 1), "bf16"), ((33,), "fp32")]


def _dp_worker(rank, world, port, q, backend):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world), LOCAL_RANK="0", LOCAL_WORLD_SIZE=str(world))
        torch.cuda.set_device(0)
        import torch.distributed as dist
        dist.init_process_group("gloo")      # two ranks share GPU 0: RCCL takes one rank per GPU
        from arena_amd.parallel.xgmi import XgmiUnavailable
        from arena_amd.parallel.zero import ShardedMasterSGD
        dev = torch.device("cuda", 0)

        def run(scheduled):
            g = torch.Generator().manual_seed(42)
            params = []
            for shp, kind in DP_SHAPES:
                t = torch.randn(shp, generator=g)
                if len(shp) == 4:
                    t = t.contiguous(memory_format=torch.channels_last)
                params.append((torch.nn.Parameter(t.to(dev)), kind))
            sched = DeviceLR(DP_SEGS, dev) if scheduled else None
            opt = ShardedMasterSGD(
                [{"params": [p for p, k in params if k == "bf16"], "weight_decay": 1e-3},
                 {"params": [p for p, k in params if k == "fp32"], "weight_decay": 0.0,
                  "weights": "fp32"}],
                lr=sched if scheduled else 1.0, momentum=0.9, bucket_mb=0.004,
                last_bucket_mb=0.001, backend=backend, order=[p for p, _ in params],
                timeout_s=30.0)
            for t in range(6):
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
            if opt.comm is not None:
                opt.comm.check()
            h = hashlib.sha256()
            for p, _ in params:
                h.update(_bits(p).numpy().tobytes())
            weights = h.hexdigest()
            for t_ in (opt.master, opt.mom, opt.mom32):
                h.update(_bits(t_).numpy().tobytes())
            res = {"weights": weights, "state": h.hexdigest(), "backend": opt.backend,
                   "nbuckets": len(opt.buckets),
                   "lr": float(sched.lr.item()) if scheduled else None,
                   "steps": sched.steps() if scheduled else None}
            opt.close()
            return res

        try:
            res = {"sched": run(True), "float": run(False)}
        except XgmiUnavailable as e:
            res = {"skip": f"xGMI communicator unavailable: {e}"}
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res, None))
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("backend", ["xgmi", "rccl"])
def test_sharded_sgd_follows_the_device_schedule(backend):
    """W = 2 ranks time-sharing GPU 0, 6 steps of ShardedMasterSGD(lr=DeviceLR) across the end of
    the warm-up and a boundary: both ranks end bit-identical, and bit-identical to the same
    optimizer driven with float lr = reference_lr(t) per step."""
    out = _spawn(_dp_worker, 2, backend)
    if any("skip" in res for res in out.values()):
        pytest.skip(next(res["skip"] for res in out.values() if "skip" in res))
    for r, res in out.items():
        assert res["sched"]["backend"] == res["float"]["backend"] == backend, (r, res)
        assert res["sched"]["nbuckets"] > 1, (r, res)
        assert res["sched"]["state"] == res["float"]["state"], (r, res)
        assert res["sched"]["lr"] == float(reference_lr(DP_SEGS, 5)), (r, res)
        assert res["sched"]["steps"] == 6, (r, res)
    assert out[0]["sched"]["weights"] == out[1]["sched"]["weights"], out
    assert out[0]["float"]["weights"] == out[1]["float"]["weights"], out


# ---------------------------------------------------------------------------------- cnn_bench
def test_cnn_bench_trains_under_a_captured_schedule(tmp_path):
    """64 images / batch 8: 8 steps per epoch, 24 steps in one hipGraph; a 1-epoch warm-up to 0.1,
    0.01 from epoch 2."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MIOPEN_FIND_MODE="FAST", ARENA_HEARTBEAT_FILE=str(tmp_path / "hb"))
    r = subprocess.run([sys.executable, "-m", "arena_amd.examples.cnn_bench", "--model",
                        "resnet18", "--width", "16", "--image_size", "32", "--batch_size", "8",
                        "--synth_images", "64", "--num_epochs", "3", "--graph", "1", "--json",
                        "--num_learning_rate_warmup_epochs", "1",
                        "--piecewise_learning_rate_schedule", "0.1;2;0.01",
                        "--num_warmup_batches", "3", "--display_every", "3"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    segs = schedule.with_warmup(schedule.piecewise("0.1;2;0.01", 8), 1, 8)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["exec"] == "hipgraph" and res["steps_per_epoch"] == 8 and res["epochs"] == 3
    assert res["final_lr"] == float(reference_lr(segs, 23))
    assert res["lr_schedule"] == [list(s) for s in segs]
    lrs = {int(m.group(1)): m.group(2)
           for m in re.finditer(r"^(\d+)\timages/sec.*  lr (\d\.\d{6})$", r.stdout, re.M)}
    assert lrs == {i: f"{float(reference_lr(segs, i - 1)):.6f}" for i in range(3, 25, 3)}, r.stdout
    assert res["final_loss"] == res["final_loss"]          # not NaN
