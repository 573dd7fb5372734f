"""Nesterov momentum on the GPU: the ``NesterovRule`` / ``NesterovScaledRule`` kernels (master,
fp32 and the three shard layouts) against the CPU references of :mod:`arena_amd.ops.reference`,
bit for bit in a configuration whose products are exact, the bindings' refusals, a captured
``MasterSGD`` + ``MultiTensorSGD32`` step, ``cnn_bench --use_nesterov`` end to end, and
``ShardedMasterSGD(nesterov=True)`` on two ranks time-sharing GPU 0 over RCCL's gloo stand-in and
over the xGMI kernels."""
from __future__ import annotations

import hashlib
import json
import math
import os
import queue
import socket
import subprocess
import sys
import traceback

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from arena_amd.ops import fused, optim, reference, schedule
from arena_amd.ops.schedule import DeviceLR, reference_lr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32
TOL = dict(rtol=1e-5, atol=1e-6)          # tests/test_optim_family_gpu.py's
SENTINEL = 96.0                           # exact in bf16 too
REAL = dict(lr=0.05, mu=0.9, wd=1e-3)
# every product by one of these is exact in fp32 (powers of two)
EXACT = dict(lr=2.0 ** -4, mu=0.5, wd=2.0 ** -10)
CPU = torch.device("cpu")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _lr_kw(hyper, lr_form, dev):
    if lr_form == "float":
        return {"lr": hyper["lr"]}
    return {"lr": 123.0, "lr_t": torch.tensor([hyper["lr"]], dtype=F32, device=dev)}


# ------------------------------------------------------------------------------- master layout
def _master_set():
    """50 tensors (a launch ends at 48 and a second begins): 4 elements, one chunk, one chunk + 4,
    three chunks + 4, the rest small multiples of 4; 4 elements past the last segment belong to no
    tensor."""
    g = torch.Generator().manual_seed(21)
    ns = [4, 1024, 1028, 3076] + [4 * (1 + i % 5) for i in range(46)]
    offs = [sum(ns[:i]) for i in range(len(ns))]
    total = sum(ns) + 4
    steps = [[(torch.randn(n, generator=g) * 0.1).to(BF16) for n in ns] for _ in range(3)]
    master = torch.randn(total, generator=g)
    mom = torch.zeros(total)
    master[-4:] = SENTINEL
    mom[-4:] = SENTINEL
    return steps, offs, master, mom, total


def _run_master(dev, hyper, lr_form):
    steps, offs, master, mom, total = _master_set()
    assert len(offs) == 50
    master, mom = master.to(dev), mom.to(dev)
    wbf = torch.full((total,), SENTINEL, dtype=BF16, device=dev)
    for grads in steps:
        fused.mt_sgd_master([g.to(dev) for g in grads], offs, master, mom, wbf,
                            momentum=hyper["mu"], weight_decay=hyper["wd"], nesterov=True,
                            **_lr_kw(hyper, lr_form, dev))
    return master.cpu(), mom.cpu(), wbf.cpu()


_REFS = {}


def _ref(key, make):
    """A CPU reference, computed once and shared by the tests that need it."""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


@pytest.mark.parametrize("lr_form", ["float", "lr_t"])
def test_mt_sgd_master_nesterov_matches_cpu_reference(cuda, lr_form):
    rw, rm, rwbf = _ref("master", lambda: _run_master(CPU, REAL, "float"))
    w, m, wbf = _run_master(cuda, REAL, lr_form)
    assert not torch.equal(rw, _master_set()[2])
    torch.testing.assert_close(w, rw, **TOL)
    torch.testing.assert_close(m, rm, **TOL)
    assert torch.equal(wbf[:-4], w[:-4].to(BF16))         # the kernel's own master, rounded
    assert torch.equal(rwbf[:-4], rw[:-4].to(BF16))
    for t in (w, m, wbf.float()):                         # nothing past the last segment
        assert t[-4:].tolist() == [SENTINEL] * 4
    # the plain rule on the same inputs ends elsewhere: the flag is not ignored
    steps, offs, pw, pm, total = _master_set()
    pw, pm = pw.to(cuda), pm.to(cuda)
    pwbf = torch.zeros(total, dtype=BF16, device=cuda)
    for grads in steps:
        fused.mt_sgd_master([g.to(cuda) for g in grads], offs, pw, pm, pwbf, lr=REAL["lr"],
                            momentum=REAL["mu"], weight_decay=REAL["wd"])
    assert not torch.allclose(pw.cpu()[:-4], w[:-4], **TOL)


# --------------------------------------------------------------------------------- fp32 layout
F32_NS = [1, 7, 33, 64, 1028]             # scalar tails of 1, 3 and 1 elements; vector-only; both


def _f32_set():
    """Sizes 1, 7, 33, 64 and 1028 in 16-byte aligned slots with 4 free elements behind each;
    everything between the segments holds a sentinel."""
    g = torch.Generator().manual_seed(22)
    offs, total = [], 0
    for n in F32_NS:
        offs.append(total)
        total += (n + 3) // 4 * 4 + 4
    live = torch.zeros(total, dtype=torch.bool)
    for n, o in zip(F32_NS, offs):
        live[o:o + n] = True
    steps = [[torch.randn(n, generator=g) * 0.1 for n in F32_NS] for _ in range(3)]
    w = torch.randn(total, generator=g)
    mom = torch.zeros(total)
    w[~live] = SENTINEL
    mom[~live] = SENTINEL
    return steps, offs, w, mom, live


def _run_f32(dev, hyper, scale, lr_form):
    steps, offs, w, mom, live = _f32_set()
    w, mom = w.to(dev), mom.to(dev)
    for grads in steps:
        fused.mt_sgd_f32([g.to(dev) for g in grads], offs, w, mom, momentum=hyper["mu"],
                         weight_decay=hyper["wd"], scale=scale, nesterov=True,
                         **_lr_kw(hyper, lr_form, dev))
    return w.cpu(), mom.cpu(), live


@pytest.mark.parametrize("lr_form", ["float", "lr_t"])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_mt_sgd_f32_nesterov_matches_cpu_reference(cuda, scale, lr_form):
    rw, rm, _ = _ref(("f32", scale), lambda: _run_f32(CPU, REAL, scale, "float"))
    w, m, live = _run_f32(cuda, REAL, scale, lr_form)
    assert not torch.equal(rw, _f32_set()[2])
    for got, want in ((w, rw), (m, rm)):
        torch.testing.assert_close(got[live], want[live], **TOL)
        assert bool((got[~live] == SENTINEL).all())


# ------------------------------------------------------------------------------- shard layouts
SHARD_NS = [4, 1024, 1028, 4096 * 1024 + 1024]   # the last: the grid-stride loop past the block cap
LAYOUTS = ["master", "f32", "wide"]       # bf16 grad + wbf; fp32 grad, no wbf; fp32 grad + wbf


def _run_shard(dev, hyper, layout, n, scale):
    """Three steps over a range of n elements, the last in the lr_t form; every buffer carries 8
    sentinels behind it."""
    g = torch.Generator().manual_seed(7 + n % 1000)
    pad = n + 8

    def buf(t, dtype=F32):
        out = torch.full((pad,), SENTINEL, dtype=dtype)
        out[:n] = t.to(dtype)
        return out.to(dev)

    w = buf(torch.randn(n, generator=g))
    mom = buf(torch.zeros(n))
    wbf = None if layout == "f32" else buf(torch.zeros(n), BF16)
    gdt = BF16 if layout == "master" else F32
    for step in range(3):
        grad = buf(torch.randn(n, generator=g) * 0.1, gdt)
        wb = None if wbf is None else wbf[:n]
        kw = _lr_kw(hyper, "float" if step < 2 else "lr_t", dev)
        if step == 0:                     # the rule by its number, as the binding takes it
            impl = fused._impl(w)
            impl.shard_update(rule=reference.OPT_NESTEROV, grad=grad[:n], w32=w[:n], st0=mom[:n],
                              wbf=wb, a=0.0, oma=0.0, b=hyper["mu"], omb=0.0, eps=0.0,
                              weight_decay=hyper["wd"], scale=scale, **kw)
        else:
            fused.shard_sgd(grad[:n], w[:n], mom[:n], wb, momentum=hyper["mu"],
                            weight_decay=hyper["wd"], scale=scale, nesterov=True, **kw)
        assert grad[n:].tolist() == [SENTINEL] * 8
    out = [w.cpu(), mom.cpu()]
    if wbf is not None:
        out.append(wbf.cpu())
    return out


@pytest.mark.parametrize("n", SHARD_NS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_shard_update_nesterov_matches_cpu_reference(cuda, layout, n):
    want = _ref(("shard", layout, n), lambda: _run_shard(CPU, REAL, layout, n, 0.5))
    got = _run_shard(cuda, REAL, layout, n, 0.5)
    assert len(got) == (2 if layout == "f32" else 3)
    assert bool((want[1][:n] != 0).any())
    for a, b in zip(got, want):
        assert a[n:].tolist() == [SENTINEL] * 8                   # nothing written past n
        if a.dtype != BF16:
            torch.testing.assert_close(a[:n], b[:n], **TOL)
    if layout != "f32":
        assert torch.equal(got[2][:n], got[0][:n].to(BF16))       # wbf = bf16(its own master)
        assert torch.equal(want[2][:n], want[0][:n].to(BF16))


# --------------------------------------------------------------------- the exact configuration
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_exact_configuration_matches_bit_for_bit(cuda, scale):
    """lr 2^-4, momentum 1/2, weight decay 2^-10, scale 1 or 1/2, gradients randn * 0.1: every
    product of the rule is by a power of two and so exact in fp32. Then ``d = g * scale + wd * w``,
    ``m = mu * m + d``, the inner sum ``d + mu * m`` and ``w = w - lr * (...)`` are each ONE
    rounding of an exact value, whichever products the compiler contracts into FMAs (an FMA rounds
    the exact product plus the addend once, which is what a separately rounded exact product plus
    the addend gives). The kernels must therefore match the CPU reference bit for bit over 3
    steps: the argument tests/test_xgmi_gpu.py makes for the plain rule. All three paths; the
    master layout takes no scale."""
    if scale == 1.0:
        for a, b in zip(_run_master(cuda, EXACT, "float"), _run_master(CPU, EXACT, "float")):
            assert _same_bits(a, b)
    want = _run_f32(CPU, EXACT, scale, "float")
    for form in ("float", "lr_t"):
        got = _run_f32(cuda, EXACT, scale, form)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    for layout in LAYOUTS:
        for n in (4, 1028):
            for a, b in zip(_run_shard(cuda, EXACT, layout, n, scale),
                            _run_shard(CPU, EXACT, layout, n, scale)):
                assert _same_bits(a, b), (layout, n)


# ----------------------------------------------------------------------------- binding refusals
def test_bindings_refuse_bad_arguments_for_the_new_rule(cuda):
    from arena_amd.ops import _ext
    ext = _ext.load()
    n = 16
    w, mom, g = (torch.zeros(n + 4, device=cuda) for _ in range(3))
    wbf = torch.zeros(n + 4, dtype=BF16, device=cuda)
    gb = torch.ones(n + 4, dtype=BF16, device=cuda)
    g.fill_(1.0)
    sgd = dict(lr=0.1, momentum=0.9, weight_decay=0.0, scale=1.0, nesterov=True)
    with pytest.raises(RuntimeError, match="misaligned"):
        fused.shard_sgd(g[:n], w[1:n + 1], mom[:n], None, **sgd)
    with pytest.raises(RuntimeError, match="misaligned"):
        fused.shard_sgd(g[2:n + 2], w[:n], mom[:n], wbf[:n], **sgd)
    with pytest.raises(RuntimeError, match="misaligned"):
        fused.shard_sgd(g[:n], w[:n], mom[3:n + 3], None, **sgd)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        fused.shard_sgd(g[:6], w[:6], mom[:6], None, **sgd)
    with pytest.raises(RuntimeError, match="need the bf16 weight range"):
        fused.shard_sgd(gb[:n], w[:n], mom[:n], None, **sgd)
    hyper = dict(lr=0.1, a=0.0, oma=0.0, omb=0.0, eps=0.0, weight_decay=0.0, scale=1.0)
    with pytest.raises(RuntimeError, match="momentum"):
        ext.shard_update(rule=reference.OPT_NESTEROV, grad=g[:n], w32=w[:n], st0=mom[:n], b=0.0,
                         **hyper)
    with pytest.raises(RuntimeError, match="unknown rule"):
        ext.shard_update(rule=4, grad=g[:n], w32=w[:n], st0=mom[:n], b=0.9, **hyper)
    with pytest.raises(RuntimeError, match="wide layout only"):       # the plain rule's stays
        ext.shard_update(rule=reference.OPT_SGD, grad=g[:n], w32=w[:n], st0=mom[:n], b=0.9,
                         **hyper)
    mt = dict(lr=0.1, momentum=0.9, weight_decay=0.0, nesterov=True)
    with pytest.raises(RuntimeError, match="misaligned"):
        fused.mt_sgd_master([gb[:6]], [0], w, mom, wbf, **mt)
    with pytest.raises(RuntimeError, match="out of bounds"):
        fused.mt_sgd_master([gb[:n]], [8], w, mom, wbf, **mt)
    with pytest.raises(RuntimeError, match="out of bounds"):
        fused.mt_sgd_f32([g[:n]], [8], w, mom, **mt)
    with pytest.raises(RuntimeError, match="momentum > 0"):
        ext.mt_sgd_master([gb[:n]], [0], w, mom, wbf, 0.1, 0.0, 0.0, nesterov=True)
    with pytest.raises(RuntimeError, match="momentum > 0"):
        ext.mt_sgd_f32([g[:n]], [0], w, mom, 0.1, 0.0, 0.0, 1.0, nesterov=True)
    with pytest.raises(ValueError, match="momentum > 0"):
        fused.mt_sgd_master([gb[:n]], [0], w, mom, wbf, lr=0.1, momentum=0.0, weight_decay=0.0,
                            nesterov=True)
    torch.cuda.synchronize()
    assert not w.any() and not mom.any() and not wbf.any()           # nothing ran


# ------------------------------------------------------------------------------- graph replay
def _param_sets(dev, steps):
    g = torch.Generator().manual_seed(7)
    bf = []
    for i, shp in enumerate([(16, 8, 3, 3), (32, 16, 1, 1), (10, 32), (8, 4)]):
        t = torch.randn(shp, generator=g) * 0.05
        if len(shp) == 4 and i % 2 == 0:
            t = t.contiguous(memory_format=torch.channels_last)
        bf.append(torch.nn.Parameter(t.to(dev)))
    f32 = [torch.nn.Parameter(torch.randn(n, generator=g).to(dev)) for n in (16, 7, 1, 33, 10)]
    values = []
    for _ in range(steps):
        vb = []
        for p in bf:
            t = (torch.randn(p.shape, generator=g) * 0.1).to(BF16)
            if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
                t = t.contiguous(memory_format=torch.channels_last)
            vb.append(t.to(dev))
        values.append(vb + [(torch.randn(p.shape, generator=g) * 0.1).to(dev) for p in f32])
    return bf, f32, values


def test_captured_nesterov_step_equals_eager_steps(cuda):
    """One graph holding DeviceLR.advance(), MasterSGD(nesterov=True).step() and
    MultiTensorSGD32(nesterov=True).step(), replayed 6 times across the end of a 4-step warm-up
    with gradients rewritten between replays: bit-identical to the same 6 steps run eagerly, and
    within the kernels' tolerance of the CPU classes."""
    segs = schedule.with_warmup(schedule.piecewise("0.1;8;0.01", 1), 4, 1)

    def build(dev, steps):
        bf, f32, values = _param_sets(dev, steps)
        sched = DeviceLR(segs, dev)
        a = optim.MasterSGD(bf, lr=sched, momentum=0.9, weight_decay=4e-5, nesterov=True)
        b = optim.MultiTensorSGD32(f32, lr=sched, momentum=0.9, nesterov=True)
        for p, v in zip(bf + f32, values[0]):
            p.grad = torch.empty_like(v).copy_(v)     # static: the captured kernels read it
        return sched, a, b, bf + f32, values

    def run(dev, graph):
        sched, a, b, params, values = build(dev, 6)

        def step():
            sched.advance()
            a.step()
            b.step()

        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                step()
            assert sched.steps() == 0                 # the capture ran nothing
        for t in range(6):
            for p, v in zip(params, values[t]):
                p.grad.copy_(v)
            g.replay() if graph else step()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        assert sched.steps() == 6
        return [a.master, a.mom, a.wbf, b.w, b.mom]

    s0, a0, b0 = build(cuda, 1)[:3]                    # load every kernel before the capture
    s0.advance(), a0.step(), b0.step()
    torch.cuda.synchronize()
    for got, eager, ref in zip(run(cuda, True), run(cuda, False), run(CPU, False)):
        assert _same_bits(got, eager)
        if got.dtype == F32:
            torch.testing.assert_close(got.cpu(), ref, **TOL)


# ---------------------------------------------------------------------------------- cnn_bench
def _cnn_bench(tmp_path, *extra, **env_extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MIOPEN_FIND_MODE="FAST", ARENA_HEARTBEAT_FILE=str(tmp_path / "hb"), **env_extra)
    argv = ["--model", "resnet_tiny", "--width", "16", "--image_size", "32", "--batch_size", "8",
            "--synth_images", "64", "--num_batches", "12", "--num_warmup_batches", "2", "--json"]
    r = subprocess.run([sys.executable, "-m", "arena_amd.examples.cnn_bench"] + argv
                       + list(extra), capture_output=True, text=True, timeout=240, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(extra, res)
    return res, r.stdout


def test_cnn_bench_use_nesterov_graph_and_eager_runs_agree(tmp_path_factory):
    """12 captured steps of Nesterov momentum SGD on 64 resident images, then the same steps run
    eagerly (three warm-up batches: the graph run takes one step more than its two before the
    measured ones) under the environment that makes two processes run the same kernels in the same
    summation order (tests/test_optim_family_gpu.py ``same_kernels``): the same loss to the 4
    decimals printed. No loss value is asserted: nobody has measured one for this rule."""
    same = {"ARENA_CONV_PLAN": str(tmp_path_factory.mktemp("plans") / "plans.json"),
            "ARENA_MIOPEN_BENCHMARK": "0", "ARENA_BN_FINAL": "0",
            # MIOpen's user databases in a folder of this test's own: its two runs share them and
            # leave nothing behind for the cnn_bench runs of other test files
            "MIOPEN_USER_DB_PATH": str(tmp_path_factory.mktemp("miopen_db")),
            "MIOPEN_CUSTOM_CACHE_DIR": str(tmp_path_factory.mktemp("miopen_cache"))}
    res, out = _cnn_bench(tmp_path_factory.mktemp("graph"), "--use_nesterov", **same)
    assert res["exec"] == "hipgraph" and res["optimizer"] == "momentum"
    assert res["nesterov"] is True and math.isfinite(res["final_loss"])
    header = [line for line in out.splitlines() if line.startswith("Model: ")]
    assert len(header) == 1 and header[0].endswith("  nesterov"), header
    eager, _ = _cnn_bench(tmp_path_factory.mktemp("eager"), "--use_nesterov", "--graph", "0",
                          "--num_warmup_batches", "3", **same)
    assert eager["exec"] == "eager" and eager["nesterov"] is True
    assert eager["final_loss"] == res["final_loss"]


# -------------------------------------------------------------------------------- data parallel
def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_SPAWN_FAILED = []


def _spawn(fn, world, *args, timeout=150):
    """Run ``fn(rank, world, port, q, *args)`` in ``world`` spawned processes and collect one
    result per rank; the first failure (or a rank that does not answer in time) takes the whole
    gang down, and no later spawn of this module starts."""
    assert not _SPAWN_FAILED, f"an earlier two-rank run failed: {_SPAWN_FAILED[0]}"
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
        if err is not None or any(p.exitcode != 0 for p in procs):
            _SPAWN_FAILED.append(err or f"exit codes {[p.exitcode for p in procs]}")
    assert err is None, err
    return out


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK="0", LOCAL_WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    import torch.distributed as dist
    dist.init_process_group("gloo")      # two ranks share GPU 0: RCCL takes one rank per GPU
    return dist


DP_SEGS = schedule.with_warmup(schedule.piecewise("0.3;4;0.03", 1), 2, 1)
DP_SHAPES = [((16, 8, 3, 3), "bf16"), ((16,), "fp32"), ((32, 16), "bf16"), ((7,), "fp32"),
             ((64, 32, 1, 1), "bf16"), ((33,), "fp32")]     # tests/test_shard_optim_gpu.py's


def _rccl_worker(rank, world, port, q):
    try:
        dist = _init(rank, world, port)
        from arena_amd.parallel.zero import ShardedMasterSGD
        dev = torch.device("cuda", 0)

        def run(reduce_fp32, scheduled, nesterov=True):
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
                timeout_s=30.0, rccl_reduce_fp32=reduce_fp32, nesterov=nesterov)
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
            for key in ("master", "momentum_buffer"):
                for t_ in sd[key]:
                    h.update(_bits(t_).numpy().tobytes())
            res = {"weights": weights, "state": h.hexdigest(), "backend": opt.backend,
                   "nbuckets": len(opt.buckets),
                   "mixed": sum(1 for b in opt.buckets if len(b.ranges) == 2),
                   "finite": all(bool(torch.isfinite(p).all()) for p, _ in params),
                   "moved": all(not torch.equal(p.detach().float().cpu(), s)
                                for (p, _), s in zip(params, start)),
                   "flag": sd.get("nesterov")}
            opt.close()
            return res

        res = {(red, form): run(red, form == "sched")
               for red in (False, True) for form in ("float", "sched")}
        res["plain"] = run(True, False, nesterov=False)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res, None))
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def test_sharded_nesterov_over_rccl_on_two_ranks():
    """W = 2 ranks time-sharing GPU 0 over gloo, 4 steps across the end of the warm-up, bf16 and
    fp32 reduce-scatter sums (master, fp32 and wide shard layouts): both ranks end with
    bit-identical weights and states, bit-identical under a float lr and a DeviceLR."""
    out = _spawn(_rccl_worker, 2)
    for red in (False, True):
        for form in ("float", "sched"):
            a, b = out[0][(red, form)], out[1][(red, form)]
            assert a["backend"] == "rccl" and a["nbuckets"] > 1 and a["mixed"] >= 1, a
            assert a["finite"] and a["moved"] and b["finite"] and b["moved"], (a, b)
            assert a["flag"] is True and b["flag"] is True
            assert a["weights"] == b["weights"] and a["state"] == b["state"], (red, form, a, b)
        for r in (0, 1):
            assert out[r][(red, "float")]["state"] == out[r][(red, "sched")]["state"], (red, out)
    for r in (0, 1):                         # the plain rule ends elsewhere and carries no flag
        assert out[r]["plain"]["flag"] is None
        assert out[r]["plain"]["state"] != out[r][(True, "float")]["state"]


# ----------------------------------------------------------------------------------- xGMI
XGMI_SHAPES = [((64, 32, 3, 3), "bf16", True), ((1000,), "fp32", False),
               ((128, 64), "bf16", False), ((7,), "fp32", False), ((3, 5), "bf16", False),
               ((64,), "fp32", False), ((256, 16, 1, 1), "bf16", True), ((33,), "fp32", False)]
#                                          tests/test_xgmi_gpu.py _sharded_sgd_kernel's 8 shapes
XGMI_WORLD = 2
# the "real" configuration's bounds (test_sharded_nesterov_over_xgmi_on_two_ranks derives them)
STATE_ULPS, WEIGHT_ULPS = 4.0, 1.0


def _bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 numbers at |x| (8 significant bits): 2^(e-8) for x = m * 2^e, m in [.5, 1)."""
    _, e = torch.frexp(x.float().abs())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), (e - 8).to(torch.int32))


def _xgmi_inputs():
    """The parameters and every rank's gradients of 3 steps, from CPU generators: every rank (and
    the CPU measurement below) holds the same bytes."""
    g0 = torch.Generator().manual_seed(42)
    params, kinds = [], []
    for shp, kind, cl in XGMI_SHAPES:
        t = torch.randn(shp, generator=g0)
        if kind == "bf16":
            t = t.to(BF16)
        if cl:
            t = t.contiguous(memory_format=torch.channels_last)
        params.append(t)
        kinds.append(kind)
    grads = []
    for step in range(3):
        rows = []
        for r in range(XGMI_WORLD):
            gg = torch.Generator().manual_seed(1000 * step + r)
            row = []
            for p in params:
                t = (torch.randn(p.shape, generator=gg) * 0.1).to(p.dtype)
                row.append(t.contiguous(memory_format=torch.channels_last if p.dim() == 4
                                        else torch.contiguous_format))
            rows.append(row)
        grads.append(rows)
    return params, kinds, grads


def _torch_reference(hyper, dtype):
    """3 steps of ``torch.optim.SGD(nesterov=True, dampening=0)`` over ``dtype`` copies of the
    parameters and the rank-averaged gradient (summed in rank order; 1 / 2 is exact), the learning
    rate doubled before the last step. ``dtype`` fp64: the same steps with the coefficients the
    kernels receive (the fp32 values of lr, momentum and weight decay), every operation in fp64.
    Returns masters and momentum buffers."""
    params, kinds, grads = _xgmi_inputs()

    def coef(v):
        return float(np.float32(v)) if dtype == torch.float64 else v

    ref = [torch.nn.Parameter(p.to(dtype).clone()) for p in params]
    opt = torch.optim.SGD(
        [{"params": [r for r, k in zip(ref, kinds) if k == "bf16"],
          "weight_decay": coef(hyper["wd"])},
         {"params": [r for r, k in zip(ref, kinds) if k == "fp32"], "weight_decay": 0.0}],
        lr=coef(hyper["lr"]), momentum=coef(hyper["mu"]), dampening=0, nesterov=True)
    for step in range(3):
        if step == 2:
            for grp in opt.param_groups:
                grp["lr"] = coef(hyper["lr"] * 2)
        for i, r in enumerate(ref):
            gsum = grads[step][0][i].to(dtype)
            for q in range(1, XGMI_WORLD):
                gsum = gsum + grads[step][q][i].to(dtype)
            r.grad = gsum * (1.0 / XGMI_WORLD)
        opt.step()
    return [r.detach() for r in ref], [opt.state[r]["momentum_buffer"] for r in ref]


def _ulps_normwise(got, want):
    """Largest |got - want| in fp32 ulps of the tensor's largest magnitude (momentum cancels:
    elementwise ulps of a near-zero result measure the cancellation, not the arithmetic)."""
    scale = float(want.abs().max()) * 2.0 ** -24 + 1e-30
    return float((got.double() - want.double()).abs().max()) / scale


def _reference_gap():
    """The largest gap, over the "real" configuration's own inputs, between the fp32 reference and
    the same three steps evaluated in fp64 and rounded once: (states, in fp32 ulps normwise;
    weights, in bf16 ulps elementwise)."""
    w32, m32 = _torch_reference(REAL, F32)
    w64, m64 = _torch_reference(REAL, torch.float64)
    kinds = [k for _, k, _ in XGMI_SHAPES]
    state = max(_ulps_normwise(a, b.float()) for a, b in zip(w32 + m32, w64 + m64))
    weight = 0.0
    for a, b, k in zip(w32, w64, kinds):
        if k == "bf16":
            ra, rb = a.to(BF16).float(), b.to(BF16).float()
            weight = max(weight, float(((ra - rb).abs() / _bf16_ulp(rb)).max()))
    return state, weight


def _xgmi_worker(rank, world, port, q):
    try:
        dist = _init(rank, world, port)
        from arena_amd.parallel.zero import ShardedMasterSGD
        res = {}
        for cfg, hyper in (("exact", EXACT), ("real", REAL)):
            cpu_params, kinds, grads = _xgmi_inputs()
            params = [torch.nn.Parameter(p.to("cuda")) for p in cpu_params]
            groups = [{"params": [p for p, k in zip(params, kinds) if k == "bf16"],
                       "weight_decay": hyper["wd"]},
                      {"params": [p for p, k in zip(params, kinds) if k == "fp32"],
                       "weight_decay": 0.0, "weights": "fp32"}]
            opt = ShardedMasterSGD(groups, lr=hyper["lr"], momentum=hyper["mu"], bucket_mb=0.005,
                                   timeout_s=30.0, nesterov=True)
            assert opt.backend == "xgmi", opt.backend          # "auto" keeps choosing xGMI
            assert len(opt.buckets) >= 4, len(opt.buckets)
            assert set().union(*(b.dtypes for b in opt.buckets)) == {BF16, F32}
            selftest = dict(opt.comm.selftest_result)
            for step in range(3):
                if step == 2:
                    for g in opt.param_groups:
                        g["lr"] = hyper["lr"] * 2
                for p, gr in zip(params, grads[step][rank]):
                    p.grad = gr.to("cuda")
                opt.step()
                opt.zero_grad()
            torch.cuda.synchronize()
            master, mom = _torch_reference(hyper, F32)
            sd = opt.state_dict()           # in the optimizer's parameter order (group order)
            pos = {id(p): i for i, p in enumerate(opt.params)}
            worst = {"w_ulp": 0.0, "master_ulp": 0.0, "mom_ulp": 0.0, "w_bits": 0,
                     "state_bits": 0, "n": 0}
            for i, p in enumerate(params):
                got_w = p.detach().cpu()
                ref_w = master[i].to(p.dtype)
                if p.dtype == BF16:
                    worst["w_bits"] += int((_bits(got_w) != _bits(ref_w)).sum())
                    worst["n"] += p.numel()
                    d = (got_w.float() - ref_w.float()).abs() / _bf16_ulp(ref_w)
                    worst["w_ulp"] = max(worst["w_ulp"], float(d.max()))
                j = pos[id(p)]
                for key, got, want in (("master_ulp", sd["master"][j].cpu(), master[i]),
                                       ("mom_ulp", sd["momentum_buffer"][j].cpu(), mom[i])):
                    worst["state_bits"] += int((_bits(got) != _bits(want)).sum())
                    worst[key] = max(worst[key], _ulps_normwise(got, want))
            opt.comm.check()
            opt.close()
            worst["selftest"] = selftest
            worst["flag"] = sd.get("nesterov")
            res[cfg] = worst
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res, None))
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def test_reference_gap_leaves_room_for_the_real_bounds():
    """The plain rule's bounds in the "real" configuration (lr 0.05, momentum 0.9, wd 1e-3) are 4
    fp32 ulps normwise for the states and 1 bf16 ulp for the weights, set for a rule with two fewer
    roundings. They are kept only where the gap between the fp32 reference and the same three
    steps evaluated in fp64 and rounded once, over this test's own inputs on the CPU, is at most
    half of them; else the bound is twice the measured gap.

    Measured: states 1.74 fp32 ulps normwise (at most half of 4: the bound stays 4); weights 0.0
    bf16 ulps (no master of this set lies close enough to a bf16 rounding boundary for the two
    evaluations to round apart: at most half of 1, so the bound stays 1)."""
    state, weight = _reference_gap()
    print(f"reference gap: states {state:.3f} fp32 ulps normwise, weights {weight:.3f} bf16 ulps")
    assert state <= STATE_ULPS / 2
    assert weight <= WEIGHT_ULPS / 2


def test_sharded_nesterov_over_xgmi_on_two_ranks():
    """``xgmi_sgd_bf16`` / ``xgmi_sgd_f32`` with NESTEROV against fp32 torch
    (``SGD(nesterov=True)``) on W = 2 ranks time-sharing GPU 0, with fixed, seeded gradients: the
    8 shapes and ``bucket_mb=0.005`` of tests/test_xgmi_gpu.py's ``_sharded_sgd_kernel``.

    "exact" (lr 2^-4, momentum 1/2, weight decay 2^-10, 1 / world = 1/2; see
    test_exact_configuration_matches_bit_for_bit): masters, momentum and bf16 weights match the
    reference bit for bit on both ranks. "real" (lr 0.05, momentum 0.9, wd 1e-3): the states
    within 4 fp32 ulps normwise and the weights within 1 bf16 ulp, the plain rule's bounds: the
    gap between the fp32 reference and an fp64 evaluation rounded once measures 1.74 fp32 ulps
    and 0.0 bf16 ulps over these inputs, at most half of each
    (test_reference_gap_leaves_room_for_the_real_bounds). The communicator's self-test ran both Nesterov kinds."""
    out = _spawn(_xgmi_worker, XGMI_WORLD)
    for r, res in out.items():
        ex, real = res["exact"], res["real"]
        print(r, {k: v for k, v in ex.items() if k != "selftest"},
              {k: v for k, v in real.items() if k != "selftest"})
        assert ex["selftest"].get("sgd_bf16_nesterov") == "ok", ex["selftest"]
        assert ex["selftest"].get("sgd_f32_nesterov") == "ok", ex["selftest"]
        assert all(v == "ok" for v in ex["selftest"].values()), ex["selftest"]
        assert ex["flag"] is True
        assert ex["w_bits"] == 0 and ex["state_bits"] == 0, (r, ex)
        assert ex["master_ulp"] == 0 and ex["mom_ulp"] == 0, (r, ex)
        assert real["master_ulp"] <= STATE_ULPS and real["mom_ulp"] <= STATE_ULPS, (r, real)
        assert real["w_ulp"] <= WEIGHT_ULPS, (r, real)
