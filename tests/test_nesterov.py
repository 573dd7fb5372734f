"""Nesterov momentum (``nesterov=True`` / ``cnn_bench --use_nesterov``) on the CPU: the three
references of :mod:`arena_amd.ops.reference` against ``torch.optim.SGD(nesterov=True)``,
``MasterSGD`` / ``MultiTensorSGD32`` against those references bit for bit (the CPU path runs
them, so a tolerance would let a silently ignored flag pass), ``ShardedMasterSGD`` over gloo at
W = 2, and the flag's parsing, refusals and reach in ``cnn_bench``. The HIP kernels are checked
against the same references in tests/test_nesterov_gpu.py."""
from __future__ import annotations

import hashlib
import os
import socket
import traceback

import pytest
import torch
import torch.multiprocessing as mp

from arena_amd.ops import fused, optim, reference

TOL = dict(rtol=1e-5, atol=1e-6)          # the optimizer tolerance of tests/test_optim_family_gpu.py
LR, MU, WD = 0.05, 0.9, 1e-3
SIZES = [4, 1024, 1028, 36]


def _inputs(sizes, seed=3, steps=3):
    g = torch.Generator().manual_seed(seed)
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 3) // 4 * 4
    w = torch.randn(total, generator=g)
    grads = [[torch.randn(n, generator=g) * 0.1 for n in sizes] for _ in range(steps)]
    return offs, w, grads


def _torch_sgd(w0, offs, grads, nesterov, scale=1.0, wd=WD):
    """``torch.optim.SGD`` in fp32 over the segments of ``w0``; returns the flat weights and
    momentum buffers."""
    ps = [torch.nn.Parameter(w0[o:o + g.numel()].clone()) for o, g in zip(offs, grads[0])]
    opt = torch.optim.SGD(ps, lr=LR, momentum=MU, weight_decay=wd, dampening=0,
                          nesterov=nesterov)
    for step in grads:
        for p, g in zip(ps, step):
            p.grad = g.float() * scale
        opt.step()
    w, m = w0.clone(), torch.zeros_like(w0)
    for p, o in zip(ps, offs):
        w[o:o + p.numel()] = p.detach()
        m[o:o + p.numel()] = opt.state[p]["momentum_buffer"]
    return w, m


def _close(a, b):
    return torch.allclose(a, b, **TOL)


# ------------------------------------------------------------------------------ the references
def test_master_reference_matches_torch_nesterov():
    offs, w0, grads = _inputs(SIZES)
    grads = [[g.to(torch.bfloat16) for g in step] for step in grads]
    want_w, want_m = _torch_sgd(w0, offs, grads, True)
    plain_w, _ = _torch_sgd(w0, offs, grads, False)
    w, m = w0.clone(), torch.zeros_like(w0)
    wbf = torch.zeros(w0.numel(), dtype=torch.bfloat16)
    for step in grads:
        reference.mt_sgd_master(step, offs, w, m, wbf, LR, MU, WD, nesterov=True)
    assert _close(w, want_w) and _close(m, want_m)
    assert torch.equal(wbf, w.to(torch.bfloat16))
    assert not _close(w, plain_w)                          # the flag is not ignored
    with pytest.raises(ValueError, match="momentum > 0"):
        reference.mt_sgd_master(grads[0], offs, w, m, wbf, LR, 0.0, WD, nesterov=True)


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_f32_reference_matches_torch_nesterov(scale):
    sizes = [1, 7, 33, 64, 1028]
    offs, w0, grads = _inputs(sizes)
    want_w, want_m = _torch_sgd(w0, offs, grads, True, scale)
    plain_w, _ = _torch_sgd(w0, offs, grads, False, scale)
    w, m = w0.clone(), torch.zeros_like(w0)
    for step in grads:
        reference.mt_sgd_f32(step, offs, w, m, LR, MU, WD, scale, nesterov=True)
    assert _close(w, want_w) and _close(m, want_m)
    assert not _close(w, plain_w)


@pytest.mark.parametrize("layout", ["master", "f32", "wide"])
def test_shard_update_reference_matches_torch_nesterov(layout):
    n, scale = 1028, 0.5
    offs, w0, grads = _inputs([n])
    if layout == "master":
        grads = [[g.to(torch.bfloat16) for g in step] for step in grads]
    want_w, want_m = _torch_sgd(w0, offs, grads, True, scale)
    plain_w, _ = _torch_sgd(w0, offs, grads, False, scale)
    w, m = w0.clone(), torch.zeros_like(w0)
    wbf = None if layout == "f32" else torch.zeros(n, dtype=torch.bfloat16)
    lr_t = torch.tensor([LR], dtype=torch.float32)
    for i, step in enumerate(grads):
        kw = {"lr": LR} if i < 2 else {"lr": 123.0, "lr_t": lr_t}
        reference.shard_update(reference.OPT_NESTEROV, step[0], w, m, wbf=wbf, a=0.0, oma=0.0,
                               b=MU, omb=0.0, eps=0.0, weight_decay=WD, scale=scale, **kw)
    assert _close(w, want_w) and _close(m, want_m)
    if wbf is not None:
        assert torch.equal(wbf, w.to(torch.bfloat16))
    assert not _close(w, plain_w)
    assert reference.OPT_NESTEROV == 3
    # fused.shard_sgd(nesterov=True) is this path
    w2, m2 = w0.clone(), torch.zeros_like(w0)
    wbf2 = None if wbf is None else torch.zeros_like(wbf)
    for step in grads:
        fused.shard_sgd(step[0], w2, m2, wbf2, lr=LR, momentum=MU, weight_decay=WD, scale=scale,
                        nesterov=True)
    assert torch.equal(w2, w) and torch.equal(m2, m)
    with pytest.raises(ValueError, match="momentum > 0"):
        fused.shard_sgd(grads[0][0], w2, m2, wbf2, lr=LR, momentum=0.0, weight_decay=WD,
                        scale=scale, nesterov=True)


# ------------------------------------------------------------ MasterSGD / MultiTensorSGD32 (CPU)
def _master_params():
    g = torch.Generator().manual_seed(11)
    shapes = [(8, 4, 3, 3), (16, 8), (4,), (12, 4, 1, 1)]
    ps = []
    for s in shapes:
        t = torch.randn(s, generator=g)
        if len(s) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(t.to(torch.bfloat16)))
    return ps


def _f32_params():
    g = torch.Generator().manual_seed(12)
    return [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (1, 7, 33, 64)]


def _grads_like(ps, step):
    g = torch.Generator().manual_seed(100 + step)
    out = []
    for p in ps:
        t = (torch.randn(p.shape, generator=g) * 0.1).to(p.dtype)
        if p.dim() == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(t)
    return out


def _run_steps(opt, ps, steps):
    for s in steps:
        for p, g in zip(ps, _grads_like(ps, s)):
            p.grad = g
        opt.step()
        opt.zero_grad()


def test_master_sgd_nesterov_is_the_reference_bit_for_bit():
    ps = _master_params()
    opt = optim.MasterSGD(ps, lr=LR, momentum=MU, weight_decay=WD, nesterov=True)
    master, mom = opt.master.clone(), torch.zeros_like(opt.master)
    wbf = torch.zeros_like(opt.wbf)
    plain = optim.MasterSGD(_master_params(), lr=LR, momentum=MU, weight_decay=WD)
    for s in range(3):
        reference.mt_sgd_master(_grads_like(ps, s), opt.offsets, master, mom, wbf, LR, MU, WD,
                                nesterov=True)
    _run_steps(opt, ps, range(3))
    _run_steps(plain, plain.params, range(3))
    assert torch.equal(opt.master, master) and torch.equal(opt.mom, mom)
    assert torch.equal(opt.wbf, wbf)
    assert not torch.equal(opt.master, plain.master)
    # state dicts: the plain one is what it was, the flagged one adds the flag
    assert "nesterov" not in plain.state_dict()
    assert sorted(set(opt.state_dict()) - set(plain.state_dict())) == ["nesterov"]
    assert opt.state_dict()["nesterov"] is True


def test_multi_tensor_sgd32_nesterov_is_the_reference_bit_for_bit():
    ps = _f32_params()
    opt = optim.MultiTensorSGD32(ps, lr=LR, momentum=MU, weight_decay=WD, scale=0.5,
                                 nesterov=True)
    w, mom = opt.w.clone(), torch.zeros_like(opt.w)
    plain = optim.MultiTensorSGD32(_f32_params(), lr=LR, momentum=MU, weight_decay=WD, scale=0.5)
    for s in range(3):
        reference.mt_sgd_f32(_grads_like(ps, s), opt.offsets, w, mom, LR, MU, WD, 0.5,
                             nesterov=True)
    _run_steps(opt, ps, range(3))
    _run_steps(plain, plain.params, range(3))
    assert torch.equal(opt.w, w) and torch.equal(opt.mom, mom)
    assert not torch.equal(opt.w, plain.w)
    assert "nesterov" not in plain.state_dict() and opt.state_dict()["nesterov"] is True


@pytest.mark.parametrize("kind", ["master", "f32"])
def test_state_round_trip_and_flag_mismatch(kind):
    def make(nesterov=True):
        if kind == "master":
            ps = _master_params()
            return ps, optim.MasterSGD(ps, lr=LR, momentum=MU, weight_decay=WD, nesterov=nesterov)
        ps = _f32_params()
        return ps, optim.MultiTensorSGD32(ps, lr=LR, momentum=MU, weight_decay=WD,
                                          nesterov=nesterov)

    def bits(opt, ps):
        return [p.detach().float().clone() for p in ps] + [opt.mom.clone()]

    pa, a = make()
    _run_steps(a, pa, range(3))
    pb, b = make()
    _run_steps(b, pb, range(2))
    sd = b.state_dict()
    weights = [p.detach().clone() for p in pb]
    pc, c = make()
    with torch.no_grad():
        for p, v in zip(pc, weights):
            p.copy_(v)                      # the fp32 group's weights are the model's own state
    c.load_state_dict(sd)
    _run_steps(c, pc, [2])
    assert all(torch.equal(x, y) for x, y in zip(bits(c, pc), bits(a, pa)))
    _, plain = make(nesterov=False)
    with pytest.raises(ValueError, match="nesterov"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="nesterov"):
        c.load_state_dict(plain.state_dict())


def test_nesterov_needs_momentum():
    with pytest.raises(ValueError, match="momentum > 0"):
        optim.MasterSGD(_master_params(), lr=LR, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError, match="momentum > 0"):
        optim.MultiTensorSGD32(_f32_params(), lr=LR, nesterov=True)
    ps = _master_params()
    with pytest.raises(ValueError, match="momentum > 0"):
        optim.MasterSGD(ps, lr=LR, momentum=0.0, nesterov=True)
    assert all(p.dtype == torch.bfloat16 and p.grad is None for p in ps)


# -------------------------------------------------------------- ShardedMasterSGD over gloo, W = 2
SHAPES = [((16, 8, 3, 3), "bf16"), ((16,), "fp32"), ((16,), "fp32"), ((32, 16), "bf16"),
          ((7,), "fp32"), ((64, 32, 1, 1), "bf16"), ((33,), "fp32"), ((10, 64), "bf16"),
          ((10,), "fp32")]                                  # tests/test_shard_optim.py's


def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _params():
    g = torch.Generator().manual_seed(42)
    ps = []
    for shp, kind in SHAPES:
        t = torch.randn(shp, generator=g)
        if len(shp) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append((torch.nn.Parameter(t.to(torch.bfloat16) if kind == "bf16" else t), kind))
    return ps


def _grads(step, rank, params):
    g = torch.Generator().manual_seed(1000 * step + rank)
    out = []
    for p, _ in params:
        t = (torch.randn(p.shape, generator=g) * 0.1).to(p.dtype)
        if p.dim() == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(t)
    return out


def _sharded(params, reduce_fp32, **kw):
    from arena_amd.parallel.zero import ShardedMasterSGD
    return ShardedMasterSGD([{"params": [p for p, k in params if k == "bf16"],
                              "weight_decay": WD},
                             {"params": [p for p, k in params if k == "fp32"],
                              "weight_decay": 0.0, "weights": "fp32"}],
                            lr=LR, momentum=MU, bucket_mb=0.004, last_bucket_mb=0.001,
                            backend="rccl", order=[p for p, _ in params],
                            rccl_reduce_fp32=reduce_fp32, **kw)


def _reference_run(world, steps=3):
    """The single-process reference of the summed gradient: ``torch.optim.SGD(nesterov=True)`` on
    fp32 copies and the rank-averaged gradient."""
    params = _params()
    ref = [torch.nn.Parameter(p.detach().float().clone()) for p, _ in params]
    ropt = torch.optim.SGD(
        [{"params": [r for r, (_, k) in zip(ref, params) if k == "bf16"], "weight_decay": WD},
         {"params": [r for r, (_, k) in zip(ref, params) if k == "fp32"], "weight_decay": 0.0}],
        lr=LR, momentum=MU, dampening=0, nesterov=True)
    for step in range(steps):
        grads = [_grads(step, r, params) for r in range(world)]
        for i, r in enumerate(ref):
            acc = grads[0][i].float()
            for q in range(1, world):
                acc = acc + grads[q][i].float()
            r.grad = acc / world
        ropt.step()
    return [r.detach() for r in ref]


def _sharded_worker(rank, world, port, q, reduce_fp32):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        torch.set_num_threads(1)
        import torch.distributed as dist
        dist.init_process_group("gloo")
        res = {}

        def run(**kw):
            params = _params()
            opt = _sharded(params, reduce_fp32, **kw)
            for step in range(3):
                for (p, _), g in zip(params, _grads(step, rank, params)):
                    p.grad = g.clone()
                opt.step()
                opt.zero_grad()
            return params, opt

        params, opt = run(nesterov=True)
        sd = opt.state_dict()
        pos = {id(p): i for i, p in enumerate(opt.params)}
        worst, w_vs_master = 0.0, 0.0
        for (p, kind), r in zip(params, _reference_run(world)):
            m = sd["master"][pos[id(p)]]
            worst = max(worst, float((m - r).abs().max()) / (float(r.abs().max()) + 1e-12))
            if kind == "bf16":
                w_vs_master = max(w_vs_master, float(
                    (p.detach().float() - m.to(torch.bfloat16).float()).abs().max()))
        res["master_rel"], res["w_vs_master"] = worst, w_vs_master
        res["bits"] = hashlib.sha256(                # a digest: no tensor crosses the queue
            torch.cat([p.detach().float().reshape(-1) for p, _ in params]
                      + [t.reshape(-1) for t in sd["momentum_buffer"]]).numpy().tobytes()
        ).hexdigest()
        res["flag"] = sd.get("nesterov")
        res["keys"] = sorted(sd)
        pp, plain = run()
        psd = plain.state_dict()
        res["plain_keys"] = sorted(psd)
        res["differs"] = not torch.equal(
            torch.cat([p.detach().float().reshape(-1) for p, _ in pp]),
            torch.cat([p.detach().float().reshape(-1) for p, _ in params]))
        for name, o, s in (("load_plain", opt, psd), ("load_flagged", plain, sd)):
            try:
                o.load_state_dict(s)
                res[name] = "loaded"
            except ValueError as e:
                res[name] = str(e)
        opt.load_state_dict(sd)
        plain.close()
        opt.close()
        for rule in ("rmsprop", "adam", "lars"):
            try:
                _sharded(_params(), reduce_fp32, rule=rule, nesterov=True)
                res[rule] = "built"
            except ValueError as e:
                res[rule] = str(e)
        try:
            from arena_amd.parallel.zero import ShardedMasterSGD
            ShardedMasterSGD([p for p, k in _params() if k == "bf16"], lr=LR, momentum=0.0,
                             backend="rccl", nesterov=True)
            res["mu0"] = "built"
        except ValueError as e:
            res["mu0"] = str(e)
        dist.destroy_process_group()
        q.put((rank, res, None))
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def _spawn(target, world, *args, timeout=180):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=target, args=(r, world, port, q, *args)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(world):
            r, res, err = q.get(timeout=timeout)
            assert err is None, f"rank {r} failed:\n{err}"
            out[r] = res
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
    return out


@pytest.mark.parametrize("reduce_fp32", [True, False])
def test_sharded_nesterov_on_two_ranks_over_gloo(reduce_fp32):
    out = _spawn(_sharded_worker, 2, reduce_fp32)
    for r, res in out.items():
        # fp32 sums in gloo's order vs the reference's: a few fp32 ulps; bf16 sums round per add
        # (the bounds of tests/test_shard_optim.py)
        assert res["master_rel"] < (1e-5 if reduce_fp32 else 2e-2), (r, res["master_rel"])
        assert res["w_vs_master"] == 0.0, (r, res["w_vs_master"])
        assert res["flag"] is True and res["differs"], r
        assert res["plain_keys"] == ["master", "momentum_buffer", "param_groups", "shapes"]
        assert res["keys"] == sorted(res["plain_keys"] + ["nesterov"])
        assert "nesterov" in res["load_plain"] and "nesterov" in res["load_flagged"], res
        for rule in ("rmsprop", "adam", "lars"):
            assert "nesterov=True belongs to rule='sgd'" in res[rule], res[rule]
        assert "momentum > 0" in res["mu0"], res["mu0"]
    assert out[0]["bits"] == out[1]["bits"]                          # replicas bit-identical


# ------------------------------------------------------------------------------------- cnn_bench
def _tiny(*extra):
    from arena_amd.examples import cnn_bench
    return cnn_bench.parse(["--model", "resnet_tiny", "--width", "8", "--image_size", "16",
                            "--batch_size", "2", "--num_classes", "10", "--device", "cpu", *extra])


def test_cnn_bench_flag_parses_and_is_off_by_default():
    assert _tiny().use_nesterov is False
    assert _tiny("--use_nesterov").use_nesterov is True
    assert _tiny("--use_nesterov", "--optimizer", "momentum", "--momentum", "0.5").momentum == 0.5


@pytest.mark.parametrize("flags,message", [
    (("--optimizer", "sgd"), "--use_nesterov needs --optimizer momentum"),
    (("--optimizer", "rmsprop"), "--use_nesterov needs --optimizer momentum"),
    (("--optimizer", "adam"), "--use_nesterov needs --optimizer momentum"),
    (("--momentum", "0"), "--use_nesterov needs --momentum > 0"),
    (("--lars",), "--use_nesterov does not apply to --lars"),
    (("--eval",), "--use_nesterov does not apply to --eval"),
])
def test_cnn_bench_refuses(flags, message, capsys):
    with pytest.raises(SystemExit):
        _tiny("--use_nesterov", *flags)
    assert message in capsys.readouterr().err


def test_cnn_bench_build_on_cpu_yields_torch_nesterov(monkeypatch):
    from arena_amd.examples import cnn_bench
    from arena_amd.parallel import hvd
    cpu = torch.device("cpu")
    _, opt, _, _ = cnn_bench.build(_tiny("--use_nesterov", "--dtype", "fp32"), cpu, 1)
    assert type(opt) is torch.optim.SGD
    assert all(g["nesterov"] is True and g["momentum"] == 0.9 for g in opt.param_groups)
    _, opt, _, _ = cnn_bench.build(_tiny("--dtype", "fp32"), cpu, 1)
    assert all(g["nesterov"] is False for g in opt.param_groups)
    # data parallel without master weights: the same optimizer under DistributedOptimizer
    monkeypatch.setattr(hvd, "DistributedOptimizer", lambda opt, **kw: opt)
    _, opt, _, _ = cnn_bench.build(_tiny("--use_nesterov", "--dtype", "fp32"), cpu, 2)
    assert type(opt) is torch.optim.SGD and all(g["nesterov"] for g in opt.param_groups)
