"""``ShardedMasterSGD(rule="rmsprop" | "adam" | "lars")`` on CPU over gloo (the shard updates run
their PyTorch references; the HIP kernels are checked against those in
tests/test_shard_optim_gpu.py): worlds 2 and 4 flat and (4, 2) hierarchical against the project's
single-process ``TFRMSprop`` / ``TFAdam`` / ``TFLars`` on fp32 copies and the rank-averaged
gradient, the state round trip, and ``cnn_bench --shard_optimizer``'s refusals."""
from __future__ import annotations

import os
import socket
import traceback

import pytest
import torch
import torch.multiprocessing as mp

from arena_amd.ops import optim
from arena_amd.ops.reference import reference_lars_trust

SHAPES = [((16, 8, 3, 3), "bf16"), ((16,), "fp32"), ((16,), "fp32"), ((32, 16), "bf16"),
          ((7,), "fp32"), ((64, 32, 1, 1), "bf16"), ((33,), "fp32"), ((10, 64), "bf16"),
          ((10,), "fp32")]                                  # tests/test_zero_rccl.py's
WD = 1e-3
HYPER = {"rmsprop": dict(lr=0.01, momentum=0.9, decay=0.9, eps=1.0),
         "adam": dict(lr=0.01, betas=(0.9, 0.999), eps=1e-8),
         "lars": dict(lr=1.0, momentum=0.9, eeta=0.001, eps=1e-9)}


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


def _reference_opt(rule, ref, params):
    """The single-process optimizer of the same rule over the fp32 copies ``ref``."""
    groups = [{"params": [r for r, (_, k) in zip(ref, params) if k == "bf16"], "weight_decay": WD},
              {"params": [r for r, (_, k) in zip(ref, params) if k == "fp32"],
               "weight_decay": 0.0}]
    if rule == "rmsprop":
        return optim.TFRMSprop(groups, **HYPER[rule])
    if rule == "adam":
        return optim.TFAdam(groups, **HYPER[rule])
    groups[0]["lars"], groups[1]["lars"] = True, False
    return optim.TFLars(groups, **HYPER[rule])


def _sharded(rule, params, reduce_fp32, backend, local_size):
    from arena_amd.parallel.zero import ShardedMasterSGD
    return ShardedMasterSGD([{"params": [p for p, k in params if k == "bf16"],
                              "weight_decay": WD},
                             {"params": [p for p, k in params if k == "fp32"],
                              "weight_decay": 0.0, "weights": "fp32"}],
                            bucket_mb=0.004, last_bucket_mb=0.001, backend=backend,
                            order=[p for p, _ in params], rccl_reduce_fp32=reduce_fp32,
                            local_size=local_size, rule=rule, **HYPER[rule])


def _averaged(grads, i, world, order=None):
    acc = None
    for r in (range(world) if order is None else order):
        acc = grads[r][i].float() if acc is None else acc + grads[r][i].float()
    return acc / world


def _step(opt, params, grads, unused):
    for i, ((p, _), g) in enumerate(zip(params, grads)):
        p.grad = None if i == unused else g.clone()
    opt.step()
    opt.zero_grad()


def _reference_run(rule, world, order=None, steps=4):
    """``steps`` steps of the reference on the gradients of ``world`` ranks, summed in ``order``:
    the lr doubles before the last step and parameter 4 gets no gradient in step 1. Returns the
    fp32 copies, and for LARS the trust ratios of the last step's (weights, averaged gradient)."""
    params = _params()
    ref = [torch.nn.Parameter(p.detach().float().clone()) for p, _ in params]
    ropt = _reference_opt(rule, ref, params)
    trust = []
    for step in range(steps):
        if step == 3:
            for grp in ropt.param_groups:
                grp["lr"] = HYPER[rule]["lr"] * 2
        grads = [_grads(step, r, params) for r in range(world)]
        for i, r in enumerate(ref):
            r.grad = (torch.zeros_like(r) if step == 1 and i == 4
                      else _averaged(grads, i, world, order))
        if rule == "lars" and step == steps - 1:
            trust = [reference_lars_trust(r.detach().reshape(-1), r.grad.reshape(-1),
                                          HYPER[rule]["eeta"], WD, HYPER[rule]["eps"])
                     for r, (_, k) in zip(ref, params) if k == "bf16"]
        ropt.step()
    return [r.detach() for r in ref], trust


def _worker(rank, world, port, q, rule, reduce_fp32, backend, local_size, mode):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                          WORLD_SIZE=str(world))
        torch.set_num_threads(1)
        import torch.distributed as dist
        dist.init_process_group("gloo")
        res = (_against_reference if mode == "ref" else _round_trip)(
            rank, world, rule, reduce_fp32, backend, local_size)
        dist.destroy_process_group()
        q.put((rank, res, None))
    except Exception:  # noqa: BLE001
        q.put((rank, None, traceback.format_exc()))


def _against_reference(rank, world, rule, reduce_fp32, backend, local_size):
    params = _params()
    opt = _sharded(rule, params, reduce_fp32, backend, local_size)
    res = {"backend": opt.backend, "nbuckets": len(opt.buckets),
           "mixed": sum(1 for b in opt.buckets if len(b.ranges) == 2)}
    for step in range(4):
        if step == 3:
            for grp in opt.param_groups:
                grp["lr"] = HYPER[rule]["lr"] * 2
        _step(opt, params, _grads(step, rank, params), 4 if step == 1 else -1)
    ref, rtrust = _reference_run(rule, world)
    sd = opt.state_dict()
    pos = {id(p): i for i, p in enumerate(opt.params)}
    worst_master, worst_w = 0.0, 0.0
    for (p, kind), r in zip(params, ref):
        m = sd["master"][pos[id(p)]]
        scale = float(r.abs().max()) + 1e-12
        worst_master = max(worst_master, float((m - r).abs().max()) / scale)
        if kind == "bf16":
            worst_w = max(worst_w, float((p.detach().float() - m.to(torch.bfloat16).float())
                                         .abs().max()))
    res["master_rel"], res["w_vs_master"] = worst_master, worst_w
    res["digest"] = float(torch.cat([p.detach().float().reshape(-1)
                                     for p, _ in params]).double().sum())
    if rule == "lars":
        got = opt.trust
        res["trust_n"] = got.numel()
        res["trust_rel"] = max(abs(float(a) - float(b)) / float(b) for a, b in zip(got, rtrust))
    if rule == "adam":
        res["clock"] = opt.clock.steps()
    res["keys"] = sorted(sd)
    opt.close()
    return res


def _state_bits(opt, params):
    sd = opt.state_dict()
    out = [p.detach().float().clone() for p, _ in params]
    for key in ("master", "momentum_buffer", "mean_square", "exp_avg_sq"):
        out += [t.clone() for t in sd.get(key, [])]
    return out


def _round_trip(rank, world, rule, reduce_fp32, backend, local_size):
    """3 steps straight against 2 steps, save, rebuild from fresh parameters, load, 1 step."""
    pa = _params()
    a = _sharded(rule, pa, reduce_fp32, backend, local_size)
    for step in range(3):
        _step(a, pa, _grads(step, rank, pa), -1)
    want = _state_bits(a, pa)
    a.close()
    pb = _params()
    b = _sharded(rule, pb, reduce_fp32, backend, local_size)
    for step in range(2):
        _step(b, pb, _grads(step, rank, pb), -1)
    sd = b.state_dict()
    b.close()
    pc = _params()
    c = _sharded(rule, pc, reduce_fp32, backend, local_size)
    c.load_state_dict(sd)
    _step(c, pc, _grads(2, rank, pc), -1)
    got = _state_bits(c, pc)
    res = {"same": len(got) == len(want) and all(torch.equal(x, y) for x, y in zip(got, want)),
           "rule": sd.get("rule"), "clock": c.clock.steps() if rule == "adam" else None}
    c.close()
    other = "adam" if rule != "adam" else "lars"
    pd = _params()
    d = _sharded(other, pd, reduce_fp32, backend, local_size)
    try:
        d.load_state_dict(sd)
        res["cross"] = "loaded"
    except ValueError as e:
        res["cross"] = str(e)
    d.close()
    return res


def _run(world, rule, reduce_fp32, backend="rccl", local_size=None, mode="ref"):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, rule, reduce_fp32, backend,
                                               local_size, mode)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(world):
            r, res, err = q.get(timeout=180)
            assert err is None, f"rank {r} failed:\n{err}"
            out[r] = res
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
    return out


@pytest.mark.parametrize("rule", ["rmsprop", "adam", "lars"])
def test_reference_spread_over_summation_orders_leaves_room(rule):
    """The bound of the fp32-sum cases below is tests/test_zero_rccl.py's 1e-5. It has to cover
    what the order of an fp32 sum alone does to the reference: 4 ranks' gradients summed as 0..3
    against 3..0 (measured: rmsprop 1.2e-8, adam 2.4e-8, lars 8.2e-8 of the largest weight),
    which must stay under a quarter of the bound."""
    a, _ = _reference_run(rule, 4, order=[0, 1, 2, 3])
    b, _ = _reference_run(rule, 4, order=[3, 2, 1, 0])
    spread = max(float((x - y).abs().max()) / (float(x.abs().max()) + 1e-12)
                 for x, y in zip(a, b))
    print(f"{rule}: spread over summation orders {spread:.3g}")
    assert spread < 1e-5 / 4


@pytest.mark.parametrize("world,backend,local_size", [(2, "rccl", None), (4, "rccl", None),
                                                      (4, "hier", 2)])
@pytest.mark.parametrize("reduce_fp32", [True, False])
@pytest.mark.parametrize("rule", ["rmsprop", "adam", "lars"])
def test_sharded_rule_matches_single_process_reference(rule, reduce_fp32, world, backend,
                                                       local_size):
    out = _run(world, rule, reduce_fp32, backend, local_size)
    for r, res in out.items():
        assert res["backend"] == backend and res["nbuckets"] >= 3 and res["mixed"] >= 1, res
        # fp32 sums in gloo's order vs the reference's: a few fp32 ulps; bf16 sums round per add
        tol = 1e-5 if reduce_fp32 else 2e-2
        assert res["master_rel"] < tol, (r, res)
        assert res["w_vs_master"] == 0.0, (r, res)         # weights = the rounded masters
        if rule == "lars":
            # against reference_lars_trust on the reference's weights and the fp32 averaged
            # gradient: 1e-5 with fp32 sums; a bf16 sum rounds every gradient element (2^-9), so
            # its norms carry that mode's bound
            assert res["trust_n"] == 4, res
            assert res["trust_rel"] < tol, (r, res)
        if rule == "adam":
            assert res["clock"] == 4, res                  # one tick per step, unused bucket or not
        assert "rule" in res["keys"], res
    assert len({res["digest"] for res in out.values()}) == 1, out     # replicas identical


@pytest.mark.parametrize("rule", ["rmsprop", "adam", "lars"])
def test_state_round_trip(rule):
    out = _run(2, rule, True, mode="trip")
    for r, res in out.items():
        assert res["same"], (r, res)
        assert res["rule"] == rule, res
        assert "cannot load the state of rule" in res["cross"], res
        if rule == "adam":
            assert res["clock"] == 3, res


def test_sgd_rule_keeps_its_state_and_rejects_bad_arguments():
    import torch.distributed as dist
    from arena_amd.parallel.zero import ShardedMasterSGD
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        def p(n=64):
            return torch.nn.Parameter(torch.randn(n).to(torch.bfloat16))
        opt = ShardedMasterSGD([p()], lr=0.1, momentum=0.9, backend="rccl")
        assert opt.rule == "sgd" and opt.aux is None and opt.clock is None
        assert sorted(opt.state_dict()) == ["master", "momentum_buffer", "param_groups", "shapes"]
        assert sorted(opt.param_groups[0]) == ["lr", "momentum", "params", "weight_decay",
                                               "weights"]
        with pytest.raises(AttributeError):
            opt.trust
        opt.close()
        with pytest.raises(ValueError, match="rule must be"):
            ShardedMasterSGD([p()], lr=0.1, rule="adagrad")
        with pytest.raises(ValueError, match="xgmi.*momentum SGD only"):
            ShardedMasterSGD([p()], lr=0.1, rule="lars", backend="xgmi")
        with pytest.raises(ValueError, match="decay must lie"):
            ShardedMasterSGD([p()], lr=0.1, rule="rmsprop", decay=1.0)
        with pytest.raises(ValueError, match="eps must be > 0"):
            ShardedMasterSGD([p()], lr=0.1, rule="adam", eps=0.0)
        with pytest.raises(ValueError, match="beta2 must lie"):
            ShardedMasterSGD([p()], lr=0.1, rule="adam", betas=(0.9, 1.0))
        with pytest.raises(ValueError, match="eeta must be > 0"):
            ShardedMasterSGD([p()], lr=0.1, rule="lars", eeta=0.0)
        with pytest.raises(ValueError, match="LARS param group"):
            ShardedMasterSGD([p(6)], lr=0.1, rule="lars")
        with pytest.raises(ValueError, match="LARS param group"):
            ShardedMasterSGD([{"params": [torch.nn.Parameter(torch.randn(8))], "weights": "fp32",
                               "lars": True}], lr=0.1, rule="lars")
        with pytest.raises(ValueError, match="clock= belongs"):
            ShardedMasterSGD([p()], lr=0.1, rule="lars", clock=optim.AdamClock())
        # the skip list: lars=False groups and fp32 groups take momentum SGD, no trust entry
        opt = ShardedMasterSGD([{"params": [p(), p(8)]}, {"params": [p(6)], "lars": False},
                                {"params": [torch.nn.Parameter(torch.randn(5))],
                                 "weights": "fp32"}], lr=0.1, momentum=0.9, rule="lars")
        assert [g["lars"] for g in opt.param_groups] == [True, False, False]
        assert opt.trust.tolist() == [1.0, 1.0]
        for q in opt.params:
            q.grad = torch.ones_like(q)
        opt.step()
        assert all(0.0 < t < 1.0 for t in opt.trust.tolist())
        opt.close()
    finally:
        dist.destroy_process_group()


def _tiny(*extra):
    from arena_amd.examples import cnn_bench
    return cnn_bench.parse(["--model", "resnet_tiny", "--width", "8", "--image_size", "16",
                            "--batch_size", "2", "--num_classes", "10", "--device", "cpu", *extra])


def test_cnn_bench_shard_optimizer_needs_bf16_on_a_gpu(monkeypatch):
    from arena_amd.examples import cnn_bench
    from arena_amd.parallel import hvd
    cpu = torch.device("cpu")
    for flags in (("--optimizer", "adam"), ("--optimizer", "rmsprop"), ("--lars",)):
        with pytest.raises(SystemExit, match="bf16 on a GPU"):
            cnn_bench.build(_tiny("--shard_optimizer", *flags), cpu, 2)
        with pytest.raises(SystemExit, match="bf16 on a GPU"):
            cnn_bench.build(_tiny("--shard_optimizer", "--dtype", "fp32", *flags), cpu, 2)
    # without the flag: the fp32 optimizer under DistributedOptimizer, as before
    monkeypatch.setattr(hvd, "DistributedOptimizer", lambda opt, **kw: opt)
    _, opt, _, _ = cnn_bench.build(_tiny("--dtype", "fp32", "--optimizer", "adam"), cpu, 2)
    assert type(opt) is optim.TFAdam
    # one rank, or momentum SGD: the flag changes nothing
    _, opt, _, _ = cnn_bench.build(_tiny("--dtype", "fp32", "--optimizer", "adam",
                                         "--shard_optimizer"), cpu, 1)
    assert type(opt) is optim.TFAdam
    assert _tiny().shard_optimizer is False
