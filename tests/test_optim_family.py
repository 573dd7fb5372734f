"""RMSProp and Adam (TF1's forms) on the CPU: the references of ``arena_amd.ops.reference`` against
an independent fp64 evaluation, Adam's clock reference, the master-weight classes (through the
reference path) against ``TFRMSprop`` / ``TFAdam``, their state round trip, and ``cnn_bench``'s
``--optimizer`` flags."""
from __future__ import annotations

import argparse
import copy
import math

import numpy as np
import pytest
import torch

from arena_amd.ops import fused, optim, reference
from arena_amd.ops.reference import reference_adam_corr

BF16 = torch.bfloat16
WD = 4e-5


# ---------------------------------------------------------------------- references against fp64
def _problem(n=4096, steps=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=g) * 0.1                                  # N(0, 0.1^2)
    grads = [torch.randn(n, generator=g).to(BF16) for _ in range(steps)]   # N(0, 1) through bf16
    return w, grads


def _rmsprop64(w, grads, lr, rho=0.9, mu=0.9, eps=1.0, wd=WD, scale=1.0):
    w = w.double().numpy().copy()
    ms, mom = np.ones_like(w), np.zeros_like(w)
    for g in grads:
        d = g.double().numpy() * scale + wd * w
        ms = rho * ms + (1.0 - rho) * (d * d)
        mom = mu * mom + lr * d / np.sqrt(ms + eps)
        w = w - mom
    return w, ms, mom


def _adam64(w, grads, lr, b1=0.9, b2=0.999, eps=1e-8, wd=WD, scale=1.0):
    w = w.double().numpy().copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    for t, g in enumerate(grads, 1):
        d = g.double().numpy() * scale + wd * w
        m = b1 * m + (1.0 - b1) * d
        v = b2 * v + (1.0 - b2) * (d * d)
        corr = math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        w = w - (lr * corr) * m / (np.sqrt(v) + eps)
    return w, m, v


def _close(got, want64):
    torch.testing.assert_close(got, torch.from_numpy(want64).float(), rtol=1e-5, atol=1e-6)


def test_rmsprop_references_match_fp64():
    w0, grads = _problem()
    n = w0.numel()
    # master form: bf16 gradients, rounded bf16 weights out
    w, ms, mom, wbf = w0.clone(), torch.ones(n), torch.zeros(n), torch.zeros(n, dtype=BF16)
    for g in grads:
        fused.mt_rmsprop_master([g], [0], w, ms, mom, wbf, lr=0.01, weight_decay=WD)
    want = _rmsprop64(w0, grads, 0.01)
    for got, ref in zip((w, ms, mom), want):
        _close(got, ref)
    assert torch.equal(wbf, w.to(BF16))
    # fp32 form, gradients scaled by 0.5
    w, ms, mom = w0.clone(), torch.ones(n), torch.zeros(n)
    for g in grads:
        fused.mt_rmsprop_f32([g.float()], [0], w, ms, mom, lr=0.01, weight_decay=WD, scale=0.5)
    for got, ref in zip((w, ms, mom), _rmsprop64(w0, grads, 0.01, scale=0.5)):
        _close(got, ref)


def test_adam_references_match_fp64():
    w0, grads = _problem()
    n = w0.numel()
    clock = optim.AdamClock((0.9, 0.999), "cpu")
    w, m, v, wbf = w0.clone(), torch.zeros(n), torch.zeros(n), torch.zeros(n, dtype=BF16)
    for g in grads:
        clock.tick()
        fused.mt_adam_master([g], [0], w, m, v, wbf, clock.corr, lr=0.001, weight_decay=WD)
    for got, ref in zip((w, m, v), _adam64(w0, grads, 0.001)):
        _close(got, ref)
    assert torch.equal(wbf, w.to(BF16)) and clock.steps() == len(grads)
    clock = optim.AdamClock((0.9, 0.999), "cpu")
    w, m, v = w0.clone(), torch.zeros(n), torch.zeros(n)
    for g in grads:
        clock.tick()
        fused.mt_adam_f32([g.float()], [0], w, m, v, clock.corr, lr=0.001, weight_decay=WD,
                          scale=0.5)
    for got, ref in zip((w, m, v), _adam64(w0, grads, 0.001, scale=0.5)):
        _close(got, ref)


def test_device_lr_value_replaces_the_float():
    """``lr_t`` wins over ``lr`` in the references, as in the kernels."""
    w0, grads = _problem(n=64, steps=2)
    lr_t = torch.tensor([0.01], dtype=torch.float32)
    outs = []
    for kw in ({"lr": 0.01}, {"lr": 123.0, "lr_t": lr_t}):
        w, ms, mom, wbf = w0.clone(), torch.ones(64), torch.zeros(64), torch.zeros(64, dtype=BF16)
        for g in grads:
            fused.mt_rmsprop_master([g], [0], w, ms, mom, wbf, weight_decay=WD, **kw)
        outs.append(w)
    assert torch.equal(*outs)
    with pytest.raises(ValueError, match="lr_t"):
        fused.mt_rmsprop_master([grads[0]], [0], w, ms, mom, wbf, lr=0.1, lr_t=lr_t.double())


# -------------------------------------------------------------------------------- Adam's clock
def test_adam_clock_reference():
    b1, b2 = 0.9, 0.999
    for t in range(1, 2001):
        want = math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        got = float(reference_adam_corr(b1, b2, t))
        assert abs(got - want) <= 1e-6 * want, (t, got, want)
    assert reference_adam_corr(b1, b2, 1).dtype == np.float32
    # once both powers have underflowed the correction is exactly 1
    assert 0.5 ** 1100 == 0.0
    assert reference_adam_corr(0.5, 0.5, 1200) == np.float32(1.0)
    with pytest.raises(ValueError):
        reference_adam_corr(b1, b2, 0)


def test_adam_clock_on_cpu_follows_the_reference():
    clock = optim.AdamClock((0.9, 0.999), "cpu")
    assert clock.pow.dtype == torch.float64 and clock.step.dtype == torch.int64
    for t in range(1, 41):
        clock.tick()
        want = reference_adam_corr(0.9, 0.999, t)
        assert clock.corr.numpy().view(np.int32)[0] == want.view(np.int32), t
    assert clock.steps() == 40
    with pytest.raises(ValueError):
        optim.AdamClock((0.9, 1.0), "cpu")


# ------------------------------------------------------------ optimizer classes on CPU tensors
def _params():
    g = torch.Generator().manual_seed(0)
    ps = []
    for i, s in enumerate([(16, 3, 3, 3), (32, 16, 1, 1), (8, 8, 3, 3), (10, 32), (8, 4)]):
        t = torch.randn(s, generator=g) * 0.1
        if len(s) == 4 and i % 2 == 0:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(t))
    return ps


def _grad_like(p, generator):
    g = torch.randn(p.shape, generator=generator).to(BF16)
    if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
        g = g.contiguous(memory_format=torch.channels_last)
    return g


FAMILY = {
    "rmsprop": (optim.MasterRMSprop, optim.TFRMSprop, {"lr": 0.01}, ("ms", "mom")),
    "adam": (optim.MasterAdam, optim.TFAdam, {"lr": 0.001}, ("m", "v")),
}


@pytest.mark.parametrize("name", ["rmsprop", "adam"])
def test_master_class_matches_plain_class_on_cpu(name):
    master_cls, plain_cls, kw, keys = FAMILY[name]
    ps = _params()
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = master_cls(ps, weight_decay=WD, **kw)
    ropt = plain_cls(ref, weight_decay=WD, **kw)
    g = torch.Generator().manual_seed(1)
    for _ in range(5):
        for p, r in zip(ps, ref):
            p.grad = _grad_like(p, g)
            r.grad = p.grad.float()
        opt.step()
        ropt.step()
    for p, r, off in zip(ps, ref, opt.offsets):
        assert p.dtype == BF16 and p.stride() == r.stride()
        m = opt.master.as_strided(p.shape, p.stride(), off)
        torch.testing.assert_close(m, r.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(p.float(), r.detach(), rtol=1e-2, atol=1e-3)
        assert torch.equal(p, m.to(BF16))
        for attr, key in zip(opt._STATE, keys):
            s = getattr(opt, attr[0]).as_strided(p.shape, p.stride(), off)
            torch.testing.assert_close(s, ropt.state[r][key], rtol=1e-5, atol=1e-6)
    if name == "adam":
        assert opt.clock.steps() == 5 and int(ropt.step_count) == 5
        assert torch.equal(opt.clock.corr, ropt.corr) and torch.equal(opt.clock.pow, ropt.pow)


def test_fp32_group_classes_share_the_clock_and_check_their_arguments():
    ps = _params()
    small = [torch.nn.Parameter(torch.randn(n)) for n in (16, 7, 1)]
    a = optim.MasterAdam(ps, lr=0.001)
    b = optim.MultiTensorAdam32(small, lr=0.001, clock=a.clock)
    group = optim.OptimizerGroup(a, b)
    g = torch.Generator().manual_seed(2)
    before = [p.detach().clone() for p in small]
    for _ in range(3):
        for p in ps:
            p.grad = _grad_like(p, g)
        for p in small:
            p.grad = torch.randn(p.shape, generator=g)
        group.step()
    assert a.clock.steps() == 3                      # one tick per step, by the clock's owner
    assert all(not torch.equal(p, q) for p, q in zip(small, before))
    assert all(p.data_ptr() == v.data_ptr() for p, v in zip(small, b._views(b.w)))
    # first Adam steps move every weight by about lr, whatever the gradient's size
    for p, q in zip(small, before):
        assert float((p.detach() - q).abs().max()) <= 3 * 0.001 * 1.01
    with pytest.raises(ValueError, match="betas"):
        optim.MultiTensorAdam32(small, lr=0.001, betas=(0.8, 0.999), clock=a.clock)
    assert small[0].grad is not None and small[0].data_ptr() == b.w.data_ptr()   # untouched
    small[0].data = small[0].data.clone()            # as a weight load re-binds it
    with pytest.raises(RuntimeError, match="re-bound"):
        b.step()
    b.sync_from_params()
    b.step()
    r = optim.MultiTensorRMSprop32([torch.nn.Parameter(torch.randn(5))], lr=0.01)
    assert torch.equal(r.ms[:5], torch.ones(5)) and not r.mom.any()
    with pytest.raises(ValueError):
        optim.MasterRMSprop(_params(), lr=0.01, decay=1.0)
    with pytest.raises(ValueError):
        optim.MasterAdam(_params(), lr=0.01, eps=0.0)
    with pytest.raises(ValueError):
        optim.MasterRMSprop([torch.nn.Parameter(torch.zeros(3))], lr=0.1)   # numel % 4


# ---------------------------------------------------------------------------- state round trip
def _make(name):
    master_cls = FAMILY[name][0]
    fp32_cls = optim.MultiTensorRMSprop32 if name == "rmsprop" else optim.MultiTensorAdam32
    ps = _params()
    small = [torch.nn.Parameter(torch.linspace(-1, 1, n)) for n in (16, 7, 1)]
    a = master_cls(ps, weight_decay=WD, **FAMILY[name][2])
    extra = {"clock": a.clock} if name == "adam" else {}
    b = fp32_cls(small, **FAMILY[name][2], **extra)
    return optim.OptimizerGroup(a, b), ps, small


def _steps(group, ps, small, seed, n):
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        for p in ps:
            p.grad = _grad_like(p, g)
        for p in small:
            p.grad = torch.randn(p.shape, generator=g)
        group.step()


@pytest.mark.parametrize("name", ["rmsprop", "adam"])
def test_state_round_trip_reproduces_the_next_steps(name):
    group, ps, small = _make(name)
    _steps(group, ps, small, 4, 4)
    state = copy.deepcopy(group.state_dict())
    weights = [p.detach().clone() for p in small]     # the fp32 weights are the model's state
    _steps(group, ps, small, 5, 3)

    group2, ps2, small2 = _make(name)
    group2.load_state_dict(state)
    with torch.no_grad():
        for p, w in zip(small2, weights):
            p.copy_(w)
    if name == "adam":
        assert group2.opts[0].clock.steps() == 4
        assert torch.equal(group2.opts[0].clock.pow, torch.tensor(state["opts"][0]["clock"]["pow"],
                                                                  dtype=torch.float64))
    _steps(group2, ps2, small2, 5, 3)
    a, a2 = group.opts[0], group2.opts[0]
    assert torch.equal(a.master, a2.master) and torch.equal(a.wbf, a2.wbf)
    for attr, _, _ in a._STATE:
        assert torch.equal(getattr(a, attr), getattr(a2, attr))
        assert torch.equal(getattr(group.opts[1], attr), getattr(group2.opts[1], attr))
    assert torch.equal(group.opts[1].w, group2.opts[1].w)
    if name == "adam":
        assert a2.clock.steps() == 7
        assert torch.equal(a.clock.pow, a2.clock.pow) and torch.equal(a.clock.corr, a2.clock.corr)


@pytest.mark.parametrize("name", ["rmsprop", "adam"])
def test_state_of_other_parameters_is_refused(name):
    master_cls, _, kw, _ = FAMILY[name]
    fp32_cls = optim.MultiTensorRMSprop32 if name == "rmsprop" else optim.MultiTensorAdam32
    a = [torch.nn.Parameter(torch.zeros(8, 4)), torch.nn.Parameter(torch.zeros(4, 8))]
    b = [torch.nn.Parameter(torch.zeros(4, 8)), torch.nn.Parameter(torch.zeros(8, 4))]
    st = master_cls(a, **kw).state_dict()
    with pytest.raises(ValueError, match="shape"):
        master_cls(b, **kw).load_state_dict(st)
    with pytest.raises(ValueError, match="2 masters"):
        master_cls(b[:1], **kw).load_state_dict(st)
    a = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(5))]
    b = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3))]
    st = fp32_cls(a, **kw).state_dict()
    with pytest.raises(ValueError, match="shape"):
        fp32_cls(b, **kw).load_state_dict(st)
    with pytest.raises(ValueError, match="for 1 parameters"):
        fp32_cls(b[:1], **kw).load_state_dict(st)


def test_plain_adam_state_round_trip():
    def make():
        ps = [torch.nn.Parameter(torch.linspace(-1, 1, n)) for n in (6, 3)]
        return ps, optim.TFAdam(ps, lr=0.01, weight_decay=WD)

    def steps(ps, opt, seed, n):
        g = torch.Generator().manual_seed(seed)
        for _ in range(n):
            for p in ps:
                p.grad = torch.randn(p.shape, generator=g)
            opt.step()

    ps, opt = make()
    steps(ps, opt, 1, 3)
    state = copy.deepcopy(opt.state_dict())
    weights = [p.detach().clone() for p in ps]
    steps(ps, opt, 2, 3)
    ps2, opt2 = make()
    opt2.load_state_dict(state)
    with torch.no_grad():
        for p, w in zip(ps2, weights):
            p.copy_(w)
    steps(ps2, opt2, 2, 3)
    assert all(torch.equal(p, q) for p, q in zip(ps, ps2))
    assert int(opt2.step_count) == 6 and torch.equal(opt.pow, opt2.pow)


@pytest.mark.parametrize("cls", [optim.TFRMSprop, optim.TFAdam])
def test_plain_classes_read_lr_from_param_groups_every_step(cls):
    """The host-side schedule path writes ``param_groups[i]["lr"]`` before each step."""
    def run(lrs):
        p = torch.nn.Parameter(torch.linspace(-1, 1, 8))
        opt = cls([p], lr=lrs[0])
        for lr in lrs:
            for g in opt.param_groups:
                g["lr"] = lr
            p.grad = torch.linspace(1, 2, 8)
            opt.step()
        return p.detach().clone()

    assert not torch.equal(run([0.01, 0.01]), run([0.01, 0.001]))
    assert torch.equal(run([0.01, 0.001]), run([0.01, 0.001]))


# ----------------------------------------------------------------------------------- cnn_bench
def test_cnn_bench_optimizer_flags_parse():
    from arena_amd.examples import cnn_bench
    a = cnn_bench.parse([])
    assert a.optimizer == "momentum" and a.momentum == 0.9
    assert (a.rmsprop_decay, a.rmsprop_momentum, a.rmsprop_epsilon) == (0.9, 0.9, 1.0)
    assert (a.adam_beta1, a.adam_beta2, a.adam_epsilon) == (0.9, 0.999, 1e-8)
    a = cnn_bench.parse(["--optimizer", "rmsprop", "--rmsprop_decay", "0.95",
                         "--rmsprop_momentum", "0", "--rmsprop_epsilon", "0.1"])
    assert (a.optimizer, a.rmsprop_decay, a.rmsprop_momentum, a.rmsprop_epsilon) == (
        "rmsprop", 0.95, 0.0, 0.1)
    a = cnn_bench.parse(["--optimizer", "adam", "--adam_beta1", "0.8", "--adam_beta2", "0.99",
                         "--adam_epsilon", "1e-6"])
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_epsilon) == ("adam", 0.8, 0.99, 1e-6)
    assert cnn_bench.parse(["--optimizer", "sgd"]).optimizer == "sgd"


@pytest.mark.parametrize("argv", [
    ["--rmsprop_decay", "0.9"],                                  # momentum: no RMSProp flags
    ["--optimizer", "adam", "--rmsprop_epsilon", "1.0"],
    ["--optimizer", "sgd", "--rmsprop_momentum", "0.5"],
    ["--adam_beta1", "0.9"],
    ["--optimizer", "rmsprop", "--adam_beta2", "0.99"],
    ["--optimizer", "rmsprop", "--adam_epsilon", "1e-8"],
    ["--optimizer", "rmsprop", "--rmsprop_decay", "1.0"],
    ["--optimizer", "rmsprop", "--rmsprop_decay", "-0.1"],
    ["--optimizer", "rmsprop", "--rmsprop_momentum", "1.5"],
    ["--optimizer", "rmsprop", "--rmsprop_epsilon", "0"],
    ["--optimizer", "adam", "--adam_beta1", "1.0"],
    ["--optimizer", "adam", "--adam_beta2", "-1"],
    ["--optimizer", "adam", "--adam_epsilon", "-1e-8"],
    ["--optimizer", "lars"],
])
def test_cnn_bench_rejects_optimizer_flags(argv, capsys):
    from arena_amd.examples import cnn_bench
    with pytest.raises(SystemExit) as e:
        cnn_bench.parse(argv)
    assert e.value.code == 2
    assert "error" in capsys.readouterr().err


def _tiny(*extra):
    from arena_amd.examples import cnn_bench
    return cnn_bench.parse(["--model", "resnet_tiny", "--width", "8", "--image_size", "16",
                            "--batch_size", "2", "--num_classes", "10", "--dtype", "fp32",
                            "--device", "cpu", *extra])


def test_cnn_bench_builds_the_chosen_optimizer_on_cpu():
    from arena_amd.examples import cnn_bench
    dev = torch.device("cpu")
    model, opt, x, y = cnn_bench.build(_tiny(), dev, 1)
    assert type(opt) is torch.optim.SGD                              # unchanged
    assert [g["momentum"] for g in opt.param_groups] == [0.9, 0.9]
    assert [g["weight_decay"] for g in opt.param_groups] == [4e-5, 0.0]
    _, opt, _, _ = cnn_bench.build(_tiny("--optimizer", "sgd"), dev, 1)
    assert type(opt) is torch.optim.SGD and opt.param_groups[0]["momentum"] == 0.0
    # a caller's namespace without the new fields (as before this flag) still builds momentum SGD
    old = argparse.Namespace(**{k: v for k, v in vars(_tiny()).items()
                                if k != "optimizer" and not k.startswith(("rmsprop", "adam"))})
    assert type(cnn_bench.build(old, dev, 1)[1]) is torch.optim.SGD

    _, opt, _, _ = cnn_bench.build(_tiny("--optimizer", "rmsprop", "--rmsprop_decay", "0.95"),
                                   dev, 1)
    assert type(opt) is optim.TFRMSprop and cnn_bench.schedule_of(opt) is None
    assert [g["weight_decay"] for g in opt.param_groups] == [4e-5, 0.0]
    assert opt.param_groups[0]["decay"] == 0.95 and opt.param_groups[0]["eps"] == 1.0

    model, opt, x, y = cnn_bench.build(_tiny("--optimizer", "adam", "--learning_rate", "0.001"),
                                       dev, 1)
    assert type(opt) is optim.TFAdam and opt.betas == (0.9, 0.999)
    assert opt.param_groups[0]["lr"] == 0.001 and opt.param_groups[1]["eps"] == 1e-8
    first = float(cnn_bench.train_step(model, opt, x, y, None))
    for _ in range(5):
        last = float(cnn_bench.train_step(model, opt, x, y, None))
    assert math.isfinite(last) and last < first          # one static batch: Adam fits it
    assert int(opt.step_count) == 6


def test_cnn_bench_master_weights_on_needs_momentum_sgd_in_data_parallel():
    from arena_amd.examples import cnn_bench
    for name in ("rmsprop", "adam"):
        with pytest.raises(SystemExit, match="momentum SGD only"):
            cnn_bench.build(_tiny("--optimizer", name, "--master_weights", "on"),
                            torch.device("cpu"), 2)


def test_schedule_of_finds_the_device_lr_in_the_new_classes():
    from arena_amd.examples import cnn_bench
    from arena_amd.ops.schedule import DeviceLR, constant
    sched = DeviceLR(constant(0.01), "cpu")
    ps = _params()
    small = [torch.nn.Parameter(torch.zeros(3))]
    a = optim.MasterAdam(ps, lr=sched)
    group = optim.OptimizerGroup(a, optim.MultiTensorAdam32(small, lr=sched, clock=a.clock))
    assert cnn_bench.schedule_of(group) is sched
    assert cnn_bench.schedule_of(optim.MasterRMSprop(_params(), lr=sched)) is sched
    assert cnn_bench.schedule_of(optim.MasterRMSprop(_params(), lr=0.1)) is None
    assert "lr_schedule" in a.state_dict()
