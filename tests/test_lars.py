"""LARS on the CPU: the reference of ``arena_amd.ops.reference`` against an independent numpy
evaluation of the definition, ``MasterLARS`` (through the reference path) against ``TFLars``, the
gradient-scale invariance bit for bit, the state round trip, and ``cnn_bench``'s ``--lars``
flags."""
from __future__ import annotations

import argparse
import copy
import math

import numpy as np
import pytest
import torch

from arena_amd.ops import fused, optim
from arena_amd.ops.schedule import DeviceLR, piecewise, with_warmup

BF16 = torch.bfloat16
WD = 4e-5
TOL = dict(rtol=1e-5, atol=1e-6)          # tests/test_optim_family_gpu.py's


# ------------------------------------------------------------------ reference against the formula
def _five():
    """Five small tensors, three steps of bf16 gradients: index 1 has an all-zero gradient at
    every step, index 3 all-zero weights (and no weight decay can revive them before step 2)."""
    g = torch.Generator().manual_seed(21)
    ns = [4, 16, 1028, 8, 260]
    offs = [sum(ns[:i]) for i in range(len(ns))]
    master = torch.randn(sum(ns), generator=g) * 0.1
    master[offs[3]:offs[3] + ns[3]] = 0.0
    steps = []
    for _ in range(3):
        grads = [(torch.randn(n, generator=g) * 0.1).to(BF16) for n in ns]
        grads[1].zero_()
        steps.append(grads)
    return ns, offs, master, steps


def _lars_numpy(w, m, g, lr, mu, wd, eeta, eps):
    """One tensor, one step of the definition: fp64 sums in memory order, fp32 norms, trust and
    step as fp32 operations in the order written; the element-wise update in fp64."""
    f = np.float32
    wn = f(math.sqrt(np.cumsum(w.astype(np.float64) ** 2)[-1]))
    gn = f(math.sqrt(np.cumsum(g.astype(np.float64) ** 2)[-1]))
    trust = f(1.0)
    if wn > 0 and gn > 0:
        trust = f(f(f(eeta) * wn) / f(f(gn + f(f(wd) * wn)) + f(eps)))
    step = f(f(lr) * trust)
    m = float(f(mu)) * m + (g.astype(np.float64) + float(f(wd)) * w)
    w = w - float(step) * m
    return w, m, trust


@pytest.mark.parametrize("eps", [0.0, 1e-6])
def test_reference_matches_the_formula_in_numpy(eps):
    ns, offs, master0, steps = _five()
    lr, mu, eeta = 0.5, 0.9, 0.001
    master, mom = master0.clone(), torch.zeros_like(master0)
    wbf = torch.zeros(master.numel(), dtype=BF16)
    trust = torch.full((len(ns),), -7.0)
    ms = [np.zeros(n) for n in ns]
    for t, grads in enumerate(steps):
        fused.mt_lars_master(grads, offs, master, mom, wbf, trust, list(range(len(ns))),
                             torch.empty(0), lr=lr, momentum=mu, weight_decay=WD, eeta=eeta,
                             eps=eps)
        for i, g in enumerate(grads):
            # the numpy side restarts from the reference's fp32 weights, so both take the norms of
            # the same values and the trust ratios can be compared exactly at every step
            w32 = master0[offs[i]:offs[i] + ns[i]].numpy() if t == 0 else prev[i]
            w, m, tr = _lars_numpy(w32, ms[i], g.float().numpy(), lr, mu, WD, eeta, eps)
            assert np.float32(trust[i].item()) == tr, (t, i, trust[i].item(), tr)
            ms[i] = m
            s = slice(offs[i], offs[i] + ns[i])
            torch.testing.assert_close(master[s], torch.from_numpy(w).float(), **TOL)
            torch.testing.assert_close(mom[s], torch.from_numpy(m).float(), **TOL)
        prev = [master[o:o + n].numpy().copy() for o, n in zip(offs, ns)]
        assert trust[1].item() == 1.0                      # all-zero gradient
        if t == 0:
            assert trust[3].item() == 1.0                  # all-zero weights, non-zero gradient
            assert bool(steps[0][3].float().abs().sum() > 0)
        assert 0.0 < trust[0].item() < 1.0 and trust[0].item() != trust[2].item()
    assert torch.equal(wbf, master.to(BF16))
    assert not torch.equal(master, master0)


def test_reference_leaves_other_trust_entries_alone():
    ns, offs, master, steps = _five()
    mom, wbf = torch.zeros_like(master), torch.zeros(master.numel(), dtype=BF16)
    trust = torch.full((7,), -7.0)
    fused.mt_lars_master(steps[0][2:4], offs[2:4], master, mom, wbf, trust, [5, 0],
                         torch.empty(0), lr=0.1, momentum=0.9)
    assert trust[[1, 2, 3, 4, 6]].tolist() == [-7.0] * 5
    assert 0.0 < trust[5].item() < 1.0 and trust[0].item() == 1.0


# ------------------------------------------------------------------------- MasterLARS / TFLars
def _params():
    g = torch.Generator().manual_seed(0)
    ps = []
    for i, s in enumerate([(16, 3, 3, 3), (32, 16, 1, 1), (8, 8, 3, 3), (10, 32), (8, 4)]):
        t = torch.randn(s, generator=g) * 0.1
        if len(s) == 4 and i % 2 == 0:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(t))
    return ps


def _grad_like(p, generator, scale=1.0):
    g = (torch.randn(p.shape, generator=generator) * scale).to(BF16)
    if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
        g = g.contiguous(memory_format=torch.channels_last)
    return g


def test_master_lars_matches_tf_lars_on_cpu():
    ps = _params()
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = optim.MasterLARS(ps, lr=0.5, momentum=0.9, weight_decay=WD, eeta=0.002, eps=1e-9)
    ropt = optim.TFLars(ref, lr=0.5, momentum=0.9, weight_decay=WD, eeta=0.002, eps=1e-9)
    assert opt.trust.tolist() == [1.0] * len(ps) and opt.trust.dtype == torch.float32
    assert opt.workspace.numel() == fused.mt_lars_workspace_floats([p.numel() for p in ps])
    g = torch.Generator().manual_seed(1)
    for _ in range(3):
        for p, r in zip(ps, ref):
            p.grad = _grad_like(p, g)
            r.grad = p.grad.float()
        opt.step()
        ropt.step()
    for p, r, off, start in zip(ps, ref, opt.offsets, _params()):
        assert p.dtype == BF16 and p.stride() == r.stride()
        m = opt.master.as_strided(p.shape, p.stride(), off)
        torch.testing.assert_close(m, r.detach(), **TOL)
        assert not torch.equal(r.detach(), start.detach())
        assert torch.equal(p, m.to(BF16))
        s = opt.mom.as_strided(p.shape, p.stride(), off)
        torch.testing.assert_close(s, ropt.state[r]["mom"], **TOL)
    assert torch.equal(opt.wbf, opt.master.to(BF16))
    assert all(0.0 < t < 1.0 for t in opt.trust.tolist())


def test_tf_lars_skip_list_group_is_plain_momentum_sgd():
    g = torch.Generator().manual_seed(2)
    a = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(7,), (3, 5)]]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    lars = optim.TFLars([{"params": a[:1], "lars": False, "weight_decay": 0.0},
                         {"params": a[1:], "weight_decay": WD}], lr=0.1, momentum=0.9)
    sgd = torch.optim.SGD(b[:1], lr=0.1, momentum=0.9)
    assert [grp["lars"] for grp in lars.param_groups] == [False, True]
    for _ in range(3):
        for p, q in zip(a, b):
            p.grad = torch.randn(p.shape, generator=g)
            q.grad = p.grad.clone()
        lars.step()
        sgd.step()
    torch.testing.assert_close(a[0].detach(), b[0].detach(), **TOL)
    # the LARS group took steps about eeta * |w| long, far shorter than plain SGD's
    moved = (a[1].detach() - b[1].detach()).norm() / b[1].detach().norm()
    assert 0 < float(moved) < 0.01
    for bad in ({"eeta": 0.0}, {"eps": -1e-9}, {"momentum": 1.0}):
        with pytest.raises(ValueError):
            optim.TFLars(a, lr=0.1, **bad)
    for bad in ({"eeta": 0.0}, {"eeta": -1.0}, {"eps": -1e-9}):
        with pytest.raises(ValueError):
            optim.MasterLARS(_params(), lr=0.1, **bad)


def _scale_run(dev, scale, sizes=(4, 1028, 3076, 40964)):
    """Three MasterLARS steps (no weight decay, eps 0) with every gradient multiplied by
    ``scale``."""
    g = torch.Generator().manual_seed(17)
    ps = [torch.nn.Parameter((torch.randn(n, generator=g) * 0.1).to(dev)) for n in sizes]
    opt = optim.MasterLARS(ps, lr=0.5, momentum=0.9, weight_decay=0.0, eeta=0.001, eps=0.0)
    trusts = []
    for _ in range(3):
        for p in ps:
            p.grad = ((torch.randn(p.shape, generator=g) * 0.1).to(BF16) * scale).to(dev)
            assert p.grad.dtype == BF16
        opt.step()
        trusts.append(opt.trust.clone())
    return opt.master.cpu(), opt.wbf.cpu(), torch.stack(trusts).cpu()


def test_gradient_scale_invariance_bit_for_bit():
    """A power-of-two gradient scale commutes with every rounding of the definition: the norm of g
    scales exactly, trust shrinks by exactly the scale, the momentum grows by it, and step * m is
    the same number. The weights do not see the scale at all."""
    m1, w1, t1 = _scale_run(torch.device("cpu"), 1.0)
    m8, w8, t8 = _scale_run(torch.device("cpu"), 8.0)
    assert torch.equal(m1, m8) and torch.equal(w1, w8)
    assert torch.equal(t8, t1 / 8) and bool((t1 > 0).all()) and bool((t1 < 1).all())


# ---------------------------------------------------------------------------------------- state
def _make(segs):
    ps = _params()
    small = [torch.nn.Parameter(torch.linspace(-1, 1, n)) for n in (16, 7, 1)]
    sched = DeviceLR(segs, "cpu")
    a = optim.MasterLARS(ps, lr=sched, momentum=0.9, weight_decay=WD)
    b = optim.MultiTensorSGD32(small, lr=sched, momentum=0.9)
    return optim.OptimizerGroup(a, b), sched, ps, small


def _steps(group, sched, ps, small, seed, n):
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        for p in ps:
            p.grad = _grad_like(p, g, 0.1)
        for p in small:
            p.grad = torch.randn(p.shape, generator=g)
        sched.advance()
        group.step()


def test_state_round_trip_carries_momentum_hyper_parameters_and_schedule():
    segs = with_warmup(piecewise("0.8;6;0.08", 1), 3, 1)
    group, sched, ps, small = _make(segs)
    group.opts[0].eeta, group.opts[0].eps = 0.002, 1e-9
    _steps(group, sched, ps, small, 4, 4)
    state = copy.deepcopy(group.state_dict())
    st = state["opts"][0]
    assert "trust" not in st and "workspace" not in st
    assert st["eeta"] == 0.002 and st["eps"] == 1e-9 and st["momentum"] == 0.9
    assert len(st["momentum_buffer"]) == len(ps) and "lr_schedule" in st
    weights = [p.detach().clone() for p in small]
    _steps(group, sched, ps, small, 5, 3)

    group2, sched2, ps2, small2 = _make(segs)
    group2.load_state_dict(state)
    with torch.no_grad():
        for p, w in zip(small2, weights):
            p.copy_(w)
    a, a2 = group.opts[0], group2.opts[0]
    assert a2.eeta == 0.002 and a2.eps == 1e-9 and sched2.steps() == 4
    assert a2.trust.tolist() == [1.0] * len(ps2)          # derived at the next step, not loaded
    _steps(group2, sched2, ps2, small2, 5, 3)
    assert torch.equal(a.master, a2.master) and torch.equal(a.wbf, a2.wbf)
    assert torch.equal(a.mom, a2.mom) and torch.equal(a.trust, a2.trust)
    assert torch.equal(group.opts[1].w, group2.opts[1].w)
    assert sched2.steps() == 7 and sched2.value() == sched.value()


# ------------------------------------------------------------------------------------ cnn_bench
def test_cnn_bench_lars_flags_parse():
    from arena_amd.examples import cnn_bench
    a = cnn_bench.parse([])
    assert a.lars is False and a.lars_eeta == 0.001 and a.lars_epsilon == 0.0
    a = cnn_bench.parse(["--lars"])
    assert a.lars is True and a.lars_eeta == 0.001 and a.lars_epsilon == 0.0
    assert a.optimizer == "momentum"
    a = cnn_bench.parse(["--lars", "--lars_eeta", "0.002", "--lars_epsilon", "1e-9"])
    assert a.lars and a.lars_eeta == 0.002 and a.lars_epsilon == 1e-9
    assert cnn_bench.parse(["--lars", "--optimizer", "sgd"]).optimizer == "sgd"


@pytest.mark.parametrize("argv", [
    ["--lars_eeta", "0.002"],
    ["--lars_epsilon", "1e-9"],
    ["--lars", "--optimizer", "rmsprop"],
    ["--lars", "--optimizer", "adam"],
    ["--lars", "--lars_eeta", "0"],
    ["--lars", "--lars_eeta", "-0.001"],
    ["--lars", "--lars_epsilon", "-1e-9"],
    ["--optimizer", "lars"],
])
def test_cnn_bench_rejects_lars_flags(argv, capsys):
    from arena_amd.examples import cnn_bench
    with pytest.raises(SystemExit) as e:
        cnn_bench.parse(argv)
    assert e.value.code == 2
    capsys.readouterr()


def _tiny(*extra):
    from arena_amd.examples import cnn_bench
    return cnn_bench.parse(["--model", "resnet_tiny", "--width", "8", "--image_size", "16",
                            "--batch_size", "2", "--num_classes", "10", "--dtype", "fp32",
                            "--device", "cpu", *extra])


def test_cnn_bench_builds_tf_lars_on_cpu():
    from arena_amd.examples import cnn_bench
    dev = torch.device("cpu")
    model, opt, x, y = cnn_bench.build(_tiny("--lars", "--lars_eeta", "0.002"), dev, 1)
    assert type(opt) is optim.TFLars and cnn_bench.schedule_of(opt) is None
    assert [g["lars"] for g in opt.param_groups] == [True, False]
    assert [g["weight_decay"] for g in opt.param_groups] == [4e-5, 0.0]
    assert [g["eeta"] for g in opt.param_groups] == [0.002, 0.002]
    assert [g["momentum"] for g in opt.param_groups] == [0.9, 0.9]
    assert all(p.ndim > 1 for p in opt.param_groups[0]["params"])
    assert all(p.ndim <= 1 for p in opt.param_groups[1]["params"])
    n = sum(len(g["params"]) for g in opt.param_groups)
    assert n == len(list(model.parameters()))
    loss = float(cnn_bench.train_step(model, opt, x, y, None))
    assert math.isfinite(loss)
    assert cnn_bench.build(_tiny("--lars", "--optimizer", "sgd"), dev, 1)[1].param_groups[0][
        "momentum"] == 0.0
    # without --lars, and from a caller's namespace without the new fields: as before
    assert type(cnn_bench.build(_tiny(), dev, 1)[1]) is torch.optim.SGD
    old = argparse.Namespace(**{k: v for k, v in vars(_tiny()).items()
                                if not k.startswith("lars")})
    assert type(cnn_bench.build(old, dev, 1)[1]) is torch.optim.SGD


def test_cnn_bench_lars_master_weights_on_is_refused_in_data_parallel():
    from arena_amd.examples import cnn_bench
    with pytest.raises(SystemExit, match="momentum SGD only"):
        cnn_bench.build(_tiny("--lars", "--master_weights", "on"), torch.device("cpu"), 2)
