"""Learning-rate schedules (``arena_amd.ops.schedule``) on the CPU: the builders and the reference
definition, ``DeviceLR`` and the optimizers that read it, checkpoints, and ``cnn_bench``'s flags.
The HIP side (``arena_lr_schedule``, the ``lr_ptr`` forms, graph replay) is in
``tests/test_lr_schedule_gpu.py``."""
import contextlib
import io
import json
import re

import numpy as np
import pytest
import torch

from arena_amd.ops import schedule
from arena_amd.ops.optim import MasterSGD, MultiTensorSGD32, OptimizerGroup
from arena_amd.ops.schedule import DeviceLR, reference_lr

SPE = 4


def _recipe():
    return schedule.with_warmup(schedule.piecewise("0.1;2;0.01;3;0.001", SPE), 1, SPE)


def test_piecewise_with_warmup_matches_hand_written_values():
    segs = _recipe()
    assert segs == [(0, 4, 0.0, 0.1), (4, 8, 0.1, 0.1), (8, 12, 0.01, 0.01),
                    (12, None, 0.001, 0.001)]
    want = [0, .025, .05, .075] + [.1] * 4 + [.01] * 4 + [.001] * 4
    got = [reference_lr(segs, t) for t in range(16)]
    assert all(isinstance(v, np.float32) for v in got)
    assert got == [np.float32(v) for v in want]
    assert reference_lr(segs, 10 ** 9) == np.float32(.001)


def test_warmup_replaces_the_base_schedule_below_it():
    # the warm-up (6 steps) swallows the first boundary (4): the ramp still aims at the first value
    segs = schedule.with_warmup(schedule.piecewise("0.4;1;0.04;3;0.004", SPE), 1.5, SPE)
    assert segs == [(0, 6, 0.0, 0.4), (6, 12, 0.04, 0.04), (12, None, 0.004, 0.004)]
    assert reference_lr(segs, 3) == np.float32(0.4 * (3 / 6))
    assert schedule.with_warmup(schedule.constant(0.1), 0, SPE) == [(0, None, 0.1, 0.1)]


def test_exponential_staircase():
    segs = schedule.exponential(.1, 1, .5, .02, steps_per_epoch=1, total_steps=5)
    assert [reference_lr(segs, t) for t in range(5)] == \
        [np.float32(v) for v in (.1, .05, .025, .02, .02)]
    # decay_steps = int(epochs * steps_per_epoch); the stairs stop where the run does
    segs = schedule.exponential(.1, 2.5, .5, 0.0, steps_per_epoch=SPE, total_steps=25)
    assert [s[0] for s in segs] == [0, 10, 20]
    assert reference_lr(segs, 19) == np.float32(.05) and reference_lr(segs, 20) == np.float32(.025)


def test_invalid_schedules_raise():
    with pytest.raises(ValueError, match="at most 64"):
        schedule.validate([(i, i + 1, .1, .1) for i in range(64)] + [(64, None, .1, .1)])
    schedule.validate([(i, i + 1, .1, .1) for i in range(63)] + [(63, None, .1, .1)])
    with pytest.raises(ValueError, match="at most 64"):
        schedule.piecewise(";".join(["0.1"] + [f"{i};0.1" for i in range(1, 66)]), SPE)
    with pytest.raises(ValueError, match="more than 64"):
        schedule.exponential(.1, 1, .99, 0.0, steps_per_epoch=1, total_steps=1000)
    with pytest.raises(ValueError, match="increase"):
        schedule.piecewise("0.1;2;0.01;1;0.001", SPE)
    with pytest.raises(ValueError, match="increase"):
        schedule.piecewise("0.1;0.1;0.01;0.2;0.001", SPE)      # both boundaries at step 0
    with pytest.raises(ValueError, match="begin where"):
        schedule.validate([(0, 4, .1, .1), (5, None, .1, .1)])
    for bad in (float("nan"), float("inf"), -0.1):
        with pytest.raises(ValueError, match="finite"):
            schedule.constant(bad)
    with pytest.raises(ValueError, match="odd number"):
        schedule.piecewise("0.1;2", SPE)


def test_device_table_round_trips_the_fp64_values():
    segs = _recipe()
    assert schedule.decode(schedule.encode(segs, "cpu")) == segs


def test_device_lr_on_cpu_runs_the_reference():
    segs = _recipe()
    s = DeviceLR(segs, "cpu")
    assert s.lr.dtype == torch.float32 and s.lr.shape == (1,)
    assert s.step.dtype == torch.int64 and s.step.shape == (1,)
    for t in range(14):
        s.advance()
        assert s.lr.numpy()[0] == reference_lr(segs, t) and s.steps() == t + 1


# ------------------------------------------------------------------------------- optimizers
def _bf16_params():
    g = torch.Generator().manual_seed(0)
    ps = []
    for i, shp in enumerate([(16, 3, 3, 3), (32, 16, 1, 1), (10, 32), (8, 4)]):
        t = torch.randn(shp, generator=g) * 0.05
        if len(shp) == 4 and i % 2 == 0:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(t))
    return ps


def _f32_params():
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (16, 7, 1, 33, 10)]


def _like(gr, p):
    cl = p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last)
    return gr.contiguous(memory_format=torch.channels_last) if cl else gr


def _set_grads(gen, ps, refs, dtype):
    for p, r in zip(ps, refs):
        gr = _like(torch.randn(r.shape, generator=gen).to(dtype), p)
        p.grad = gr
        if r is not p:
            r.grad = gr.float()


def test_optimizers_follow_the_schedule_like_torch_sgd():
    """12 steps of the recipe: MasterSGD / MultiTensorSGD32 reading a DeviceLR against
    torch.optim.SGD whose lr the host sets to reference_lr(t) each step (tests/test_optim.py's
    tolerances for MasterSGD)."""
    segs = _recipe()
    sched = DeviceLR(segs, "cpu")
    ps, qs = _bf16_params(), _f32_params()
    rps = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    rqs = [torch.nn.Parameter(q.detach().clone()) for q in qs]
    opt = OptimizerGroup(MasterSGD(ps, lr=sched, momentum=0.9, weight_decay=4e-5),
                         MultiTensorSGD32(qs, lr=sched, momentum=0.9))
    ropt = torch.optim.SGD([{"params": rps, "weight_decay": 4e-5},
                            {"params": rqs, "weight_decay": 0.0}], lr=1.0, momentum=0.9)
    gen = torch.Generator().manual_seed(1)
    for t in range(12):
        sched.advance()
        for grp in ropt.param_groups:
            grp["lr"] = float(reference_lr(segs, t))
        _set_grads(gen, ps, rps, torch.bfloat16)
        _set_grads(gen, qs, rqs, torch.float32)
        opt.step()
        ropt.step()
    msgd = opt.opts[0]
    for p, r, off in zip(ps, rps, msgd.offsets):
        m = msgd.master.as_strided(p.shape, p.stride(), off)
        torch.testing.assert_close(m, r.detach(), rtol=1e-5, atol=1e-6)
        assert torch.equal(p, m.to(torch.bfloat16))
    for q, r in zip(qs, rqs):
        assert q.dtype == torch.float32
        torch.testing.assert_close(q.detach(), r.detach(), rtol=1e-5, atol=1e-6)
    assert not torch.equal(rqs[0].detach(), _f32_params()[0].detach())   # it did train


def test_multi_tensor_sgd32_checks_and_reference_order():
    from arena_amd.ops import fused
    with pytest.raises(ValueError):
        MultiTensorSGD32([], lr=0.1)
    with pytest.raises(ValueError, match="fp32"):
        MultiTensorSGD32([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))], lr=0.1)
    with pytest.raises(ValueError, match="lr_t"):
        fused.mt_sgd_f32([torch.ones(4)], [0], torch.zeros(4), torch.zeros(4), lr=0.1,
                         momentum=0.0, lr_t=torch.zeros(2))
    # d = g * scale + wd * w; m = mu * m + d; w -= lr * m, on the named segments only
    w, m = torch.full((12,), 2.0), torch.full((12,), 1.0)
    fused.mt_sgd_f32([torch.full((3,), 4.0), torch.full((2,), 8.0)], [1, 8], w, m, lr=0.5,
                     momentum=0.5, weight_decay=0.25, scale=0.5)
    assert m.tolist() == [1, 3, 3, 3, 1, 1, 1, 1, 5, 5, 1, 1]
    assert w.tolist() == [2, .5, .5, .5, 2, 2, 2, 2, -.5, -.5, 2, 2]


def test_schedule_and_optimizer_state_round_trip():
    segs = _recipe()

    def make():
        sched = DeviceLR(segs, "cpu")
        ps, qs = _bf16_params(), _f32_params()
        return sched, ps, qs, OptimizerGroup(MasterSGD(ps, lr=sched, momentum=0.9),
                                             MultiTensorSGD32(qs, lr=sched, momentum=0.9))

    sched, ps, qs, opt = make()
    gen = torch.Generator().manual_seed(2)
    for _ in range(7):
        sched.advance()
        _set_grads(gen, ps, ps, torch.bfloat16)
        _set_grads(gen, qs, qs, torch.float32)
        opt.step()
    st = opt.state_dict()
    assert st["opts"][0]["lr_schedule"] == {"step": 7, "segments": [list(s) for s in segs]}
    # into a schedule that was built differently: the checkpoint's segments and step win
    sched2 = DeviceLR(schedule.constant(0.5), "cpu")
    ps2, qs2 = _bf16_params(), _f32_params()
    opt2 = OptimizerGroup(MasterSGD(ps2, lr=sched2, momentum=0.9),
                          MultiTensorSGD32(qs2, lr=sched2, momentum=0.9))
    for q, q2 in zip(qs, qs2):            # fp32 weights are the model's state, not the optimizer's
        q2.data.copy_(q.data)
    opt2.load_state_dict(st)
    assert sched2.segments == segs and sched2.steps() == 7
    assert sched2.lr.numpy()[0] == reference_lr(segs, 6)
    assert torch.equal(opt2.opts[0].mom, opt.opts[0].mom)
    assert torch.equal(opt2.opts[1].mom, opt.opts[1].mom)
    for s_, o_, a, b in ((sched, opt, ps, qs), (sched2, opt2, ps2, qs2)):
        s_.advance()
        gen_ = torch.Generator().manual_seed(9)
        _set_grads(gen_, a, a, torch.bfloat16)
        _set_grads(gen_, b, b, torch.float32)
        o_.step()
    assert sched2.lr.numpy()[0] == sched.lr.numpy()[0] == reference_lr(segs, 7)
    for a, b in zip(ps + qs, ps2 + qs2):
        assert torch.equal(a, b)
    # a checkpoint from before schedules existed: the schedule starts over
    old = {k: v for k, v in st["opts"][0].items() if k != "lr_schedule"}
    opt2.opts[0].load_state_dict(old)
    assert sched2.steps() == 0 and sched2.lr.numpy()[0] == reference_lr(segs, 0)
    # DeviceLR alone
    s3 = DeviceLR(segs, "cpu")
    s3.load_state_dict(sched.state_dict())
    s3.advance()
    assert s3.lr.numpy()[0] == reference_lr(segs, 8)


# --------------------------------------------------------------------------------- cnn_bench
def test_cnn_bench_parse_schedule_flags(capsys):
    from arena_amd.examples import cnn_bench
    a = cnn_bench.parse([])
    assert not cnn_bench.has_schedule(a) and cnn_bench.schedule_segments(a, 10, 100) is None
    a = cnn_bench.parse(["--piecewise_learning_rate_schedule", "0.4;30;0.04;60;0.004;80;0.0004",
                         "--num_learning_rate_warmup_epochs", "5"])
    segs = cnn_bench.schedule_segments(a, 10, 900)
    assert segs == [(0, 50, 0.0, 0.4), (50, 300, 0.4, 0.4), (300, 600, 0.04, 0.04),
                    (600, 800, 0.004, 0.004), (800, None, 0.0004, 0.0004)]
    a = cnn_bench.parse(["--init_learning_rate", "0.2", "--num_epochs_per_decay", "2",
                         "--learning_rate_decay_factor", "0.5", "--minimum_learning_rate", "0.05"])
    assert [s[2] for s in cnn_bench.schedule_segments(a, 10, 1000)] == [0.2, 0.1, 0.05]
    a = cnn_bench.parse(["--learning_rate", "0.3", "--num_learning_rate_warmup_epochs", "1"])
    assert cnn_bench.schedule_segments(a, 10, 100) == [(0, 10, 0.0, 0.3), (10, None, 0.3, 0.3)]
    for extra in (["--init_learning_rate", "0.1"], ["--num_epochs_per_decay", "2"],
                  ["--learning_rate_decay_factor", "0.5"], ["--minimum_learning_rate", "0.01"]):
        with pytest.raises(SystemExit):
            cnn_bench.parse(["--piecewise_learning_rate_schedule", "0.1;2;0.01"] + extra)
    with pytest.raises(SystemExit):
        cnn_bench.parse(["--num_epochs_per_decay", "2"])          # no decay factor
    capsys.readouterr()


_RUN = ["--device", "cpu", "--model", "resnet18", "--width", "8", "--image_size", "32",
        "--batch_size", "4", "--synth_images", "16", "--num_epochs", "3", "--num_classes", "10",
        "--num_warmup_batches", "1", "--display_every", "1", "--json"]


def _main(argv):
    from arena_amd.examples import cnn_bench
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = cnn_bench.main(argv)
    return rc, out.getvalue()


def test_cnn_bench_cpu_run_prints_the_schedule():
    """16 images / batch 4: 4 steps per epoch, 12 steps; a 1-epoch warm-up and one boundary."""
    rc, out = _main(_RUN + ["--piecewise_learning_rate_schedule", "0.1;2;0.01",
                            "--num_learning_rate_warmup_epochs", "1"])
    assert rc == 0, out
    segs = schedule.with_warmup(schedule.piecewise("0.1;2;0.01", SPE), 1, SPE)
    lrs = {int(m.group(1)): m.group(2)
           for m in re.finditer(r"^(\d+)\timages/sec.*  lr (\d\.\d{6})$", out, re.M)}
    assert lrs == {i: f"{float(reference_lr(segs, i - 1)):.6f}" for i in range(1, 13)}, out
    res = json.loads(out.strip().splitlines()[-1])
    assert res["final_lr"] == float(reference_lr(segs, 11))
    assert res["lr_schedule"] == [list(s) for s in segs]
    assert res["exec"] == "eager"


def test_default_cnn_bench_run_builds_no_schedule(monkeypatch):
    """Without a schedule flag nothing of the feature runs: no DeviceLR, no schedule launch, the
    BN / bias group on torch.optim.SGD, no lr column."""
    from arena_amd.ops import fused, reference

    def boom(*a, **k):
        raise AssertionError("the default run touched the learning-rate schedule")

    monkeypatch.setattr(schedule.DeviceLR, "__init__", boom)
    monkeypatch.setattr(fused, "lr_schedule", boom)
    monkeypatch.setattr(reference, "lr_schedule", boom)
    rc, out = _main(_RUN[:-1] + ["--num_epochs", "1", "--json"])
    assert rc == 0, out
    assert "  lr " not in out
    res = json.loads(out.strip().splitlines()[-1])
    assert "final_lr" not in res and "lr_schedule" not in res


def test_basic_block_resnets_build_and_backpropagate():
    """resnet18 / resnet34 (basic blocks), the small models of the schedule runs above."""
    from arena_amd.models.resnet import BASIC_DEPTHS, BasicBlock, resnet
    assert BASIC_DEPTHS == {"resnet18": [2, 2, 2, 2], "resnet34": [3, 4, 6, 3]}
    m = resnet("resnet18", num_classes=10, width=8)
    blocks = list(m.layers)
    assert len(blocks) == 8 and all(isinstance(b, BasicBlock) for b in blocks)
    assert [b.down_conv is not None for b in blocks] == [False, False, True, False, True, False,
                                                         True, False]
    out = m(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10)
    out.square().mean().backward()
    # the zero-initialised last BN of each block passes no gradient to what is before it, so
    # only require gradients where they can be non-zero: everything has one, the head's is live
    assert all(p.grad is not None for p in m.parameters())
    assert float(m.fc.weight.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="resnet18"):
        resnet("resnet19")
