"""LARS on the GPU: the two ``mt_lars_master`` kernels against the CPU reference, run to run and
under a gradient scale bit for bit, a captured step whose learning rate and trust ratios move
from replay to replay, ``TFLars`` under capture, the binding's argument checks, and ``cnn_bench
--lars`` end to end."""
from __future__ import annotations

import json
import math
import os
import subprocess
import sys

import pytest
import torch

from arena_amd.ops import fused, optim, schedule
from arena_amd.ops.schedule import DeviceLR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
WD = 4e-5
TOL = dict(rtol=1e-5, atol=1e-6)          # tests/test_optim_family_gpu.py's
LR, EETA, EPS = 0.5, 0.001, 1e-9
SENTINEL = 96.0           # exact in bf16 too
UNUSED = -7.0             # trust entries that no slot names
BIG, ZERO_G, ZERO_W, LATE = 5, 6, 7, 50


# ------------------------------------------------------------------------------------- kernels
def _lars_set():
    """51 tensors, two launch groups (48 + 3): the 49 of ``test_optim_family_gpu._master_set`` (4
    elements, one block, one block + 4, three blocks + 4, a channels_last [8, 4, 3, 3] weight with
    a channels_last gradient, small multiples of 4), a 40-block + 4 tensor at index 5 of the first
    group, and a 5-block + 4 tensor at index 50, whose partials lie behind the first group's.
    Tensor 6's gradient is zero at every step, tensor 7's weights are zero before the first. 4
    elements past the last segment belong to no tensor."""
    g = torch.Generator().manual_seed(11)
    shapes = [(4,), (1024,), (1028,), (3076,), (8, 4, 3, 3)] + [(4 * (1 + i % 5),)
                                                                 for i in range(44)]
    shapes.insert(BIG, (40 * 1024 + 4,))
    shapes.append((5 * 1024 + 4,))
    assert len(shapes) == 51 and shapes[LATE] == (5 * 1024 + 4,)
    ns = [math.prod(s) for s in shapes]
    offs = [sum(ns[:i]) for i in range(len(ns))]
    total = sum(ns) + 4
    steps = []
    for _ in range(3):
        grads = []
        for i, s in enumerate(shapes):
            t = (torch.randn(s, generator=g) * 0.1).to(BF16)
            if len(s) == 4:
                t = t.contiguous(memory_format=torch.channels_last)
            if i == ZERO_G:
                t.zero_()
            grads.append(t)
        steps.append(grads)
    master = torch.randn(total, generator=g) * 0.1
    master[offs[ZERO_W]:offs[ZERO_W] + ns[ZERO_W]] = 0.0
    mom = torch.rand(total, generator=g) * 0.01
    mom[offs[ZERO_W]:offs[ZERO_W] + ns[ZERO_W]] = 0.0
    for t in (master, mom):
        t[-4:] = SENTINEL
    return steps, ns, offs, master, mom, total


def _run_lars(dev, lr_form):
    """Three steps; returns master, mom, wbf, the trust buffer after every step, the workspace."""
    steps, ns, offs, master, mom, total = _lars_set()
    master, mom = master.to(dev), mom.to(dev)
    wbf = torch.full((total,), SENTINEL, dtype=BF16, device=dev)
    n = len(ns)
    trust = torch.full((n + 2,), UNUSED, dtype=torch.float32, device=dev)
    slots = [n - i for i in range(n)]                   # reversed; entries 0 and n + 1 unused
    need = fused.mt_lars_workspace_floats(ns)
    assert need == 2 * sum((k + 1023) // 1024 for k in ns)
    work = torch.full((need + 4,), SENTINEL, dtype=torch.float32, device=dev)
    lr_t = torch.tensor([LR], dtype=torch.float32, device=dev)
    kw = {"float": {"lr": LR}, "lr_t": {"lr": 0.0, "lr_t": lr_t},
          "ignored_float": {"lr": 123.0, "lr_t": lr_t}}[lr_form]
    seen = []
    for grads in steps:
        grads = [g.to(dev) for g in grads]
        assert grads[4].is_contiguous(memory_format=torch.channels_last)
        fused.mt_lars_master(grads, offs, master, mom, wbf, trust, slots, work, momentum=0.9,
                             weight_decay=WD, eeta=EETA, eps=EPS, **kw)
        seen.append(trust.clone())
    return master.cpu(), mom.cpu(), wbf.cpu(), torch.stack(seen).cpu(), work.cpu()


_REF = []


def _lars_ref():
    """The CPU reference of the set, computed once."""
    if not _REF:
        _REF.append(_run_lars(torch.device("cpu"), "float"))
    return _REF[0]


@pytest.mark.parametrize("lr_form", ["float", "lr_t", "ignored_float"])
def test_lars_kernels_match_cpu_reference(cuda, lr_form):
    """trust at rtol 1e-5: at most 41 K non-negative fp32 terms summed as 16 serial per lane + a
    64-lane tree per 1024-element chunk (22 fp32 roundings on any term's path), then at most 41
    partials in fp64, are within 50 * 2^-24 = 3e-6 of the fp64 sum and the norm within half of
    that (measured: 1.4e-7 on trust); a dropped 4-element tail of the 1028 tensor would move its
    norm by about 2e-3."""
    w, m, wbf, trust, work = _run_lars(cuda, lr_form)
    rw, rm, _, rtrust, _ = _lars_ref()
    n = rtrust.shape[1] - 2
    assert not torch.equal(rw, _lars_set()[3])                 # the reference did move
    print("max relative trust error", float(((trust - rtrust) / rtrust).abs().max()))
    torch.testing.assert_close(trust, rtrust, rtol=1e-5, atol=0.0)
    for t in (trust, rtrust):
        assert t[:, n - ZERO_G].tolist() == [1.0] * 3          # all-zero gradient: every step
        assert t[0, n - ZERO_W].item() == 1.0                  # all-zero weights: the first step
        assert t[:, [0, n + 1]].tolist() == [[UNUSED] * 2] * 3  # no slot names these
        live = t[:, 1:n + 1]
        assert bool((live > 0).all()) and bool((live <= 1.0).all())
        assert int((live == 1.0).sum()) == 4                   # the zero cases and nothing else
    torch.testing.assert_close(w, rw, **TOL)
    torch.testing.assert_close(m, rm, **TOL)
    assert torch.equal(wbf[:-4], w[:-4].to(BF16))              # the kernel's own master, rounded
    for t in (w, m, wbf.float(), work):                        # nothing past the last segment
        assert t[-4:].tolist() == [SENTINEL] * 4


def test_lars_kernels_are_deterministic(cuda):
    a = _run_lars(cuda, "lr_t")
    b = _run_lars(cuda, "lr_t")
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)


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
        opt.step()
        trusts.append(opt.trust.clone())
    return opt.master.cpu(), opt.wbf.cpu(), torch.stack(trusts).cpu()


def test_gradient_scale_invariance_bit_for_bit_on_the_gpu(cuda):
    """A power-of-two gradient scale commutes with every rounding in the kernels (fused or not):
    the weights do not see it, and trust shrinks by exactly the scale."""
    m1, w1, t1 = _scale_run(cuda, 1.0)
    m8, w8, t8 = _scale_run(cuda, 8.0)
    assert torch.equal(m1, m8) and torch.equal(w1, w8)
    assert torch.equal(t8, t1 / 8) and bool((t1 > 0).all()) and bool((t1 < 1).all())


def test_binding_checks_its_arguments(cuda):
    n = 2048
    g = torch.ones(n, dtype=BF16, device=cuda)
    w, m = torch.ones(n, device=cuda), torch.zeros(n, device=cuda)
    wbf = torch.zeros(n, dtype=BF16, device=cuda)
    trust = torch.full((2,), UNUSED, device=cuda)
    work = torch.zeros(fused.mt_lars_workspace_floats([n]), device=cuda)
    assert work.numel() == 4

    def call(trust=trust, slots=(1,), work=work, eeta=EETA, eps=0.0, off=0):
        fused.mt_lars_master([g], [off], w, m, wbf, trust, slots, work, lr=0.1, momentum=0.9,
                             eeta=eeta, eps=eps)

    for bad in (dict(trust=trust.double()), dict(trust=trust.cpu()), dict(slots=(2,)),
                dict(slots=(-1,)), dict(slots=(0, 1)), dict(work=work[:2]),   # one block short
                dict(work=work.double()), dict(work=torch.zeros(8, device=cuda)[1:5]),
                dict(eeta=0.0), dict(eps=-1e-9), dict(off=4)):
        with pytest.raises(RuntimeError):
            call(**bad)
    torch.cuda.synchronize()
    assert bool((w == 1).all()) and not m.any() and not wbf.any() and not work.any()
    assert trust.tolist() == [UNUSED] * 2
    call()                                                     # and the good call does run
    torch.cuda.synchronize()
    assert trust[0].item() == UNUSED and 0 < trust[1].item() < 1 and bool((w != 1).all())


# ------------------------------------------------------------------------------- graph replay
def _param_sets(dev, steps):
    """Parameters for the master and the fp32 group, one static gradient buffer each, and
    ``steps`` sets of gradient values to copy into them."""
    g = torch.Generator().manual_seed(7)
    bf = []
    for i, shp in enumerate([(16, 8, 3, 3), (32, 16, 1, 1), (10, 32), (8, 4), (1300, 4)]):
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


def _build(dev, segs, steps):
    bf, f32, values = _param_sets(dev, steps)
    sched = DeviceLR(segs, dev)
    a = optim.MasterLARS(bf, lr=sched, momentum=0.9, weight_decay=WD, eeta=EETA)
    b = optim.MultiTensorSGD32(f32, lr=sched, momentum=0.9)
    for p, v in zip(bf + f32, values[0]):
        p.grad = torch.empty_like(v).copy_(v)         # static: the captured kernels read it
    return sched, a, b, bf + f32, values


def test_captured_lars_step_keeps_its_schedule_and_trust_moving(cuda):
    """One graph holding DeviceLR.advance(), MasterLARS.step() and MultiTensorSGD32.step(),
    replayed 8 times across the end of a 4-step warm-up with gradients rewritten between replays:
    bit-identical to the same steps run eagerly on the GPU, and within the kernels' tolerance of
    the CPU classes. A learning rate or a trust ratio baked into the graph would repeat step 1's."""
    replays = 8
    segs = schedule.with_warmup(schedule.piecewise("5.0;6;0.5", 1), 4, 1)

    def run(dev, graph):
        sched, a, b, params, values = _build(dev, segs, replays)
        first = None

        def step():
            sched.advance()
            a.step()
            b.step()

        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                step()
            assert sched.steps() == 0                 # the capture ran nothing
            assert a.trust.tolist() == [1.0] * len(a.params)
        for t in range(replays):
            for p, v in zip(params, values[t]):
                p.grad.copy_(v)
            g.replay() if graph else step()
            if t == 0:
                first = a.trust.clone()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        return sched, a, b, first

    # load every kernel's code object before the capture (on a throw-away set)
    s0, a0, b0 = _build(cuda, segs, 1)[:3]
    s0.advance(), a0.step(), b0.step()
    torch.cuda.synchronize()

    sg, ag, bg, first = run(cuda, True)
    se, ae, be, _ = run(cuda, False)
    sc, ac, bc, _ = run(torch.device("cpu"), False)
    state = lambda a, b: [a.master, a.wbf, a.mom, a.trust, b.w, b.mom]   # noqa: E731
    for got, eager, ref in zip(state(ag, bg), state(ae, be), state(ac, bc)):
        assert torch.equal(got, eager)
        if got.dtype == torch.float32:
            torch.testing.assert_close(got.cpu(), ref, **TOL)
    assert sg.steps() == replays and sg.value() == sc.value() == 0.5
    assert bool((first != ag.trust).all())             # derived at every replay, not baked in
    assert bool((ag.trust > 0).all()) and bool((ag.trust < 1).all())
    for p, v in zip(bg.params, bg._views(bg.w)):       # the parameters are the updated buffer
        assert p.data_ptr() == v.data_ptr()


def test_plain_lars_replays_as_it_steps(cuda):
    """TFLars on GPU fp32 parameters, one captured step replayed 6 times against 6 eager steps:
    bit-identical, so no norm and no guard went through the host."""
    def make():
        g = torch.Generator().manual_seed(5)
        ps = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.1).to(cuda))
              for s in [(8, 4, 3, 3), (10, 32), (33,), (1,)]]
        ps[1].data.zero_()                              # the guard's branch, on the device
        for p in ps:
            p.grad = (torch.randn(p.shape, generator=g) * 0.1).to(cuda)
        return ps, optim.TFLars([{"params": ps[:2], "weight_decay": WD},
                                 {"params": ps[2:], "lars": False}], lr=0.5, momentum=0.9)

    make()[1].step()                                   # load the kernels before the capture
    torch.cuda.synchronize()
    ps, opt = make()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        opt.step()
    assert not ps[1].any()                             # the capture ran nothing
    for _ in range(6):
        graph.replay()
    es, eopt = make()
    for _ in range(6):
        eopt.step()
    torch.cuda.synchronize()
    for p, e, start in zip(ps, es, make()[0]):
        assert torch.equal(p, e) and not torch.equal(p, start)
        assert bool(torch.isfinite(p).all())
        assert torch.equal(opt.state[p]["mom"], eopt.state[e]["mom"])


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
    return res


@pytest.fixture(scope="module")
def same_kernels(tmp_path_factory):
    """The environment of ``tests/test_optim_family_gpu.py``'s fixture of this name, under which
    two ``cnn_bench`` processes run the same kernels in the same summation order: one shared conv
    plan file, MIOpen's untimed solver choice, BatchNorm sums in a fixed order."""
    return {"ARENA_CONV_PLAN": str(tmp_path_factory.mktemp("plans") / "plans.json"),
            "ARENA_MIOPEN_BENCHMARK": "0", "ARENA_BN_FINAL": "0"}


LARS_FLAGS = ("--lars", "--num_learning_rate_warmup_epochs", "0.5")


def test_cnn_bench_lars_trains_in_one_graph_and_eagerly_alike(tmp_path, same_kernels):
    """12 captured LARS steps on 64 resident images (8 steps per epoch) with a 4-step warm-up, so
    the device schedule is live inside the graph; then the same steps eagerly. The graph run takes
    one step more than its two warm-up batches before the measured ones (the untimed replay), so
    the eager run that performs the same updates is the one with three warm-up batches; both end
    at the same loss to the 4 decimals printed."""
    res = _cnn_bench(tmp_path, *LARS_FLAGS, **same_kernels)
    assert res["exec"] == "hipgraph" and res["lars"] is True and res["optimizer"] == "momentum"
    assert math.isfinite(res["final_loss"])
    assert abs(res["final_lr"] - 0.1) < 1e-6          # past the warm-up: the default rate
    eager = _cnn_bench(tmp_path, *LARS_FLAGS, "--graph", "0", "--num_warmup_batches", "3",
                       **same_kernels)
    assert eager["exec"] == "eager" and eager["lars"] is True
    assert eager["final_loss"] == res["final_loss"]
