#!/usr/bin/env python3
"""One sha256 per output buffer of every optimizer kernel, over fixed seeded inputs.

    python tools/optim_bits.py [--tree DIR] > bits.jsonl        # needs a GPU and DIR's built _C
    python tools/optim_bits.py --compare a.jsonl b.jsonl        # -> the equivalence JSON

Run it once per build (``--tree``: the checkout whose ``arena_amd`` is imported, default this one),
each in a process of its own, and compare: two builds whose kernels perform the same fp32
operations in the same order print the same hashes. Inputs: the 49-tensor master set and the fp32
set of tests/test_optim_family_gpu.py, the fp32 set of tests/test_lr_schedule_gpu.py, and one flat
range of 4096 + 12 elements. Every update runs 3 consecutive steps, once with the float ``lr`` and
once with the device ``lr_t``. The sets are always read from THIS checkout's tests, so both builds
see the same bytes.
"""
from __future__ import annotations

import argparse
import hashlib
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, MU, WD, SCALE = 0.05, 0.9, 1e-3, 1.0 / 3
BETAS, ADAM_EPS, DECAY, RMS_EPS, EETA = (0.9, 0.999), 1e-8, 0.9, 1.0, 1e-3


def _test_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(out):
    import torch
    from arena_amd.ops import fused, optim, schedule
    fam, sch = _test_module("test_optim_family_gpu"), _test_module("test_lr_schedule_gpu")
    dev = torch.device("cuda:0")
    bf16 = torch.bfloat16

    def emit(name, **bufs):
        torch.cuda.synchronize()
        for k, t in bufs.items():
            raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
            out.write(json.dumps({"name": f"{name}.{k}", "numel": t.numel(),
                                  "sha256": hashlib.sha256(raw).hexdigest()}) + "\n")

    for form in ("float", "lr_t"):
        lr_t = torch.tensor([LR], dtype=torch.float32, device=dev)
        kw = {"lr": LR} if form == "float" else {"lr": 123.0, "lr_t": lr_t}

        # master layout: SGD, RMSProp, Adam, LARS over the 49-tensor set
        for name in ("sgd", "rmsprop", "adam", "lars"):
            steps, offs, master, s0, s1, total = fam._master_set()
            master, s0, s1 = master.to(dev), s0.to(dev), s1.to(dev)
            wbf = torch.full((total,), fam.SENTINEL, dtype=bf16, device=dev)
            clock = optim.AdamClock(BETAS, dev)
            ns = [g.numel() for g in steps[0]]
            trust = torch.full((len(ns) + 2,), -7.0, device=dev)
            work = torch.full((fused.mt_lars_workspace_floats(ns) + 4,), fam.SENTINEL, device=dev)
            for grads in steps:
                grads = [g.to(dev) for g in grads]
                if name == "sgd":
                    fused.mt_sgd_master(grads, offs, master, s0, wbf, momentum=MU, weight_decay=WD,
                                        **kw)
                elif name == "rmsprop":
                    fused.mt_rmsprop_master(grads, offs, master, s0, s1, wbf, decay=DECAY,
                                            momentum=MU, eps=RMS_EPS, weight_decay=WD, **kw)
                elif name == "adam":
                    clock.tick()
                    fused.mt_adam_master(grads, offs, master, s0, s1, wbf, clock.corr, betas=BETAS,
                                         eps=ADAM_EPS, weight_decay=WD, **kw)
                else:
                    fused.mt_lars_master(grads, offs, master, s0, wbf, trust,
                                         [len(ns) - i for i in range(len(ns))], work, momentum=MU,
                                         weight_decay=WD, eeta=EETA, eps=0.0, **kw)
            extra = {"trust": trust, "workspace": work} if name == "lars" else {}
            emit(f"mt_{name}_master[{form}]", master=master, s0=s0, s1=s1, wbf=wbf, **extra)

        # fp32 layout: both fp32 sets
        for name in ("sgd", "rmsprop", "adam"):
            for which in ("family", "schedule"):
                if which == "family":
                    steps, offs, w, s0, s1, _ = fam._f32_set()
                    steps = [[g.to(dev) for g in grads] for grads in steps]
                else:
                    grads, offs, w, s0, _ = sch._f32_set(dev)
                    steps, s1 = [grads] * 3, s0.abs()       # Adam's v is never negative
                w, s0, s1 = w.to(dev), s0.to(dev), s1.to(dev)
                clock = optim.AdamClock(BETAS, dev)
                for grads in steps:
                    if name == "sgd":
                        fused.mt_sgd_f32(grads, offs, w, s0, momentum=MU, weight_decay=WD,
                                         scale=SCALE, **kw)
                    elif name == "rmsprop":
                        fused.mt_rmsprop_f32(grads, offs, w, s0, s1, decay=DECAY, momentum=MU,
                                             eps=RMS_EPS, weight_decay=WD, scale=SCALE, **kw)
                    else:
                        clock.tick()
                        fused.mt_adam_f32(grads, offs, w, s0, s1, clock.corr, betas=BETAS,
                                          eps=ADAM_EPS, weight_decay=WD, scale=SCALE, **kw)
                emit(f"mt_{name}_f32[{which},{form}]", w=w, s0=s0, s1=s1)

        # one flat range: shard_sgd in both dtypes, adam_flat, sgd_flat
        n = 4096 + 12
        g = torch.Generator().manual_seed(5)
        grad = torch.randn(n, generator=g) * 0.1
        w0, m0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01
        v0 = torch.rand(n, generator=g) * 0.01
        for dtype in (bf16, torch.float32):
            gd, w, m = grad.to(dtype).to(dev), w0.to(dev), m0.to(dev)
            wb = torch.zeros(n, dtype=bf16, device=dev) if dtype == bf16 else None
            for _ in range(3):
                fused.shard_sgd(gd, w, m, wb, momentum=MU, weight_decay=WD, scale=SCALE, **kw)
            emit(f"shard_sgd[{str(dtype)[6:]},{form}]", w=w, mom=m,
                 **({"wbf": wb} if wb is not None else {}))
        gd, p, m, v = grad.to(dev), w0.to(dev), m0.to(dev), v0.to(dev)
        t = torch.zeros(1, dtype=torch.int64, device=dev)
        for i in range(3):
            t.fill_(i + 1)
            fused.adam_flat(p, m, v, gd, betas=BETAS, eps=ADAM_EPS, weight_decay=WD, t_step=t,
                            grad_scale=SCALE, **kw)
        emit(f"adam_flat[{form}]", p=p, m=m, v=v)
        p = w0.to(dev)
        for _ in range(3):
            fused.sgd_flat(p, gd, grad_scale=SCALE, **kw)
        emit(f"sgd_flat[{form}]", p=p)

    # mt_copy_scale both ways, over the schedule set's 57 tensors (two launches)
    grads, offs, w, _, _ = sch._f32_set(dev)
    flat = w.clone()
    fused.flatten_into(grads, offs, flat, SCALE)
    outs = [torch.zeros_like(x) for x in grads]
    fused.unflatten_from(outs, offs, w, SCALE)
    emit("mt_copy_scale", flat=flat, tensors=torch.cat(outs))

    # the two clocks: 40 steps of a warm-up + piecewise schedule, 40 ticks of Adam's
    sched = schedule.DeviceLR(schedule.with_warmup(schedule.piecewise("0.05;8;0.005", 1), 4, 1),
                              dev)
    clock = optim.AdamClock(BETAS, dev)
    lrs, corrs = [], []
    for _ in range(40):
        sched.advance()
        clock.tick()
        lrs.append(sched.lr.clone())
        corrs.append(clock.corr.clone())
    emit("lr_schedule", lr=torch.cat(lrs), step=sched.step)
    emit("adam_tick", corr=torch.cat(corrs), pow=clock.pow, step=clock.step)


def compare(a, b):
    rows = []
    ra, rb = ([json.loads(x) for x in open(p)] for p in (a, b))
    assert [r["name"] for r in ra] == [r["name"] for r in rb], "the two runs list other buffers"
    for x, y in zip(ra, rb):
        rows.append({"name": x["name"], "numel": x["numel"],
                     "bit_identical": x["sha256"] == y["sha256"] and x["numel"] == y["numel"]})
    json.dump({"buffers": rows, "all_bit_identical": all(r["bit_identical"] for r in rows)},
              sys.stdout, indent=1)
    print()
    return 0 if all(r["bit_identical"] for r in rows) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=HERE, help="checkout whose built arena_amd is imported")
    ap.add_argument("--compare", nargs=2, metavar="JSONL")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    sys.path.insert(0, os.path.abspath(args.tree))
    run(sys.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
