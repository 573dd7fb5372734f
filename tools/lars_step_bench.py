"""Optimizer-step time on ResNet-50's parameter set: fused LARS (``MasterLARS`` +
``MultiTensorSGD32``) against ``TFLars`` (the same math in plain tensor ops) and against momentum
SGD's fused pair (``MasterSGD`` + ``MultiTensorSGD32``), on static gradients.

Each arm is timed eagerly and as a captured graph, with device events around ``--steps`` steps,
``--rounds`` times, the arms alternating inside every round. One JSON line per arm and round, then
a summary line. Needs a GPU.

    python tools/lars_step_bench.py --out out/lars_step_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from arena_amd.models.resnet import resnet          # noqa: E402
from arena_amd.ops import optim                     # noqa: E402

WD = 4e-5


def param_sets(dev, model, width):
    """(decay, no_decay) parameters of the model as fresh leaves."""
    torch.manual_seed(1234)
    net = resnet(model, num_classes=1000, width=width).to(dev).to(memory_format=torch.channels_last)
    decay, no_decay = [], []
    for p in net.parameters():
        (no_decay if p.ndim <= 1 else decay).append(torch.nn.Parameter(p.detach().clone()))
    return decay, no_decay


def give_grads(params, dtype, seed):
    g = torch.Generator(device=params[0].device).manual_seed(seed)
    for p in params:
        t = torch.randn(p.shape, device=p.device, generator=g) * 0.01
        if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last):
            t = t.contiguous(memory_format=torch.channels_last)
        p.grad = t.to(dtype)


def make_arm(name, dev, model, width):
    decay, no_decay = param_sets(dev, model, width)
    if name == "tf_lars":
        opt = optim.TFLars([{"params": decay, "weight_decay": WD},
                            {"params": no_decay, "weight_decay": 0.0, "lars": False}], lr=0.1,
                           momentum=0.9)
        give_grads(decay, torch.float32, 1)
    else:
        cls = optim.MasterLARS if name == "fused_lars" else optim.MasterSGD
        opt = optim.OptimizerGroup(cls(decay, lr=0.1, momentum=0.9, weight_decay=WD),
                                   optim.MultiTensorSGD32(no_decay, lr=0.1, momentum=0.9))
        give_grads(decay, torch.bfloat16, 1)
    give_grads(no_decay, torch.float32, 2)
    elements = sum(p.numel() for p in decay)
    return opt, elements, len(decay), len(no_decay)


def timed(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / steps      # us per step


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--arms", default="fused_lars,tf_lars,fused_sgd",
                    help="comma-separated subset of fused_lars, tf_lars, fused_sgd")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lars_step_bench needs a GPU")
    dev = torch.device("cuda", 0)
    arms = {}
    for name in args.arms.split(","):
        if name not in ("fused_lars", "tf_lars", "fused_sgd"):
            raise SystemExit(f"unknown arm {name!r}")
        opt, elements, n_decay, n_rest = make_arm(name, dev, args.model, args.width)
        for _ in range(3):                             # load the kernels, settle the allocator
            opt.step()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            opt.step()
        graph.replay()
        torch.cuda.synchronize()
        arms[name] = {"eager": opt.step, "graph": graph.replay, "opt": opt}
    lines = []
    for r in range(args.rounds):
        for mode in ("graph", "eager"):
            for name, arm in arms.items():
                us = timed(arm[mode], args.steps)
                lines.append({"arm": name, "mode": mode, "round": r, "us_per_step": round(us, 2),
                              "steps": args.steps})
                print(json.dumps(lines[-1]), flush=True)
    summary = {"model": args.model, "decay_elements": elements, "decay_tensors": n_decay,
               "fp32_group_tensors": n_rest, "gpu": torch.cuda.get_device_name(0)}
    for mode in ("graph", "eager"):
        for name in arms:
            v = sorted(x["us_per_step"] for x in lines if x["arm"] == name and x["mode"] == mode)
            summary[f"{name}_{mode}_us"] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
