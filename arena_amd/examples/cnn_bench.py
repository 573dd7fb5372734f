"""Synthetic-ImageNet CNN training benchmark with the Horovod-style API (tf_cnn_benchmarks shape).

The reference's MPI demo runs the Horovod TF image's ``hvd-distribute.sh``
(charts/tf-horovod/README.md:66-69). That image benchmarks the ResNet family on synthetic data
with Horovod allreduce. The script is not in the reference repo, so exact flags are unpinned.
This is the same workload, built for MI355X:

* ResNet v1.5 (``arena_amd.models.resnet``), NHWC (``channels_last``), bf16 autocast on the MFMA
  conv/GEMM paths, fp32 master weights;
* momentum SGD with weight decay, as in tf_cnn_benchmarks; ``--optimizer`` selects its plain
  SGD, RMSProp or Adam instead (TF1's forms; fused master-weight kernels on one rank),
  ``--use_nesterov`` gives momentum SGD Nesterov momentum (in the same fused kernels, xGMI ones
  included), and ``--lars`` scales momentum SGD's rate per weight tensor (norms reduced on the
  device);
* one process per GPU: ``hvd.DistributedOptimizer`` buckets (RCCL or the xGMI kernel on a comm
  stream) overlap the gradient allreduce with backward;
* output lines shaped like tf_cnn_benchmarks' ``images/sec`` and ``total images/sec``;
* by default one static random batch; with ``--data_dir`` / ``--synth_images`` a uint8 dataset
  resident in GPU memory, fed by one kernel at the head of every (captured) step
  (``arena_amd.ops.data.DeviceImageLoader``), with epochs and an ``--eval`` pass over ``val``;
  ``--distortions`` adds tf_cnn_benchmarks' random resized crop to that kernel and
  ``--distort_color`` its colour distortion (YIQ form);
* tf_cnn_benchmarks' learning-rate flags (piecewise schedule, warm-up epochs, exponential
  staircase). The schedule advances on the device at the head of every step
  (``arena_amd.ops.schedule.DeviceLR``), inside the captured graph, and counts the measured steps:
  it is set back to step 0 where epoch 1 starts, after the warm-up batches.

    arena submit mpijob --name r50 --workers 8 --gpus 1 \\
        "python -m arena_amd.examples.cnn_bench --model resnet50 --batch_size 128"
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

from ..runtime import heartbeat
from .common import pick_device, share_cpu_threads


def pair(text: str):
    """argparse type of 'LO,HI'."""
    try:
        lo, hi = (float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected LO,HI, got {text!r}")
    return lo, hi


def distort_of(args):
    """``DeviceImageLoader``'s ``distort`` for the run's flags (None without --distortions)."""
    if not getattr(args, "distortions", False):
        return None
    from ..ops import reference
    distort = {"area": args.distortion_area or reference.CROP_AREA,
               "aspect": args.distortion_aspect or reference.CROP_ASPECT}
    if getattr(args, "distort_color", False):
        distort["color"] = True
    return distort


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--batch_size", type=int, default=128, help="per-rank batch")
    ap.add_argument("--image_size", type=int, default=224)
    ap.add_argument("--num_classes", type=int, default=1000)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--num_batches", type=int, default=100)
    ap.add_argument("--num_warmup_batches", type=int, default=10)
    ap.add_argument("--display_every", type=int, default=10)
    ap.add_argument("--learning_rate", type=float, default=0.1)
    ap.add_argument("--piecewise_learning_rate_schedule", default=None, metavar="LR0;E1;LR1;...",
                    help="learning rate LR0 until epoch E1, LR1 until E2, ... (tf_cnn_benchmarks' "
                         "flag), e.g. '0.4;30;0.04;60;0.004;80;0.0004'")
    ap.add_argument("--num_learning_rate_warmup_epochs", type=float, default=0.0,
                    help="ramp the learning rate linearly from 0 to its first value over this "
                         "many epochs")
    ap.add_argument("--init_learning_rate", type=float, default=None,
                    help="first value of the exponential staircase (default: --learning_rate)")
    ap.add_argument("--num_epochs_per_decay", type=float, default=0.0,
                    help="exponential staircase: multiply the learning rate by "
                         "--learning_rate_decay_factor every this many epochs")
    ap.add_argument("--learning_rate_decay_factor", type=float, default=0.0)
    ap.add_argument("--minimum_learning_rate", type=float, default=0.0,
                    help="lower bound of the exponential staircase")
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--optimizer", choices=["momentum", "sgd", "rmsprop", "adam"],
                    default="momentum",
                    help="tf_cnn_benchmarks' flag: momentum SGD, plain SGD (momentum 0), or TF1's "
                         "RMSProp / Adam; with master weights on one rank the fused multi-tensor "
                         "kernels inside the captured step, else plain tensor ops")
    ap.add_argument("--use_nesterov", action="store_true",
                    help="Nesterov momentum for --optimizer momentum (TF's MomentumOptimizer("
                         "use_nesterov=True), torch's SGD(nesterov=True)): the step goes along "
                         "d + momentum * m instead of m. Off by default")
    ap.add_argument("--rmsprop_decay", type=float, default=None, help="default 0.9")
    ap.add_argument("--rmsprop_momentum", type=float, default=None, help="default 0.9")
    ap.add_argument("--rmsprop_epsilon", type=float, default=None,
                    help="default 1.0 (inside the square root, as in TF1)")
    ap.add_argument("--adam_beta1", type=float, default=None, help="default 0.9")
    ap.add_argument("--adam_beta2", type=float, default=None, help="default 0.999")
    ap.add_argument("--adam_epsilon", type=float, default=None, help="default 1e-8")
    ap.add_argument("--lars", action="store_true",
                    help="layer-wise adaptive rate scaling on top of --optimizer momentum / sgd "
                         "(tf.contrib's LARSOptimizer, the MLPerf ResNet form): every conv / fc "
                         "weight steps with lr * eeta * |w| / (|g| + weight_decay * |w| + "
                         "epsilon); BatchNorm scales / shifts and biases keep plain momentum SGD. "
                         "With master weights on one rank the norms and the update are fused "
                         "kernels inside the captured step, else plain tensor ops")
    ap.add_argument("--lars_eeta", type=float, default=None,
                    help="LARS trust coefficient (default 0.001)")
    ap.add_argument("--lars_epsilon", type=float, default=None,
                    help="added to the trust ratio's denominator (default 0.0)")
    ap.add_argument("--weight_decay", type=float, default=4e-5)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--data_format", choices=["NHWC", "NCHW"], default="NHWC")
    ap.add_argument("--bucket_mb", type=float, default=12.0,
                    help="gradient bucket size (Horovod fusion buffer). 12 MB splits ResNet-50's "
                         "51 MB of bf16 gradients into 5 buckets, so the first buckets' "
                         "collectives run while backward is still producing the rest")
    ap.add_argument("--comm", choices=["auto", "xgmi", "rccl", "hier"], default="auto",
                    help="DP gradient path: xgmi kernels (one node), rccl (flat), hier (node-level "
                         "then inter-node RCCL on 1/local_size of the bytes); auto picks")
    ap.add_argument("--device", default="auto")
    ap.add_argument("--graph", type=int, default=1,
                    help="1: capture the whole training step (fwd, bwd, optimizer) in one hipGraph "
                         "and replay it (single rank; DP ranks run eagerly)")
    ap.add_argument("--master_weights", choices=["auto", "on", "off"], default="auto",
                    help="bf16 conv/linear weights with fp32 master copies updated by one "
                         "multi-tensor HIP kernel; with several ranks by the sharded xGMI "
                         "reduce-scatter/SGD/all-gather kernel (auto: on for bf16 GPU runs, "
                         "data parallel only when the xGMI collective is usable)")
    ap.add_argument("--shard_optimizer", action="store_true",
                    help="data parallel with --optimizer rmsprop / adam or --lars (bf16 on GPUs): "
                         "keep bf16 conv / fc weights with fp32 masters sharded over the ranks and "
                         "run the rule in fused kernels between an RCCL reduce-scatter and "
                         "all-gather (--comm auto, rccl or hier), instead of the fp32 "
                         "DistributedOptimizer path. Opt-in: the two have not been compared on "
                         "a multi-GPU node")
    ap.add_argument("--async_wgrad", choices=["on", "off"], default="off",
                    help="conv weight gradients on a second HIP stream, concurrent with the "
                         "backward-data/BatchNorm chain (single rank; measured slower on "
                         "ResNet-50 bs128: 16.18 vs 15.49 ms/step, docs/perf.md)")
    ap.add_argument("--verify_every", type=int, default=0,
                    help="data parallel: every K steps check that all replicas hold bit-identical "
                         "parameters (and that no xGMI barrier timed out); abort if not. The "
                         "replicas are always verified once at the end")
    ap.add_argument("--label_smoothing", type=float, default=0.0,
                    help="label smoothing of the loss (tf_cnn_benchmarks' flag; 0.1 is the usual "
                         "ResNet-50 recipe)")
    ap.add_argument("--print_training_accuracy", action="store_true",
                    help="top_1_accuracy / top_5_accuracy on every display line, counted on the "
                         "device by the loss kernels (no extra pass, no per-step host read)")
    ap.add_argument("--eval", action="store_true",
                    help="forward-only run (model.eval(), no optimizer): images/sec lines, then "
                         "tf_cnn_benchmarks' 'Accuracy @ 1 = ... Accuracy @ 5 = ...' line")
    ap.add_argument("--json", action="store_true", help="print one JSON summary line at the end")
    ap.add_argument("--data_dir", default=None,
                    help="train on the image shards of this directory (arena_amd.data.images; the "
                         "mount point of 'arena submit --data'), resident in GPU memory; "
                         "num_classes comes from its meta. Default: one static random batch")
    ap.add_argument("--synth_images", type=int, default=0, metavar="N",
                    help="train on a resident synthetic dataset of N learnable images (no files); "
                         "--eval reads a second draw of N // 10 images")
    ap.add_argument("--stored_size", type=int, default=0,
                    help="stored size S of the synthetic images (default image_size * 8 // 7); "
                         "each step crops image_size x image_size out of it")
    ap.add_argument("--num_epochs", type=int, default=0,
                    help="with a dataset: train this many epochs (overrides --num_batches)")
    ap.add_argument("--data_seed", type=int, default=0,
                    help="seed of the shuffle, the crops / flips and the synthetic images")
    ap.add_argument("--distortions", action="store_true",
                    help="with a dataset: random resized crop (tf_cnn_benchmarks' --distortions; "
                         "its colour distortion is --distort_color): each image is a box of "
                         "random area and aspect ratio, resized to image_size by the input "
                         "kernel. Off by default (tf_cnn_benchmarks defaults it to on)")
    ap.add_argument("--distortion_area", type=pair, default=None, metavar="LO,HI",
                    help="the box's share of the stored image's area (default 0.05,1.0)")
    ap.add_argument("--distortion_aspect", type=pair, default=None, metavar="LO,HI",
                    help="the box's width / height (default 0.75,1.33)")
    ap.add_argument("--distort_color", action="store_true",
                    help="with --distortions: tf_cnn_benchmarks' colour distortion in its YIQ "
                         "form (--distort_color_in_yiq): per image a random brightness (up to "
                         "32/255), saturation and contrast (0.5 to 1.5 each) and hue rotation (up "
                         "to 0.2 pi), clipped to the valid range, in the input kernel")
    args = ap.parse_args(argv)
    if args.distortions or args.distortion_area or args.distortion_aspect:
        if not args.distortions:
            ap.error("--distortion_area / --distortion_aspect need --distortions")
        if not has_data(args):
            ap.error("--distortions needs --data_dir or --synth_images")
        if args.eval:
            ap.error("--distortions does not apply to --eval (evaluation takes the centre crop)")
    if args.distort_color:
        if args.eval:
            ap.error("--distort_color does not apply to --eval (evaluation takes the centre crop)")
        if not args.distortions:
            ap.error("--distort_color needs --distortions")
    if not 0.0 <= args.label_smoothing <= 1.0:
        ap.error("--label_smoothing must lie in [0, 1]")
    if args.data_dir and args.synth_images:
        ap.error("--data_dir and --synth_images exclude each other")
    if (args.num_epochs or args.stored_size) and not has_data(args):
        ap.error("--num_epochs / --stored_size need --data_dir or --synth_images")
    expo = (args.init_learning_rate is not None or args.num_epochs_per_decay
            or args.learning_rate_decay_factor or args.minimum_learning_rate)
    if args.piecewise_learning_rate_schedule is not None and expo:
        ap.error("--piecewise_learning_rate_schedule excludes --init_learning_rate, "
                 "--num_epochs_per_decay, --learning_rate_decay_factor and "
                 "--minimum_learning_rate")
    if bool(args.num_epochs_per_decay) != bool(args.learning_rate_decay_factor) or (
            args.minimum_learning_rate and not args.num_epochs_per_decay):
        ap.error("the exponential schedule needs --num_epochs_per_decay and "
                 "--learning_rate_decay_factor together")
    if args.num_learning_rate_warmup_epochs < 0:
        ap.error("--num_learning_rate_warmup_epochs must be >= 0")
    if has_schedule(args) and args.eval:
        ap.error("the learning-rate flags do not apply to --eval")
    for family, defaults in OPTIMIZER_FLAGS.items():
        given = [f for f in defaults if getattr(args, f) is not None]
        if given and args.optimizer != family:
            ap.error(f"--{given[0]} needs --optimizer {family}")
        for f, default in defaults.items():
            v = default if getattr(args, f) is None else getattr(args, f)
            if f.endswith("epsilon"):
                if not v > 0.0:
                    ap.error(f"--{f} must be > 0")
            elif not 0.0 <= v < 1.0:
                ap.error(f"--{f} must lie in [0, 1)")
            setattr(args, f, v)
    given = [f for f in LARS_FLAGS if getattr(args, f) is not None]
    if given and not args.lars:
        ap.error(f"--{given[0]} needs --lars")
    if args.lars and args.optimizer not in ("momentum", "sgd"):
        ap.error(f"--lars modifies --optimizer momentum / sgd, not {args.optimizer}")
    for f, default in LARS_FLAGS.items():
        if getattr(args, f) is None:
            setattr(args, f, default)
    if not args.lars_eeta > 0.0:
        ap.error("--lars_eeta must be > 0")
    if not args.lars_epsilon >= 0.0:
        ap.error("--lars_epsilon must be >= 0")
    if args.use_nesterov:
        if args.optimizer != "momentum":
            ap.error(f"--use_nesterov needs --optimizer momentum, not {args.optimizer}")
        if not args.momentum > 0.0:
            ap.error("--use_nesterov needs --momentum > 0")
        if args.lars:
            ap.error("--use_nesterov does not apply to --lars (Nesterov momentum under LARS is "
                     "not implemented)")
        if args.eval:
            ap.error("--use_nesterov does not apply to --eval (evaluation has no optimizer)")
    return args


# the flags that belong to one --optimizer each, with tf_cnn_benchmarks' defaults
OPTIMIZER_FLAGS = {
    "rmsprop": {"rmsprop_decay": 0.9, "rmsprop_momentum": 0.9, "rmsprop_epsilon": 1.0},
    "adam": {"adam_beta1": 0.9, "adam_beta2": 0.999, "adam_epsilon": 1e-8},
}

# the flags that belong to --lars, with the MLPerf ResNet reference's defaults
LARS_FLAGS = {"lars_eeta": 0.001, "lars_epsilon": 0.0}


IMAGENET_TRAIN_IMAGES = 1281167    # tf_cnn_benchmarks' epoch when no dataset defines one


def has_schedule(args) -> bool:
    """True if any learning-rate schedule flag was given (a plain ``--learning_rate`` is not one)."""
    return (getattr(args, "piecewise_learning_rate_schedule", None) is not None
            or getattr(args, "init_learning_rate", None) is not None
            or bool(getattr(args, "num_learning_rate_warmup_epochs", 0))
            or bool(getattr(args, "num_epochs_per_decay", 0)))


def schedule_segments(args, steps_per_epoch: float, total_steps: int):
    """The segments the schedule flags describe (None without any), as tf_cnn_benchmarks reads
    them. ``steps_per_epoch``: the dataset's, else ImageNet's size over the global batch."""
    if not has_schedule(args):
        return None
    from ..ops import schedule
    try:
        if args.piecewise_learning_rate_schedule is not None:
            segs = schedule.piecewise(args.piecewise_learning_rate_schedule, steps_per_epoch)
        else:
            init = (args.learning_rate if args.init_learning_rate is None
                    else args.init_learning_rate)
            if args.num_epochs_per_decay:
                segs = schedule.exponential(init, args.num_epochs_per_decay,
                                            args.learning_rate_decay_factor,
                                            args.minimum_learning_rate, steps_per_epoch,
                                            total_steps)
            else:
                segs = schedule.constant(init)
        return schedule.with_warmup(segs, args.num_learning_rate_warmup_epochs, steps_per_epoch)
    except ValueError as e:
        raise SystemExit(f"learning-rate schedule: {e}")


def has_data(args) -> bool:
    return bool(getattr(args, "data_dir", None)) or getattr(args, "synth_images", 0) > 0


def synth_val_count(n: int) -> int:
    """Validation images that go with ``--synth_images n``."""
    return max(1, n // 10)


def open_data(args, dev, world, rank, split):
    """This rank's resident shard of the run's dataset: ``(images, labels, meta, name)``; sets
    ``args.num_classes`` from the data."""
    from ..data import images as imgdata
    if args.data_dir:
        im, lb, meta = imgdata.load_images(args.data_dir, split, dev, rank, world)
        name = args.data_dir
    else:
        size = args.stored_size or args.image_size * 8 // 7
        n = args.synth_images if split == "train" else synth_val_count(args.synth_images)
        if n < world:
            raise SystemExit(f"--synth_images: {n} {split} images for {world} ranks")
        imgdata.check_fits(n * size * size * 3, dev, 16.0)
        im, lb = imgdata.synthetic_images(n, size, args.num_classes, args.data_seed,
                                          draw=0 if split == "train" else 1, device=dev)
        if world > 1:
            im, lb = im[rank::world].contiguous(), lb[rank::world].contiguous()
        meta = {"num_classes": args.num_classes, "mean": list(imgdata.IMAGENET_MEAN),
                "std": list(imgdata.IMAGENET_STD), "size": size, "n": n}
        name = "synthetic-images"
    args.num_classes = meta["num_classes"]
    if args.image_size % 2 or args.image_size > meta["size"]:
        raise SystemExit(f"--image_size {args.image_size} must be even and at most the stored "
                         f"size {meta['size']}")
    return im, lb, meta, name


def make_loader(args, dev, rank, model, data, train):
    """The device loader over ``open_data``'s shard, in the layout the model's stem takes."""
    from ..ops.data import DeviceImageLoader
    im, lb, meta, _ = data
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    s2d = args.data_format == "NHWC" and model.takes_s2d(dev, dtype)
    try:
        return DeviceImageLoader(im, lb, args.batch_size, args.image_size, train=train,
                                 seed=args.data_seed, stream=rank, mean=meta["mean"],
                                 std=meta["std"], layout="s2d" if s2d else "nhwc", dtype=dtype,
                                 distort=distort_of(args) if train else None)
    except ValueError as e:
        raise SystemExit(f"image loader: {e}")


def build_model(args, dev):
    """The model, with rank 0's initial weights on every rank."""
    from ..models.resnet import resnet
    from ..parallel import hvd
    torch.manual_seed(1234)
    model = resnet(args.model, num_classes=args.num_classes, width=args.width).to(dev)
    if dev.type == "cuda" and args.data_format == "NHWC":
        model = model.to(memory_format=torch.channels_last)
    hvd.broadcast_parameters(model.state_dict(), root_rank=0)
    return model


def synthetic_batch(args, dev):
    """One synthetic batch (per-rank seed)."""
    from ..parallel import hvd
    g = torch.Generator(device=dev).manual_seed(hvd.rank())
    x = torch.randn(args.batch_size, 3, args.image_size, args.image_size, device=dev, generator=g)
    if dev.type == "cuda" and args.data_format == "NHWC":
        x = x.contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, args.num_classes, (args.batch_size,), device=dev, generator=g)
    return x, y


def build(args, dev, world, segments=None):
    """Model, optimizer (wrapped for DP) and one synthetic batch, ready to step. ``segments``: a
    learning-rate schedule (``schedule_segments``). The master-weight optimizers then read a
    ``DeviceLR`` (``schedule_of(opt)``) in every update kernel; the other paths keep their float
    ``lr`` and the caller sets it on the host each step."""
    from ..parallel import hvd
    mw = getattr(args, "master_weights", "auto")
    name = getattr(args, "optimizer", "momentum")
    momentum = 0.0 if name == "sgd" else args.momentum
    lars = bool(getattr(args, "lars", False))
    rule = "lars" if lars else name if name in ("rmsprop", "adam") else "sgd"
    nesterov = bool(getattr(args, "use_nesterov", False))
    if nesterov and (rule != "sgd" or not momentum > 0.0):
        raise SystemExit("--use_nesterov needs --optimizer momentum with --momentum > 0 and no "
                         "--lars")
    # the keyword reaches an optimizer only with the flag: without it every call is what it was
    nest = {"nesterov": True} if nesterov else {}
    comm = getattr(args, "comm", "auto")
    bf16_gpu = dev.type == "cuda" and getattr(args, "dtype", "bf16") == "bf16"
    # --shard_optimizer: the rule runs inside ShardedMasterSGD over RCCL (opt-in; momentum SGD and
    # single-rank runs are what they were without it)
    shard = bool(getattr(args, "shard_optimizer", False)) and world > 1 and rule != "sgd"
    if shard:
        if not bf16_gpu:
            raise SystemExit("--shard_optimizer needs --dtype bf16 on a GPU (the conv / fc weights "
                             "become bf16 with sharded fp32 masters, updated by HIP kernels)")
        if comm == "xgmi":
            raise SystemExit(f"--shard_optimizer --comm xgmi: the xGMI kernels implement momentum "
                             f"SGD only; {rule} shards over --comm auto, rccl or hier")
        if mw == "off":
            raise SystemExit("--shard_optimizer keeps sharded master weights: it excludes "
                             "--master_weights off")
        mw = "on"
    elif name in ("rmsprop", "adam") and world > 1:
        if mw == "on":
            raise SystemExit(f"--optimizer {name} --master_weights on: the xGMI kernels of the "
                             "sharded data-parallel update (ShardedMasterSGD) implement "
                             "momentum SGD only; add --shard_optimizer (RCCL / hier, bf16 on a "
                             "GPU) or use --master_weights off")
        mw = "off"
    elif lars and world > 1:
        if mw == "on":
            raise SystemExit("--lars --master_weights on: the xGMI kernels of the sharded "
                             "data-parallel update (ShardedMasterSGD) implement momentum SGD only; "
                             "add --shard_optimizer (RCCL / hier, bf16 on a GPU) or use "
                             "--master_weights off")
        mw = "off"
    model = build_model(args, dev)
    decay, no_decay = [], []
    for n, p in model.named_parameters():
        (no_decay if p.ndim <= 1 else decay).append(p)   # no decay on BN / bias
    if shard and lars and any(p.numel() % 4 for p in decay):
        raise SystemExit("--shard_optimizer --lars needs every conv / fc weight's element count "
                         "to be a multiple of 4")
    master = mw == "on" or (
        mw == "auto" and dev.type == "cuda"
        and getattr(args, "dtype", "bf16") == "bf16" and all(p.numel() % 4 == 0 for p in decay))
    if master and (getattr(args, "dtype", "bf16") != "bf16" or dev.type != "cuda"):
        raise SystemExit("--master_weights on needs --dtype bf16 on a GPU (the weights become "
                         "bf16 and the update runs in the HIP multi-tensor kernel)")
    sched = None
    if segments is not None and master:
        from ..ops.schedule import DeviceLR
        sched = DeviceLR(segments, dev)
    lr = args.learning_rate if sched is None else sched
    opt = None
    if master and world > 1:
        # data parallel keeps the bf16-weight design: ShardedMasterSGD over the xGMI kernels
        # where every rank's GPU is mapped into every rank (one node), else over RCCL
        # reduce-scatter / shard update / all-gather (decided collectively: all ranks agree)
        from ..parallel.zero import ShardedMasterSGD
        hyper = {}
        if shard and rule == "rmsprop":
            momentum = args.rmsprop_momentum
            hyper = {"rule": rule, "decay": args.rmsprop_decay, "eps": args.rmsprop_epsilon}
        elif shard and rule == "adam":
            hyper = {"rule": rule, "betas": (args.adam_beta1, args.adam_beta2),
                     "eps": args.adam_epsilon}
        elif shard:
            hyper = {"rule": rule, "eeta": getattr(args, "lars_eeta", LARS_FLAGS["lars_eeta"]),
                     "eps": getattr(args, "lars_epsilon", LARS_FLAGS["lars_epsilon"])}
        opt = ShardedMasterSGD(
            [{"params": decay, "weight_decay": args.weight_decay},
             {"params": no_decay, "weight_decay": 0.0, "weights": "fp32"}],
            lr=lr, momentum=momentum, bucket_mb=args.bucket_mb,
            backend=comm, order=list(model.parameters()), **hyper, **nest)
        if hvd.rank() == 0 and opt.backend != "xgmi" and comm == "auto":
            print(f"[rank 0] ShardedMasterSGD over RCCL, {opt.backend} (ranks cannot map each "
                  "other's GPUs)", file=sys.stderr, flush=True)
    if opt is not None:
        pass                   # data parallel, sharded
    elif name in ("rmsprop", "adam"):
        opt = build_rmsprop_or_adam(args, name, decay, no_decay, lr if master else None)
    elif lars:
        opt = build_lars(args, momentum, decay, no_decay, lr if master else None)
    elif master and sched is not None:
        # as below, with the BN / bias group on the multi-tensor kernel that reads the device lr
        from ..ops.optim import MasterSGD, MultiTensorSGD32, OptimizerGroup
        opt = OptimizerGroup(
            MasterSGD(decay, lr=sched, momentum=momentum, weight_decay=args.weight_decay, **nest),
            MultiTensorSGD32(no_decay, lr=sched, momentum=momentum, **nest))
    elif master:
        # conv/fc weights live in bf16 (fp32 masters inside MasterSGD): no per-step casts
        from ..ops.optim import MasterSGD, OptimizerGroup
        opt = OptimizerGroup(
            MasterSGD(decay, lr=args.learning_rate, momentum=momentum,
                      weight_decay=args.weight_decay, **nest),
            # BN scales / shifts and biases (fp32): torch's fused multi-tensor SGD, one launch
            # instead of the five of the foreach form
            torch.optim.SGD(no_decay, lr=args.learning_rate, momentum=momentum,
                            fused=dev.type == "cuda", foreach=None if dev.type == "cuda" else True,
                            **nest))
    else:
        opt = torch.optim.SGD([{"params": decay, "weight_decay": args.weight_decay},
                               {"params": no_decay, "weight_decay": 0.0}],
                              lr=args.learning_rate, momentum=momentum,
                              foreach=dev.type == "cuda", **nest)
    if world > 1 and not master:
        opt = hvd.DistributedOptimizer(opt, named_parameters=model.named_parameters(),
                                       bucket_mb=args.bucket_mb, comm=args.comm)
    # with a dataset (--data_dir / --synth_images) the batch comes from the device loader
    x, y = (None, None) if has_data(args) else synthetic_batch(args, dev)
    return model, opt, x, y


def build_rmsprop_or_adam(args, name, decay, no_decay, master_lr):
    """``--optimizer rmsprop`` / ``adam``. ``master_lr`` (a float or a ``DeviceLR``): the fused
    master-weight pair, the decayed weights in bf16 with fp32 masters and the BN / bias group in
    fp32, both on the multi-tensor kernels (Adam: one shared clock, ticked by the first). None:
    the same formulas in plain tensor ops over fp32 parameters (``TFRMSprop`` / ``TFAdam``)."""
    from ..ops import optim
    if name == "rmsprop":
        hyper = {"decay": args.rmsprop_decay, "momentum": args.rmsprop_momentum,
                 "eps": args.rmsprop_epsilon}
        fused_pair, plain = (optim.MasterRMSprop, optim.MultiTensorRMSprop32), optim.TFRMSprop
    else:
        hyper = {"betas": (args.adam_beta1, args.adam_beta2), "eps": args.adam_epsilon}
        fused_pair, plain = (optim.MasterAdam, optim.MultiTensorAdam32), optim.TFAdam
    if master_lr is None:
        return plain([{"params": decay, "weight_decay": args.weight_decay},
                      {"params": no_decay, "weight_decay": 0.0}], lr=args.learning_rate, **hyper)
    first = fused_pair[0](decay, lr=master_lr, weight_decay=args.weight_decay, **hyper)
    if name == "adam":
        hyper["clock"] = first.clock
    return optim.OptimizerGroup(first, fused_pair[1](no_decay, lr=master_lr, **hyper))


def build_lars(args, momentum, decay, no_decay, master_lr):
    """``--lars``. ``master_lr`` (a float or a ``DeviceLR``): ``MasterLARS`` over the decayed
    weights (bf16 with fp32 masters; norms, trust ratio and update on the device) and the BN /
    bias group, LARS's skip list, on ``MultiTensorSGD32``. None: ``TFLars``, the same formula in
    plain tensor ops over fp32 parameters."""
    from ..ops import optim
    hyper = {"eeta": getattr(args, "lars_eeta", LARS_FLAGS["lars_eeta"]),
             "eps": getattr(args, "lars_epsilon", LARS_FLAGS["lars_epsilon"])}
    if master_lr is None:
        return optim.TFLars([{"params": decay, "weight_decay": args.weight_decay, "lars": True},
                             {"params": no_decay, "weight_decay": 0.0, "lars": False}],
                            lr=args.learning_rate, momentum=momentum, **hyper)
    return optim.OptimizerGroup(
        optim.MasterLARS(decay, lr=master_lr, momentum=momentum, weight_decay=args.weight_decay,
                         **hyper),
        optim.MultiTensorSGD32(no_decay, lr=master_lr, momentum=momentum))


def schedule_of(opt):
    """The ``DeviceLR`` an optimizer's update kernels read (None: float learning rates)."""
    from ..ops.schedule import DeviceLR
    for o in getattr(opt, "opts", (opt,)):
        # ShardedMasterSGD / every flat-buffer optimizer of ops.optim (SGD, RMSProp, Adam)
        for name in ("lr_sched", "lr"):
            s = getattr(o, name, None)
            if isinstance(s, DeviceLR):
                return s
    return None


def comm_name(opt) -> str:
    """How the optimizer moves gradients (for logs and the JSON line)."""
    from ..parallel.zero import ShardedMasterSGD
    if isinstance(opt, ShardedMasterSGD):
        red = ""
        if opt.backend in ("rccl", "hier"):
            red = ",fp32-reduce" if opt.rccl_reduce_fp32 else ",bf16-ring-reduce"
        return f"{opt.backend}-sharded-{opt.rule}[{len(opt.buckets)} buckets{red}]"
    c = getattr(opt, "comm", None)
    return c if isinstance(c, str) else "none"


def comms_of(opt) -> list:
    """The xGMI communicators an optimizer owns (for ReplicaCheck's barrier-timeout check)."""
    from ..parallel.zero import ShardedMasterSGD
    if isinstance(opt, ShardedMasterSGD):
        return [opt.comm]       # None on the RCCL backend (ReplicaCheck skips it)
    return [getattr(opt, "xgmi", None)]


def train_step(model, opt, x, y, amp_dtype, zero_grad=True, *, head=None, loader=None,
               loss_sum=None, sched=None, host_lr=False):
    """One training step. ``head``: keyword arguments for ``ops.pool.cross_entropy``
    (``label_smoothing``, ``stats``, ``ignore_index``); None is the plain mean loss.
    ``loader``: a ``DeviceImageLoader`` whose ``next()`` opens the step (x and y are then its
    static buffers), so a captured step holds the input pipeline and every replay advances.
    ``loss_sum``: a device scalar the step adds its loss to (an epoch's mean without a host read
    or a launch between replays). ``sched``: a ``DeviceLR`` whose ``advance()`` opens the step
    (one launch, captured with the rest); with ``host_lr`` it lives on the host and its value is
    written into the optimizer's ``param_groups`` (the paths without a device learning rate)."""
    if sched is not None:
        sched.advance()
        if host_lr:
            for g in opt.param_groups:
                g["lr"] = sched.value()
    s2d = False
    if loader is not None:
        x, y = loader.next()
        s2d = loader.layout == "s2d"
    with torch.autocast(device_type=x.device.type, dtype=amp_dtype, enabled=amp_dtype is not None,
                        cache_enabled=False):
        logits = model(x, s2d=True) if s2d else model(x)
    # (outside autocast: the fused loss takes the bf16 logits as they are and sums in fp32, as
    # autocast's fp32 cross_entropy does after its upcast copy)
    if head is not None:
        from ..ops.pool import cross_entropy
        loss = cross_entropy(logits, y, **head)
    elif x.is_cuda:
        from ..ops.pool import cross_entropy
        loss = cross_entropy(logits, y)
    else:
        loss = F.cross_entropy(logits.float(), y)
    if zero_grad:
        opt.zero_grad(set_to_none=True)
    loss.backward()
    if x.is_cuda:
        from ..ops import conv
        conv.sync_wgrad()   # weight gradients computed on the side stream (if enabled)
    opt.step()
    if loss_sum is not None:
        loss_sum.add_(loss.detach().float())
    return loss.detach()


def capture_step(model, opt, x, y, amp_dtype, *, head=None, loader=None, loss_sum=None,
                 sched=None):
    """The whole step as one hipGraph: ~800 kernels per ResNet-50 step replay without host
    launches or inter-kernel gaps. Gradients are None at capture, so the captured backward writes
    (not accumulates) them, and every replay reuses the same memory (static x, y)."""
    opt.zero_grad(set_to_none=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        loss = train_step(model, opt, x, y, amp_dtype, zero_grad=False, head=head, loader=loader,
                          loss_sum=loss_sum, sched=sched)
    return g, loss


def main(argv=None) -> int:
    args = parse(argv)
    from ..parallel import hvd
    dev = pick_device(args.device)
    hvd.init("nccl" if dev.type == "cuda" else "gloo")
    world, rank = hvd.size(), hvd.rank()
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
        # MIOpen: pick the fastest conv solvers once. The pick is timed, so it can differ from
        # process to process; ARENA_MIOPEN_BENCHMARK=0 leaves the library its untimed choice
        # (for comparing two runs exactly)
        torch.backends.cudnn.benchmark = os.environ.get("ARENA_MIOPEN_BENCHMARK", "1") == "1"
    else:
        share_cpu_threads(int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    amp = torch.bfloat16 if args.dtype == "bf16" else None
    if dev.type == "cuda":
        from ..ops import conv
        if args.async_wgrad == "on" and world > 1:
            raise SystemExit("--async_wgrad on is single-rank only (DP hooks read gradients "
                             "as soon as autograd produces them)")
        conv.set_async_wgrad(args.async_wgrad == "on")
    if args.eval:
        return evaluate(args, dev, world, rank, amp)
    data = loader = None
    if has_data(args):
        data = open_data(args, dev, world, rank, "train")    # sets args.num_classes
    spe = 0                       # steps per epoch, the same on every rank
    if data is not None:
        meta = data[2]
        spe = (meta["n"] // world) // args.batch_size
        if spe < 1:
            raise SystemExit(f"{meta['n']} images over {world} ranks do not fill one batch of "
                             f"{args.batch_size}")
        if args.num_epochs:
            args.num_batches = args.num_epochs * spe
    segments = schedule_segments(
        args, spe or IMAGENET_TRAIN_IMAGES / (args.batch_size * world), args.num_batches)
    model, opt, x, y = build(args, dev, world, segments)
    sched, host_lr = schedule_of(opt), False
    if segments is not None and sched is None:
        # no device learning rate on this path: the same schedule, evaluated on the host
        from ..ops.schedule import DeviceLR
        sched, host_lr = DeviceLR(segments, "cpu"), True
        if rank == 0 and args.graph and dev.type == "cuda":
            print("learning-rate schedule without master weights: the host sets lr every step, "
                  "so the step runs eagerly (no hipGraph)", flush=True)
    data_name = "synthetic"
    ep_loss, ep_steps = None, 0   # the running epoch's loss sum (device) and step count (host)
    if data is not None:
        loader = make_loader(args, dev, rank, model, data, train=True)
        x, y = loader.out, loader.labels_out
        ep_loss = torch.zeros((), dtype=torch.float32, device=dev)
        data_name = (f"{data[3]} ({meta['n']} images, {meta['size']} -> {args.image_size}"
                     f"{' distorted' if loader.boxes is not None else ''}"
                     f"{'+color' if loader.color_table is not None else ''})")
    head = stats = None
    if args.label_smoothing != 0.0 or args.print_training_accuracy:
        # [kept, top-1, top-5, invalid labels], added to by the loss kernels on the device (so a
        # replayed graph keeps counting); allocated before warm-up and capture
        stats = torch.zeros(4, dtype=torch.int64, device=dev)
        head = {"label_smoothing": args.label_smoothing, "stats": stats}

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    if rank == 0:
        print(f"Model: {args.model}  Batch size: {args.batch_size} per device, "
              f"{args.batch_size * world} global  Devices: {world} x {dev.type}  "
              f"Data: {data_name}  dtype: {args.dtype}  graph: {args.graph}  comm: "
              f"{comm_name(opt)}{'  nesterov' if args.use_nesterov else ''}", flush=True)
    for i in range(args.num_warmup_batches):
        t = time.perf_counter()
        train_step(model, opt, x, y, amp, head=head, loader=loader, loss_sum=ep_loss,
                   sched=sched, host_lr=host_lr)
        sync()
        if rank == 0:   # the first steps include MIOpen's solver search: show progress
            print(f"warmup {i + 1}/{args.num_warmup_batches}: {time.perf_counter() - t:.2f} s",
                  flush=True)
    sync()
    graph = None
    if args.graph and dev.type == "cuda" and not host_lr:
        # Data parallel too: the bucket hooks fire during the captured backward, so the graph
        # holds the pack + collective (xGMI kernel on the comm stream, or RCCL) of every bucket
        # exactly where eager mode issues them; all ranks replay the same collective sequence.
        ok = True
        try:
            graph, g_loss = capture_step(model, opt, x, y, amp, head=head, loader=loader,
                                         loss_sum=ep_loss, sched=sched)
        except RuntimeError as e:  # capture refused by a library call: run eagerly
            graph, ok = None, False
            print(f"[rank {rank}] hipGraph capture failed, running eagerly: {e}", flush=True)
        if world > 1:  # every rank replays, or none does (a lone eager rank would still match
            # the collective sequence, but the timing would not be one mode)
            t = torch.tensor([1 if ok else 0], device=dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MIN)
            if not int(t.item()):
                graph = None
            torch.distributed.barrier()
        if graph is not None:
            graph.replay()  # one untimed replay: the step the capture recorded is now executed
            sync()
    if world > 1:
        torch.distributed.barrier()
    sync()
    check = None
    if world > 1:
        from ..parallel.verify import ReplicaCheck
        check = ReplicaCheck(args.verify_every, lambda: list(model.parameters()),
                             comms=comms_of(opt))
    seen0 = seen = stats.tolist() if stats is not None else None   # warm-up's counts excluded
    if loader is not None:
        # epoch 1 starts here, after warm-up's batches. The host knows the step count, so the
        # reshuffle between replays needs no device read; the epoch's loss sum stays on the device
        loader.new_epoch()
        ep_loss.zero_()
    if sched is not None:
        sched.reset(0)   # the schedule counts the measured steps, as the epochs do
    t0 = t_last = time.perf_counter()
    loss = None
    for i in range(1, args.num_batches + 1):
        if loader is not None and i > 1 and (i - 1) % spe == 0:
            loader.new_epoch()
            ep_loss.zero_()
            ep_steps = 0
        if graph is not None:
            graph.replay()
            loss = g_loss
        else:
            loss = train_step(model, opt, x, y, amp, head=head, loader=loader, loss_sum=ep_loss,
                              sched=sched, host_lr=host_lr)
        ep_steps += 1
        heartbeat.beat(i)
        if check is not None:
            check.maybe(i)
        if i % args.display_every == 0 or i == args.num_batches:
            sync()
            now = time.perf_counter()
            n = args.display_every if i % args.display_every == 0 else i % args.display_every
            acc = ""
            if args.print_training_accuracy:   # one read per display line, at its sync
                cur = stats.tolist()
                kept = max(cur[0] - seen[0], 1)
                acc = (f"  top_1_accuracy: {(cur[1] - seen[1]) / kept:.4f}"
                       f"  top_5_accuracy: {(cur[2] - seen[2]) / kept:.4f}")
                seen = cur
            if rank == 0:
                ips = n * args.batch_size / (now - t_last)
                lr_col = f"  lr {sched.value():.6f}" if sched is not None else ""
                print(f"{i}\timages/sec: {ips:.1f} (per device)  loss {float(loss):.3f}{acc}"
                      f"{lr_col}", flush=True)
            t_last = now
    sync()
    elapsed = time.perf_counter() - t0
    if check is not None:
        check.verify(args.num_batches)   # every rank raises on divergence: no number printed
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    total = args.num_batches * args.batch_size * world / elapsed
    counts = None
    if stats is not None:
        counts = global_counts(stats, seen0, world)
    if rank == 0:
        print("-" * 64)
        print(f"total images/sec: {total:.2f}", flush=True)
        print("-" * 64)
        if args.json:
            res = {"model": args.model, "images_per_s": round(total, 2),
                   "ms_per_step": round(elapsed / args.num_batches * 1e3, 3),
                   "batch_per_device": args.batch_size, "devices": world,
                   "dtype": args.dtype, "comm": comm_name(opt), "optimizer": args.optimizer,
                   "lars": bool(args.lars),
                   "exec": "hipgraph" if graph is not None else "eager",
                   "final_loss": round(float(loss), 4)}
            if args.use_nesterov:
                res["nesterov"] = True
            if counts is not None:
                res.update(accuracy_fields(counts))
            if sched is not None:
                res.update({"final_lr": sched.value(),
                            "lr_schedule": [list(s) for s in sched.segments]})
            if loader is not None:
                res.update({"data": data[3], "images": data[2]["n"], "layout": loader.layout,
                            "steps_per_epoch": spe, "epochs": loader.epoch,
                            "last_epoch_loss": round(float(ep_loss) / max(ep_steps, 1), 4)})
                if counts is not None:
                    res["kept"] = counts[0]
                if loader.boxes is not None:
                    res.update({"distortions": True, "crop_boxes": loader.boxes.shape[0]})
                if loader.color_table is not None:
                    res["distort_color"] = True
            print(json.dumps(res), flush=True)
    if rank == 0 and os.environ.get("ARENA_CONV_LOG"):
        from ..ops import conv
        for key, plan in conv.plans().items():
            print(f"conv {key[0]} w{key[1]} s{key[2]} p{key[3]}: fwd={plan.fwd} bwd={plan.bwd} "
                  f"bwd_bn={plan.bwd_bn} wgrad={plan.wgrad} {plan.times}", file=sys.stderr)
    hvd.shutdown()
    return invalid_labels_error(counts, rank)


def global_counts(stats, base, world) -> list:
    """[kept, top-1, top-5, invalid] since ``base`` (a host copy of ``stats``), summed over ranks."""
    t = stats - torch.tensor(base, dtype=stats.dtype, device=stats.device)
    if world > 1:
        torch.distributed.all_reduce(t)
    return t.tolist()


def accuracy_fields(counts) -> dict:
    kept = max(counts[0], 1)
    return {"top_1_accuracy": round(counts[1] / kept, 4),
            "top_5_accuracy": round(counts[2] / kept, 4), "invalid_labels": counts[3]}


def invalid_labels_error(counts, rank) -> int:
    """Exit status: labels outside [0, classes) were dropped from the loss, which is an error in
    the input pipeline, not something to average over."""
    if counts is None or counts[3] == 0:
        return 0
    if rank == 0:
        print(f"error: {counts[3]} labels outside [0, num_classes) were dropped from the loss",
              file=sys.stderr, flush=True)
    return 1


def evaluate(args, dev, world, rank, amp) -> int:
    """``--eval``: forward-only passes over the synthetic batch in eval mode (BatchNorm on its
    running statistics), eager, with training's warm-up and display cadence; ends with
    tf_cnn_benchmarks' accuracy line, counted over all ranks."""
    from ..ops.pool import cross_entropy
    from ..parallel import hvd
    if has_data(args):
        return evaluate_data(args, dev, world, rank, amp)
    model = build_model(args, dev).eval()
    x, y = synthetic_batch(args, dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def step():
        with torch.no_grad():
            with torch.autocast(device_type=dev.type, dtype=amp, enabled=amp is not None,
                                cache_enabled=False):
                logits = model(x)
            return cross_entropy(logits, y, label_smoothing=args.label_smoothing, stats=stats)

    if rank == 0:
        print(f"Model: {args.model}  Batch size: {args.batch_size} per device, "
              f"{args.batch_size * world} global  Devices: {world} x {dev.type}  "
              f"Data: synthetic  dtype: {args.dtype}  mode: eval", flush=True)
    for i in range(args.num_warmup_batches):
        step()
    sync()
    if world > 1:
        torch.distributed.barrier()
    base = stats.tolist()
    t0 = t_last = time.perf_counter()
    loss = None
    for i in range(1, args.num_batches + 1):
        loss = step()
        heartbeat.beat(i)
        if i % args.display_every == 0 or i == args.num_batches:
            sync()
            now = time.perf_counter()
            n = args.display_every if i % args.display_every == 0 else i % args.display_every
            if rank == 0:
                ips = n * args.batch_size / (now - t_last)
                print(f"{i}\timages/sec: {ips:.1f} (per device)  loss {float(loss):.3f}",
                      flush=True)
            t_last = now
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    total = args.num_batches * args.batch_size * world / elapsed
    counts = global_counts(stats, base, world)
    if rank == 0:
        kept = max(counts[0], 1)
        print("-" * 64)
        print(f"total images/sec: {total:.2f}")
        print("-" * 64)
        print("Accuracy @ 1 = %.4f Accuracy @ 5 = %.4f [%d examples]"
              % (counts[1] / kept, counts[2] / kept, counts[0]), flush=True)
        if args.json:
            res = {"model": args.model, "images_per_s": round(total, 2),
                   "ms_per_step": round(elapsed / args.num_batches * 1e3, 3),
                   "batch_per_device": args.batch_size, "devices": world, "dtype": args.dtype,
                   "exec": "eval", "final_loss": round(float(loss), 4)}
            res.update(accuracy_fields(counts))
            print(json.dumps(res), flush=True)
    hvd.shutdown()
    return invalid_labels_error(counts, rank)


def evaluate_data(args, dev, world, rank, amp) -> int:
    """``--eval`` with a dataset: one pass over this rank's rows of the ``val`` split in order
    (centre crop, no flip), ``ceil(rows / batch)`` batches. The loader pads the last batch with
    label -100, which the loss ignores, so the example count is the number of validation images
    exactly."""
    from ..ops.pool import cross_entropy
    from ..parallel import hvd
    data = open_data(args, dev, world, rank, "val")    # sets args.num_classes
    model = build_model(args, dev).eval()
    loader = make_loader(args, dev, rank, model, data, train=False)
    s2d = loader.layout == "s2d"
    meta = data[2]
    stats = torch.zeros(4, dtype=torch.int64, device=dev)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def step():
        with torch.no_grad():
            x, y = loader.next()
            with torch.autocast(device_type=dev.type, dtype=amp, enabled=amp is not None,
                                cache_enabled=False):
                logits = model(x, s2d=True) if s2d else model(x)
            return cross_entropy(logits, y, ignore_index=-100,
                                 label_smoothing=args.label_smoothing, stats=stats)

    if rank == 0:
        print(f"Model: {args.model}  Batch size: {args.batch_size} per device, "
              f"{args.batch_size * world} global  Devices: {world} x {dev.type}  "
              f"Data: {data[3]} ({meta['n']} images, {meta['size']} -> {args.image_size})  "
              f"dtype: {args.dtype}  mode: eval", flush=True)
    for i in range(min(args.num_warmup_batches, loader.steps_per_epoch)):
        step()
    loader.new_epoch()           # the counted pass starts at row 0
    sync()
    if world > 1:
        torch.distributed.barrier()
    base = stats.tolist()
    steps = loader.steps_per_epoch
    t0 = time.perf_counter()
    loss = None
    for i in range(1, steps + 1):
        loss = step()
        heartbeat.beat(i)
        if rank == 0 and (i % args.display_every == 0 or i == steps):
            print(f"{i}\tloss {float(loss):.3f}", flush=True)
    sync()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    counts = global_counts(stats, base, world)
    total = counts[0] / elapsed
    if rank == 0:
        kept = max(counts[0], 1)
        print("-" * 64)
        print(f"total images/sec: {total:.2f}")
        print("-" * 64)
        print("Accuracy @ 1 = %.4f Accuracy @ 5 = %.4f [%d examples]"
              % (counts[1] / kept, counts[2] / kept, counts[0]), flush=True)
        if args.json:
            res = {"model": args.model, "images_per_s": round(total, 2),
                   "ms_per_step": round(elapsed / steps * 1e3, 3),
                   "batch_per_device": args.batch_size, "devices": world, "dtype": args.dtype,
                   "exec": "eval", "final_loss": round(float(loss), 4), "data": data[3],
                   "images": meta["n"], "layout": loader.layout, "kept": counts[0]}
            res.update(accuracy_fields(counts))
            print(json.dumps(res), flush=True)
    hvd.shutdown()
    return invalid_labels_error(counts, rank)


if __name__ == "__main__":
    sys.exit(main())
