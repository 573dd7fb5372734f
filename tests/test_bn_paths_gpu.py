"""Every reduction and grid path of the BatchNorm kernels (csrc/ops/bn_kernels.hip) against fp64.

tests/test_bn_gpu.py reaches the default paths at loose tolerances; the A/B tools flip eight
runtime switches that no test sets. Here each path is selected with those switches (``knobs``
restores the defaults), asserted through the read-only bindings ``bn_reduce_blocks`` /
``bn_fin_blocks`` / ``bn_acc_ok`` (a shape that stops reaching its path fails there), and compared
with a plain fp64 PyTorch evaluation of the same operation on the same (already rounded) inputs.

Tolerances. A stored element may differ from fp64 by its format's unit roundoff (bf16 2^-8, fp32
2^-24) times |ref| plus an fp32 evaluation slack E. E is measured on the reference side only: the
error of the same quantity evaluated by torch in fp32 (``F.batch_norm`` / ``x.float()`` sums,
native kernels) against fp64 is the yardstick; the kernels get ``MARGIN`` times it, with a floor
of ``FLOOR_ULPS`` fp32 ulps of the tensor's largest magnitude. Per-channel sums (mean, invstd,
running statistics, dgamma, dbeta, accumulator totals) are compared relative to sum |terms|.
Mask bits, dres, xsel, zeroed sets, counters and run-to-run equality on the partial / ticket
paths are exact.
"""
from __future__ import annotations

import contextlib
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
MOM = 0.1
U_STORE = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
ULP32 = 2.0 ** -23
# The kernels sum in another order than torch (Welford per thread, Chan over row slots, fp64
# across blocks), and coefficient error enters y and dx multiplied by |x - mean| * scale: 8x the
# fp32 yardstick, at least 4 fp32 ulps. Measured on an MI355X over this whole file: largest fp32
# yardstick / largest kernel error beyond the store roundoff [largest fraction of its allowance
# E that any tensor used]; sums relative to sum |terms|:
#   A  mean, invstd, running stats  2.1e-7 / 1.5e-7  [0.29]   (x + 1000: invstd 1.1e-5 / 1.6e-5)
#      (sum x, sum x^2) of acc mode 1.7e-7 / 1.5e-7  [0.29]
#      y                            1.2e-6 / 4.2e-7  [0.08]   (x + 1000: 1.3e-4 / 1.8e-4 [0.17])
#   B  y                            1.9e-6 / 1.1e-6  [0.15]
#      module: y, dx, running stats 8.2e-7 / 8.4e-7  [0.16]   (dweight, dbias 1.0e-5 / 1.3e-5 [0.28])
#   C  dx                           5.0e-7 / 3.2e-7  [0.13]
#      dgamma, dbeta                2.4e-7 / 1.4e-7  [0.18]
#      acc2 totals (x2 form)        2.8e-8 / 1.5e-8  [0.03]
#   D  y                            8.5e-7 / 2.5e-7  [0.08]
#      dx                           7.0e-7 / 5.6e-7  [0.15]
#      dgamma, dbeta                3.0e-7 / 1.5e-7  [0.14]
# (the module fixture prints the current figures; ARENA_BN_PATHS_REPORT=<file> writes them as JSON)
MARGIN = 8.0
FLOOR_ULPS = 4.0
DTYPES = [torch.float32, torch.bfloat16]
DT_ID = {torch.float32: "f32", torch.bfloat16: "bf16"}
MODES = ["relu", "relu_res", "plain", "res"]
# (3,64,53,53): with 64 blocks a thread does two full rounds and a partial third;
# (7,512,10,10): sliced 32 x 2 grid, 700 rows against 512 per iteration / flat 512-channel
# prologue; (3,2048,3,3): 8 slices; (2,8,5,5): one block, lanes beyond the data
B_SHAPES = [(3, 64, 53, 53), (7, 512, 10, 10), (3, 2048, 3, 3), (2, 8, 5, 5)]

_NOTES: dict = {}


def _note(tag, yard, err, allow):
    key = re.sub(r"\[.*?\]", "", tag)
    y0, e0, r0 = _NOTES.get(key, (0.0, 0.0, 0.0))
    _NOTES[key] = (max(y0, yard), max(e0, err), max(r0, err / allow if allow > 0 else 0.0))


@pytest.fixture(scope="module", autouse=True)
def _report(cuda):
    """Needs the GPU (skips without one); prints the measured figures when the module is done."""
    yield
    lines = [f"{k}: yardstick {y:.3e}  kernel {e:.3e}  ({r:.2f} of E)"
             for k, (y, e, r) in sorted(_NOTES.items())]
    print("\n[bn paths] measured fp32 yardsticks and kernel errors\n" + "\n".join(lines))
    path = os.environ.get("ARENA_BN_PATHS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({k: list(v) for k, v in _NOTES.items()}, f, indent=1, sort_keys=True)


def _ext():
    from arena_amd.ops import _ext as e
    return e.load()


@contextlib.contextmanager
def knobs(acc=True, geometry=(512, 8), fin_max=64, slice_=1, nt=1, elem=1024, dx=1024, quad=2,
          fin_bwd=True, res_sums=True):
    """Set the BatchNorm switches; the defaults are back in place on exit."""
    from arena_amd.ops import batchnorm
    ext = _ext()

    def put(acc, geometry, fin_max, slice_, nt, elem, dx, quad, fin_bwd, res_sums):
        ext.bn_set_acc(bool(acc))
        ext.bn_set_reduce_geometry(*geometry)
        ext.bn_set_fin_max_blocks(fin_max)
        ext.bn_set_slice(slice_)
        ext.bn_set_nt(nt)
        ext.bn_set_elem_max_blocks(elem)
        ext.bn_set_dx_max_blocks(dx)
        ext.bn_set_pool_quad_mult(quad)
        batchnorm.set_fin_bwd(fin_bwd)
        batchnorm.set_res_sums(res_sums)

    try:
        put(acc, geometry, fin_max, slice_, nt, elem, dx, quad, fin_bwd, res_sums)
        yield ext
    finally:
        put(True, (512, 8), 64, 1, 1, 1024, 1024, 2, True, True)


# ------------------------------------------------------------------------------------ helpers
def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rows(t):
    """[M, C] view of an NHWC tensor (memory order)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _bc(v):
    return v[None, :, None, None]


def _data(shape, dtype, seed=0, res=False, offset=0.5, scale=2.0):
    torch.manual_seed(seed)
    C = shape[1]
    x = _nhwc((torch.randn(shape, device="cuda") * scale + offset).to(dtype))
    r = _nhwc(torch.randn(shape, device="cuda").to(dtype)) if res else None
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda") * 0.1
    dy = _nhwc(torch.randn(shape, device="cuda").to(dtype))
    return x, r, gamma, beta, dy


def _running(C):
    g = torch.Generator(device="cuda").manual_seed(77)
    rm = torch.randn(C, device="cuda", generator=g)
    rv = torch.rand(C, device="cuda", generator=g) + 0.5
    return rm, rv, torch.full((), 5, dtype=torch.int64, device="cuda")


def _stats(x, dt):
    var, mean = torch.var_mean(_rows(x).to(dt), 0, unbiased=False)
    return mean, var


def _compose(x, res, gamma, beta, relu, dt, maskf=None, stats=None, native=False):
    """act(bn(x) (+ res)) in precision dt. stats: (mean, biased var) instead of x's own;
    maskf: a 0/1 tensor multiplied in instead of the ReLU (the backward references);
    native: torch's own batch_norm (the fp32 yardstick) instead of the written-out formula."""
    xd = x.to(dt)
    C = x.shape[1]
    g = gamma.to(dt) if gamma is not None else torch.ones(C, dtype=dt, device=x.device)
    b = beta.to(dt) if beta is not None else torch.zeros(C, dtype=dt, device=x.device)
    if native and stats is None and xd.numel() // C > 1:
        with torch.backends.cudnn.flags(enabled=False):
            y = F.batch_norm(xd, None, None, g, b, True, 0.0, EPS)
    else:
        mean, var = stats if stats is not None else _stats(xd, dt)
        mean, var = mean.to(dt), var.to(dt)
        y = (xd - _bc(mean)) * _bc(torch.rsqrt(var + EPS) * g) + _bc(b)
    if res is not None:
        y = y + res.to(dt)
    if maskf is not None:
        return y * maskf.to(dt)
    return F.relu(y) if relu else y


def _slack(yard, scale):
    return max(MARGIN * yard, FLOOR_ULPS * ULP32 * scale)


def _check_elem(tag, out, ref64, ref32):
    """|out - ref64| <= u_T |ref64| + E per element (E: see the module docstring)."""
    ref64 = ref64.detach()
    u = U_STORE[out.dtype]
    yard = float((ref32.detach().double() - ref64).abs().max())
    allow = _slack(yard, float(ref64.abs().max()))
    err = (out.detach().double() - ref64).abs()
    store = u * ref64.abs()
    beyond = float((err - store).clamp_min(0).max())
    _note(tag, yard, beyond, allow)
    bad = err > store + allow * (1 + u)
    assert not bool(bad.any()), (
        f"{tag}: {int(bad.sum())} elements off; error beyond the store roundoff {beyond:.3e} "
        f"> E {allow:.3e} (fp32 yardstick {yard:.3e})")


def _check_sum(tag, out, ref64, ref32, terms):
    """Per-channel sums, relative to sum |terms| (terms: fp64, per channel)."""
    den = terms.double().clamp_min(1e-300)
    ref64 = ref64.detach().double()
    yard = float(((ref32.detach().double() - ref64).abs() / den).max())
    allow = max(MARGIN * yard, FLOOR_ULPS * ULP32)
    err = (out.detach().double() - ref64).abs() / den
    store = U_STORE[torch.float32] * ref64.abs() / den
    beyond = float((err - store).clamp_min(0).max())
    _note(tag, yard, beyond, allow)
    bad = err > store + allow
    assert not bool(bad.any()), (
        f"{tag}: {int(bad.sum())} channels off; relative error {beyond:.3e} > E {allow:.3e} "
        f"(fp32 yardstick {yard:.3e})")


def _fwd(ext, x, res=None, gamma=None, beta=None, rm=None, rv=None, nb=None, relu=False,
         training=True, mom=MOM, part=None, rpb=0, fin=None, zero_b=None):
    return ext.bn_fwd(x, res, gamma, beta, rm, rv, training, mom, EPS, relu, nb, part, rpb, fin,
                      zero_b)


def _check_stats(tag, x, out, run, run0, stats64=None, stats32=None, mom=MOM):
    """mean, invstd, running_mean, running_var (unbiased) and the batch counter (exactly +1)."""
    M = x.numel() // x.shape[1]
    mean64, var64 = stats64 if stats64 is not None else _stats(x, torch.float64)
    mean32, var32 = stats32 if stats32 is not None else _stats(x, torch.float32)
    absx = _rows(x).double().abs().mean(0)
    rm0, rv0, nb0 = run0
    ub = M / (M - 1.0) if M > 1 else 1.0     # M = 1: the biased value (0)
    _check_sum(tag + ".mean", out[1], mean64, mean32, absx)
    i64, i32 = torch.rsqrt(var64 + EPS), torch.rsqrt(var32 + EPS)
    _check_sum(tag + ".invstd", out[2], i64, i32, i64)
    if run is None:
        return
    rm, rv, nb = run
    _check_sum(tag + ".running_mean", rm, (1 - mom) * rm0.double() + mom * mean64,
               (1 - mom) * rm0 + mom * mean32, (1 - mom) * rm0.double().abs() + mom * absx)
    _check_sum(tag + ".running_var", rv, (1 - mom) * rv0.double() + mom * ub * var64,
               (1 - mom) * rv0 + mom * ub * var32, (1 - mom) * rv0.double() + mom * ub * var64)
    assert int(nb) == int(nb0) + 1, f"{tag}: num_batches {int(nb0)} -> {int(nb)}"


def _run_stats_case(tag, ext, x, gamma, beta, relu=False, part=None, rpb=0, fin=None,
                    stats64=None, stats32=None):
    """One training forward with running statistics; statistics and y against fp64."""
    C = x.shape[1]
    rm0, rv0, nb0 = _running(C)
    rm, rv, nb = rm0.clone(), rv0.clone(), nb0.clone()
    out = _fwd(ext, x, None, gamma, beta, rm, rv, nb, relu=relu, part=part, rpb=rpb, fin=fin)
    _check_stats(tag, x, out, (rm, rv, nb), (rm0, rv0, nb0), stats64, stats32)
    y64 = _compose(x, None, gamma, beta, relu, torch.float64, stats=stats64)
    y32 = _compose(x, None, gamma, beta, relu, torch.float32, stats=stats32,
                   native=stats32 is None)
    _check_elem(tag + ".y", out[0], y64, y32)
    return out, (rm, rv, nb)


def _n(t):
    """Elements of an optional output (an undefined tensor arrives as None)."""
    return 0 if t is None else t.numel()


def _zero(t):
    if t is not None:
        t.zero_()


def _same(a, b):
    return all(torch.equal(p, q) for p, q in zip(a, b))


def _sentinel(n):
    """A non-zero fp64 slice of n elements inside a larger buffer, and a check that exactly the
    slice was cleared."""
    buf = torch.full((3 * n,), 7.0, dtype=torch.float64, device="cuda")
    sl = buf[n:2 * n]

    def check(tag):
        assert bool((sl == 0).all()), f"{tag}: the set was not cleared"
        assert bool((buf[:n] == 7.0).all()) and bool((buf[2 * n:] == 7.0).all()), \
            f"{tag}: cleared beyond the set"
    return sl, check


def _pos_bits(y):
    """(stored y > 0) in NHWC memory order, from the stored bits (y has no NaN here)."""
    f = _rows(y).reshape(-1)
    return f.view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32) > 0


def _pack(bits):
    w = (1 << torch.arange(8, device=bits.device, dtype=torch.int32))
    return (bits.view(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


def _unpack(mask, like):
    """The mask bits as a 0/1 bool tensor shaped (and laid out) like `like`."""
    N, C, H, W = like.shape
    sh = torch.arange(8, device=mask.device, dtype=torch.int32)
    bits = ((mask.view(-1, 1).to(torch.int32) >> sh) & 1).bool()
    return bits.view(N, H, W, C).permute(0, 3, 1, 2)


def _spread(tot, rep):
    """[rep, 2, C] fp64 set whose replicas sum to tot [2, C]: uneven, one replica all zero."""
    w = {1: [1.0], 2: [0.7, 0.3], 3: [0.9, -0.2, 0.3]}.get(rep, [0.9, -0.2, 0.0, 0.3] +
                                                            [0.0] * (rep - 4))
    s = torch.stack([tot * wi for wi in w])
    return s.contiguous()


# ---------------------------------------------------------------------- A. forward statistics
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("shape", [(8, 32, 9, 11), (3, 2048, 3, 3)])
@pytest.mark.parametrize("path", ["acc", "partials"])
def test_stats_acc_and_own_partials(path, shape, dtype):
    """A1 / A2: the statistics pass in acc mode, and its own partials merged by one finalize
    block per channel group (P = 1)."""
    x, _, gamma, beta, _ = _data(shape, dtype)
    M, C = x.numel() // shape[1], shape[1]
    with knobs(acc=path == "acc") as ext:
        nblk, rpb = ext.bn_reduce_blocks(M, C)
        assert nblk >= 1 and nblk * rpb >= M and ext.bn_acc_ok(M, C)
        if path == "partials":
            assert ext.bn_fin_blocks(nblk) == 1
        out, _ = _run_stats_case(f"A.{path}", ext, x, gamma, beta)
        assert _n(out[4]) == (ext.acc_rep * 2 * C if path == "acc" else 0)
        if path == "acc":   # the sums themselves: (sum x, sum x^2), left in place
            r = _rows(x)
            tot = out[4].view(-1, 2, C).sum(0)
            _check_sum("A.acc.sums1", tot[0], r.double().sum(0), r.float().sum(0),
                       r.double().abs().sum(0))
            _check_sum("A.acc.sums2", tot[1], (r.double() ** 2).sum(0), (r.float() ** 2).sum(0),
                       (r.double() ** 2).sum(0))
            _zero(out[4])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("shape,nblk,P", [((5, 64, 21, 20), 66, 2), ((3, 64, 53, 53), 264, 5)])
def test_stats_own_partials_ticket_merge(shape, nblk, P, dtype):
    """A3: P > 1 finalize blocks per channel group, merged by the last one to take a ticket
    (P = 5: one 4-batch plus the scalar tail). The merge order is fixed: runs are bit-identical,
    and the tickets are left at zero (66 runs visit every ticket set twice)."""
    x, _, gamma, beta, _ = _data(shape, dtype)
    M, C = x.numel() // shape[1], shape[1]
    with knobs(acc=False, geometry=(4096, 1)) as ext:
        assert tuple(ext.bn_reduce_blocks(M, C)) == (nblk, 32)
        assert ext.bn_fin_blocks(nblk) == P
        out, run = _run_stats_case("A.ticket", ext, x, gamma, beta, relu=True)
        assert _n(out[4]) == 0
        for _ in range(66):
            rm, rv, nb = _running(C)
            again = _fwd(ext, x, None, gamma, beta, rm, rv, nb, relu=True)
            assert _same(again[:4], out[:4]) and _same((rm, rv, nb), run)


def test_stats_acc_falls_back_to_partials():
    """A4: acc mode on, but the reduction would emit more than 2^18 (block, channel) sums: the
    pass writes partials and the finalize merges them with P = 17 (a 16-batch plus the tail)."""
    shape = (1, 256, 80, 103)
    x, _, gamma, beta, _ = _data(shape, torch.bfloat16)
    with knobs(geometry=(4096, 1)) as ext:
        assert not ext.bn_acc_ok(8240, 256)
        assert tuple(ext.bn_reduce_blocks(8240, 256)) == (1030, 8)
        assert ext.bn_fin_blocks(1030) == 17
        out, _ = _run_stats_case("A.fallback", ext, x, gamma, beta, relu=True)
        assert _n(out[4]) == 0


def _block_partials(x, rpb):
    """Per-block (mean, M2) of x's rows in fp64, cast to fp32: [nblk, 2, C]; and the rows per
    block."""
    r = _rows(x).double()
    M, C = r.shape
    nblk = (M + rpb - 1) // rpb
    idx = torch.arange(M, device=x.device) // rpb
    n = torch.bincount(idx, minlength=nblk).double()
    mean = torch.zeros(nblk, C, dtype=torch.float64, device=x.device).index_add_(0, idx, r)
    mean = mean / n[:, None]
    m2 = torch.zeros_like(mean).index_add_(0, idx, (r - mean[idx]) ** 2)
    return torch.stack([mean, m2], 1).float().contiguous(), n


def _merge_partials(part, n, dt):
    """(mean, biased var) of the merged partials, evaluated in dt."""
    p, n = part.to(dt), n.to(dt)
    tot = n.sum()
    mean = (n[:, None] * p[:, 0]).sum(0) / tot
    m2 = (p[:, 1] + n[:, None] * (p[:, 0] - mean) ** 2).sum(0)
    return mean, m2 / tot


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("shape,rpb,fin_max,P", [
    ((1, 8, 23, 113), 2, 64, 21), ((1, 8, 23, 113), 2, 7, 7), ((1, 8, 23, 113), 2, 3, 3),
    ((1, 8, 23, 113), 2, 1, 1), ((1, 2048, 10, 13), 1, 64, 3)])
def test_stats_external_partials(shape, rpb, fin_max, P, dtype):
    """A5: hand-made per-block (mean, M2) partials. C = 8: lanes beyond the channels clamp,
    1300 partials with a short last block, P = 21 (16 + 4 + 1), 7 (4 + 3), 3, 1 (each wave loops
    over more than one 16-partial batch). C = 2048: 32 channel groups, a ticket each."""
    x, _, gamma, beta, _ = _data(shape, dtype, seed=5)
    M, C = x.numel() // shape[1], shape[1]
    part, n = _block_partials(x, rpb)
    nblk = part.shape[0]
    assert nblk == (1300 if C == 8 else 130) and int(n[-1]) == M - (nblk - 1) * rpb
    s64, s32 = _merge_partials(part, n, torch.float64), _merge_partials(part, n, torch.float32)
    keep = part.clone()
    with knobs(fin_max=fin_max) as ext:
        assert ext.bn_fin_blocks(nblk) == P
        out, run = _run_stats_case("A.extpart", ext, x, gamma, beta, relu=True, part=part,
                                   rpb=rpb, stats64=s64, stats32=s32)
        assert _n(out[4]) == 0 and torch.equal(part, keep)
        for _ in range(66):   # every ticket set again: they were left at zero
            rm, rv, nb = _running(C)
            again = _fwd(ext, x, None, gamma, beta, rm, rv, nb, relu=True, part=part, rpb=rpb)
            assert _same(again[:4], out[:4]) and _same((rm, rv, nb), run)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("slice_", [1, 0])
def test_stats_fin_replicas_summed(C, slice_, dtype):
    """A6: hand-filled [rep, 2, C] sums (sum x, sum x^2), spread unevenly over the replicas with
    one replica all zero: the apply pass sums every replica and leaves the set in place."""
    shape = (4, C, 7, 7)
    x, _, gamma, beta, _ = _data(shape, dtype, seed=6)
    r = _rows(x).double()
    with knobs(slice_=slice_) as ext:
        fin = _spread(torch.stack([r.sum(0), (r * r).sum(0)]), ext.acc_rep)
        tot = fin[0].clone()
        for k in range(1, fin.shape[0]):
            tot += fin[k]
        mean = tot[0] / r.shape[0]
        s64 = (mean, (tot[1] / r.shape[0] - mean * mean).clamp_min(0))
        keep = fin.clone()
        out, _ = _run_stats_case("A.fin", ext, x, gamma, beta, relu=True, fin=fin, stats64=s64)
        assert out[4].data_ptr() == fin.data_ptr() and torch.equal(fin, keep)


def _edge_paths(ext, x, path):
    """(knob settings, bn_fwd statistics arguments, reference statistics) of an edge case."""
    if path == "extpart":
        part, n = _block_partials(x, 3)
        return dict(), dict(part=part, rpb=3), (_merge_partials(part, n, torch.float64),
                                                _merge_partials(part, n, torch.float32))
    return dict(acc=path == "acc"), dict(), (None, None)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("path", ["acc", "partials", "extpart"])
def test_stats_large_offset_and_constant_channel(path, dtype):
    """A7: x + 1000 with unit variance must keep its variance; a channel constant at 1000.0 has
    variance 0 (the m2 clamp): invstd = 1 / sqrt(eps) and y = beta."""
    shape = (8, 32, 9, 11)
    x, _, gamma, beta, _ = _data(shape, dtype, seed=7, offset=1000.0, scale=1.0)
    x[:, 3] = 1000.0
    ext = _ext()
    kn, args, (s64, s32) = _edge_paths(ext, x, path)
    with knobs(**kn):
        M, C = x.numel() // 32, 32
        assert ext.bn_acc_ok(M, C) and ext.bn_fin_blocks(ext.bn_reduce_blocks(M, C)[0]) == 1
        out, _ = _run_stats_case(f"A.edge.{path}", ext, x, gamma, beta, stats64=s64,
                                 stats32=s32, **args)
        if _n(out[4]):
            _zero(out[4])
    assert abs(float(out[2][3]) * EPS ** 0.5 - 1.0) <= FLOOR_ULPS * ULP32
    assert bool((out[0][:, 3] == beta[3].to(dtype)).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("path", ["acc", "partials", "extpart"])
def test_stats_single_row(path, dtype):
    """A7: M = 1. The biased variance is 0, running_var takes the biased value, y = beta."""
    x, _, gamma, beta, _ = _data((1, 64, 1, 1), dtype, seed=8)
    ext = _ext()
    if path == "extpart":
        part = torch.stack([_rows(x).float(), torch.zeros(1, 64, device="cuda")], 1).contiguous()
        kn, args = dict(), dict(part=part, rpb=1)
    else:
        kn, args = dict(acc=path == "acc"), dict()
    mean = _rows(x)[0]
    with knobs(**kn):
        assert tuple(ext.bn_reduce_blocks(1, 64)) == (1, 32)
        out, (rm, rv, nb) = _run_stats_case(
            f"A.m1.{path}", ext, x, gamma, beta,
            stats64=(mean.double(), torch.zeros(64, dtype=torch.float64, device="cuda")),
            stats32=(mean.float(), torch.zeros(64, device="cuda")), **args)
        if _n(out[4]):
            _zero(out[4])
    assert torch.equal(out[1], mean.float())
    assert torch.equal(_rows(out[0])[0], beta.to(dtype))


# ------------------------------------------------------------------------------ B. apply pass
def _mode(mode):
    return mode.startswith("relu"), mode.endswith("res")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", B_SHAPES)
def test_apply_matrix(shape, mode, dtype):
    """B: y against fp64, the mask bits against the stored y, and the zero_b side duty, for
    non-temporal / plain loads and sliced / flat grids, with at most 64 blocks (several rounds
    per thread, partial tails)."""
    relu, with_res = _mode(mode)
    x, res, gamma, beta, _ = _data(shape, dtype, res=with_res)
    M, C = x.numel() // shape[1], shape[1]
    y64 = _compose(x, res, gamma, beta, relu, torch.float64)
    y32 = _compose(x, res, gamma, beta, relu, torch.float32, native=True)
    rm0, rv0, nb0 = _running(C)
    for nt in (1, 0):
        for sl in (1, 0):
            tag = f"B.apply[{mode},nt{nt},slice{sl}]"
            with knobs(nt=nt, slice_=sl, elem=64) as ext:
                assert ext.bn_acc_ok(M, C)
                zero_b, zcheck = _sentinel(ext.acc_rep * 2 * C)
                rm, rv, nb = rm0.clone(), rv0.clone(), nb0.clone()
                out = _fwd(ext, x, res, gamma, beta, rm, rv, nb, relu=relu, zero_b=zero_b)
                assert _n(out[4]) == ext.acc_rep * 2 * C
                _zero(out[4])
            y = out[0]
            assert y.dtype == dtype and y.is_contiguous(memory_format=torch.channels_last)
            _check_elem(tag + ".y", y, y64, y32)
            _check_stats(tag, x, out, (rm, rv, nb), (rm0, rv0, nb0))
            zcheck(tag)
            if relu:
                assert torch.equal(out[3], _pack(_pos_bits(y))), tag + ": mask bits"
            else:
                assert _n(out[3]) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_mask_is_taken_from_the_stored_value(dtype):
    """B: a channel whose outputs underflow when stored as bf16 (|y| below half the smallest
    bf16 subnormal): the mask must say 0 where the stored y is 0, whatever the unrounded sign."""
    shape = (2, 64, 9, 9)
    x, _, gamma, beta, _ = _data(shape, dtype, seed=9)
    gamma[5] = 2e-41
    beta[5] = 0.0
    with knobs(elem=64) as ext:
        out = _fwd(ext, x, None, gamma, beta, relu=True)
        _zero(out[4])
    bits = _pos_bits(out[0])
    assert torch.equal(out[3], _pack(bits))
    want = _compose(x, None, gamma, beta, True, torch.float64)[:, 5] > 0
    got = _unpack(out[3], x)[:, 5]
    assert bool(want.any())
    if dtype == torch.bfloat16:   # positive before the store, stored as 0: the bit is 0
        under = want & (out[0][:, 5] == 0)
        assert bool(under.any()) and not bool((got & under).any())
    else:
        assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("shape", [(7, 512, 10, 10), (2, 8, 5, 5)])
@pytest.mark.parametrize("sl", [1, 0])
def test_apply_eval_noaffine_norunning(shape, sl, dtype):
    """B: eval mode with and without a residual, gamma / beta None, no running statistics."""
    x, res, gamma, beta, _ = _data(shape, dtype, res=True, seed=10)
    M, C = x.numel() // shape[1], shape[1]
    rm, rv, _ = _running(C)
    with knobs(slice_=sl, elem=64) as ext:
        assert ext.bn_acc_ok(M, C)
        for r in (None, res):
            keep = (rm.clone(), rv.clone())
            out = _fwd(ext, x, r, gamma, beta, rm, rv, None, relu=True, training=False)
            assert _same((rm, rv), keep) and _n(out[3]) == 0 and _n(out[4]) == 0
            s64, s32 = (rm.double(), rv.double()), (rm, rv)
            _check_elem("B.eval.y", out[0],
                        _compose(x, r, gamma, beta, True, torch.float64, stats=s64),
                        _compose(x, r, gamma, beta, True, torch.float32, stats=s32))
        out = _fwd(ext, x, res, None, None, None, None, None, relu=True)
        _zero(out[4])
        _check_stats("B.noaffine", x, out, None, (None, None, None))
        _check_elem("B.noaffine.y", out[0], _compose(x, res, None, None, True, torch.float64),
                    _compose(x, res, None, None, True, torch.float32, native=True))
        assert torch.equal(out[3], _pack(_pos_bits(out[0])))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("kw", [dict(affine=False), dict(track_running_stats=False),
                                dict(momentum=None)], ids=lambda k: next(iter(k)))
def test_module_variants_match_batchnorm2d(kw, dtype):
    """B: affine=False, track_running_stats=False and momentum=None (the cumulative average)
    against nn.BatchNorm2d in fp64 over three steps."""
    from arena_amd.ops.batchnorm import BatchNormAct2d
    C, shape = 64, (4, 64, 9, 7)
    m = BatchNormAct2d(C, act="none", **kw).cuda()
    r64 = torch.nn.BatchNorm2d(C, **kw).cuda().double()
    r32 = torch.nn.BatchNorm2d(C, **kw).cuda()
    if m.affine:
        with torch.no_grad():
            m.weight.copy_(torch.rand(C) + 0.5)
            m.bias.copy_(torch.randn(C) * 0.1)
    r32.load_state_dict(m.state_dict())
    r64.load_state_dict(m.state_dict())
    tag = "B.module." + next(iter(kw))
    with knobs():
        for step in range(3):
            x, _, _, _, dy = _data(shape, dtype, seed=20 + step, offset=step)
            xs = [x.clone().requires_grad_(True), x.double().requires_grad_(True),
                  x.float().requires_grad_(True)]
            y = m(xs[0])
            y64 = r64(xs[1])
            with torch.backends.cudnn.flags(enabled=False):
                y32 = r32(xs[2])
            _check_elem(tag + ".y", y, y64, y32)
            y.backward(dy)
            y64.backward(dy.double())
            y32.backward(dy.float())
            _check_elem(tag + ".dx", xs[0].grad, xs[1].grad, xs[2].grad)
            if m.track_running_stats:
                _check_elem(tag + ".running_mean", m.running_mean, r64.running_mean,
                            r32.running_mean)
                _check_elem(tag + ".running_var", m.running_var, r64.running_var,
                            r32.running_var)
                assert int(m.num_batches_tracked) == step + 1
            else:
                assert m.running_mean is None and m.num_batches_tracked is None
            if m.affine:
                for a, b, c in ((m.weight, r64.weight, r32.weight), (m.bias, r64.bias, r32.bias)):
                    _check_elem(tag + ".dparam", a.grad, b.grad, c.grad)
                    a.grad = b.grad = c.grad = None


# -------------------------------------------------------------------------------- C. backward
def _bwd_ref(x, res, gamma, beta, maskf, dy, dt):
    """(dx, dgamma, dbeta) by autograd of the composition in dt; the ReLU is the forward's
    stored mask, so a flip at the ReLU boundary cannot pass for an error."""
    xd = x.to(dt).detach().clone().requires_grad_(True)
    g = gamma.to(dt).detach().clone().requires_grad_(True)
    b = beta.to(dt).detach().clone().requires_grad_(True)
    y = _compose(xd, res, g, b, False, dt, maskf=maskf, native=dt == torch.float32)
    y.backward(dy.to(dt))
    return xd.grad, g.grad, b.grad


def _bwd_terms(x, maskf, dy):
    """sum |g| and sum |g xhat| per channel (fp64): what dbeta and dgamma are relative to."""
    g = dy.double() if maskf is None else dy.double() * maskf.double()
    mean, var = _stats(x, torch.float64)
    xhat = (x.double() - _bc(mean)) * _bc(torch.rsqrt(var + EPS))
    return g.abs().sum((0, 2, 3)), (g * xhat).abs().sum((0, 2, 3))


def _check_bwd(tag, out, ref64, ref32, terms, dy, maskb, with_res):
    dx, dres, dgamma, dbeta = out[:4]
    _check_elem(tag + ".dx", dx, ref64[0], ref32[0])
    _check_sum(tag + ".dgamma", dgamma, ref64[1], ref32[1], terms[1])
    _check_sum(tag + ".dbeta", dbeta, ref64[2], ref32[2], terms[0])
    if with_res:
        want = dy if maskb is None else torch.where(maskb, dy, torch.zeros_like(dy))
        assert torch.equal(dres, want), tag + ": dres"
    else:
        assert _n(dres) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", B_SHAPES)
def test_bwd_matrix(shape, mode, dtype):
    """C (a) (b) (c): the layer's own sums with coefficients derived in the dx pass; a pool set
    with the acc finalize, three calls in a row (the finalize re-zeroes the set); the BN's own
    partials with P = 1 -- for nt x slice, at most 64 dx blocks."""
    relu, with_res = _mode(mode)
    x, res, gamma, beta, dy = _data(shape, dtype, res=with_res, seed=30)
    M, C = x.numel() // shape[1], shape[1]
    with knobs() as ext:
        f = _fwd(ext, x, res, gamma, beta, relu=relu)
        _zero(f[4])
    mean, invstd, mask = f[1], f[2], (f[3] if relu else None)
    maskb = _unpack(mask, x) if relu else None
    ref64 = _bwd_ref(x, res, gamma, beta, maskb, dy, torch.float64)
    ref32 = _bwd_ref(x, res, gamma, beta, maskb, dy, torch.float32)
    terms = _bwd_terms(x, maskb, dy)

    def call(ext, **kw):
        return ext.bn_bwd(dy, mask, x, mean, invstd, gamma, relu, with_res, True, **kw)

    for nt in (1, 0):
        for sl in (1, 0):
            tag = f"[{mode},nt{nt},slice{sl}]"
            with knobs(nt=nt, slice_=sl, dx=64) as ext:
                assert ext.bn_acc_ok(M, C)
                n = ext.acc_rep * 2 * C
                zero_f, zcheck = _sentinel(n)
                acc_b = torch.zeros(n, dtype=torch.float64, device="cuda")
                out = call(ext, acc_b=acc_b, zero_f=zero_f)
                _check_bwd("C.own" + tag, out, ref64, ref32, terms, dy, maskb, with_res)
                zcheck("C.own" + tag)
                tot = acc_b.view(-1, 2, C).sum(0)   # the sums stay in place
                _check_sum("C.own.sums", tot[0], ref64[2], ref32[2], terms[0])
                for i in range(3):
                    out = call(ext)
                    _check_bwd("C.pool" + tag, out, ref64, ref32, terms, dy, maskb, with_res)
            with knobs(acc=False, nt=nt, slice_=sl, dx=64) as ext:
                assert ext.bn_fin_blocks(ext.bn_reduce_blocks(M, C)[0]) == 1
                out = call(ext)
                _check_bwd("C.part" + tag, out, ref64, ref32, terms, dy, maskb, with_res)


def test_bwd_pool_sets_rezeroed_over_the_whole_pool():
    """C (b): more finalize calls than the pool has sets, one block so the sums are
    order-independent: every call gives the first call's result."""
    x, _, gamma, beta, dy = _data((2, 8, 5, 5), torch.float32, seed=31)
    with knobs() as ext:
        assert tuple(ext.bn_reduce_blocks(50, 8))[0] == 1 and ext.bn_acc_ok(50, 8)
        f = _fwd(ext, x, None, gamma, beta, relu=True)
        _zero(f[4])
        first = ext.bn_bwd(dy, f[3], x, f[1], f[2], gamma, True, False, True)
        for _ in range(300):
            out = ext.bn_bwd(dy, f[3], x, f[1], f[2], gamma, True, False, True)
            assert _same((out[0], out[2], out[3]), (first[0], first[2], first[3]))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_bwd_own_partials_ticket_merge(dtype):
    """C (c): the backward's own partials with P = 2 (66 partials): fp64, bit-identical runs."""
    shape = (5, 64, 21, 20)
    x, res, gamma, beta, dy = _data(shape, dtype, res=True, seed=32)
    with knobs() as ext:
        f = _fwd(ext, x, res, gamma, beta, relu=True)
        _zero(f[4])
    maskb = _unpack(f[3], x)
    ref64 = _bwd_ref(x, res, gamma, beta, maskb, dy, torch.float64)
    ref32 = _bwd_ref(x, res, gamma, beta, maskb, dy, torch.float32)
    terms = _bwd_terms(x, maskb, dy)
    with knobs(acc=False, geometry=(4096, 1), dx=64) as ext:
        assert tuple(ext.bn_reduce_blocks(2100, 64)) == (66, 32) and ext.bn_fin_blocks(66) == 2
        out = ext.bn_bwd(dy, f[3], x, f[1], f[2], gamma, True, True, True)
        _check_bwd("C.ticket", out, ref64, ref32, terms, dy, maskb, True)
        for _ in range(66):
            again = ext.bn_bwd(dy, f[3], x, f[1], f[2], gamma, True, True, True)
            assert _same(again[:4], out[:4])


def _dx_from_sums(x, g, gamma, mean, invstd, a, b, dt):
    """dx, dgamma, dbeta from given totals a = sum g, b = sum g (x - mean), evaluated in dt."""
    M = x.numel() // x.shape[1]
    xd, g, a, b = x.to(dt), g.to(dt), a.to(dt), b.to(dt)
    mean, invstd, gamma = mean.to(dt), invstd.to(dt), gamma.to(dt)
    dx = _bc(gamma * invstd) * (g - _bc(a / M) - (xd - _bc(mean)) * _bc(invstd * invstd * b / M))
    return dx, b * invstd, a


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("fin_max,P", [(64, 21), (7, 7), (1, 1)])
def test_bwd_external_partials(fin_max, P, relu, dtype):
    """C (d): hand-made (sum g, sum g (x - mean)) partials, C = 8, 1300 of them."""
    shape, rpb = (1, 8, 23, 113), 2
    x, _, gamma, beta, dy = _data(shape, dtype, seed=33)
    with knobs() as ext:
        f = _fwd(ext, x, None, gamma, beta, relu=relu)
        _zero(f[4])
    mean, invstd, mask = f[1], f[2], (f[3] if relu else None)
    maskb = _unpack(mask, x) if relu else None
    g = dy.double() * maskb.double() if relu else dy.double()
    gr, xr = _rows(g), _rows(x).double() - mean.double()
    idx = torch.arange(2599, device="cuda") // rpb
    z = torch.zeros(1300, 8, dtype=torch.float64, device="cuda")
    part = torch.stack([z.clone().index_add_(0, idx, gr), z.clone().index_add_(0, idx, gr * xr)],
                       1).float().contiguous()
    ref64 = _dx_from_sums(x, g, gamma, mean, invstd, part.double()[:, 0].sum(0),
                          part.double()[:, 1].sum(0), torch.float64)
    ref32 = _dx_from_sums(x, g, gamma, mean, invstd, part[:, 0].sum(0), part[:, 1].sum(0),
                          torch.float32)
    terms = (part.double()[:, 0].abs().sum(0), part.double()[:, 1].abs().sum(0) * invstd.double())
    with knobs(fin_max=fin_max, dx=64) as ext:
        assert ext.bn_fin_blocks(1300) == P
        out = ext.bn_bwd(dy, mask, x, mean, invstd, gamma, relu, False, True, ext_part=part,
                         ext_rpb=rpb)
        _check_bwd("C.extpart", out, ref64, ref32, terms, dy, maskb, False)
        for _ in range(66):
            again = ext.bn_bwd(dy, mask, x, mean, invstd, gamma, relu, False, True,
                               ext_part=part, ext_rpb=rpb)
            assert _same((again[0], again[2], again[3]), (out[0], out[2], out[3]))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("shape", [(7, 512, 10, 10), (2, 8, 5, 5)])
@pytest.mark.parametrize("sl", [1, 0])
def test_bwd_sums_ready_in_replicas(shape, sl, dtype):
    """C (e): acc_ready: the producer already summed into the layer's set; the sums are spread
    over the replicas (one all zero) and the dx pass must add every replica."""
    x, res, gamma, beta, dy = _data(shape, dtype, res=True, seed=34)
    C = shape[1]
    with knobs() as ext:
        f = _fwd(ext, x, res, gamma, beta, relu=True)
        _zero(f[4])
    mean, invstd, mask = f[1], f[2], f[3]
    maskb = _unpack(mask, x)
    g = dy.double() * maskb.double()
    xc = x.double() - _bc(mean.double())
    tot = torch.stack([g.sum((0, 2, 3)), (g * xc).sum((0, 2, 3))])
    tot32 = torch.stack([g.float().sum((0, 2, 3)), (g.float() * xc.float()).sum((0, 2, 3))])
    ref64 = _dx_from_sums(x, g, gamma, mean, invstd, tot[0], tot[1], torch.float64)
    ref32 = _dx_from_sums(x, g, gamma, mean, invstd, tot32[0], tot32[1], torch.float32)
    terms = (g.abs().sum((0, 2, 3)), (g * xc).abs().sum((0, 2, 3)) * invstd.double())
    with knobs(slice_=sl, dx=64) as ext:
        acc_b = _spread(tot, ext.acc_rep)
        keep = acc_b.clone()
        out = ext.bn_bwd(dy, mask, x, mean, invstd, gamma, True, True, True, acc_b=acc_b,
                         acc_ready=True)
        _check_bwd("C.ready", out, ref64, ref32, terms, dy, maskb, True)
        assert torch.equal(acc_b, keep)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("dxb", [1024, 64])
@pytest.mark.parametrize("sl", [1, 0])
@pytest.mark.parametrize("shape", [(3, 64, 53, 53), (7, 512, 10, 10)])
def test_bwd_second_bn_sums(shape, sl, dxb, dtype):
    """C: the x2 / mean2 / acc2 form: the dx pass also adds the backward sums of a second BN
    (sum g, sum g (x2 - mean2)) into that layer's set. Flat grids with C > 256 have more
    channels than threads per block."""
    x, _, gamma, beta, dy = _data(shape, dtype, seed=35)
    x2 = _data(shape, dtype, seed=36)[0]
    C = shape[1]
    with knobs() as ext:
        f = _fwd(ext, x, None, gamma, beta, relu=True)
        _zero(f[4])
    mean, invstd, mask = f[1], f[2], f[3]
    mean2 = _stats(x2, torch.float64)[0].float()
    g = dy.double() * _unpack(mask, x).double()
    x2c = x2.double() - _bc(mean2.double())
    want = torch.stack([g.sum((0, 2, 3)), (g * x2c).sum((0, 2, 3))])
    want32 = torch.stack([g.float().sum((0, 2, 3)), (g.float() * x2c.float()).sum((0, 2, 3))])
    terms = torch.stack([g.abs().sum((0, 2, 3)), (g * x2c).abs().sum((0, 2, 3))])
    with knobs(slice_=sl, dx=dxb) as ext:
        n = ext.acc_rep * 2 * C
        assert ext.bn_acc_ok(x.numel() // C, C)

        def call(**kw):
            return ext.bn_bwd(dy, mask, x, mean, invstd, gamma, True, False, True,
                              acc_b=torch.zeros(n, dtype=torch.float64, device="cuda"), **kw)
        plain = call()
        acc2 = torch.zeros(ext.acc_rep, 2, C, dtype=torch.float64, device="cuda")
        for k in (1, 2):   # the set accumulates: a second call doubles the totals
            out = call(x2=x2, mean2=mean2, acc2=acc2)
            assert out[4] is not None and out[4].data_ptr() == acc2.data_ptr()
            tot = acc2.sum(0)
            for j, name in ((0, "sum_g"), (1, "sum_gx2")):
                _check_sum("C.s2." + name, tot[j], k * want[j], k * want32[j], k * terms[j])
            assert _same((out[0], out[2], out[3]), (plain[0], plain[2], plain[3]))


# ---------------------------------------------------------------------- D. fused stem pool
POOLS = [(3, 2, 1), (3, 2, 0), (2, 1, 0), (2, 1, 1), (4, 2, 2), (4, 3, 1)]


def _pool_ref(x, gamma, beta, k, s, p, dt, dy=None):
    xd = x.to(dt).detach().clone().requires_grad_(dy is not None)
    g = gamma.to(dt).detach().clone().requires_grad_(dy is not None)
    b = beta.to(dt).detach().clone().requires_grad_(dy is not None)
    y = F.max_pool2d(_compose(xd, None, g, b, True, dt, native=dt == torch.float32), k, s, p)
    if dy is None:
        return y.detach(), None
    y.backward(dy.to(dt))
    return y.detach(), (xd.grad, g.grad, b.grad)


def _pool_terms(x, gamma, beta, dy, k, s, p):
    """sum |g| and sum |g xhat| per channel (fp64), g the pooled gradient at the BN output."""
    t = _compose(x, None, gamma, beta, False, torch.float64).detach().requires_grad_(True)
    F.max_pool2d(F.relu(t), k, s, p).backward(dy.double().abs())
    mean, var = _stats(x, torch.float64)
    xhat = (x.double() - _bc(mean)) * _bc(torch.rsqrt(var + EPS))
    return t.grad.sum((0, 2, 3)), (t.grad * xhat.abs()).sum((0, 2, 3))


def _check_xsel(x, pos, xsel, k, s, p):
    """xsel == x at the reported in-window argmax (kh * k + kw), exactly; argmax inside x."""
    N, C, OH, OW = xsel.shape
    q = pos.view(N, OH, OW, C).long()
    dev = x.device
    h = torch.arange(OH, device=dev)[None, :, None, None] * s - p + q // k
    w = torch.arange(OW, device=dev)[None, None, :, None] * s - p + q % k
    assert bool(((q >= 0) & (q < k * k)).all())
    assert bool(((h >= 0) & (h < x.shape[2]) & (w >= 0) & (w < x.shape[3])).all())
    n = torch.arange(N, device=dev)[:, None, None, None].expand_as(q)
    c = torch.arange(C, device=dev)[None, None, None, :].expand_as(q)
    assert torch.equal(xsel.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1)[n, h, w, c])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("pool", POOLS, ids=lambda t: "k%ds%dp%d" % t)
@pytest.mark.parametrize("hw", [(7, 9), (8, 8), (3, 2)], ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("C", [8, 256])
def test_stem_pool_against_fp64(C, hw, pool, dtype):
    """D: BN + ReLU + max pool fused, against fp64 BN -> ReLU -> max_pool2d with autograd, for
    every pool geometry the launcher takes; statistics as fin sums and as hand-made partials,
    xsel on and off. fp32: output, dx, dgamma, dbeta; bf16 (rounding makes ties fp64 does not
    have): forward only. Both: xsel equals x at the reported argmax."""
    k, s, p = pool
    H, W = hw
    shape = (2, C, H, W)
    M = 2 * H * W
    x, _, gamma, beta, _ = _data(shape, dtype, seed=40)
    ext = _ext()
    rep = ext.acc_rep
    r = _rows(x).double()
    fin0 = _spread(torch.stack([r.sum(0), (r * r).sum(0)]), rep)
    part, _ = _block_partials(x, 5)
    if H + 2 * p < k or W + 2 * p < k:   # no window fits: the launcher must refuse
        with pytest.raises(RuntimeError):
            ext.bn_pool_fwd(x, gamma, beta, None, None, MOM, EPS, None, fin0, None, 0, k, s, p,
                            None, True)
        return
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    torch.manual_seed(41)
    dy = _nhwc(torch.randn(2, C, OH, OW, device="cuda").to(dtype))
    grads = dtype == torch.float32
    y64, g64 = _pool_ref(x, gamma, beta, k, s, p, torch.float64, dy if grads else None)
    y32, g32 = _pool_ref(x, gamma, beta, k, s, p, torch.float32, dy if grads else None)
    terms = _pool_terms(x, gamma, beta, dy, k, s, p) if grads else None
    quads = (1, 16) if pool == (3, 2, 1) else (2,)
    for stats in ("fin", "partials"):
        for with_xsel in (True, False):
            for quad in quads:
                tag = f"D.pool[{stats},xsel{int(with_xsel)}]"
                with knobs(quad=quad):
                    if stats == "partials":
                        assert ext.bn_fin_blocks(part.shape[0]) == 1
                    rm0, rv0, nb0 = _running(C)
                    rm, rv, nb = rm0.clone(), rv0.clone(), nb0.clone()
                    fin = fin0.clone() if stats == "fin" else None
                    zero_b, zcheck = _sentinel(rep * 2 * C)
                    o = ext.bn_pool_fwd(x, gamma, beta, rm, rv, MOM, EPS, nb, fin,
                                        part if stats == "partials" else None,
                                        5 if stats == "partials" else 0, k, s, p, zero_b,
                                        with_xsel)
                    y, pos, mean, invstd, scale, shift, xsel = o
                    zcheck(tag)
                    assert tuple(y.shape) == (2, C, OH, OW)
                    _check_elem(tag + ".y", y, y64, y32)
                    _check_stats(tag, x, (None, mean, invstd), (rm, rv, nb), (rm0, rv0, nb0))
                    if with_xsel:
                        _check_xsel(x, pos, xsel, k, s, p)
                    if not grads:
                        continue
                    acc_b = torch.zeros(rep * 2 * C, dtype=torch.float64, device="cuda")
                    zero_f, fcheck = _sentinel(rep * 2 * C)
                    dx, dgamma, dbeta = ext.bn_pool_bwd(
                        dy, pos, x, mean, invstd, scale, shift, gamma, True, k, s, p, acc_b,
                        zero_f, xsel if with_xsel else None)
                    fcheck(tag)
                    _check_elem(tag + ".dx", dx, g64[0], g32[0])
                    _check_sum(tag + ".dgamma", dgamma, g64[1], g32[1], terms[1])
                    _check_sum(tag + ".dbeta", dbeta, g64[2], g32[2], terms[0])
