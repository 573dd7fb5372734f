"""The convolution variant tables and everything that reasons about variant codes.

A variant is an integer code that the autotuner stores in plans and plan files, so a code keeps
its meaning for good. What a code means is ONE row here per direction -- ``FWD_ROWS`` (forward and
backward-data) and ``WGRAD_ROWS`` -- with the same fields as ``ArenaConvVariant`` /
``ArenaConvWgradVariant`` in ``csrc/ops/abi.h``, whose rows (``kFwdRows`` / ``kWgradRows`` in
``conv_kernels.hip``) instantiate the launches. tests/test_conv.py compares the two tables field
by field and tests/golden/conv_variants.json pins both.

Pure Python (no torch, no extension): the planner and the CPU tests run without a build.
"""
from __future__ import annotations

import os
from typing import Dict, List, NamedTuple, Tuple

V1, V1_W8, V2_TILE, V2_OCC4, V2_HALO_FAMILY = "v1", "v1_w8", "v2", "v2_occ4", "v2_halo"


class FwdVariant(NamedTuple):
    code: int
    base: int             # the unsplit code of the same tile (== code when ksplit == 1)
    bm: int               # output tile: pixels x channels
    bn: int
    family: str
    nwm: int              # waves along bm / bn
    nwn: int
    nbuf: int             # stage buffers (halo: weight ring buffers)
    ksplit: int = 1       # split-K factor of this code
    max_width: int = 0    # halo: the widest image its window holds; 0: no limit
    even_chunks: bool = False   # two wave groups split the 64-channel chunks: C / 64 even
    wide8: bool = False   # an 8-wave halo form (set_halo_wide, for A/Bs)
    c16: bool = False     # has a c16 (stem) form
    phases: bool = False  # runs strided-dgrad phases in one launch
    may_split: bool = False   # the codes kvariant(base, ks) exist

    @property
    def v2(self) -> bool:
        return self.family in (V2_TILE, V2_OCC4, V2_HALO_FAMILY)

    @property
    def halo(self) -> bool:
        return self.family == V2_HALO_FAMILY


class WgradVariant(NamedTuple):
    code: int
    bm: int               # Cout x R*S*C tile
    bn: int
    family: str           # V1 or V2_TILE
    nwm: int
    nwn: int
    nbuf: int
    serial: bool = False  # single stage buffer, four waves per SIMD
    groups: int = 1       # wave groups per block that split its pixel steps
    c16: bool = False


# + SPLIT_STRIDE * (k - 1): the same tile with its K steps split over k blocks (in-kernel ticket
# reduction, bit-reproducible): for the layers whose tile count leaves CUs idle (14x14 / 7x7 at
# batch 128). The kernel takes every k <= SPLIT_STRIDE; the planner offers KSPLITS.
SPLIT_STRIDE = 16
KSPLITS = (2, 3, 4, 6, 8)
# 4096 + i: the v2 tile kernel (conv_kernels.hip conv2_body): 32x32x16 MFMAs, 8-wave 256-row
# tiles (4-wave 128x128), two K steps in flight, epilogue through an fp32 LDS tile. Forward and
# backward-data (incl. the strided phases): plain, masked addend, BatchNorm statistics, BatchNorm-
# backward partials or sums (BNGradLink).
V2 = 4096
HALO_MAX_W = 63


def _v1(code, bm, bn, nbuf):      # 16x16x32 MFMAs on 4 waves; c16 needs BN = 64
    return FwdVariant(code, code, bm, bn, V1, 2, 2, nbuf, c16=bn == 64, may_split=True)


def _w8(code, bn, nbuf):          # 256-row tiles on 8 waves
    return FwdVariant(code, code, 256, bn, V1_W8, 4, 2, nbuf, may_split=True)


def _v2(i, bm, bn, nwm, nwn, nbuf):
    return FwdVariant(V2 + i, V2 + i, bm, bn, V2_OCC4 if nbuf == 1 else V2_TILE, nwm, nwn, nbuf,
                      phases=True)


def _halo(i, bm, bn, nwm, nwn, ring, max_w=HALO_MAX_W, even_chunks=False):
    return FwdVariant(V2 + i, V2 + i, bm, bn, V2_HALO_FAMILY, nwm, nwn, ring, max_width=max_w,
                      even_chunks=even_chunks, wide8=nwm * nwn == 8)


# The forward / backward-data table. Row ORDER is the order the enumerators offer (and the tuner
# times) candidates, which decides ties: it is pinned by tests/golden/conv_candidates.json.
FWD_ROWS: Tuple[FwdVariant, ...] = (
    # 0..3: 128x128, 128x64, 64x128, 64x64, two stage buffers
    _v1(0, 128, 128, 2), _v1(1, 128, 64, 2), _v1(2, 64, 128, 2), _v1(3, 64, 64, 2),
    # + 4: four-stage K pipeline (3 steps in flight); + 8: single stage buffer, serial K loop,
    # high occupancy
    _v1(4, 128, 128, 4), _v1(8, 128, 128, 1), _v1(5, 128, 64, 4), _v1(9, 128, 64, 1),
    _v1(6, 64, 128, 4), _v1(10, 64, 128, 1), _v1(7, 64, 64, 4), _v1(11, 64, 64, 1),
    # 12 / 13: 256x128 / 256x64 tiles on 8 waves, two stage buffers; 14 / 15: three
    _w8(12, 128, 2), _w8(13, 64, 2), _w8(14, 128, 3), _w8(15, 64, 3),
    _v2(0, 256, 128, 4, 2, 3), _v2(1, 256, 256, 2, 4, 2), _v2(2, 128, 128, 2, 2, 2),
    _v2(3, 256, 64, 4, 2, 3), _v2(4, 128, 256, 2, 4, 3), _v2(5, 128, 64, 2, 2, 2),
    _v2(6, 64, 64, 2, 2, 2), _v2(7, 64, 128, 2, 2, 2),
    # serial single-buffer forms with wave-row epilogue bands: 4 waves per SIMD
    _v2(8, 128, 128, 2, 2, 1), _v2(9, 128, 64, 2, 2, 1), _v2(10, 64, 128, 2, 2, 1),
    _v2(11, 64, 64, 2, 2, 1),
    # 3x3 / stride 1 / pad 1 halo forms (width <= 63): the tile's input window is staged once per
    # 64-channel chunk and the nine taps read it shifted (conv_kernels.hip Conv2Geo::HALO)
    _halo(12, 128, 128, 2, 2, 3), _halo(13, 128, 64, 2, 2, 2),
    _halo(14, 128, 64, 2, 2, 2, max_w=31),   # the window of <= 31-wide images (four blocks per CU)
    # 15: two groups of four waves split the 64-channel chunks (two waves per SIMD; even chunk
    # counts only)
    _halo(15, 128, 128, 2, 2, 3, max_w=31, even_chunks=True),
    # 16..18: eight waves, a 256-pixel or 256-channel tile per block (each weight tap staged into
    # LDS feeds twice the MFMAs of a 128x128 tile)
    _halo(16, 256, 128, 4, 2, 3), _halo(17, 128, 256, 2, 4, 3), _halo(18, 256, 64, 4, 2, 3),
)
FWD: Dict[int, FwdVariant] = {r.code: r for r in FWD_ROWS}


def _wg1(code, bm, bn, serial=False):
    return WgradVariant(code, bm, bn, V1, 2, 2, 1 if serial else 2, serial, c16=bn == 64)


def _wg2(code, bm, bn, nwm, nwn, nbuf, groups=1):
    return WgradVariant(code, bm, bn, V2_TILE, nwm, nwn, nbuf, nbuf == 1, groups)


WGRAD_ROWS: Tuple[WgradVariant, ...] = (
    _wg1(0, 128, 128), _wg1(1, 128, 64), _wg1(2, 64, 128), _wg1(3, 64, 64),
    # + 4: serial
    _wg1(4, 128, 128, True), _wg1(5, 128, 64, True), _wg1(6, 64, 128, True),
    _wg1(7, 64, 64, True),
    # 8..11: the v2 weight-gradient kernel (32x32x16 MFMAs, 128/256-wide tiles, two steps in
    # flight)
    _wg2(8, 128, 128, 2, 2, 2), _wg2(9, 256, 128, 4, 2, 2), _wg2(10, 128, 256, 2, 4, 2),
    _wg2(11, 256, 256, 2, 4, 2),
    _wg2(12, 128, 128, 2, 2, 1),   # 12: serial single-buffer, four waves per SIMD
    # 13 / 14: 12 with two / four wave groups per block splitting its pixel steps (the same waves
    # per CU in 1/2 / 1/4 of the blocks: that many fewer fp32 split slabs)
    _wg2(13, 128, 128, 2, 2, 1, groups=2), _wg2(14, 128, 128, 2, 2, 1, groups=4),
)
WGRAD: Dict[int, WgradVariant] = {r.code: r for r in WGRAD_ROWS}


def kvariant(v: int, ks: int) -> int:
    """Variant code of unsplit tile variant ``v`` with its K steps split over ``ks`` blocks."""
    return v + SPLIT_STRIDE * (ks - 1)


def fwd_variant(code: int) -> FwdVariant:
    """The row of a forward code, split codes included (KeyError: no kernel has it)."""
    row = FWD.get(code)
    if row is None and 0 <= code < SPLIT_STRIDE * SPLIT_STRIDE:
        base = FWD.get(code % SPLIT_STRIDE)
        if base is not None and base.may_split:
            row = base._replace(code=code, ksplit=code // SPLIT_STRIDE + 1)
    if row is None:
        raise KeyError(code)
    return row


def split_of(v: int) -> int:
    return fwd_variant(v).ksplit


# Derived views: {code: (bm, bn)} of every code the planner knows (TILES: the splits of KSPLITS
# included), and the subsets by field.
TILES = {r.code: (r.bm, r.bn) for r in FWD_ROWS if not r.v2}
TILES.update({kvariant(r.code, k): (r.bm, r.bn) for r in sorted(FWD_ROWS) if r.may_split
              for k in KSPLITS})
V2_TILES = {r.code: (r.bm, r.bn) for r in FWD_ROWS if r.v2}
V2_HALO = {r.code: (r.bm, r.bn) for r in FWD_ROWS if r.halo}
HALO_SMALL = {r.code: r.max_width for r in FWD_ROWS if r.halo and r.max_width < HALO_MAX_W}
HALO_SPLIT2 = {r.code for r in FWD_ROWS if r.even_chunks}
HALO_WIDE = {r.code for r in FWD_ROWS if r.wide8}
TILES.update(V2_TILES)
WGRAD_TILES = {r.code: (r.bm, r.bn) for r in WGRAD_ROWS}
WGRAD_V2 = {r.code: (r.bm, r.bn) for r in WGRAD_ROWS if r.family == V2_TILE}
WGRAD_GROUPS = {r.code: r.groups for r in WGRAD_ROWS if r.groups > 1}

_HALO_WIDE_ON = True
_V2_ON = os.environ.get("ARENA_CONV_V2", "1") != "0"
_CUS = 256


def set_v2(on: bool) -> None:
    """A/B switch: offer the v2 tile kernel to the autotuner (part of the plan key)."""
    global _V2_ON
    _V2_ON = bool(on)


def set_halo_wide(on: bool) -> None:
    """A/B switch: offer the 8-wave halo forms to the autotuner (part of the plan key)."""
    global _HALO_WIDE_ON
    _HALO_WIDE_ON = bool(on)


def variants_for(cout: int) -> List[int]:
    """Unsplit v1 tile variants for ``cout`` output channels."""
    return [r.code for r in FWD_ROWS if not r.v2 and cout % r.bn == 0]


def v2_variants_for(cout: int) -> List[int]:
    """v2 tile variants for ``cout`` output channels (forward / backward-data, incl. the strided
    phases); the halo forms come from ``halo_variants_for``."""
    return [r.code for r in FWD_ROWS if r.v2 and not r.halo and cout % r.bn == 0] \
        if _V2_ON else []


def halo_variants_for(cout: int, k, stride: int, pad: int, width: int,
                      cin: int | None = None) -> List[int]:
    """The 3x3 halo forms, for a 3x3 / stride 1 / pad 1 convolution of a <= 63-wide image
    (``cin``: the input channels; the two-group forms need an even number of 64-channel chunks)."""
    if not _V2_ON or tuple(k) != (3, 3) or stride != 1 or pad != 1:
        return []
    return [r.code for r in FWD_ROWS
            if r.halo and cout % r.bn == 0 and width <= r.max_width
            and (not r.even_chunks or cin is None or (cin // 64) % 2 == 0)
            and (_HALO_WIDE_ON or not r.wide8)]


def split_variants_for(m: int, cout: int, ktot: int) -> List[int]:
    """Split-K candidates for a GEMM of ``m`` rows, ``cout`` columns and ``ktot`` reduction: for
    tiles whose grid gives fewer than two blocks per CU, the splits that bring it to about 2 or 4
    blocks per CU with at least 4 K steps per slice."""
    out: List[int] = []
    if os.environ.get("ARENA_CONV_KSPLIT", "1") == "0":
        return out
    steps = ktot // 64
    for v in variants_for(cout):
        row = FWD[v]
        if not row.may_split or row.nbuf >= 3:
            continue   # the deep pipelines need long K loops: not split candidates
        tiles = -(-m // row.bm) * (cout // row.bn)
        if tiles >= 2 * _CUS or tiles > 65536:
            continue
        ks_set = set()
        for want in (2 * _CUS, 4 * _CUS):
            need = -(-want // tiles)
            ks = next((k for k in KSPLITS if k >= need), KSPLITS[-1])
            if steps // ks >= 4:
                ks_set.add(ks)
        out += [kvariant(v, k) for k in sorted(ks_set)]
    return out


def pick_variant(m: int, cout: int) -> int:
    """Largest tile that still gives every CU at least two blocks; else the most blocks."""
    best, best_blocks = None, 0
    for v in (0, 1, 2, 3):
        bm, bn = TILES[v]
        if cout % bn:
            continue
        blocks = -(-m // bm) * (cout // bn)
        if blocks >= 2 * _CUS:
            return v
        if blocks > best_blocks:
            best, best_blocks = v, blocks
    return best


def wgrad_variants_for(cin: int, cout: int) -> List[int]:
    return [r.code for r in WGRAD_ROWS if cout % r.bm == 0 and cin % r.bn == 0
            and (r.family == V1 or _V2_ON)]


# blocks per CU the weight-gradient split counts aim at (ARENA_WGRAD_BPC, for A/Bs)
_WGRAD_BPC = tuple(float(b) for b in os.environ.get("ARENA_WGRAD_BPC", "1,2,4").split(","))


def _wgrad_candidates(cin, cout, k):
    """(tile variant, split count) pairs: splits that give ~1, 2 or 4 blocks per CU."""
    out = []
    for v in wgrad_variants_for(cin, cout):
        row = WGRAD[v]
        tiles = (cout // row.bm) * (k[0] * k[1] * cin // row.bn)
        # wave-group forms: a block already holds GRP x 4 waves -- one or two blocks per CU
        bpcs = (1, 2) if row.groups > 1 else _WGRAD_BPC
        for bpc in bpcs:
            blocks = int(bpc * _CUS)
            out.append((v, max(1, -(-blocks // tiles))))
    return sorted(set(out))


def out_hw(h: int, w: int, r: int, s: int, stride: int, pad: int) -> Tuple[int, int]:
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


def plan_candidates(n: int, cin: int, h: int, w: int, cout: int, k, stride: int, pad: int,
                    bn_links: bool) -> Dict[str, list]:
    """Every candidate ``plan_for`` times for one convolution, in timing order: forward codes,
    backward-data codes (stride 1: the flipped-weight forward; else -1, the per-phase heuristic,
    and one tile for every phase), the backward-data codes of the BNGradLink form (stride 1 with
    ``bn_links``), and (variant, splits) weight-gradient pairs."""
    ho, wo = out_hw(h, w, k[0], k[1], stride, pad)

    def tiles_for(c, kc):      # kc: the channels the K loop runs over
        return variants_for(c) + v2_variants_for(c) + halo_variants_for(c, k, stride, pad, w, kc)

    out = {"fwd": tiles_for(cout, cin) + split_variants_for(n * ho * wo, cout, cin * k[0] * k[1]),
           "bwd": [], "bwdbn": [], "wgrad": _wgrad_candidates(cin, cout, k)}
    if stride == 1:
        out["bwd"] = tiles_for(cin, cout) + split_variants_for(n * h * w, cin, cout * k[0] * k[1])
        if bn_links:
            out["bwdbn"] = tiles_for(cin, cout)
    else:
        out["bwd"] = [-1] + variants_for(cin) + v2_variants_for(cin)
    return out
