"""The oracle, the case table and the simulated bugs of the fp32 direct convolutions with the PLAIN epilogue (igemm_kernel in
csrc/conv.hip at OFX_PREC_FP32: the 12 `prec == 0` rows of kTiles, each on every A-side schedule it has -- general gather, scalar
chunk coordinates, halo patch -- and in its three kernel families: OFX_EPI_PLAIN, kEpiPlainT (tanh / sigmoid) and the norm on load).
Not a conftest: imported by name, and importable without a device.  The pattern of bf16_check.py and gru_check.py, whose checker,
guard rows, workspace size and seeding are used, not restated (wino_check.check / worst_ratio / violations, gru_check.GUARD /
WS_BYTES / MAPS, sd_ops_check._gen; wino_check.reference is the cross-check of this oracle in test_fp32_check_host.py).

Out of scope, because each has an oracle of its own: the GRU gate epilogues (gru_check.py), OFX_EPI_FLOW (recurrence_check.py),
kEpiVolPool and nz > 1 (pyramid_check.py), ofx_conv2d_stats (inorm_check.py).

Oracle.  The float64 convolution of the exact fp32 operands, the epilogue in float64 in the kernel's order:
    v = acc scale + shift + addend,   y = act(v),   with `res`: relu(y + res)
    M = conv64(|x|, |w|) |scale| + |shift| + |addend| + |res|
    |out - ref| <= slope K 2^-24 M + extra,   K = wino_check.K_DIRECT (not measured again on the code under test)
ReLU is 1-Lipschitz; tanh and sigmoid carry the bound through their Lipschitz constants 1 and 1/4 plus wc.ACT_ULP, as gru_check
does.  Norm on load: the operand is fmaxf((x - mean) * rstd, 0) formed in float32 by the kernel's formula (conv.hip: a_commit /
norm_a; padding stays 0), and the oracle allows NORM_ULP conv64(|x_norm|, |w|) |scale|, NORM_ULP = 2^-24, for a one-ulp difference of
that fp32 value (a fused multiply-add of the subtraction and the multiplication would be one), as bf16_check.NORM_ULP does.

`reference` asserts of every case, not assumes: |shift| + |addend| + |res| <= the convolution part of M at every element (so
the epilogue's own roundings stay inside the constant); for tanh / sigmoid at least 3/4 of the pre-activations have |v| < 2 (a
saturated activation hides a wrong pre-activation); for the `spread` cases M >> |ref|.

Inputs follow f16_check / bf16_check: seeded N(0, 1.5^2) activations, fan-in-scaled N(0, 1 / K) weights, shift / addend / res
N(0, 0.5^2), scale around 1.  `spread`: channel pairs scaled by 2^-12 ... 2^12 (the weight by the inverse), the second channel of a
pair nearly equal with the opposite weight: M >> |ref|, so a term lost under cancellation shows.

Geometry.  A case may carry `pad` = (padH, padW) and `out_hw` = (Hout, Wout) (wino_check.geometry_of); the default, which every
case of this table has, is 'same' padding k // 2 and the output size that follows.  With either key the reference is
wino_check.conv64_geometry -- zero-pad (after the norm on load: padding stays 0), F.conv2d with no padding, crop -- and `descriptor`
passes the four integers on.  geom_check.py holds the cases off 'same' padding and registers them here (`register`), so that inputs,
oracle, guarded buffers and descriptor are this module's; its `ring` cases (`exact_zero`, `shift_amp`) have outputs with no tap inside
the image, where the accumulator is an exact 0, the shift alone is stored, and the assertion below applies where there is a tap.

Case table.  Every case names the row of kTiles it runs (ROWS) and carries the plan it must reach, (bm, bn, bk, ks, ksplit, mode);
test_fp32_check_host.py holds every case to it through ofx_conv2d_plan and the table to kTiles / tile_has_patch / tile_has_scalar
as conv.hip has them.  Maps: gru_check.MAPS (W 1x8x16 whole patches, R 1x9x17 overhanging / ragged, D 2x16x16), G 1x10x14 (with
Cin 4: K = 36 ends inside a chunk, 140 rows), S 1x8x32 (a seam between two 8x16 patches), Q 1x17x18 (overhanging 16x16 patches,
306 rows) and E 1x16x16 for the K-edge GEMM.  What the plan turned out not to admit, each asserted by the host test:
    split-K at Cout 72    the automatic rule gives a 72-channel layer the 128x32 tile (waste(32) = 1.33 < waste(64) - 0.1), and
                          only an automatic 64x64 plan splits K: the ragged-N split-K cases have Cout 120 (64 + 56)
    a forced BK           of the 256x64, 128x192, 128x96 (BK 16 only) and 128x32 (BK 32 only) tiles is not a choice: the rows
                          exist with one chunk length.  A `tile` that names the other one, or the 2e9 marker on anything but
                          64x64 / BK 32, is OFX_EINVAL (it used to run the row's own chunk length, or one pipeline, silently:
                          found while writing this table, fixed in conv_plan)
    two segments on the   c0 and c1 are multiples of 32 (conv_validate), so a two-segment layer always qualifies for the scalar
    general gather        schedule: only the 128x192 tile, which has none, gathers two segments
Split-K reaches ksplit 2, 3 and 4 at 13, 18 and 27 32-wide chunks; on the halo patch it cuts the 32-channel slabs, so `sk3-patch`
(two slabs) leaves its third split an empty range that parks a zero tile.

Simulated bugs (`simulated_bugs`), each applied on the CPU to the reference's terms, with the cases it concerns in `bugs_for`:
    last_chunk_dropped              the last BK-wide chunk of K missing (every case)
    split_partial_missing / _twice  the second split's partial tile left out of / added twice into the reduction (split-K cases)
    second_pipeline_dropped         the odd 32-wide chunks missing (KS = 2 cases with more than one chunk: `ks2-forced-one-chunk`
                                    has no odd chunk to lose, the bug would be the reference itself there)
    second_segment_four_off         in1 read four channels off (two-segment cases)
    halo_staged_zero                the halo column right of / row below a patch staged as zero, at the pixels next to it
                                    (halo-patch cases whose map has such a seam inside it)
    padding_normalised              padding run through the norm instead of left at 0 (norm cases with a padded filter: not the
                                    1x1 `n-128x64-scalar-1x1`, which reads no padding)
    norm_relu_missing               the norm's ReLU left out (norm cases)
    scale_after_shift               (acc + shift) scale (cases with both)
    res_before_activation           act(v + res) instead of relu(act(v) + res) (cases with res)
    columns_slipped_by_a_sub_tile   output columns shifted by one 32-wide sub-tile (out-slice cases and the 96- / 192-wide tiles)
"""
import functools
import math

import torch
import torch.nn.functional as F

import gru_check as gc
import sd_ops_check as SC
import wino_check as wc

GUARD = gc.GUARD
WS_BYTES = gc.WS_BYTES
NORM_ULP = 2.0 ** -24
NORM_EPS = 1e-5
ACTS = {None: 0, "relu": 1, "sigmoid": 2, "tanh": 3}                    # include/ofx.h
NAN = float("nan")
K_FP32 = wc.K_DIRECT
MAPS = dict(gc.MAPS, G=(1, 10, 14), S=(1, 8, 32), Q=(1, 17, 18), E=(1, 16, 16))
FILTERS = {"3x3": (3, 3), "1x5": (1, 5), "5x1": (5, 1), "1x1": (1, 1), "7x7": (7, 7)}
GATHER, SCALAR, PATCH = 0, 1, 2
MODE_NAME = {GATHER: "gather", SCALAR: "scalar", PATCH: "patch"}
FAMILIES = ("plain", "plaint", "norm")

# the fp32 rows of kTiles: name -> (the `tile` that forces it, bm, bn, bk, ks, split-K).  The split-K row has no forcing value:
# it is reached by tile == 0 with a workspace; the paired row by tile + 2e9 or by the automatic small-grid rule
ROWS = {
    "128x128": (16128128, 128, 128, 16, 1, False), "256x64": (16256064, 256, 64, 16, 1, False),
    "128x192": (16128192, 128, 192, 16, 1, False), "128x96": (16128096, 128, 96, 16, 1, False),
    "128x64": (16128064, 128, 64, 16, 1, False), "128x128k32": (32128128, 128, 128, 32, 1, False),
    "128x64k32": (32128064, 128, 64, 32, 1, False), "128x32": (32128032, 128, 32, 32, 1, False),
    "64x64k16": (16064064, 64, 64, 16, 1, False), "64x64sk": (0, 64, 64, 32, 1, True),
    "64x64x2": (2032064064, 64, 64, 32, 2, False), "64x64": (32064064, 64, 64, 32, 1, False),
}


def row_key(row):
    """(bm, bn, bk, ks, sk): a row as kTiles names it."""
    return ROWS[row][1:]


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table

CASES = []


def _c(name, mp, c0, cout, filt, row, mode, *, ksplit=1, auto=False, stride=1, c1=0, **extra):
    """One case: map, channels, filter, the row of kTiles and the A-side schedule it must reach.  auto: tile == 0 (the split-K row
    always; its cases carry a workspace)."""
    tile, bm, bn, bk, ks, sk = ROWS[row]
    assert (ksplit > 1) == sk
    if sk:
        extra["ws"] = True
    B, H, W = MAPS[mp]
    kh, kw = FILTERS[filt]
    fam = "norm" if extra.get("norm") else "plaint" if extra.get("act") in ("tanh", "sigmoid") else "plain"
    CASES.append(dict(name=name, map=mp, B=B, H=H, W=W, c0=c0, c1=c1, cout=cout, kh=kh, kw=kw, stride=stride, row=row, fam=fam,
                      tile=0 if auto else tile, plan=(bm, bn, bk, ks, ksplit, mode), extra=extra))


# ---- OFX_EPI_PLAIN: every row on every schedule it has
_c("p-128x128-patch-seam-x2", "S", 32, 72, "1x5", "128x128", PATCH, c1=32)            # two segments on a BK 16 row, in the patch
_c("p-128x128-patch-over", "R", 32, 72, "3x3", "128x128", PATCH)
_c("p-128x128-scalar-s2", "Q", 32, 72, "3x3", "128x128", SCALAR, stride=2)
_c("p-128x128-gather", "G", 4, 72, "3x3", "128x128", GATHER)
_c("p-256x64-patch", "D", 32, 64, "3x3", "256x64", PATCH)
_c("p-256x64-patch-over", "Q", 32, 72, "3x3", "256x64", PATCH)
_c("p-256x64-scalar-1x1", "Q", 32, 64, "1x1", "256x64", SCALAR)                       # off the patch: 306 rows, two tiles
_c("p-256x64-scalar-s2", "D", 32, 64, "3x3", "256x64", SCALAR, stride=2)
_c("p-256x64-gather", "Q", 4, 72, "3x3", "256x64", GATHER)
_c("p-128x192-patch-200", "R", 32, 200, "3x3", "128x192", PATCH)
_c("p-128x192-gather-200", "G", 4, 200, "3x3", "128x192", GATHER)
_c("p-128x192-gather-x2", "R", 32, 96, "1x1", "128x192", GATHER, c1=32)               # no scalar schedule: two segments gathered
_c("p-128x96-patch-96", "W", 32, 96, "3x3", "128x96", PATCH)
_c("p-128x96-patch-200", "R", 32, 200, "3x3", "128x96", PATCH)                        # three N tiles
_c("p-128x96-gather-96", "G", 4, 96, "3x3", "128x96", GATHER)
_c("p-128x96-gather-200", "G", 4, 200, "3x3", "128x96", GATHER)
_c("p-128x96-scalar-s2", "Q", 32, 96, "3x3", "128x96", SCALAR, stride=2)
_c("p-128x64-patch-5x1", "D", 32, 64, "5x1", "128x64", PATCH)                         # the vertical halo across a batch seam
_c("p-128x64-scalar-x2-s2", "Q", 32, 72, "3x3", "128x64", SCALAR, stride=2, c1=32)    # two segments on a BK 16 row, off the patch
_c("p-128x64-gather", "G", 4, 72, "3x3", "128x64", GATHER)
_c("p-128x128k32-scalar-x2", "R", 32, 72, "3x3", "128x128k32", SCALAR, c1=32)         # two segments on a BK 32 128-row tile
_c("p-128x128k32-k324", "E", 324, 72, "1x1", "128x128k32", GATHER)                    # K = 324 ends 4 into a 32-chunk
_c("p-128x128k32-c48", "G", 48, 72, "3x3", "128x128k32", GATHER)                      # Cin 48: a tap straddles 32-chunks
_c("p-128x64k32-scalar", "R", 64, 72, "3x3", "128x64k32", SCALAR)
_c("p-128x64k32-k324", "E", 324, 72, "1x1", "128x64k32", GATHER)
_c("p-128x32-cout2-scalar", "R", 32, 2, "3x3", "128x32", SCALAR)
_c("p-128x32-cout24-scalar-x2", "R", 32, 24, "1x1", "128x32", SCALAR, c1=32)
_c("p-128x32-cout2-gather", "G", 4, 2, "3x3", "128x32", GATHER)
_c("p-128x32-cout24-gather", "G", 4, 24, "3x3", "128x32", GATHER)
_c("p-64x64k16-scalar", "R", 32, 72, "3x3", "64x64k16", SCALAR)
_c("p-64x64k16-gather", "G", 4, 72, "3x3", "64x64k16", GATHER)
_c("p-64x64-patch-x2", "W", 32, 64, "3x3", "64x64", PATCH, c1=32)                     # two segments on a BK 32 row, in the patch
_c("p-64x64-patch-seam", "D", 32, 72, "1x5", "64x64", PATCH)                          # 8x8 patches side by side
_c("p-64x64-scalar", "R", 32, 72, "3x3", "64x64", SCALAR)
_c("p-64x64-gather", "G", 4, 72, "3x3", "64x64", GATHER)
_c("ks2-forced-k36", "G", 4, 72, "3x3", "64x64x2", GATHER)                            # exactly two chunks
_c("ks2-forced-one-chunk", "R", 32, 64, "1x1", "64x64x2", SCALAR)                     # the second pipeline has nothing to do
_c("ks2-auto-9-chunks", "W", 32, 64, "3x3", "64x64x2", SCALAR, auto=True)             # small grid, no workspace, Kpad 288: odd count
_c("sk3-patch", "W", 64, 64, "3x3", "64x64sk", PATCH, ksplit=3)                       # 18 chunks; two 32-channel slabs for three splits
_c("sk2-patch", "D", 96, 64, "1x5", "64x64sk", PATCH, ksplit=2)                       # 15 chunks; slabs 2 + 1
_c("sk4-scalar", "R", 96, 120, "3x3", "64x64sk", SCALAR, ksplit=4)                    # 27 chunks; ragged M (153) and N (120)
_c("sk2-gather", "G", 44, 120, "3x3", "64x64sk", GATHER, ksplit=2)                    # K = 396: 13 chunks, 7 + 6; ragged M and N
# strides and taps on the automatic plan
_c("auto-1x1-s2", "R", 32, 64, "1x1", "64x64", SCALAR, auto=True, stride=2)           # Kpad 32 < 256: not paired
_c("auto-stem-7x7-s2", "Q", 4, 64, "7x7", "64x64", GATHER, auto=True, stride=2, zero_last=True)   # Cin 3 + a zero channel
# epilogue
_c("e-ssrr-patch", "W", 32, 64, "3x3", "128x64", PATCH, scale=True, shift=True, res=True, act="relu")
_c("e-ssrr-gather", "G", 20, 72, "3x3", "64x64k16", GATHER, scale=True, shift=True, res=True, act="relu")
_c("e-ssrr-sk", "R", 96, 120, "3x3", "64x64sk", SCALAR, ksplit=4, scale=True, shift=True, res=True, act="relu")
_c("e-addend-shift-gather", "G", 12, 72, "3x3", "128x128", GATHER, addend=True, shift=True, ldadd=96)
_c("e-addend-shift-patch", "R", 32, 72, "3x3", "128x64", PATCH, addend=True, shift=True, ldadd=96)
_c("o-slice-126-gather", "G", 4, 126, "3x3", "64x64", GATHER, ldo=384, out_off=64)
_c("o-slice-126-patch", "W", 32, 126, "3x3", "128x128", PATCH, ldo=384, out_off=64)
_c("o-slice-126-128x96", "R", 32, 126, "3x3", "128x96", PATCH, ldo=384, out_off=64)
_c("o-slice-126-128x192", "G", 4, 126, "3x3", "128x192", GATHER, ldo=384, out_off=64)
# M >> |ref|
_c("s-spread-patch", "W", 32, 72, "3x3", "128x64", PATCH, spread=True)
_c("s-spread-gather", "G", 8, 72, "3x3", "128x128k32", GATHER, spread=True)
_c("s-spread-ks2", "W", 32, 64, "3x3", "64x64x2", SCALAR, auto=True, spread=True)
# ---- kEpiPlainT: every row, on the patch where it has one and on one schedule off it
_c("t-128x128-patch", "W", 32, 72, "3x3", "128x128", PATCH, act="tanh", shift=True)
_c("t-128x128-gather", "G", 8, 72, "3x3", "128x128", GATHER, act="sigmoid")
_c("t-256x64-patch", "D", 32, 64, "3x3", "256x64", PATCH, act="tanh")
_c("t-256x64-scalar", "Q", 32, 64, "1x1", "256x64", SCALAR, act="sigmoid", shift=True)
_c("t-128x192-patch", "W", 32, 96, "3x3", "128x192", PATCH, act="tanh")
_c("t-128x192-gather", "G", 8, 200, "3x3", "128x192", GATHER, act="sigmoid")
_c("t-128x96-patch", "R", 32, 96, "3x3", "128x96", PATCH, act="sigmoid")
_c("t-128x96-scalar", "Q", 32, 96, "3x3", "128x96", SCALAR, stride=2, act="tanh")
_c("t-128x64-patch", "W", 32, 64, "1x5", "128x64", PATCH, act="tanh")
_c("t-128x64-gather", "G", 8, 72, "3x3", "128x64", GATHER, act="tanh")
_c("t-128x128k32-scalar", "R", 32, 72, "3x3", "128x128k32", SCALAR, act="tanh")
_c("t-128x64k32-gather", "G", 48, 72, "3x3", "128x64k32", GATHER, act="sigmoid")
_c("t-128x32-scalar", "R", 32, 24, "3x3", "128x32", SCALAR, act="tanh")
_c("t-64x64k16-gather", "G", 8, 72, "3x3", "64x64k16", GATHER, act="sigmoid")
_c("t-64x64-patch", "W", 32, 64, "3x3", "64x64", PATCH, act="tanh")
_c("t-64x64-scalar", "R", 32, 72, "3x3", "64x64", SCALAR, act="sigmoid")
_c("t-ks2-auto", "W", 32, 64, "3x3", "64x64x2", SCALAR, auto=True, act="tanh")
_c("t-sk3-patch", "W", 64, 64, "3x3", "64x64sk", PATCH, ksplit=3, act="tanh")
_c("t-sk2-gather", "G", 44, 120, "3x3", "64x64sk", GATHER, ksplit=2, act="sigmoid")
# ---- norm on load: likewise
_c("n-128x128-patch", "W", 32, 72, "3x3", "128x128", PATCH, norm=True, act="relu")
_c("n-128x128-scalar", "Q", 32, 72, "3x3", "128x128", SCALAR, stride=2, norm=True)
_c("n-256x64-patch-over", "Q", 32, 64, "3x3", "256x64", PATCH, norm=True)             # padding and overhang must both stay 0
_c("n-256x64-gather", "Q", 4, 64, "3x3", "256x64", GATHER, norm=True)
_c("n-128x192-patch", "R", 32, 96, "3x3", "128x192", PATCH, norm=True)
_c("n-128x192-gather", "G", 8, 200, "3x3", "128x192", GATHER, norm=True, act="relu")
_c("n-128x96-patch", "W", 32, 96, "3x3", "128x96", PATCH, norm=True)
_c("n-128x96-gather", "G", 8, 96, "3x3", "128x96", GATHER, norm=True)
_c("n-128x64-patch", "D", 32, 64, "3x3", "128x64", PATCH, norm=True)                  # two images: statistics per image
_c("n-128x64-scalar-1x1", "R", 32, 72, "1x1", "128x64", SCALAR, norm=True)
_c("n-128x128k32-gather", "G", 48, 72, "3x3", "128x128k32", GATHER, norm=True)
_c("n-128x64k32-scalar", "R", 32, 72, "3x3", "128x64k32", SCALAR, norm=True)
_c("n-128x32-gather", "G", 8, 24, "3x3", "128x32", GATHER, norm=True)
_c("n-64x64k16-scalar", "D", 32, 64, "3x3", "64x64k16", SCALAR, stride=2, norm=True)
_c("n-64x64-patch", "D", 32, 64, "3x3", "64x64", PATCH, norm=True)
_c("n-64x64-gather", "G", 8, 72, "3x3", "64x64", GATHER, norm=True)
_c("n-ks2-forced", "G", 8, 72, "3x3", "64x64x2", GATHER, norm=True)                   # three chunks
_c("n-sk3-patch", "W", 64, 64, "3x3", "64x64sk", PATCH, ksplit=3, norm=True)
_c("n-sk4-scalar", "R", 96, 120, "3x3", "64x64sk", SCALAR, ksplit=4, norm=True, act="relu")
IDS = [c["name"] for c in CASES]
assert len(set(IDS)) == len(IDS)


OTHER = {}                          # cases of another table that uses this module's inputs, oracle and launch (geom_check.py), by name


def register(c):
    """Make a case of another table known to `case` (hence to inputs / reference / buffers).  Its name must be new."""
    assert c["name"] not in IDS and c["name"] not in OTHER, c["name"]
    OTHER[c["name"]] = c
    return c


def case(name):
    return OTHER[name] if name in OTHER else CASES[IDS.index(name)]


def pad_of(c):
    """(padH, padW): the case's optional `pad`, default 'same' (k // 2)."""
    return wc.geometry_of(c)[0]


def out_hw(c):
    """(Hout, Wout): the case's optional `out_hw`, default the size that follows from the padding."""
    return wc.geometry_of(c)[1]


def pad_amounts(c):
    """(top, bottom, left, right) zeros around the case's image (wino_check.pad_amounts)."""
    return wc.pad_amounts(c["H"], c["W"], c["kh"], c["kw"], c["stride"], pad_of(c), out_hw(c))


def rows_of(c):
    Ho, Wo = out_hw(c)
    return c["B"] * Ho * Wo


def k_of(c):
    return c["kh"] * c["kw"] * (c["c0"] + c["c1"])


def covered():
    """{(row name, family, mode)} the table reaches."""
    return {(c["row"], c["fam"], c["plan"][5]) for c in CASES}


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs

@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict of float32 CPU tensors: x [B,H,W,c0 + c1], w OIHW, and whichever of scale / shift [cout], addend / res [B,Ho,Wo,cout],
    nmean / nrstd [B,c0] the case has (else None)."""
    c = case(name)
    e = c["extra"]
    g = SC._gen("fp32-" + name)
    B, H, W, cin, co, kh, kw = c["B"], c["H"], c["W"], c["c0"] + c["c1"], c["cout"], c["kh"], c["kw"]
    x = torch.randn((B, H, W, cin), generator=g) * 1.5
    w = torch.randn((co, cin, kh, kw), generator=g) / math.sqrt(cin * kh * kw)
    if e.get("zero_last"):
        x[..., cin - 1] = 0.0
    if e.get("spread"):
        pair = torch.arange(cin) // 2
        s = torch.ldexp(torch.ones(cin), ((7 * pair) % 25 - 12).int())
        x[..., 1::2] = x[..., 0::2] * (1.0 + 2.0 ** -6 * torch.randn((B, H, W, cin // 2), generator=g))
        w[:, 1::2] = -w[:, 0::2]
        x, w = x * s, w / s.view(1, -1, 1, 1)
    if e.get("norm"):
        x = x * (0.5 + torch.rand((cin,), generator=g)) + torch.randn((cin,), generator=g)
    Ho, Wo = out_hw(c)
    t = dict(x=x, w=w, scale=None, shift=None, addend=None, res=None, nmean=None, nrstd=None)
    if e.get("scale"):
        t["scale"] = 1.0 + 0.25 * torch.randn((co,), generator=g)
    if e.get("shift"):
        t["shift"] = e.get("shift_amp", 0.5) * torch.randn((co,), generator=g)
    if e.get("addend"):
        t["addend"] = 0.5 * torch.randn((B, Ho, Wo, co), generator=g)
    if e.get("res"):
        t["res"] = 0.5 * torch.randn((B, Ho, Wo, co), generator=g)
    if e.get("norm"):
        f = x.reshape(B, H * W, cin)
        t["nmean"] = f.mean(1).contiguous()
        t["nrstd"] = (1.0 / torch.sqrt(f.var(1, unbiased=False) + NORM_EPS)).contiguous()
    return t


def norm_on_load(x, mean, rstd, relu=True):
    """The operand the kernel multiplies (header): float32, one subtraction, one multiplication, ReLU."""
    assert x.dtype == mean.dtype == rstd.dtype == torch.float32
    v = (x - mean[:, None, None, :]) * rstd[:, None, None, :]
    return torch.relu(v) if relu else v


def conv(c, x, w, padded=False):
    """x NHWC, w OIHW (any float dtype) -> the case's convolution in float64, NHWC.  padded: x already carries its padding
    (pad_amounts).  A case with a geometry of its own (`pad` / `out_hw`) goes through wino_check.conv64_geometry."""
    if "pad" in c or "out_hw" in c:
        return wc.conv64_geometry(x, w, c["stride"], pad_of(c), out_hw(c), padded)
    pad = (0, 0) if padded else (c["kh"] // 2, c["kw"] // 2)
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=c["stride"], padding=pad).permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle

class Ref:
    """The float64 side of one case: c, t (inputs), x (the operand that is multiplied: after the norm on load), acc, v, out, mag,
    slope, extra, unsaturated."""

    def epilogue(self, acc, scale_after_shift=False, res_before_activation=False):
        """acc [B,Ho,Wo,cout] float64 -> (v, out): the pre-activation and the stored value."""
        t, act = self.t, self.c["extra"].get("act")
        sc = 1.0 if t["scale"] is None else t["scale"].double()
        sh = 0.0 if t["shift"] is None else t["shift"].double()
        v = (acc + sh) * sc if scale_after_shift else acc * sc + sh
        if t["addend"] is not None:
            v = v + t["addend"].double()
        f = torch.tanh if act == "tanh" else torch.sigmoid if act == "sigmoid" else torch.relu if act == "relu" else (lambda z: z)
        if t["res"] is None:
            return v, f(v)
        return v, f(v + t["res"].double()) if res_before_activation else torch.relu(f(v) + t["res"].double())


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    e, t = c["extra"], inputs(name)
    r = Ref()
    r.c, r.t = c, t
    r.x = t["x"]
    if e.get("norm"):
        assert c["c1"] == 0
        r.x = norm_on_load(t["x"], t["nmean"], t["nrstd"])
    conv_abs = conv(c, r.x.abs(), t["w"].abs())
    r.acc = conv(c, r.x, t["w"])
    sc = torch.ones((), dtype=torch.float64) if t["scale"] is None else t["scale"].double().abs()
    mag = conv_abs * sc
    derived = NORM_ULP * conv_abs * sc if e.get("norm") else torch.zeros_like(conv_abs)
    side = sum((t[n].double().abs() for n in ("shift", "addend", "res") if t[n] is not None), torch.zeros_like(mag))
    r.no_tap = conv_abs == 0                                             # outputs with no tap inside the image (a geometry's ring)
    if e.get("exact_zero"):
        # there the accumulator is an exact 0 and 0 * scale + shift rounds nowhere: the epilogue's roundings need no cover, as long
        # as nothing else is added (the caller holds such outputs to relu(shift) bit for bit)
        assert bool(r.no_tap.any()) and t["addend"] is None and t["res"] is None and t["scale"] is None and not e.get("norm"), name
        assert bool(((side <= mag) | r.no_tap).all()), f"{name}: |shift| above the convolution's magnitude where it has one"
    else:
        assert bool((side <= mag).all()), f"{name}: |shift| + |addend| + |res| above the convolution's magnitude"
    r.mag = mag + side
    r.v, r.out = r.epilogue(r.acc)
    act = e.get("act")
    r.slope = 0.25 if act == "sigmoid" else 1.0
    r.extra = r.slope * derived + (wc.ACT_ULP if act in ("tanh", "sigmoid") else 0.0)
    r.unsaturated = float((r.v.abs() < 2).double().mean())
    if act in ("tanh", "sigmoid"):
        assert r.unsaturated >= 0.75, (name, r.unsaturated)
    if e.get("spread"):
        r.cancel = float(r.mag.mean() / r.out.abs().mean())
        assert r.cancel > 16, (name, r.cancel)
    return r


def violates(r, got, K=K_FP32):
    return bool(wc.violations(got, r.out, r.mag, K, r.slope, r.extra).any())


def check(r, got, what, K=K_FP32):
    """Assert the bound and return the worst ratio."""
    return wc.check(got, r.out, r.mag, K, what, r.slope, r.extra)


def ratio(r, got):
    return wc.worst_ratio(got, r.out, r.mag, r.slope, r.extra)


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch: one descriptor for the host's plan query and the device run

def ldo_of(c):
    return c["extra"].get("ldo", c["cout"])


def out_off_of(c):
    return c["extra"].get("out_off", 0)


def ldadd_of(c):
    return c["extra"].get("ldadd", c["cout"])


def _guarded(body, ld=None):
    """[GUARD + rows + GUARD, ld] of NaN with `body` [rows, <= ld] in its first columns."""
    body = body.reshape(-1, body.shape[-1])
    buf = torch.full((body.shape[0] + 2 * GUARD, ld or body.shape[1]), NAN)
    buf[GUARD:GUARD + body.shape[0], :body.shape[1]] = body
    return buf


def buffers(c, t=None):
    """{name: CPU float32 [GUARD + rows + GUARD, ld]} of everything the descriptor points at but the workspace: NaN guard rows
    around every one, NaN in the addend's columns past Cout, `out` all NaN over its full ldo.  t: the tensors, default the case's
    `inputs` (a table with inputs of its own passes them in this module's layout)."""
    from sd_animation_optical_flow_amd import ops
    t = inputs(c["name"]) if t is None else t
    b = dict(in0=_guarded(t["x"][..., :c["c0"]]), w=_guarded(ops.pack_conv_weight(t["w"])),
             out=torch.full((rows_of(c) + 2 * GUARD, ldo_of(c)), NAN))
    if c["c1"]:
        b["in1"] = _guarded(t["x"][..., c["c0"]:])
    for n in ("scale", "shift"):
        if t[n] is not None:
            b[n] = _guarded(t[n][None])
    if t["addend"] is not None:
        b["addend"] = _guarded(t["addend"], ldadd_of(c))
    if t["res"] is not None:
        b["res"] = _guarded(t["res"])
    for n in ("nmean", "nrstd"):
        if t[n] is not None:
            b[n] = _guarded(t[n])
    return b


def descriptor(c, ptr, ws=0):
    """The case's ConvDesc.  ptr(buffer name) -> the address of row 0 of its body (past the guard rows); ws: the address of
    WS_BYTES of split-K workspace for the cases that carry one."""
    from sd_animation_optical_flow_amd import _lib
    e = c["extra"]
    Ho, Wo = out_hw(c)
    d = _lib.ConvDesc()
    d.in0, d.ld0, d.c0 = ptr("in0"), c["c0"], c["c0"]
    if c["c1"]:
        d.in1, d.ld1, d.c1 = ptr("in1"), c["c1"], c["c1"]
    d.w = ptr("w")
    d.out, d.ldo = ptr("out") + 4 * out_off_of(c), ldo_of(c)
    if e.get("scale"):
        d.scale = ptr("scale")
    if e.get("shift"):
        d.shift = ptr("shift")
    if e.get("addend"):
        d.addend, d.ldadd = ptr("addend"), ldadd_of(c)
    if e.get("res"):
        d.res, d.ldres = ptr("res"), c["cout"]
    if e.get("norm"):
        d.nmean, d.nrstd = ptr("nmean"), ptr("nrstd")
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = c["B"], c["H"], c["W"], Ho, Wo, c["cout"]
    d.KH, d.KW, d.stride, (d.padH, d.padW) = c["kh"], c["kw"], c["stride"], pad_of(c)
    d.act, d.epi, d.tile, d.precision = ACTS[e.get("act")], 0, c["tile"], c.get("precision", 0)
    if e.get("ws"):
        d.splitk_ws, d.splitk_ws_bytes = ws, WS_BYTES
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# simulated kernel bugs

def _k_index(c):
    """The packed index k = (ky KW + kx) cin + ci of every weight element, as an [cin, kh, kw] tensor."""
    cin, kh, kw = c["c0"] + c["c1"], c["kh"], c["kw"]
    ci, ky, kx = torch.meshgrid(torch.arange(cin), torch.arange(kh), torch.arange(kw), indexing="ij")
    return (ky * kw + kx) * cin + ci


def _masked(w, keep):
    """w OIHW with the elements outside the [cin, kh, kw] mask `keep` zeroed."""
    return w * keep.to(w.dtype)[None]


def chunk_masks(c, bk):
    """The [cin, kh, kw] masks of the BK-wide chunks of K, in the kernel's order."""
    kidx = _k_index(c)
    return [(kidx >= k0) & (kidx < k0 + bk) for k0 in range(0, k_of(c), bk)]


def patch_hw(c):
    bm = c["plan"][0]
    return (16, 16) if bm == 256 else (8, 16) if bm == 128 else (8, 8)


def seam_axis(c):
    """'x' / 'y': the axis along which the patches of a halo-patch case meet under a tap of the filter; None: no such seam."""
    if c["plan"][5] != PATCH:
        return None
    ph, pw = patch_hw(c)
    return "x" if c["kw"] > 1 and c["W"] > pw else "y" if c["kh"] > 1 and c["H"] > ph else None


def second_split(c):
    """The [cin, kh, kw] mask of the second split's share of K: 32-channel slabs on the halo patch, 32-wide chunks off it, each split
    ceil(count / ksplit) of them (conv.hip: cb_per / per_split)."""
    S, kidx = c["plan"][4], _k_index(c)
    if c["plan"][5] == PATCH:
        per = -(-((c["c0"] + c["c1"]) // 32) // S)
        ci = torch.arange(c["c0"] + c["c1"])[:, None, None].expand_as(kidx)
        return (ci >= 32 * per) & (ci < 64 * per)
    per = -(-(-(-k_of(c) // 32)) // S)
    return (kidx >= 32 * per) & (kidx < 64 * per)


def bugs_for(c):
    """The names of the simulated bugs that concern case c (header)."""
    e, (bm, bn, bk, ks, ksplit, mode) = c["extra"], c["plan"]
    names = {"last_chunk_dropped"}
    if ksplit > 1:
        names |= {"split_partial_missing", "split_partial_twice"}
    if ks == 2 and k_of(c) > 32:
        names.add("second_pipeline_dropped")
    if c["c1"]:
        names.add("second_segment_four_off")
    if seam_axis(c):
        names.add("halo_staged_zero")
    if e.get("norm"):
        names.add("norm_relu_missing")
        if c["kh"] * c["kw"] > 1:
            names.add("padding_normalised")
    if e.get("scale") and e.get("shift"):
        names.add("scale_after_shift")
    if e.get("res"):
        names.add("res_before_activation")
    if e.get("ldo") or bn in (96, 192):
        names.add("columns_slipped_by_a_sub_tile")
    return names


def simulated_bugs(c):
    """{bug name: the float64 output} for every simulated bug that concerns case c."""
    r = reference(c["name"])
    names, t = bugs_for(c), r.t
    w, kidx, K = t["w"], _k_index(c), k_of(c)
    bk = c["plan"][2]
    accs = {}
    accs["last_chunk_dropped"] = conv(c, r.x, _masked(w, kidx < ((K - 1) // bk) * bk))
    if "split_partial_missing" in names:
        part = conv(c, r.x, _masked(w, second_split(c)))
        accs["split_partial_missing"], accs["split_partial_twice"] = r.acc - part, r.acc + part
    if "second_pipeline_dropped" in names:
        accs["second_pipeline_dropped"] = conv(c, r.x, _masked(w, (kidx // 32) % 2 == 0))
    if "second_segment_four_off" in names:
        x = torch.cat([r.x[..., :c["c0"]], torch.roll(r.x[..., c["c0"]:], -4, 3)], 3)
        accs["second_segment_four_off"] = conv(c, x, w)
    if "halo_staged_zero" in names:
        Ho, Wo = out_hw(c)
        ph, pw = patch_hw(c)
        yy, xx = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
        tap = torch.zeros_like(kidx, dtype=torch.bool)
        if seam_axis(c) == "x":                                          # the halo column right of a patch
            tap[:, :, c["kw"] - 1] = True
            pixels = xx % pw == pw - 1
        else:                                                            # the halo row below it
            tap[:, c["kh"] - 1, :] = True
            pixels = yy % ph == ph - 1
        accs["halo_staged_zero"] = r.acc - conv(c, r.x, _masked(w, tap)) * pixels.double()[None, :, :, None]
    if "norm_relu_missing" in names:
        accs["norm_relu_missing"] = conv(c, norm_on_load(t["x"], t["nmean"], t["nrstd"], relu=False), w)
    if "padding_normalised" in names:
        xpad = wc.pad_nhwc(t["x"], pad_amounts(c))                       # ('same': k // 2 all round, but for a stride's unused last row)
        accs["padding_normalised"] = conv(c, norm_on_load(xpad, t["nmean"], t["nrstd"]), w, padded=True)
    out = {k: r.epilogue(v)[1] for k, v in accs.items()}
    if "scale_after_shift" in names:
        out["scale_after_shift"] = r.epilogue(r.acc, scale_after_shift=True)[1]
    if "res_before_activation" in names:
        out["res_before_activation"] = r.epilogue(r.acc, res_before_activation=True)[1]
    if "columns_slipped_by_a_sub_tile" in names:
        out["columns_slipped_by_a_sub_tile"] = torch.roll(r.out, -32, 3)
    assert set(out) == names, (set(out), names)
    return out
