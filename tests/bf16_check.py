"""The oracle, the case table and the simulated bugs of the split-bf16 direct convolutions with the PLAIN epilogue (igemm_kernel in
csrc/conv.hip, OFX_PREC_BF16X3 / _W and OFX_PREC_BF16X6 / _W: 13 tile instances, each on the general gather, the 128-row BK = 16 ones
also on the halo patch).  Not a conftest: imported by name, and importable without a device.  The pattern of f16_check.py and
gru_check.py (whose splits, weight formats and checker are used, not restated): the oracle absorbs the operand arithmetic, so that
what the bound has to cover is the fp32 accumulation alone -- a lower piece missing for one tap of one 16-channel chunk, ~2^-9 |x||w|
over 16 of several hundred terms, is then far outside it, where a flat 2e-4 on N(0, 1) data let it pass.

Oracle.  Operands are split on the CPU with torch's round-to-nearest-even bfloat16 cast (gru_check.split2 / split3), after the norm
on load where the case has one.  Two arithmetic families, each shared by the on-the-fly and the pre-split weight precision:

    x3 (bf16x3, bf16x3_w)   ref = conv64(x_hi, w_hi) + conv64(x_hi, w_lo) + conv64(x_lo, w_hi), the three products the kernel forms;
                            M = the same three convolutions of absolute values.
    x6 (bf16x6, bf16x6_w)   ref = conv64(x, w), the float64 convolution of the exact operands; M = conv64(|x|, |w|).  `reference`
                            asserts hi + mid + lo == x exactly for both operands of every case (no lo piece underflows), so the six
                            products the kernel forms differ from x w by the three it drops, ml + lm + ll.  Their size follows from
                            the piece widths (conv.hip's header: 3 x 8 mantissa bits): with 2^e <= |x| < 2^(e+1), hi keeps 8 bits,
                            so |x - hi| <= 2^-9 2^e <= 2^-9 |x| and |mid| <= 2^-9 |x| (rounding is monotone and 2^-9 2^e is a
                            bfloat16 value); mid keeps 8 bits of that, so |lo| = |x - hi - mid| <= 2^-9 2^-9 2^e <= 2^-18 |x|.
                            Hence |ml + lm + ll| <= (2 2^-27 + 2^-36) |x||w| and the oracle allows
                                DROPPED conv64(|x|, |w|),    DROPPED = 2^-26 + 2^-36,
                            as a term of its own beside K 2^-24 M -- derived, never folded into the measured constant.  (The
                            `exact` cases have lo == 0 and carry no such term.)

Epilogue, float64: v = acc scale + shift + addend, y = act(v), then relu(y + res) with `res`.  M takes |scale| as a factor and
|shift|, |addend|, |res| as terms, as wino_check.reference does; ReLU is 1-Lipschitz; tanh and sigmoid (the kEpiPlainT instantiation)
carry the bound through their Lipschitz constants 1 and 1/4 plus wc.ACT_ULP, as gru_check does.  `reference` asserts of every case
|shift| + |addend| + |res| <= conv part of M (so the epilogue's own roundings stay inside the constant) and, for tanh / sigmoid, that
at least 3/4 of the pre-activations have |v| < 2 (a saturated activation hides a wrong pre-activation).

Norm on load.  The kernel splits the normalised, ReLU'd fp32 value fmaxf((x - mean) * rstd, 0) (conv.hip: a_commit / norm_a: one
fp32 subtraction, one fp32 multiplication, padding stays 0).  The oracle forms that value in float32 by the same formula, splits it,
and allows NORM_ULP conv64(|x_norm|, |w|), NORM_ULP = 2^-24, for a possible one-ulp difference of that fp32 value.

Bound.  |out - ref| <= slope (K 2^-24 M + derived terms) + ACT_ULP, K = wc.K_DIRECT_BF16X3 / wc.K_DIRECT_BF16X6 as wino_check.py
holds them (measured; the maxima of these cases are in its header).

OFX_EPI_FLOW.  The small network, the only caller of OFX_EPI_FLOW through the conv launcher, refuses the split-bf16 flags
(raft_engine.cpp: S_UNSUPPORTED; raft.RaftEngine raises ValueError before any device call), so no bf16 engine reaches that epilogue:
test_bf16_check_host.py asserts the rejection and the table has no flow case.

Inputs follow f16_check: seeded N(0, 1.5^2) activations, fan-in-scaled N(0, 1 / K) weights, shift / addend / res N(0, 0.5^2), scale
around 1.  `exact`: operands that are already bf16 values (x3) / have at most 16 mantissa bits (x6), lo == 0: the split path must
meet the float64 convolution of those operands within the accumulation bound alone.  `spread`: channel pairs scaled by 2^-12 ... 2^12
(the weight by the inverse), the second channel of a pair nearly equal with the opposite weight: M >> |ref|.

Geometry.  A case may carry `pad` = (padH, padW) and `out_hw` = (Hout, Wout) (wino_check.geometry_of: default 'same' padding and the
size that follows, which every case of this table has); geom_check.py holds the cases off 'same' padding and registers them here.

Simulated bugs (`simulated_bugs`), each applied on the CPU to the pieces or the products, with the cases it concerns in `bugs_for`.
`lower` pieces: lo (x3), mid and lo (x6).
    lower_a_dropped_in_the_last_chunk          the products of A's lower pieces missing over the last BK-wide chunk of K
    lower_a_dropped_for_a_border_tap           ... for the taps that read the halo column right of an 8x16 patch (maps one patch
                                               wide: the halo row below it), at the pixels next to it: a halo column staged
                                               without its lower pieces.  Concerns the halo-patch cases whose map has such a
                                               seam inside it (on a 2x8x16 map every halo pixel is padding)
    lower_a_dropped_in_the_second_segment      ... for the channels of in1
    lower_b_of_the_last_group_from_its_neighbour   the weight's first lower piece of the last four k taken from the four before:
                                               the pre-split format read 8 bytes off
    mm_dropped, lh_dropped                     x6 only: one of the six products missing everywhere (lh: not where lo == 0).  They
                                               sum like sqrt(K) where the bound grows like K: the narrowest margin of the table is
                                               at its largest K, 864, where the worst element still stands at 9.9 x 2^-24 M
    norm_applied_after_the_split               the lower pieces taken from the raw value (norm cases)
    columns_slipped_by_a_sub_tile              output columns shifted by one 32-wide sub-tile (out-slice cases)
"""
import functools
import math

import torch
import torch.nn.functional as F

import gru_check as gc
import sd_ops_check as SC
import wino_check as wc

PRECISIONS = {"bf16x3": 1, "bf16x3_w": 2, "bf16x6": 3, "bf16x6_w": 4}     # include/ofx.h
FAMILY = {1: "x3", 2: "x3", 3: "x6", 4: "x6"}
PRODUCTS = {"x3": ((0, 0), (0, 1), (1, 0)), "x6": ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0))}   # (piece of x, piece of w)
DROPPED = 2.0 ** -26 + 2.0 ** -36         # ml + lm + ll (header)
NORM_ULP = 2.0 ** -24
NORM_EPS = 1e-5
GUARD = gc.GUARD
WS_BYTES = 1 << 20
ACTS = {None: 0, "relu": 1, "sigmoid": 2, "tanh": 3}
NAN = float("nan")


def K_of(prec):
    return wc.K_DIRECT_BF16X3 if FAMILY[prec] == "x3" else wc.K_DIRECT_BF16X6


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table

def _c(name, B, H, W, c0, cout, kh, kw, plan, stride=1, tile=0, c1=0, **extra):
    """plan: (bm, bn, bk, patch) the launcher must reach, for all four precisions or {precision number: ...}."""
    plan = plan if isinstance(plan, dict) else {p: plan for p in (1, 2, 3, 4)}
    return dict(name=name, B=B, H=H, W=W, c0=c0, c1=c1, cout=cout, kh=kh, kw=kw, stride=stride, tile=tile, plan=plan, extra=extra)


BK32 = {1: (128, 128, 32, 0), 2: (128, 128, 16, 0), 3: (128, 128, 16, 0), 4: (128, 128, 16, 0)}   # only bf16x3 has the BK = 32 tile
CASES = [
    # the halo patch: one per 128-row tile and filter family, whole and overhanging patches
    _c("patch-3x3-128x64", 2, 8, 16, 32, 64, 3, 3, (128, 64, 16, 1), tile=16128064),
    _c("patch-1x5-128x128-x2", 2, 16, 16, 32, 128, 1, 5, (128, 128, 16, 1), tile=16128128, c1=32),
    _c("patch-5x1-128x128-x2", 2, 16, 16, 32, 128, 5, 1, (128, 128, 16, 1), tile=16128128, c1=32),
    _c("patch-1x5-seam-128x128-x2", 1, 8, 32, 32, 128, 1, 5, (128, 128, 16, 1), tile=16128128, c1=32),   # two patches side by side
    _c("patch-over-128x64", 1, 9, 17, 32, 64, 3, 3, (128, 64, 16, 1), tile=16128064),
    _c("patch-over-128x128", 1, 9, 17, 32, 128, 3, 3, (128, 128, 16, 1), tile=16128128),
    # the general gather, all three tiles: K = 36 ends inside a chunk, ragged M (140 rows) and ragged N (72 channels)
    _c("gather-64x64", 1, 10, 14, 4, 72, 3, 3, (64, 64, 16, 0), tile=16064064),
    _c("gather-128x64", 1, 10, 14, 4, 72, 3, 3, (128, 64, 16, 0), tile=16128064),
    _c("gather-128x128", 1, 10, 14, 4, 72, 3, 3, (128, 128, 16, 0), tile=16128128),
    _c("gather-auto", 1, 10, 14, 4, 72, 3, 3, (128, 128, 16, 0)),
    _c("gather-auto-ws", 1, 10, 14, 4, 72, 3, 3, (128, 128, 16, 0), ws=True),        # a split-K workspace: no split in these arithmetics
    _c("small-grid-auto-ws", 1, 8, 16, 96, 64, 3, 3, (64, 64, 16, 0), ws=True),      # K = 864: the fp32 plan of this one splits K four ways
    # bf16x3 BK = 32: K = 324 ends 4 into a 32-chunk; Cin 48: a tap straddles chunks
    _c("bk32-k324", 1, 16, 16, 324, 256, 1, 1, BK32, tile=32128128),
    _c("bk32-3x3-c48", 1, 10, 14, 48, 128, 3, 3, BK32, tile=32128128),
    # strided and large taps
    _c("stride2-3x3-96", 1, 11, 13, 64, 96, 3, 3, (128, 128, 16, 0), stride=2, tile=16128096),     # 128x96 -> 128x128
    _c("stride2-1x1", 3, 10, 6, 64, 64, 1, 1, (64, 64, 16, 0), stride=2),
    _c("stem-7x7-s2", 1, 16, 24, 4, 64, 7, 7, (64, 64, 16, 0), stride=2, zero_last=True),          # Cin 3 + a zero channel
    _c("convf1-7x7", 1, 10, 14, 4, 128, 7, 7, (64, 64, 16, 0)),
    # N edges
    _c("cout2", 1, 8, 16, 32, 2, 3, 3, (128, 128, 16, 1)),
    _c("out-slice-126", 2, 8, 16, 32, 126, 3, 3, (64, 64, 16, 0), ldo=384),
    _c("out-slice-126-patch", 2, 8, 16, 32, 126, 3, 3, (128, 128, 16, 1), tile=16128128, ldo=384),
    # epilogue
    _c("epi-scale-shift-res-relu", 2, 8, 16, 32, 64, 3, 3, (128, 64, 16, 1), tile=16128064, scale=True, shift=True, res=True, act="relu"),
    _c("epi-addend-shift", 2, 8, 16, 32, 64, 3, 3, (64, 64, 16, 0), addend=True, shift=True),
    _c("epi-tanh-patch", 2, 8, 16, 32, 128, 3, 3, (128, 128, 16, 1), tile=16128128, shift=True, act="tanh"),
    _c("epi-sigmoid-gather", 2, 8, 16, 32, 64, 3, 3, (64, 64, 16, 0), shift=True, act="sigmoid"),
    _c("epi-tanh-gather-128x64", 1, 10, 14, 8, 72, 3, 3, (128, 64, 16, 0), tile=16128064, act="tanh"),
    _c("norm-gather-relu", 1, 10, 14, 8, 72, 3, 3, (64, 64, 16, 0), tile=16064064, norm=True, act="relu"),
    _c("norm-patch", 2, 8, 16, 32, 64, 3, 3, (128, 64, 16, 1), tile=16128064, norm=True),
    # number format
    _c("exact-patch", 2, 8, 16, 32, 64, 3, 3, (128, 64, 16, 1), tile=16128064, exact=True),
    _c("exact-gather", 1, 10, 14, 4, 72, 3, 3, (64, 64, 16, 0), tile=16064064, exact=True),
    _c("spread-patch", 2, 8, 16, 32, 128, 3, 3, (128, 128, 16, 1), tile=16128128, spread=True),
    _c("spread-gather", 1, 10, 14, 8, 72, 3, 3, (128, 64, 16, 0), tile=16128064, spread=True),
]
IDS = [c["name"] for c in CASES]


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


def k_of(c):
    return c["kh"] * c["kw"] * (c["c0"] + c["c1"])


def same_plan(c):
    """Whether the on-the-fly and the pre-split precision of each family reach one plan: then, and only then, their results are
    bit-identical by construction (the bf16x3 BK = 32 tile has no pre-split twin: bf16x3_w runs such a case on BK = 16)."""
    return c["plan"][1] == c["plan"][2] and c["plan"][3] == c["plan"][4]


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs

@functools.lru_cache(maxsize=None)
def inputs(name, fam):
    """-> dict of float32 CPU tensors: x [B,H,W,c0 + c1], w OIHW, and whichever of scale / shift [cout], addend / res [B,Ho,Wo,cout],
    nmean / nrstd [B,c0] the case has (else None).  Only the `exact` cases depend on the family."""
    c = case(name)
    e = c["extra"]
    g = SC._gen("bf16-" + name)
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
    if e.get("exact"):
        if fam == "x3":
            x, w = gc.split2(x)[0], gc.split2(w)[0]
        else:
            x, w = (lambda p: p[0] + p[1])(gc.split3(x)), (lambda p: p[0] + p[1])(gc.split3(w))
    Ho, Wo = out_hw(c)
    t = dict(x=x, w=w, scale=None, shift=None, addend=None, res=None, nmean=None, nrstd=None)
    if e.get("scale"):
        t["scale"] = 1.0 + 0.25 * torch.randn((co,), generator=g)
    if e.get("shift"):
        t["shift"] = 0.5 * torch.randn((co,), generator=g)
    if e.get("addend"):
        t["addend"] = 0.5 * torch.randn((B, Ho, Wo, co), generator=g)
    if e.get("res"):
        t["res"] = 0.5 * torch.randn((B, Ho, Wo, co), generator=g)
    if e.get("norm"):
        f = x.reshape(B, H * W, cin)
        t["nmean"] = f.mean(1).contiguous()
        t["nrstd"] = (1.0 / torch.sqrt(f.var(1, unbiased=False) + NORM_EPS)).contiguous()
    return t


def norm_on_load(x, mean, rstd):
    """The operand the kernel splits (header): float32, one subtraction, one multiplication, ReLU."""
    assert x.dtype == mean.dtype == rstd.dtype == torch.float32
    return torch.relu((x - mean[:, None, None, :]) * rstd[:, None, None, :])


def pieces(t, fam):
    """fp32 -> the float32 tensors of bf16 values the kernel multiplies: [hi, lo] or [hi, mid, lo]."""
    return list(gc.split2(t)) if fam == "x3" else list(gc.split3(t))


def conv(c, x, w):
    """x NHWC, w OIHW (any float dtype) -> the case's convolution in float64, NHWC.  A case with a geometry of its own (`pad` /
    `out_hw`) goes through wino_check.conv64_geometry."""
    if "pad" in c or "out_hw" in c:
        return wc.conv64_geometry(x, w, c["stride"], pad_of(c), out_hw(c))
    out = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=c["stride"], padding=(c["kh"] // 2, c["kw"] // 2))
    return out.permute(0, 2, 3, 1)


def products(c, xp, wp, fam, keep=None):
    """The float64 sum of the family's products of pieces (`keep`: a subset of PRODUCTS[fam])."""
    return sum(conv(c, xp[i], wp[j]) for i, j in (PRODUCTS[fam] if keep is None else keep))


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle

class Ref:
    """The float64 side of one (case, family): t (inputs), x (the operand that is split), xp / wp (pieces), acc, v, out, mag,
    slope, extra, unsaturated."""

    def epilogue(self, acc):
        """acc [B,Ho,Wo,cout] float64 -> (v, out): the pre-activation and the stored value."""
        t, act = self.t, self.c["extra"].get("act")
        v = acc if t["scale"] is None else acc * t["scale"].double()
        for name in ("shift", "addend"):
            if t[name] is not None:
                v = v + t[name].double()
        y = torch.tanh(v) if act == "tanh" else torch.sigmoid(v) if act == "sigmoid" else v.clamp_min(0.0) if act == "relu" else v
        if t["res"] is not None:
            y = (y + t["res"].double()).clamp_min(0.0)
        return v, y


@functools.lru_cache(maxsize=None)
def reference(name, fam):
    c = case(name)
    e, t = c["extra"], inputs(name, fam)
    r = Ref()
    r.c, r.fam, r.t = c, fam, t
    r.x = t["x"]
    if e.get("norm"):
        r.x = torch.cat([norm_on_load(t["x"][..., :c["c0"]], t["nmean"], t["nrstd"]), t["x"][..., c["c0"]:]], 3)
    r.xp, r.wp = pieces(r.x, fam), pieces(t["w"], fam)
    conv_abs = conv(c, r.x.abs(), t["w"].abs())
    derived = torch.zeros_like(conv_abs)
    if fam == "x3":
        r.acc = products(c, r.xp, r.wp, fam)
        mag = products(c, [p.abs() for p in r.xp], [p.abs() for p in r.wp], fam)
    else:
        for whole, parts in ((r.x, r.xp), (t["w"], r.wp)):               # three pieces are exact: no lo piece underflows
            assert torch.equal(sum(p.double() for p in parts), whole.double()), name
        r.acc, mag = conv(c, r.x, t["w"]), conv_abs
        if not e.get("exact"):
            derived = derived + DROPPED * conv_abs
    if e.get("exact"):                                                   # lo == 0: the operands are what the kernel multiplies
        assert not bool(r.xp[-1].any()) and not bool(r.wp[-1].any()), name
        assert fam == "x6" or torch.equal(r.acc, conv(c, r.x, t["w"]))
    if e.get("norm"):
        derived = derived + NORM_ULP * conv_abs
    sc = torch.ones((), dtype=torch.float64) if t["scale"] is None else t["scale"].double().abs()
    mag, derived = mag * sc, derived * sc
    side = sum((t[n].double().abs() for n in ("shift", "addend", "res") if t[n] is not None), torch.zeros_like(mag))
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


def violates(r, got, K):
    return bool(wc.violations(got, r.out, r.mag, K, r.slope, r.extra).any())


def check(r, got, K, what):
    """Assert the bound and return the worst ratio."""
    return wc.check(got, r.out, r.mag, K, what, r.slope, r.extra)


def ratio(r, got):
    return wc.worst_ratio(got, r.out, r.mag, r.slope, r.extra)


# ---------------------------------------------------------------------------------------------------------------------------------
# the launch: one descriptor for the host's plan query and the device run

def packed_weight(c, prec):
    """The weight operand of the arithmetic (CPU): packed fp32, or the pre-split formats of the _w precisions."""
    from sd_animation_optical_flow_amd import ops
    wp = ops.pack_conv_weight(inputs(c["name"], FAMILY[prec])["w"])
    return ops.split_conv_weight(wp) if prec == 2 else ops.split_conv_weight3(wp) if prec == 4 else wp


def ldo_of(c):
    return c["extra"].get("ldo", c["cout"])


def buffers(c, prec):
    """{name: CPU tensor} of everything the descriptor points at; `out`: [GUARD + M + GUARD, ldo] of NaN."""
    t = inputs(c["name"], FAMILY[prec])
    Ho, Wo = out_hw(c)
    M = c["B"] * Ho * Wo
    b = dict(x=t["x"][..., :c["c0"]].contiguous(), w=packed_weight(c, prec), out=torch.full((M + 2 * GUARD, ldo_of(c)), NAN))
    if c["c1"]:
        b["x2"] = t["x"][..., c["c0"]:].contiguous()
    for n in ("scale", "shift", "addend", "res", "nmean", "nrstd"):
        if t[n] is not None:
            b[n] = t[n]
    if c["extra"].get("ws"):
        b["ws"] = torch.zeros((WS_BYTES,), dtype=torch.uint8)
    return b


def descriptor(c, prec, ptr):
    """The case's ConvDesc; ptr(buffer name) -> the address of its first byte."""
    from sd_animation_optical_flow_amd import _lib
    e = c["extra"]
    Ho, Wo = out_hw(c)
    d = _lib.ConvDesc()
    d.in0, d.ld0, d.c0 = ptr("x"), c["c0"], c["c0"]
    if c["c1"]:
        d.in1, d.ld1, d.c1 = ptr("x2"), c["c1"], c["c1"]
    d.w = ptr("w")
    d.out, d.ldo = ptr("out") + 4 * GUARD * ldo_of(c), ldo_of(c)
    if e.get("scale"):
        d.scale = ptr("scale")
    if e.get("shift"):
        d.shift = ptr("shift")
    if e.get("addend"):
        d.addend, d.ldadd = ptr("addend"), c["cout"]
    if e.get("res"):
        d.res, d.ldres = ptr("res"), c["cout"]
    if e.get("norm"):
        d.nmean, d.nrstd = ptr("nmean"), ptr("nrstd")
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = c["B"], c["H"], c["W"], Ho, Wo, c["cout"]
    d.KH, d.KW, d.stride, (d.padH, d.padW) = c["kh"], c["kw"], c["stride"], pad_of(c)
    d.act, d.epi, d.tile, d.precision = ACTS[e.get("act")], 0, c["tile"], prec
    if e.get("ws"):
        d.splitk_ws, d.splitk_ws_bytes = ptr("ws"), WS_BYTES
    return d


def signature(c, prec):
    """(bm, bn, bk, prec, patch) of the case under the precision: the instantiation and the A-side schedule it runs."""
    bm, bn, bk, patch = c["plan"][prec]
    return (bm, bn, bk, prec, patch)


def covered():
    return {signature(c, p) for c in CASES for p in (1, 2, 3, 4)}


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


def _lower_a_term(r, keep, pixels=None):
    """The float64 sum of the products that have a lower piece of A, over the weight elements `keep` (at the output pixels `pixels`
    [Ho, Wo], default all): what a launch loses when those pieces of A are staged as zeros there."""
    lost = [(i, j) for i, j in PRODUCTS[r.fam] if i >= 1]
    term = products(r.c, r.xp, [_masked(p, keep) for p in r.wp], r.fam, lost)
    return term if pixels is None else term * pixels.to(term.dtype)[None, :, :, None]


def seam_axis(c):
    """'x' / 'y': the axis along which 8x16 patches of the map meet under a tap of the filter, None: the map has no such seam."""
    Ho, Wo = out_hw(c)
    return "x" if c["kw"] > 1 and Wo > 16 else "y" if c["kh"] > 1 and Ho > 8 else None


def bugs_for(c, fam):
    """The names of the simulated bugs that concern case c in the family (header)."""
    e = c["extra"]
    names = set()
    if e.get("ldo"):
        names.add("columns_slipped_by_a_sub_tile")
    if fam == "x6":
        names.add("mm_dropped")
        if not e.get("exact"):
            names.add("lh_dropped")
    if e.get("exact") and fam == "x3":                                   # lo == 0: nothing of the pieces to lose
        return names
    names |= {"lower_a_dropped_in_the_last_chunk", "lower_b_of_the_last_group_from_its_neighbour"}
    if all(c["plan"][p][3] for p in PRECISIONS.values() if FAMILY[p] == fam) and seam_axis(c):
        names.add("lower_a_dropped_for_a_border_tap")
    if c["c1"]:
        names.add("lower_a_dropped_in_the_second_segment")
    if e.get("norm"):
        names.add("norm_applied_after_the_split")
    return names


def simulated_bugs(c, fam):
    """{bug name: the float64 output} for every simulated bug that concerns case c in the family."""
    r = reference(c["name"], fam)
    names = bugs_for(c, fam)
    kidx, K, cin = _k_index(c), k_of(c), c["c0"] + c["c1"]
    made = products(c, r.xp, r.wp, fam)                                  # what the kernel forms (x3: the reference itself)
    bugs = {}
    if "lower_a_dropped_in_the_last_chunk" in names:
        bk = max(c["plan"][p][2] for p in PRECISIONS.values() if FAMILY[p] == fam)
        bugs["lower_a_dropped_in_the_last_chunk"] = made - _lower_a_term(r, kidx >= ((K - 1) // bk) * bk)
    if "lower_a_dropped_for_a_border_tap" in names:
        Ho, Wo = out_hw(c)
        yy, xx = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
        tap = torch.zeros_like(kidx, dtype=torch.bool)
        if seam_axis(c) == "x":                                          # the halo column right of an 8x16 patch
            tap[:, :, c["kw"] - 1] = True
            pixels = xx % 16 == 15
        else:                                                            # the halo row below it
            tap[:, c["kh"] - 1, :] = True
            pixels = yy % 8 == 7
        bugs["lower_a_dropped_for_a_border_tap"] = made - _lower_a_term(r, tap, pixels)
    if "lower_a_dropped_in_the_second_segment" in names:
        seg = torch.zeros_like(kidx, dtype=torch.bool)
        seg[c["c0"]:] = True
        bugs["lower_a_dropped_in_the_second_segment"] = made - _lower_a_term(r, seg)
    if "lower_b_of_the_last_group_from_its_neighbour" in names:
        co, kh, kw = c["cout"], c["kh"], c["kw"]
        flat = r.wp[1].permute(0, 2, 3, 1).reshape(co, -1).clone()       # [cout, K] in packed order
        flat[:, K - 4:] = flat[:, K - 8:K - 4]
        wp = list(r.wp)
        wp[1] = flat.reshape(co, kh, kw, cin).permute(0, 3, 1, 2).contiguous()
        bugs["lower_b_of_the_last_group_from_its_neighbour"] = products(c, r.xp, wp, fam)
    if "mm_dropped" in names:
        bugs["mm_dropped"] = made - conv(c, r.xp[1], r.wp[1])
    if "lh_dropped" in names:
        bugs["lh_dropped"] = made - conv(c, r.xp[2], r.wp[0])
    if "norm_applied_after_the_split" in names:
        bugs["norm_applied_after_the_split"] = products(c, r.xp[:1] + pieces(r.t["x"], fam)[1:], r.wp, fam)
    out = {k: r.epilogue(v)[1] for k, v in bugs.items()}
    if "columns_slipped_by_a_sub_tile" in names:
        out["columns_slipped_by_a_sub_tile"] = torch.roll(r.out, -32, 3)
    assert set(out) == names
    return out
