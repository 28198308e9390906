"""The oracle and the case table of the fp16 convolution arithmetic (OFX_PREC_F16, `ops.conv2d_nhwc(precision="fp16")`).
Not a conftest: imported by name, and importable without a device.

Arithmetic under test.  Both operands of the contraction are rounded fp32 -> fp16 (round-to-nearest-even) as the kernel stages
them, every product is formed on v_mfma_f32_32x32x16_f16 and accumulated in fp32; scale, shift, addend, res and the stored result
stay fp32.

Oracle.  The reference is the float64 convolution of the ROUNDED operands, x.half().double() and w.half().double(), with scale,
shift, addend and res in float64.  The product of two fp16 values has at most 22 significant bits and an exponent inside the
fp32 range: it is exact in fp32.  What is left is the fp32 accumulation: whatever the order of the additions, a term passes
through at most K of them (K = KH KW Cin), so with u = 2^-24

    |out - ref| <= (K + 2) u sum_k |x_h| |w_h| |scale| + 2 u |ref| + FLOOR

the bound `unet_check.emb_linear_reference` uses for the fp32 Linear.  Nothing in it is measured.  The epilogue's own roundings
(one for acc * scale + shift, one for the addend, one for res) are at most u (sum |x_h||w_h| |scale| + |shift| + |addend|) and
2 u |ref| (ReLU is 1-Lipschitz); they fit the "+ 2" as long as |shift| + |addend| + |res| <= sum |x_h||w_h| |scale| at every
element, which `reference` asserts of every case instead of assuming it.

Subnormals.  fp16 values below 2^-14 are subnormal (multiples of 2^-24).  The convert instruction produces them and the matrix
core multiplies them as they are (include/ofx.h, OFX_PREC_F16): the bound above has NO flush term, and the "small" case (operands
N(0, 1) * 1e-3: a few percent of them subnormal in fp16) holds the device to it.  Were subnormal operands flushed to zero, every
flushed operand would lose up to 2^-14 * |other operand| and that case's bound would need the extra term
K * 2^-14 * max |other operand|.

Range.  65504 is the largest fp16 value: the "max" case holds +-65504 exactly in a few positions of x and w and stays finite.
Beyond it an operand becomes an infinity (as under torch.autocast); no case goes there.

Geometry.  A case may carry `kh` / `kw` in place of the square `k`, and `pad` = (padH, padW) and `out_hw` = (Hout, Wout)
(wino_check.geometry_of: default 'same' padding and the size that follows, which every case of this table has); geom_check.py holds
the cases off 'same' padding.  Its `ring` cases (`exact_zero`, `shift_amp`) have outputs with no tap inside the image: there the
accumulator is an exact 0, the shift alone is stored, and the assertion on |shift| applies where there is a tap.

Inputs.  Seeded N(0, 1.5^2) activations and fan-in-scaled N(0, 1/K) weights; shift / addend / res N(0, 0.5^2), scale around 1.
"""
import math

import torch
import torch.nn.functional as F

import sd_ops_check as SC
import wino_check as wc

U, FLOOR = SC.U, SC.FLOOR
PREC_F16 = 5                               # include/ofx.h
NAN = float("nan")


def _c(name, B, H, W, c0, cout, k, stride=1, tile=0, c1=0, plan=None, **extra):
    """plan: (bm, bn, bk, mode) the launcher must choose for the case (mode 0 general gather, 1 scalar coordinates, 2 halo patch)."""
    return dict(name=name, B=B, H=H, W=W, c0=c0, c1=c1, cout=cout, k=k, stride=stride, tile=tile, plan=plan, extra=extra)


CASES = [
    # the halo-patch schedule, one case per tile
    _c("patch-128x64", 2, 8, 16, 32, 64, 3, tile=128064, plan=(128, 64, 16, 2)),
    _c("patch-128x128-x2", 2, 16, 16, 32, 128, 3, tile=128128, c1=32, plan=(128, 128, 16, 2)),
    _c("patch-64x64", 2, 16, 8, 32, 64, 3, tile=64064, plan=(64, 64, 16, 2)),
    # the general gather: K = 36 ends inside a chunk, ragged M (140 rows) and N (40 channels)
    _c("gather-k36", 1, 10, 14, 4, 40, 3, plan=(64, 64, 32, 0)),
    _c("stride2", 1, 11, 13, 64, 96, 3, stride=2, plan=(128, 128, 32, 1)),
    # the transformers' GEMM shape class: scalar chunk coordinates
    _c("gemm-m77", 1, 1, 77, 320, 40, 1, plan=(64, 64, 32, 1)),
    _c("gemm-k2560", 1, 1, 77, 2560, 64, 1, plan=(64, 64, 32, 1)),
    # epilogue
    _c("shift-addend", 2, 8, 16, 32, 64, 3, tile=128064, plan=(128, 64, 16, 2), shift=True, addend=True),
    _c("scale-res-relu", 1, 9, 11, 32, 48, 3, plan=(64, 64, 32, 1), scale=True, res=True, act="relu"),
    _c("out-slice", 1, 9, 11, 32, 40, 1, plan=(64, 64, 32, 1), shift=True, out_slice=(8, 56)),      # channels [8, 48) of a 56-wide NaN tensor
    # number format
    _c("small", 1, 9, 11, 32, 40, 3, plan=(64, 64, 32, 1), mag=1e-3),
    _c("max", 1, 9, 11, 32, 40, 3, plan=(64, 64, 32, 1), extreme=True),
]
# every other instantiation: three tiles x two chunk lengths x (general gather: Cin 4; scalar coordinates: Cin 64, stride 2 --
# at stride 1 a forced BK = 16 tile takes the halo patch), on maps with ragged M; BK = 16 on the general / scalar schedules only exists through a forced tile
for _bm, _bn in ((128, 128), (128, 64), (64, 64)):
    for _bk in (16, 32):
        _t = _bk * 1000000 + _bm * 1000 + _bn
        CASES.append(_c(f"gather-{_bm}x{_bn}-bk{_bk}", 1, 10, 14, 4, 72, 3, tile=_t, plan=(_bm, _bn, _bk, 0)))
        CASES.append(_c(f"scalar-{_bm}x{_bn}-bk{_bk}", 2, 10, 14, 64, 72, 3, stride=2, tile=_t, c1=32 if _bm == 128 and _bn == 128 else 0,
                        plan=(_bm, _bn, _bk, 1)))
IDS = [c["name"] for c in CASES]


def filter_of(c):
    """(KH, KW): the square `k`, or the optional `kh` / `kw`."""
    return c.get("kh", c.get("k")), c.get("kw", c.get("k"))


def pad_of(c):
    """(padH, padW): the case's optional `pad`, default 'same' (k // 2)."""
    return wc.geometry_of(c)[0]


def out_hw(c):
    """(Hout, Wout): the case's optional `out_hw`, default the size that follows from the padding."""
    return wc.geometry_of(c)[1]


def inputs(c):
    """-> dict of float32 CPU tensors: x [B,H,W,c0], x2 [B,H,W,c1] or None, w OIHW [cout, c0 + c1, k, k], and whichever of scale /
    shift [cout], addend / res [B,Ho,Wo,cout] the case has (else None)."""
    g = SC._gen("f16-" + c["name"])
    e = c["extra"]
    B, H, W, c0, c1, co, (kh, kw) = c["B"], c["H"], c["W"], c["c0"], c["c1"], c["cout"], filter_of(c)
    cin = c0 + c1
    mag = e.get("mag", 1.0)
    x = torch.randn((B, H, W, cin), generator=g) * 1.5 * mag
    w = torch.randn((co, cin, kh, kw), generator=g) * (mag / math.sqrt(cin * kh * kw))
    if e.get("extreme"):
        x[0, 0, 0, 0], x[0, 4, 5, 7], x[0, H - 1, W - 1, cin - 1] = 65504.0, -65504.0, 65504.0
        w[0, 0, 0, 0], w[co - 1, cin - 1, kh - 1, kw - 1] = 65504.0, -65504.0
    Ho, Wo = out_hw(c)
    r = dict(x=x[..., :c0].contiguous(), x2=x[..., c0:].contiguous() if c1 else None, w=w, scale=None, shift=None, addend=None, res=None)
    if e.get("scale"):
        r["scale"] = 1.0 + 0.25 * torch.randn((co,), generator=g)
    if e.get("shift"):
        r["shift"] = e.get("shift_amp", 0.5) * torch.randn((co,), generator=g)
    if e.get("addend"):
        r["addend"] = 0.5 * torch.randn((B, Ho, Wo, co), generator=g)
    if e.get("res"):
        r["res"] = 0.5 * torch.randn((B, Ho, Wo, co), generator=g)
    return r


def reference(c, t):
    """-> (ref, bound) float64 [B,Ho,Wo,cout] for the tensors `t` of `inputs(c)` (header).  A case with a geometry of its own
    (`pad` / `out_hw`, with `H` and `W`) goes through wino_check.conv64_geometry: taps outside the image are zero."""
    s = c["stride"]
    x = t["x"] if t["x2"] is None else torch.cat([t["x"], t["x2"]], dim=3)
    xh = x.half().double().permute(0, 3, 1, 2)
    wh = t["w"].half().double()
    assert bool(torch.isfinite(xh).all()) and bool(torch.isfinite(wh).all())
    K = wh[0].numel()
    nhwc = lambda a: a.permute(0, 2, 3, 1)
    if "pad" in c or "out_hw" in c:
        conv = lambda a, b: wc.conv64_geometry(nhwc(a), b, s, pad_of(c), out_hw(c))
    else:
        conv = lambda a, b: nhwc(F.conv2d(a, b, stride=s, padding=(wh.shape[2] // 2, wh.shape[3] // 2)))
    acc, mag = conv(xh, wh), conv(xh.abs(), wh.abs())
    sc = torch.ones(()) .double() if t["scale"] is None else t["scale"].double()
    v = acc * sc
    side = torch.zeros_like(v)
    for name in ("shift", "addend"):
        if t[name] is not None:
            v = v + t[name].double()
            side = side + t[name].double().abs()
    if c["extra"].get("act") == "relu":
        v = v.clamp_min(0.0)
    if t["res"] is not None:
        v = (v + t["res"].double()).clamp_min(0.0)
        side = side + t["res"].double().abs()
    covered = side <= mag * sc.abs()
    if c["extra"].get("exact_zero"):
        # outputs with no tap inside the image (a geometry's ring, geom_check.py): the accumulator is an exact 0 and 0 + shift rounds
        # nowhere, so there is no rounding to cover as long as a shift is all there is (the caller holds them to relu(shift) bit for bit)
        assert bool((mag == 0).any()) and t["scale"] is None and t["addend"] is None and t["res"] is None
        covered = covered | (mag == 0)
    assert bool(covered.all()), f"{c['name']}: outside the range in which the bound covers the epilogue's roundings"
    bound = (K + 2) * U * mag * sc.abs() + 2 * U * v.abs() + FLOOR
    return v, bound


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over every element; NaN / inf count as infinite."""
    return SC._worst((got.double() - ref).abs(), bound)
