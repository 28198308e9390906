"""-m gpu: the fp16 kernels on weights stored in half (OFX_PREC_F16_W; `ops.conv2d_nhwc(precision="fp16_w")` and
`ops.upconv2x(precision="fp16")` with a float16 operand).

The bar needs no tolerance: for any fp32 weights w, "fp16_w" on `ops.half_conv_weight(w)` must equal "fp16" on w bit for bit -- the
kernel commits to LDS the halves it would have formed itself, and forms the same products in the same order.  So that the pair cannot
be equal and wrong, every case of tests/f16_check.py is also held to its float64 bound (f16_check.reference, derived there).  Cases:
all of f16_check.CASES (every tile, chunk length and schedule instantiation, the subnormal and the +-65504 case, the out-slice with
its NaN border compared too), the off-'same' geometries of tests/geom_check.py that OFX_PREC_F16 serves, and the shapes of
tests/test_gpu_upconv_f16.py."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import f16_check as FC   # noqa: E402
import geom_check as gc   # noqa: E402
import sd_ops_check as SC   # noqa: E402
from test_gpu_upconv_f16 import CASES as UP_CASES, IDS as UP_IDS, _inputs as up_inputs   # noqa: E402

pytestmark = pytest.mark.gpu
PREC_F16_W = 7
GEOM = [c for c in gc.F16 if c["precision"] == gc.PREC_F16]          # (the norm cases are OFX_PREC_F16_EPI's: fp32 weights only)
bits = lambda t: t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def ops(cuda):
    from sd_animation_optical_flow_amd import ops as O
    return O


def _plan(c, x_c0, x_c1, precision):
    """The launcher's plan of the case's descriptor under `precision` (dummy pointers: nothing is read)."""
    from sd_animation_optical_flow_amd import _lib
    (kh, kw), (ph, pw), (Ho, Wo) = FC.filter_of(c), FC.pad_of(c), FC.out_hw(c)
    d = _lib.ConvDesc()
    d.in0, d.ld0, d.c0, d.w = 0x10000, x_c0, x_c0, 0x10000
    if x_c1:
        d.in1, d.ld1, d.c1 = 0x10000, x_c1, x_c1
    d.out, d.ldo = 0x10000, c["cout"]
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = c["B"], c["H"], c["W"], Ho, Wo, c["cout"]
    d.KH, d.KW, d.stride, d.padH, d.padW = kh, kw, c["stride"], ph, pw
    d.tile, d.precision = c["tile"], precision
    p = _lib.ConvPlan()
    assert _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 0, C.byref(p)) == 0, c["name"]
    return p


def _run(ops, c, t, w_dev, precision, out=None, out_off=0):
    dev = lambda a: None if a is None else a.cuda()
    kh, kw = FC.filter_of(c)
    return ops.conv2d_nhwc(dev(t["x"]), w_dev, kh, kw, c["cout"], stride=c["stride"], shift=dev(t["shift"]), scale=dev(t["scale"]),
                           act=c["extra"].get("act"), x2=dev(t.get("x2")), res=dev(t["res"]), addend=dev(t["addend"]), tile=c["tile"],
                           precision=precision, out=out, out_off=out_off, pad=FC.pad_of(c), out_hw=FC.out_hw(c))


def _pair(ops, c, t):
    """-> (the output under "fp16" on the packed fp32 weights, under "fp16_w" on their halves); an out-slice case: the whole wide
    NaN-filled tensors."""
    packed = ops.pack_conv_weight(t["w"])
    w32, w16 = packed.cuda(), ops.half_conv_weight(packed).cuda()
    assert w16.dtype == torch.float16 and w16.shape == w32.shape and 2 * w16.numel() * w16.element_size() == w32.numel() * w32.element_size()
    sl = c["extra"].get("out_slice")
    if sl is None:
        return _run(ops, c, t, w32, "fp16"), _run(ops, c, t, w16, "fp16_w")
    off, ldo = sl
    Ho, Wo = FC.out_hw(c)
    wide = [torch.full((c["B"], Ho, Wo, ldo), FC.NAN, device="cuda") for _ in range(2)]
    _run(ops, c, t, w32, "fp16", out=wide[0], out_off=off)
    _run(ops, c, t, w16, "fp16_w", out=wide[1], out_off=off)
    return wide[0], wide[1]


@pytest.mark.parametrize("c", FC.CASES, ids=FC.IDS)
def test_half_weights_give_the_bits_of_fp16_and_stay_inside_the_float64_bound(ops, c):
    t = FC.inputs(c)
    ref, bound = FC.reference(c, t)
    p = _plan(c, c["c0"], c["c1"], PREC_F16_W)
    assert (p.path, p.prec, p.bm, p.bn, p.bk, p.mode) == (0, PREC_F16_W, *c["plan"])                  # the instantiation the case is there for
    a, b = _pair(ops, c, t)
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
    assert torch.equal(bits(a), bits(b)), c["name"]                      # bit for bit, the NaN border of the out-slice case included
    sl = c["extra"].get("out_slice")
    if sl is not None:
        gap = torch.ones(sl[1], dtype=torch.bool)
        gap[sl[0]:sl[0] + c["cout"]] = False
        assert bool(torch.isnan(b[..., gap.cuda()]).all())               # nothing was written around the slice
        b = b[..., sl[0]:sl[0] + c["cout"]]
    worst = FC.worst_ratio(b.cpu(), ref, bound)
    print(f"{c['name']}: fp16_w == fp16 bit for bit; |error| / float64 bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("c", GEOM, ids=[c["name"] for c in GEOM])
def test_half_weights_give_the_bits_of_fp16_off_same_padding(ops, c):
    t = gc.f16_tensors(c)                                                # x holds both segments
    c0, c1 = c["c0"], c["c1"]
    t = dict(t, x=t["x"][..., :c0].contiguous(), x2=t["x"][..., c0:].contiguous() if c1 else None)
    p5, p7 = _plan(c, c0, c1, gc.PREC_F16), _plan(c, c0, c1, PREC_F16_W)
    assert (p7.bm, p7.bn, p7.bk, p7.mode) == c["plan"] == (p5.bm, p5.bn, p5.bk, p5.mode) and p7.prec == PREC_F16_W
    a, b = _pair(ops, c, t)
    assert tuple(b.shape) == (c["B"], *FC.out_hw(c), c["cout"])
    assert torch.equal(bits(a), bits(b)), c["name"]
    ref, bound = gc.f16_reference(c)
    worst = FC.worst_ratio(b.cpu(), ref, bound)
    print(f"{c['name']}: fp16_w == fp16 bit for bit; |error| / float64 bound {worst:.3f}")
    assert worst <= 1.0


def test_a_dtype_mismatch_raises_before_any_launch(ops):
    c = FC.CASES[0]
    t = FC.inputs(c)
    packed = ops.pack_conv_weight(t["w"])
    w32, w16 = packed.cuda(), ops.half_conv_weight(packed).cuda()
    Ho, Wo = FC.out_hw(c)
    out = torch.full((c["B"], Ho, Wo, c["cout"]), 7.25, device="cuda")
    for prec in ("fp32", "fp16", "fp16_epi", "bf16x3", "bf16x3_w", "bf16x6", "bf16x6_w"):
        with pytest.raises(RuntimeError, match="w_packed"):
            _run(ops, c, t, w16, prec, out=out)                          # half weights under a precision that reads fp32
    with pytest.raises(RuntimeError, match="w_packed"):
        _run(ops, c, t, w32, "fp16_w", out=out)                          # fp32 weights under the precision that reads halves
    x = torch.zeros((1, 2, 2, 8), device="cuda")
    wf = torch.zeros((4, 8, 4, 8), device="cuda")
    up = torch.full((1, 4, 4, 8), 7.25, device="cuda")
    with pytest.raises(RuntimeError, match="w_folded"):
        ops.upconv2x(x, wf.half(), out=up)                               # a half operand under precision="fp32"
    with pytest.raises(RuntimeError, match="w_folded"):
        ops.upconv2x(x, wf.half(), out=up, precision="fp32")
    with pytest.raises(RuntimeError, match="w_folded"):
        ops.upconv2x(x, wf.to(torch.bfloat16), out=up, precision="fp16")
    torch.cuda.synchronize()
    assert bool((out == 7.25).all()) and bool((up == 7.25).all())       # nothing was launched
    # 7 | 256 does not exist: OFX_EINVAL from the launcher, nothing written
    from sd_animation_optical_flow_amd import _lib
    d = _lib.ConvDesc()
    xs = t["x"].cuda()
    d.in0, d.ld0, d.c0, d.w = xs.data_ptr(), c["c0"], c["c0"], w16.data_ptr()
    d.out, d.ldo = out.data_ptr(), c["cout"]
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = c["B"], c["H"], c["W"], Ho, Wo, c["cout"]
    d.KH, d.KW, d.stride, d.padH, d.padW = 3, 3, 1, 1, 1
    d.precision = PREC_F16_W | 256
    assert _lib.lib().ofx_conv2d(C.byref(d), None) == SC.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())


@pytest.mark.parametrize("c", UP_CASES, ids=UP_IDS)
def test_upconv2x_on_half_folded_weights_gives_the_bits_of_fp16(ops, c):
    x, wf, bias = up_inputs(c)
    B, H, W, co = c["B"], c["H"], c["W"], c["co"]
    xd, w32, bd = x.cuda(), wf.cuda(), bias.cuda()
    w16 = ops.half_conv_weight(wf).cuda()
    assert w16.dtype == torch.float16 and tuple(w16.shape) == tuple(wf.shape) and torch.equal(w16.cpu(), wf.half())
    sl = c["extra"].get("out_slice")
    for b in (bd, None):
        if sl:
            off, wide = sl
            full = [torch.full((B, 2 * H, 2 * W, wide), float("nan"), device="cuda") for _ in range(2)]
            ops.upconv2x(xd, w32, b, out=full[0], out_off=off, precision="fp16")
            ops.upconv2x(xd, w16, b, out=full[1], out_off=off, precision="fp16")
            want, got = full
            assert bool(torch.isnan(got[..., :off]).all()) and bool(torch.isnan(got[..., off + co:]).all())
        else:
            want, got = ops.upconv2x(xd, w32, b, precision="fp16"), ops.upconv2x(xd, w16, b, precision="fp16")
            assert tuple(got.shape) == (B, 2 * H, 2 * W, co) and bool(torch.isfinite(got).all())
            assert not torch.equal(got, ops.upconv2x(xd, w32, b))        # the half arithmetic, not the fp32 kernel
        assert torch.equal(bits(want), bits(got)), c["name"]
