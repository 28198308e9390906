"""-m gpu: the fp16 form of the fused nearest-2x upsample convolution (`ops.upconv2x(precision="fp16")`, ofx_upconv2x_prec with
OFX_PREC_F16) against the float64 contraction of the operands it rounds.

Arithmetic under test.  x and the FOLDED weights (`ops.upconv2x_weight`) are rounded fp32 -> fp16, to nearest even, as the kernel
stages them; every product is formed on v_mfma_f32_32x32x16_f16 and accumulated in fp32; the bias add and the stored result are fp32.

Oracle.  The float64 contraction of x.half().double() and w_folded.half().double() over the four taps of each parity, plus the bias.
The product of two fp16 values is exact in fp32, so what is left is the fp32 accumulation of K = 4 Cin terms and the bias add: with
u = 2^-24 (tests/f16_check.py)

    |out - ref| <= (K + 2) u sum |x_h| |w_h| + u |bias| + 2 u |ref| + FLOOR

Nothing in it is measured, and it has no flush term: the "small" case (operands N(0, 1) * 1e-3, a few percent of them subnormal in
fp16) holds the device to it.  The "max" case holds +-65504 exactly in a few positions of x and of the folded w and stays finite."""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sd_ops_check as SC   # noqa: E402

U, FLOOR = SC.U, SC.FLOOR


def _c(name, B, H, W, ci, co, bn, **extra):
    return dict(name=name, B=B, H=H, W=W, ci=ci, co=co, bn=bn, extra=extra)


CASES = [
    _c("one-pixel", 1, 1, 1, 4, 4, 64),                      # three of four taps in the padding; K ends inside the first chunk
    _c("ragged", 2, 5, 7, 36, 40, 64),                       # M = 70 < one tile; Cin ends inside the second 32-chunk; ragged BN = 64
    _c("multi-tile", 3, 9, 11, 64, 136, 128),                # M = 297 crosses image boundaries inside tiles; two ragged BN = 128 column tiles
    _c("long-k", 1, 4, 6, 256, 256, 128),                    # the VAE's own width; 32 chunks
    _c("out-slice", 2, 5, 7, 36, 40, 64, out_slice=(8, 56)),  # channels [8, 48) of a 56-wide NaN-filled tensor
    _c("small", 2, 5, 7, 36, 40, 64, mag=1e-3),              # fp16 subnormals
    _c("max", 2, 5, 7, 36, 40, 64, extreme=True),            # +-65504
]
IDS = [c["name"] for c in CASES]


def _inputs(c):
    """-> x NHWC [B,H,W,ci], folded w [4,co,4,ci], bias [co]: float32 CPU tensors."""
    from sd_animation_optical_flow_amd import ops
    g = SC._gen("upconv-f16-" + c["name"])
    B, H, W, ci, co = c["B"], c["H"], c["W"], c["ci"], c["co"]
    mag = c["extra"].get("mag", 1.0)
    x = torch.randn((B, H, W, ci), generator=g) * 1.5 * mag
    w = torch.randn((co, ci, 3, 3), generator=g) * (mag / math.sqrt(9 * ci))
    bias = 0.1 * mag * torch.randn((co,), generator=g)
    wf = ops.upconv2x_weight(w)
    if c["extra"].get("extreme"):
        x[0, 0, 0, 0], x[1, 2, 3, 7], x[B - 1, H - 1, W - 1, ci - 1] = 65504.0, -65504.0, 65504.0
        wf[0, 0, 0, 0], wf[3, co - 1, 3, ci - 1], wf[2, 5, 1, 33] = 65504.0, -65504.0, 65504.0
    return x, wf, bias


def _reference(x, wf, bias):
    """-> (ref, bound) float64 NHWC [B,2H,2W,co] of the rounded operands (header); bias may be None."""
    B, H, W, ci = x.shape
    co = wf.shape[1]
    xh = F.pad(x.half().double().permute(0, 3, 1, 2), (1, 1, 1, 1))           # low-resolution pixel (y, x) at (y + 1, x + 1)
    wh = wf.half().double()
    assert bool(torch.isfinite(xh).all()) and bool(torch.isfinite(wh).all())
    ref = torch.zeros((B, co, 2 * H, 2 * W), dtype=torch.float64)
    mag = torch.zeros_like(ref)
    for py in range(2):
        for px in range(2):
            k = wh[2 * py + px].reshape(co, 2, 2, ci).permute(0, 3, 1, 2)     # tap 2 ty + tx over pixel (y - 1 + py + ty, x - 1 + px + tx)
            win = xh[:, :, py:py + H + 1, px:px + W + 1]
            ref[:, :, py::2, px::2] = F.conv2d(win, k)
            mag[:, :, py::2, px::2] = F.conv2d(win.abs(), k.abs())
    bound = (4 * ci + 2) * U * mag
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1, 1)
        bound = bound + U * bias.double().abs().view(1, -1, 1, 1)
    bound = bound + 2 * U * ref.abs() + FLOOR
    return ref.permute(0, 2, 3, 1), bound.permute(0, 2, 3, 1)


@pytest.fixture(scope="module")
def cases():
    """Inputs and float64 references, computed once and left unchanged."""
    out = {}
    for c in CASES:
        x, wf, bias = _inputs(c)
        out[c["name"]] = dict(x=x, wf=wf, bias=bias, with_bias=_reference(x, wf, bias), no_bias=_reference(x, wf, None))
    return out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_upconv2x_fp16_against_float64_of_the_rounded_operands(cuda, cases, c):
    from sd_animation_optical_flow_amd import ops
    t = cases[c["name"]]
    B, H, W, co = c["B"], c["H"], c["W"], c["co"]
    assert ops.upconv2x_bn(co, "fp16") == c["bn"]                             # the instantiation this case is there for
    x, wf, bias = t["x"].cuda(), t["wf"].cuda(), t["bias"].cuda()
    sl = c["extra"].get("out_slice")
    for label, b in (("with_bias", bias), ("no_bias", None)):
        ref, bound = t[label]
        if sl:
            off, wide = sl
            full = torch.full((B, 2 * H, 2 * W, wide), float("nan"), device="cuda")
            ops.upconv2x(x, wf, b, out=full, out_off=off, precision="fp16")
            full = full.cpu()
            assert bool(torch.isnan(full[..., :off]).all()) and bool(torch.isnan(full[..., off + co:]).all())   # nothing outside the slice
            got = full[..., off:off + co]
        else:
            got = ops.upconv2x(x, wf, b, precision="fp16").cpu()
        assert tuple(got.shape) == (B, 2 * H, 2 * W, co) and got.dtype == torch.float32
        assert bool(torch.isfinite(got).all())
        err = (got.double() - ref).abs()
        worst = SC._worst(err, bound)
        print(f"upconv2x fp16 {c['name']} {label}: BN {c['bn']}, max |err| {float(err.max()):.3e}, worst |err| / bound {worst:.4f}")
        assert worst <= 1.0, (c["name"], label, worst)
    if c["extra"].get("mag"):
        sub = float(((t["x"].abs() < 2.0 ** -14) & (t["x"] != 0)).float().mean())
        assert sub > 0.01, sub                                                # the case does hold fp16 subnormals
    if not sl:
        # the half arithmetic ran: the fp32 kernel on the same operands gives other bits
        assert not torch.equal(got, ops.upconv2x(x, wf, None).cpu())


@pytest.mark.parametrize("c", CASES[:4], ids=IDS[:4])
def test_precision_fp32_is_the_call_without_the_argument(cuda, cases, c):
    from sd_animation_optical_flow_amd import ops
    t = cases[c["name"]]
    x, wf, bias = t["x"].cuda(), t["wf"].cuda(), t["bias"].cuda()
    assert ops.upconv2x_bn(c["co"], "fp32") == c["bn"]
    assert torch.equal(ops.upconv2x(x, wf, bias, precision="fp32"), ops.upconv2x(x, wf, bias))
    assert torch.equal(ops.upconv2x(x, wf, None, precision="fp32"), ops.upconv2x(x, wf, None))


def test_ofx_upconv2x_prec_rejects_bad_arguments_without_launching(cuda):
    from sd_animation_optical_flow_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros((1, 2, 2, 8), device="cuda")
    w = torch.zeros((4, 8, 4, 8), device="cuda")
    o = torch.full((1, 4, 4, 8), 7.0, device="cuda")
    s = ops._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.ofx_upconv2x_prec(p(x), p(w), None, p(o), 8, 1, 2, 2, 8, 8, 1, s) == SC.EINVAL             # bf16x3: not a precision of this kernel
    assert L.ofx_upconv2x_prec(p(x), p(w), None, p(o), 8, 1, 2, 2, 8, 8, 6, s) == SC.EINVAL
    for prec in (0, 5):
        assert L.ofx_upconv2x_prec(None, p(w), None, p(o), 8, 1, 2, 2, 8, 8, prec, s) == SC.EINVAL      # null pointer
        assert L.ofx_upconv2x_prec(p(x), p(w), None, p(o), 7, 1, 2, 2, 8, 8, prec, s) == SC.EINVAL      # ldo < Cout
        assert L.ofx_upconv2x_prec(p(x), p(w), None, p(o), 8, 1, 2, 2, 6, 8, prec, s) == SC.EALIGN      # Cin % 4
        assert L.ofx_upconv2x_prec(C.c_void_p(x.data_ptr() + 4), p(w), None, p(o), 8, 1, 2, 2, 8, 8, prec, s) == SC.EALIGN   # x not 16-byte aligned
        assert L.ofx_upconv2x_prec(p(x), C.c_void_p(w.data_ptr() + 4), None, p(o), 8, 1, 2, 2, 8, 8, prec, s) == SC.EALIGN   # w not 16-byte aligned
    torch.cuda.synchronize()
    assert bool((o == 7.0).all())
    assert L.ofx_upconv2x_prec(p(x), p(w), None, p(o), 8, 1, 2, 2, 8, 8, 5, s) == 0
    torch.cuda.synchronize()
    assert bool((o == 0.0).all())
    with pytest.raises(ValueError):
        ops.upconv2x(x, w, precision="bf16x3")
