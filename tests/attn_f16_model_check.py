"""`attention_precision="fp16"` at the level of the modules: float64 restatements of SpatialTransformer and of the UNet with the
roundings of the fp16 modes put in, and the bars of tests/test_gpu_attn_f16_model.py.  Not a conftest: imported by name, and
importable without a device.

transformer_check.spatial_transformer64 and unet_check.unet64 have no hooks for roundings, so `spatial_transformer64_r` restates the
block once more with two switches, and `unet64_r` runs unet_check.unet64 with that block and a rounding convolution in place:
  attn = "half"    the restatement of the MODE: q, k and v rounded to fp16, softmax in float64, P rounded to fp16, float64 products.
  attn = "kernel"  the kernel's own arithmetic (flash_attn_f16_check.fa16_emulate in float32: P rounded as exp2(x - m) stood when it
                   was used, before the division by l): what the device can at best reproduce.  Host tests only.
  gemm = True      both operands of every contraction that `precision="fp16"` runs on the fp16 matrix cores rounded to fp16: the
                   convolutions (not Upsample's, which stays fp32 on the device), proj_in / proj_out and every Linear of the
                   transformer blocks.  The timestep path stays exact, as on the device.
A float64 value is rounded through float32 (the device's activations are fp32 in memory) and then to half.

Bars.
  SpatialTransformer (c0, c1), against spatial_transformer64_r(attn="half"):
      bar_st(ref) = transformer_check.bar_of(ref) + 2 u16 max(1, max |ref|),   u16 = 2^-11.
    bar_of is the project's bar for the fp32 module and covers everything but the attention's new roundings.  Those: the kernel
    rounds exp2(x_j - m) at the running maximum, the restatement rounds the final p_j -- different grid points, up to u16 relative
    per key and of either sign; q, k, v are rounded from fp32 activations that differ from the float64 ones in the last bits, so a
    value next to a rounding boundary falls on the other side, one half-precision step (2 u16 relative) of one operand in about one
    element in a thousand.  An attention output is a convex combination of v rows, so each of the block's two attentions is off by
    at most about u16 of the magnitude of its values; both are added to the residual stream after LayerNorm-scaled, order-one
    activations.  Two attentions, u16 each, relative to the scale of the output: 2 u16 max(1, max |ref|).  First order, gains of
    the projections taken as one; the host test checks, on the arithmetic alone (attn = "kernel" against attn = "half"), that this
    reasoning holds at c0 and c1 before any device is asked: measured 5.2e-4 (c0) and 9.1e-4 (c1) against bars of 7.9e-3 and
    9.3e-3 (max |ref| is 6.7 and 7.9 there; the mode itself, attn = "half" against the exact restatement, is 9.2e-4 and 1.2e-3).
  UNet (u0): the bar of tests/test_gpu_unet_precision.py, 2 x autocast_vs_f64 per output (tests/golden/unet_ref_u0_autocast.npz):
    twice the distance of the reference's own half-attention mode from float64.  Arithmetic alone, on the CPU, before the GPU run
    (test_attn_f16_host.py::test_the_arithmetic_alone_stays_inside_the_unet_bar prints them), against unet64, over the five outputs:
        unet64_r(gemm=True,  attn="kernel")   2.6e-3 .. 2.8e-3     bars 7.4e-3 .. 9.0e-3
        unet64_r(gemm=False, attn="kernel")   4.4e-4 .. 4.8e-4     (precision="fp32" with attention_precision="fp16")
        unet64_r(gemm=True,  attn=None)       2.8e-3 .. 4.1e-3     (precision="fp16" alone, what is merged)
    The fp16 attention adds less than the contractions' roundings move from one sample to the next: the arithmetic fits with a
    factor of 2.7 to spare, so the bar stays that file's own (2 x, not bar4's 4 x).
  The K/V a transformer records is taken before its attention: on the same input it is bit for bit what the module built without
  the argument records (asserted per transformer).  Inside a whole UNet forward only the first transformer's input is independent
  of every attention, so there the whole-model comparison asserts bit-identity for the first transformer and dtype / shape for the
  rest, whose inputs have legitimately moved.

Measured on an MI355X (gfx950), 2026-10-19, tests/test_gpu_attn_f16_model.py (-s prints them); largest |difference|:
  SpatialTransformer against spatial_transformer64_r(attn="half"), plain / reference K/V of batch B / of batch B - 1:
      c0   5.01e-4 / 5.34e-4 / 5.34e-4    bar 7.9e-3 .. 8.0e-3     (the fp32 module against the same restatement: 8.0e-4 .. 9.2e-4)
      c1   9.13e-4 / 9.89e-4 / 9.13e-4    bar 9.3e-3 .. 9.5e-3     (1.2e-3 .. 1.6e-3)
    the device is where the CPU arithmetic put it (5.2e-4, 9.1e-4).
  UNetModel at u0 against unet64, out / out_refall / out_refpos / out_ctl / out_ctl_mid; bars 7.86e-3 / 8.41e-3 / 7.86e-3 / 7.42e-3 / 9.02e-3:
      precision="fp16", attention_precision="fp16"   2.55e-3 / 3.19e-3 / 2.63e-3 / 2.88e-3 / 3.00e-3
      precision="fp16" alone, same run               3.54e-3 / 3.02e-3 / 3.02e-3 / 2.90e-3 / 2.88e-3
      precision="fp32", attention_precision="fp16"   5.17e-4 / 5.21e-4 / 5.21e-4 / 4.76e-4 / 4.75e-4
      precision="fp32" alone, same run               4.84e-6 / 4.57e-6 / 4.84e-6 / 4.69e-6 / 4.72e-6
    fp16 attention moves the fp16 model by less than its own distance from float64, in either direction; on the fp32 model it is the
    whole distance, 5e-4, a fifteenth of the bar.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

import flash_attn_f16_check as f16
import transformer_check as TC
import unet_check as UC

U16 = f16.U16


def r16(t):
    """float64 -> the fp32 the device holds -> fp16 (nearest even) -> float64."""
    return t.float().half().double()


def bar_st(ref):
    return TC.bar_of(ref) + 2.0 * U16 * max(1.0, float(ref.abs().max()))


def attend(q, k, v, h, attn):
    """q [B,Nq,inner], k / v [B,Nk,inner] float64 -> [B,Nq,inner] float64 (header)."""
    if attn is None:
        return TC._attend(q, k, v, h)
    qh, kh, vh = TC._heads(q, h), TC._heads(k, h), TC._heads(v, h)
    d = qh.shape[-1]
    if attn == "half":
        p = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", r16(qh), r16(kh)) * (d ** -0.5), -1)
        o = torch.einsum("bhqk,bhkd->bhqd", r16(p), r16(vh))
    else:
        assert attn == "kernel"
        B, H, Nq, _ = qh.shape
        f = lambda t: t.reshape(B * H, t.shape[2], d).float()
        o = f16.fa16_emulate(f(qh), f(kh), f(vh), None, d ** -0.5).double().view(B, H, Nq, d)
    return o.permute(0, 2, 1, 3).reshape(q.shape)


@torch.no_grad()
def spatial_transformer64_r(sd64, x, heads, context=None, reference_kv=(), depth=1, gemm=False, attn=None):
    """transformer_check.spatial_transformer64 with the roundings of the header; the K/V history is taken before the attention and
    is not rounded (the device records fp32 tensors)."""
    R = r16 if gemm else (lambda t: t)
    x = x.double()
    B, C, h, w = x.shape
    t = F.group_norm(x, 32, sd64["norm.weight"], sd64["norm.bias"], eps=1e-6)
    t = F.conv2d(R(t), R(sd64["proj_in.weight"]), sd64["proj_in.bias"])
    inner = t.shape[1]
    t = t.reshape(B, inner, h * w).permute(0, 2, 1)
    N = h * w
    ctxs = list(context) if isinstance(context, (list, tuple)) else [context] * depth
    hists = []
    for i in range(depth):
        b = f"transformer_blocks.{i}"
        lin = lambda name, z, bias=False: R(z) @ R(sd64[f"{b}.{name}.weight"]).T + (sd64[f"{b}.{name}.bias"] if bias else 0.0)
        hn = TC._ln(sd64, f"{b}.norm1", t)
        q, k, v = lin("attn1.to_q", hn), lin("attn1.to_k", hn), lin("attn1.to_v", hn)
        hists.append((k, v))
        if reference_kv:
            k2 = torch.cat([e[0].double() for e in reference_kv], 1)
            v2 = torch.cat([e[1].double() for e in reference_kv], 1)
            if k2.shape[0] == B:
                k, v = k2, v2
            else:
                assert k2.shape[0] == B - 1 and k2.shape[1] == N
                k, v = torch.cat([k[:1], k2]), torch.cat([v[:1], v2])
        t = lin("attn1.to_out.0", attend(q, k, v, heads, attn), True) + t
        hn = TC._ln(sd64, f"{b}.norm2", t)
        src = hn if ctxs[i] is None else ctxs[i].double()
        t = lin("attn2.to_out.0", attend(lin("attn2.to_q", hn), lin("attn2.to_k", src), lin("attn2.to_v", src), heads, attn), True) + t
        a = lin("ff.net.0.proj", TC._ln(sd64, f"{b}.norm3", t), True)
        half = a.shape[-1] // 2
        gate = a[..., half:]
        t = lin("ff.net.2", a[..., :half] * (0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0)))), True) + t
    t = t.permute(0, 2, 1).reshape(B, inner, h, w)
    return F.conv2d(R(t), R(sd64["proj_out.weight"]), sd64["proj_out.bias"]) + x, hists


@contextlib.contextmanager
def _patched(gemm, attn):
    """unet_check.unet64 looks `_conv`, `upsample64` and `TC.spatial_transformer64` up when it runs: swap them for the call."""
    keep = (UC._conv, UC.upsample64, TC.spatial_transformer64)
    exact_conv = UC._conv

    def conv_r(sd, name, x, stride=1, pad=1):
        return F.conv2d(r16(x), r16(sd[f"{name}.weight"]), sd[f"{name}.bias"], stride=stride, padding=pad)

    def upsample_exact(sd, name, x):
        return exact_conv(sd, f"{name}.conv", F.interpolate(x, scale_factor=2, mode="nearest"))

    def st(sub, h, heads, ctx, ref, depth=1):
        return spatial_transformer64_r(sub, h, heads, ctx, ref, depth=depth, gemm=gemm, attn=attn)

    try:
        if gemm:
            UC._conv, UC.upsample64 = conv_r, upsample_exact
        TC.spatial_transformer64 = st
        yield
    finally:
        UC._conv, UC.upsample64, TC.spatial_transformer64 = keep


def unet64_r(sd64, layout, x, timesteps, context, gemm=False, attn=None, **kw):
    """unet_check.unet64 with the roundings of the header."""
    with _patched(gemm, attn):
        return UC.unet64(sd64, layout, x, timesteps, context, **kw)
