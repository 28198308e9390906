"""Float64 references and an operand-scaled error bound for the convolution tests (not a conftest: imported by name).

A float32 convolution's rounding error at an output is bounded by a multiple of the unit round-off times the magnitude of the
operation, M = conv(|x|, |w|) |scale| + |shift| + |addend|: Winograd transforms add and scale inputs and products before they
cancel, so their error follows the input's magnitude, not the output's.  The check is |out - ref| <= K 2^-24 M + TINY with one K
per kernel.
"""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
TINY = 1e-30
# K per kernel: at most 2x the largest |err| / (2^-24 M) measured on MI355X over tests/test_gpu_conv_winograd_sweep.py (the plain
# sweep, the engine-layer and the GRU cases; the direct kernel over the same cases).  Measured maxima:
#   direct (fp32 MFMA kernels)                5.83
#   F(2x2,3x3)                                3.17
#   F(4,5) plain                              21.5
#   F(4,5) GRU_ZR / GRU_Q (pre-activation)    15.7 / 16.1
# The direct kernels' GRU gate epilogues over the cases of tests/gru_check.py (test_gpu_conv_gru_direct.py), measured on MI355X:
#   fp32, every tile / schedule / split-K      2.85  (inside the 5.83 above: K_DIRECT as it stands)
#   bf16x3 / bf16x3_w                          1.94  against the float64 sum of the three products of the CPU-split operands
#   bf16x6 / bf16x6_w                          2.31  against the float64 convolution of the exact operands
# What the split-bf16 constants cover is the fp32 accumulation on the bf16 matrix cores (and, bf16x6, the three dropped products
# below 2^-23); the operand arithmetic is in the reference.  K_DIRECT_BF16X6 <= 3 K_DIRECT whatever is measured (fp32-accurate).
K_DIRECT = 11.0
K_DIRECT_BF16X3 = 3.8
K_DIRECT_BF16X6 = 4.6
K_F23 = 6.0
K_F45 = 42.0
K_F45_GRU = 32.0
# the sweep's worst fused ratio over its worst direct ratio, per algorithm (measured: 3x3 0.48, 1x5 3.92, 5x1 3.63)
K_SAME_SCALE = 7.5
ACT_ULP = 2e-7           # the activation's own evaluation (ofx_sigmoid / ofx_tanh: __expf and a hardware reciprocal), absolute


def pad_of(kh, kw):
    return (kh // 2, kw // 2)


def conv64(x, w, kh, kw):
    """x NCHW, w OIHW (any float dtype) -> the 'same' correlation in float64."""
    return F.conv2d(x.double(), w.double().view(w.shape[0], -1, kh, kw), padding=pad_of(kh, kw))


def _chan(v):
    return v.double().view(1, -1, 1, 1)


def reference(x, w, kh, kw, scale=None, shift=None, addend=None, relu=False):
    """The plain epilogue in float64 and its magnitude M (both NCHW).  addend NCHW."""
    acc = conv64(x, w, kh, kw)
    mag = conv64(x.abs(), w.abs(), kh, kw)
    if scale is not None:
        acc, mag = acc * _chan(scale), mag * _chan(scale).abs()
    if shift is not None:
        acc, mag = acc + _chan(shift), mag + _chan(shift).abs()
    if addend is not None:
        acc, mag = acc + addend.double(), mag + addend.double().abs()
    return (torch.relu(acc) if relu else acc), mag


def violations(out, ref, mag, K, slope=1.0, extra=0.0):
    """Mask of the elements outside |out - ref| <= slope (K 2^-24 M) + extra + TINY (NaN counts as outside)."""
    err = (out.double() - ref.double()).abs()
    return ~(err <= slope * K * EPS * mag.double() + extra + TINY)


def worst_ratio(out, ref, mag, slope=1.0, extra=0.0):
    """max over the elements of (|out - ref| - extra) / (slope 2^-24 M): the smallest K the elements satisfy."""
    err = (out.double() - ref.double()).abs() - extra
    r = err.clamp_min(0) / (slope * EPS * mag.double()).clamp_min(TINY)
    return float(r.max()) if r.numel() else 0.0


def check(out, ref, mag, K, what, slope=1.0, extra=0.0):
    """Assert the bound and return the worst ratio."""
    bad = violations(out, ref, mag, K, slope, extra)
    ratio = worst_ratio(out, ref, mag, slope, extra)
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside K = {K} (worst ratio {ratio:.3g}); "
                             f"first at {idx}: got {float(out[tuple(idx)])}, want {float(ref[tuple(idx)])}")
    return ratio
