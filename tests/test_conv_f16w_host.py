"""Half-stored weights (OFX_PREC_F16_W = 7, `ops.conv2d_nhwc(precision="fp16_w")`, `weight_dtype="fp16"` of the SD models) as far
as the host can tell: the launcher's plan under 7 is the plan under OFX_PREC_F16 in every field but `prec` -- for every case of
tests/f16_check.py and every `ofx_conv2d` launch of the v1.5 UNet -- and 7 rejects what 5 rejects; `ofx_half_conv_weight` rounds as
`torch.Tensor.half()` does, bit for bit, at every boundary of the format; the constructors check `weight_dtype` before a checkpoint or
a device is looked at; the precision tables read as documented.  No GPU: the descriptors carry dummy, aligned, never-dereferenced
pointers."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import f16_check as FC   # noqa: E402
import test_conv_f16_host as H16   # noqa: E402  (its descriptor builder and the v1.5 UNet's launch list)
import unet_check as UC   # noqa: E402

PTR, EINVAL = H16.PTR, H16.EINVAL
PREC_F16_W = 7
PLAN_FIELDS = ("path", "bm", "bn", "wm", "wn", "bk", "ks", "ksplit", "mode", "mtiles", "ntiles", "group_m", "stats_rows")


def _lib():
    from sd_animation_optical_flow_amd import _lib
    return _lib


def _plans(**kw):
    """-> ((status, plan) under OFX_PREC_F16, the same under OFX_PREC_F16_W) of one descriptor."""
    return H16._query(H16._desc(precision=FC.PREC_F16, **kw)), H16._query(H16._desc(precision=PREC_F16_W, **kw))


def _same_but_prec(p5, p7):
    assert p5.prec == FC.PREC_F16 and p7.prec == PREC_F16_W
    assert [getattr(p7, f) for f in PLAN_FIELDS] == [getattr(p5, f) for f in PLAN_FIELDS]


def test_plan_fields_cover_the_structure():
    assert sorted(PLAN_FIELDS + ("prec",)) == sorted(n for n, _ in _lib().ConvPlan._fields_)


@pytest.mark.parametrize("c", FC.CASES, ids=FC.IDS)
def test_every_case_plans_as_under_fp16(c):
    (s5, p5), (s7, p7) = _plans(B=c["B"], H=c["H"], W=c["W"], c0=c["c0"], cout=c["cout"], k=c["k"], stride=c["stride"], tile=c["tile"], c1=c["c1"])
    assert s5 == 0 and s7 == 0
    _same_but_prec(p5, p7)
    assert (p7.bm, p7.bn, p7.bk, p7.mode) == c["plan"]


def test_every_layer_of_the_v15_unet_plans_as_under_fp16():
    layers = H16.v15_conv_layers()
    assert len(layers) == 207
    for name, B, h, w, c0, c1, cout, k, stride in layers:
        (s5, p5), (s7, p7) = _plans(B=B, H=h, W=w, c0=c0, cout=cout, k=k, stride=stride, c1=c1, shift=PTR)
        assert s5 == 0 and s7 == 0, name
        _same_but_prec(p5, p7)
    # wino_w / wino4_w are ignored, as they are under OFX_PREC_F16
    (s5, p5), (s7, p7) = _plans(B=16, H=64, W=96, c0=128, cout=128, k=3, wino_w=PTR, wino4_w=PTR)
    assert s5 == 0 and s7 == 0 and p7.path == 0 and p7.mode == 2
    _same_but_prec(p5, p7)


def test_plan_rejections_are_those_of_fp16():
    base = dict(B=2, H=8, W=16, c0=64, cout=64, k=3)
    gru = dict(aux_z=PTR, aux_rh=PTR, aux_h=PTR, ldh=64)
    flow = dict(aux_coords=PTR, aux_h=PTR, aux_flow4=PTR, cout=2)
    for prec in (FC.PREC_F16, PREC_F16_W):
        ok = lambda **kw: H16._query(H16._desc(**dict(base, precision=prec, **kw)))[0]
        assert ok() == 0
        assert ok(epi=1, **gru) == EINVAL                       # OFX_EPI_GRU_ZR
        assert ok(epi=2, **gru) == EINVAL                       # OFX_EPI_GRU_Q
        assert ok(epi=3, **flow) == EINVAL                      # OFX_EPI_FLOW
        assert ok(nmean=PTR, nrstd=PTR) == EINVAL               # fused instance norm
        assert H16._query(H16._desc(**dict(base, precision=prec)), stats_cap=1 << 40)[0] == EINVAL      # ofx_conv2d_stats
        assert ok(splitk_ws=PTR, splitk_ws_bytes=1 << 40) == EINVAL       # split-K workspace
        assert ok(tile=2032064064) == EINVAL                    # the paired-pipeline marker
        assert ok(nz=2) == EINVAL                               # batched GEMM
        assert H16._query(H16._desc(1, 16, 16, 256, 256, 1, precision=prec), pool=1)[0] == EINVAL       # pooled correlation volume
        st, p = H16._query(H16._desc(**dict(base, precision=prec, tile=16128192)))                      # a tile it lacks: mapped
        assert st == 0 and (p.bm, p.bn) == (128, 128)
    bad = lambda prec: H16._query(H16._desc(**dict(base, precision=prec)))[0]
    assert bad(6) == EINVAL and bad(-1) == EINVAL               # still no precision
    assert bad(PREC_F16_W | 256) == EINVAL                      # the extensions of OFX_PREC_F16_EPI stay with fp32 weights
    assert bad(256) == EINVAL and bad(5 | 512) == EINVAL
    # what OFX_PREC_F16_EPI lets through, 7 does not
    assert H16._query(H16._desc(**dict(base, precision=5 | 256, nmean=PTR, nrstd=PTR)))[0] == 0


def _boundary_vector():
    """fp32 values at every boundary of the conversion, with both signs: ties between neighbouring halves (to even, both ways),
    the subnormal range and its ends, the overflow threshold, zeros, fp32 denormals, NaN, and a seeded spread of ordinary values."""
    two = lambda e: 2.0 ** e
    v = [0.0, 1.0, 1.0 + two(-11), 1.0 + two(-10) + two(-11), 1.0 + two(-11) + two(-23), 1.0 + two(-11) - two(-24),   # ties at 1: down to even, up to even, just above, just below
         2048.0 + 1.0, 2048.0 + 3.0, 1.0 / 3.0, 0.1, 3.14159265,
         two(-14), two(-14) - two(-25), two(-14) - two(-26), two(-14) + two(-25),                     # smallest normal and its neighbourhood
         two(-15), 3 * two(-24), 2.5 * two(-24), 3.5 * two(-24), 1023.5 * two(-24), 1023.0 * two(-24),      # subnormals, their ties
         two(-24), 1.5 * two(-24), 0.5 * two(-24), two(-25), two(-25) * (1 + two(-23)), two(-25) * (1 - two(-24)), two(-26), 0.75 * two(-24),
         65504.0, 65519.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 3e38, float("inf"),
         1e-40, 1.4e-45, two(-126), two(-127)]                                                          # fp32 denormals and the smallest normal
    t = torch.tensor(v + [-x for x in v], dtype=torch.float32)
    g = torch.Generator().manual_seed(20240)
    spread = torch.randn(4096, generator=g) * torch.exp(torch.randn(4096, generator=g) * 6.0)           # ~ +-2^-26 .. 2^26
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (4096,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)   # any pattern, NaNs among them
    nan = torch.tensor([float("nan"), -float("nan")], dtype=torch.float32)
    return torch.cat([t, spread, bits, nan])


def test_half_conv_weight_rounds_as_torch_half_does_bit_for_bit():
    from sd_animation_optical_flow_amd import ops
    x = _boundary_vector()
    got = ops.half_conv_weight(x)
    want = x.half()
    assert got.dtype == torch.float16 and got.shape == x.shape
    isn = torch.isnan(want)
    assert int(isn.sum()) >= 2 and torch.equal(torch.isnan(got), isn)                                  # NaN stays NaN, and only NaN
    assert torch.equal(got.view(torch.int16)[~isn], want.view(torch.int16)[~isn])
    # and the table says what the boundaries are: subnormals are produced, 2^-25 is the tie that goes to zero, 65520 is the first infinity
    f = lambda v: ops.half_conv_weight(torch.tensor([v], dtype=torch.float32))
    assert float(f(2.0 ** -24)) == 2.0 ** -24 and float(f(2.0 ** -25)) == 0.0 and float(f(2.0 ** -25 * (1 + 2.0 ** -23))) == 2.0 ** -24
    assert float(f(65504.0)) == 65504.0 and float(f(65519.996)) == 65504.0 and float(f(-65504.0)) == -65504.0
    assert float(f(65520.0)) == float("inf") and float(f(1e5)) == float("inf") and float(f(-1e5)) == -float("inf")
    assert f(-0.0).view(torch.int16).item() == -32768 and f(0.0).view(torch.int16).item() == 0         # the sign of zero is kept
    assert float(f(1e-40)) == 0.0
    # shapes are kept, the packed matrix of a convolution included
    w = torch.randn((5, 8, 3, 3), generator=torch.Generator().manual_seed(1))
    packed = ops.pack_conv_weight(w)
    assert torch.equal(ops.half_conv_weight(packed), packed.half()) and ops.half_conv_weight(packed).shape == packed.shape
    L = _lib().lib()
    buf = torch.empty(4, dtype=torch.float16)
    src = torch.zeros(4)
    assert L.ofx_half_conv_weight(None, 4, C.c_void_p(buf.data_ptr())) == EINVAL
    assert L.ofx_half_conv_weight(C.c_void_p(src.data_ptr()), 4, None) == EINVAL
    assert L.ofx_half_conv_weight(C.c_void_p(src.data_ptr()), 0, C.c_void_p(buf.data_ptr())) == EINVAL


def test_upconv2x_bn_answers_for_7_as_for_5():
    L = _lib().lib()
    for cout in (1, 4, 64, 65, 128, 136, 512):
        assert L.ofx_upconv2x_bn(cout, PREC_F16_W) == L.ofx_upconv2x_bn(cout, 5) in (64, 128)
    assert L.ofx_upconv2x_bn(0, PREC_F16_W) == EINVAL
    for prec in (1, 2, 3, 4, 6, 261, -1):
        assert L.ofx_upconv2x_bn(64, prec) == EINVAL
        # a precision the kernel lacks is rejected before the alignment of the operands is looked at
        assert L.ofx_upconv2x_prec(C.c_void_p(PTR + 4), C.c_void_p(PTR), None, C.c_void_p(PTR), 8, 1, 2, 2, 8, 8, prec, None) == EINVAL


def test_weight_dtype_argument_is_checked_first():
    from sd_animation_optical_flow_amd import modelbase
    from sd_animation_optical_flow_amd.controlnet import ControlNet
    from sd_animation_optical_flow_amd.transformer import MODEL_PRECISIONS, SpatialTransformer
    from sd_animation_optical_flow_amd.unet import UNetModel
    from sd_animation_optical_flow_amd.vae import VAE_PRECISIONS, VaeDecoder, VaeEncoder
    assert modelbase.WEIGHT_DTYPES == ("fp32", "fp16")
    assert MODEL_PRECISIONS == ("fp32", "fp16", "bf16x3", "bf16x6") and VAE_PRECISIONS == ("fp32", "fp16")
    # an empty checkpoint would be a KeyError and a missing device a RuntimeError: weight_dtype is looked at before either
    builders = [lambda **kw: UNetModel({}, UC.U0, **kw), lambda **kw: ControlNet({}, dict(UC.U0, hint_channels=3), **kw),
                lambda **kw: SpatialTransformer({}, 1, 64, **kw), lambda **kw: VaeEncoder({}, **kw), lambda **kw: VaeDecoder({}, **kw)]
    for build in builders:
        with pytest.raises(ValueError, match="weight_dtype"):
            build(precision="fp16", weight_dtype="fp17")
        with pytest.raises(ValueError, match="weight_dtype"):
            build(precision="fp16", weight_dtype=None)
        with pytest.raises(ValueError, match="weight_dtype.*precision"):                # names both arguments
            build(precision="fp32", weight_dtype="fp16")
        with pytest.raises(ValueError, match="weight_dtype.*precision"):
            build(weight_dtype="fp16")                                                  # the default precision is fp32
        with pytest.raises(ValueError, match="precision"):
            build(precision="fp17", weight_dtype="fp16")
    for build in builders[:3]:
        with pytest.raises(ValueError, match="weight_dtype.*precision"):
            build(precision="bf16x3", weight_dtype="fp16")


def test_precision_tables():
    from sd_animation_optical_flow_amd import ops
    assert ops.CONV_PRECISIONS == {"fp32": 0, "bf16x3": 1, "bf16x3_w": 2, "bf16x6": 3, "bf16x6_w": 4, "fp16": 5, "fp16_epi": 5 | 256, "fp16_w": 7}
    assert ops.UPCONV_PRECISIONS == {"fp32": 0, "fp16": 5}
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ofx.h")).read()
    assert "#define OFX_PREC_F16_W 7" in hdr and "int ofx_half_conv_weight(const float* packed, long n_floats, void* out_halves);" in hdr
    assert "ofx_half_conv_weight" in _lib().SIGNATURES
