"""The fp16 arithmetic of the convolution launcher (OFX_PREC_F16) on the device: every case of tests/f16_check.py against the
float64 convolution of the fp16-rounded operands, every element inside the derived bound; the mode really ran (the result differs
from the fp32 kernel's); repeats are bit-identical; what the arithmetic does not serve is rejected before any launch.  Every test
prints its figures (-s)."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import f16_check as FC   # noqa: E402
import sd_ops_check as SC   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from sd_animation_optical_flow_amd import ops as O
    return O


def _run(ops, c, t, precision, out=None, out_off=0):
    dev = lambda a: None if a is None else a.cuda()
    return ops.conv2d_nhwc(dev(t["x"]), ops.pack_conv_weight(t["w"]).cuda(), c["k"], c["k"], c["cout"], stride=c["stride"],
                           shift=dev(t["shift"]), scale=dev(t["scale"]), act=c["extra"].get("act"), x2=dev(t["x2"]), res=dev(t["res"]),
                           addend=dev(t["addend"]), tile=c["tile"], precision=precision, out=out, out_off=out_off)


@pytest.mark.parametrize("c", FC.CASES, ids=FC.IDS)
def test_fp16_convolution_against_float64(ops, c):
    t = FC.inputs(c)
    ref, bound = FC.reference(c, t)
    sl = c["extra"].get("out_slice")
    if sl is None:
        got = _run(ops, c, t, "fp16")
        again = _run(ops, c, t, "fp16")
        exact = _run(ops, c, t, "fp32")
        assert torch.equal(got, again)                               # a second call repeats the bits
    else:
        off, ldo = sl
        Ho, Wo = FC.out_hw(c)
        wide = torch.full((c["B"], Ho, Wo, ldo), FC.NAN, device="cuda")
        ret = _run(ops, c, t, "fp16", out=wide, out_off=off)
        assert ret.data_ptr() == wide.data_ptr()
        gap = torch.ones(ldo, dtype=torch.bool)
        gap[off:off + c["cout"]] = False
        assert bool(torch.isnan(wide[..., gap.cuda()]).all())        # the channels around the slice were not written
        got = wide[..., off:off + c["cout"]].contiguous()
        wide2 = torch.full_like(wide, FC.NAN)
        _run(ops, c, t, "fp16", out=wide2, out_off=off)
        assert torch.equal(wide2[..., off:off + c["cout"]], got)
        exact = _run(ops, c, t, "fp32")
    assert tuple(got.shape) == tuple(ref.shape)
    worst = FC.worst_ratio(got.cpu(), ref, bound)
    rel32 = float((exact.cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"{c['name']}: |error| / bound {worst:.3f}; the fp32 kernel is {rel32:.2e} of max |ref| away from the rounded-operand reference")
    assert worst <= 1.0
    assert not torch.equal(got, exact)                               # the fp16 arithmetic ran, not the fp32 kernel


def test_fp16_rejects_before_any_launch(ops):
    """What OFX_PREC_F16 does not serve is OFX_EINVAL, with nothing launched: a poisoned output stays poisoned."""
    from sd_animation_optical_flow_amd import _lib
    L = _lib.lib()
    B, H, W, cin, cout, POISON = 2, 8, 16, 64, 64, 7.25
    g = SC._gen("f16-reject")
    x = torch.randn((B, H, W, cin), generator=g).cuda()
    w4 = torch.randn((cout, cin, 3, 3), generator=g) / 24.0
    w = ops.pack_conv_weight(w4).cuda()
    out = torch.full((B, H, W, cout), POISON, device="cuda")
    aux = torch.full((B, H, W, cout), POISON, device="cuda")
    stat = torch.full((B * 64 * cout * 2,), POISON, device="cuda")
    ws = torch.zeros((1 << 22,), dtype=torch.uint8, device="cuda")
    small = torch.zeros((B, cin), device="cuda")
    p = lambda t: t.data_ptr()

    def desc(**kw):
        d = _lib.ConvDesc()
        d.in0, d.ld0, d.c0, d.w = p(x), cin, cin, p(w)
        d.out, d.ldo = p(out), cout
        d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, H, W, H, W, cout
        d.KH, d.KW, d.stride, d.padH, d.padW = 3, 3, 1, 1, 1
        d.precision = FC.PREC_F16
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    rows = C.c_int(-1)
    gru = dict(epi=1, aux_z=p(aux), aux_rh=p(aux), aux_h=p(aux), ldh=cout)       # OFX_EPI_GRU_ZR
    cases = [
        ("GRU z|r epilogue", L.ofx_conv2d(C.byref(desc(**gru)), None)),
        ("GRU q epilogue", L.ofx_conv2d(C.byref(desc(**dict(gru, epi=2))), None)),
        ("fused instance norm", L.ofx_conv2d(C.byref(desc(nmean=p(small), nrstd=p(small))), None)),
        ("ofx_conv2d_stats", L.ofx_conv2d_stats(C.byref(desc()), C.c_void_p(p(stat)), stat.numel(), C.byref(rows), None)),
        ("split-K workspace", L.ofx_conv2d(C.byref(desc(splitk_ws=p(ws), splitk_ws_bytes=ws.numel())), None)),
        ("paired pipelines", L.ofx_conv2d(C.byref(desc(tile=2032064064)), None)),
        ("nz = 2", L.ofx_conv2d(C.byref(desc(nz=2, a_zs=0, w_zs=0, o_zs=0)), None)),
        ("precision 6", L.ofx_conv2d(C.byref(desc(precision=6)), None)),
    ]
    # the same descriptors with the fp32 arithmetic are launches the library takes: the rejection is the precision's
    plan = _lib.ConvPlan()
    assert L.ofx_conv2d_plan(C.byref(desc(precision=0, splitk_ws=p(ws), splitk_ws_bytes=ws.numel())), 0, 0, C.byref(plan)) == 0
    assert plan.ksplit > 1                                           # (this shape does split K in fp32: the workspace is no formality)
    assert L.ofx_conv2d_plan(C.byref(desc(precision=0, **gru)), 0, 0, C.byref(plan)) == 0
    torch.cuda.synchronize()
    for what, got in cases:
        assert got == SC.EINVAL, (what, got)
    for t in (out, aux, stat):
        assert bool((t == POISON).all())                             # nothing was launched
    assert not bool(ws.any())
    # the valid call on the same buffers runs
    assert L.ofx_conv2d(C.byref(desc()), None) == 0
    torch.cuda.synchronize()
    c = dict(name="valid", k=3, stride=1, extra={})
    ref, bound = FC.reference(c, dict(x=x.cpu(), x2=None, w=w4, scale=None, shift=None, addend=None, res=None))
    assert FC.worst_ratio(out.cpu(), ref, bound) <= 1.0
