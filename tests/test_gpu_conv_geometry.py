"""The direct convolutions off 'same' padding on the device: every case of tests/geom_check.py -- pads, output sizes and strides that
padH = KH // 2 with the size that follows never reaches, the VAE encoder's Downsample (3x3, stride 2, pad (0, 0), out (H / 2, W / 2))
on every fp32 row of kTiles and every fp16 instantiation among them -- as a raw ConvDesc launch through ofx_conv2d.  The geometries,
the case table (with the plan every case reaches, never the halo patch: held on the CPU by test_geom_check_host.py) and the simulated
bugs are geom_check.py's; oracles and bounds are fp32_check.py's (K_DIRECT), bf16_check.py's (K_of(prec)) and f16_check.py's (the
derived bound), unchanged: a geometry changes which terms enter a sum, not the arithmetic.

Per case: the plan, asked again of the device build; every buffer the descriptor names between GUARD rows of NaN, the output NaN over
its full ldo; the result inside the bound (the worst ratio is printed as a RATIO line; the table of them is in the header of
wino_check.py); every output with no tap inside the image -- the frame of the `ring` cases, the rows and columns beyond the natural
output of `over` -- equal to the epilogue of an exact zero, relu(shift[n]) or 0, bit for bit; every byte outside the destination
unchanged, guards included, and no input changed; a second launch bit for bit.  Split-K cases: the arrival counters back at zero after
every launch, three launches on one workspace bit for bit.  The model's call goes through ops.conv2d_nhwc(pad=(0, 0), out_hw=...) as
vae.py makes it, and gives the bits of the raw launch.

Measured on MI355X: all 150 runs pass; the worst |err| / (slope 2^-24 M) is 5.34 in fp32 (`g-wide-scalar`, pad (2, 2) on two 256-row
tiles) against K_DIRECT = 11.0, 3.00 for bf16x3 / bf16x3_w against 3.8, 3.04 for bf16x6 / bf16x6_w against 7.3, and 0.26 of the derived
bound in fp16 (`g-f16-ring-1x1-gather`, K = 4); the Downsample as the model calls it stands at 2.03 (fp32) and 0.002 (fp16).  No
kernel defect found; the table per case is in the header of wino_check.py."""
import ctypes as C

import pytest
import torch

import bf16_check as bc
import fp32_check as fc
import geom_check as gc

pytestmark = pytest.mark.gpu

G = fc.GUARD
EINVAL = -1
bits = lambda t: t.contiguous().view(torch.int32)
_raw = {}                           # case name -> the output of the raw launch, on the CPU


def _launch(c, host, ws):
    """One ofx_conv2d of an fp32 / fp16 case on fresh device copies of the guarded host buffers -> {name: the buffer afterwards}."""
    from sd_animation_optical_flow_amd import _lib
    dev = {k: v.cuda() for k, v in host.items()}
    d = fc.descriptor(c, lambda name: dev[name].data_ptr() + 4 * G * dev[name].shape[1], ws.data_ptr() if ws is not None else 0)
    p = _lib.ConvPlan()
    st = _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 0, C.byref(p))
    want = c["plan"] if len(c["plan"]) == 6 else c["plan"][:3] + (1, 1, c["plan"][3])
    assert st == 0 and p.path == 0 and (p.bm, p.bn, p.bk, p.ks, p.ksplit, p.mode) == want, (c["name"], st)
    st = _lib.lib().ofx_conv2d(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, (c["name"], st)
    return {k: v.cpu() for k, v in dev.items()}


def _output(c, host, after, off=0):
    """Everything but rows [0, M) x columns [off, off + cout) of `out` unchanged -> those, [B, Ho, Wo, cout]."""
    Ho, Wo = fc.out_hw(c)
    M, co = c["B"] * Ho * Wo, c["cout"]
    for name, before in host.items():
        a, b = bits(after[name]).clone(), bits(before)
        if name == "out":
            a[G:G + M, off:off + co] = b[G:G + M, off:off + co]
        assert torch.equal(a, b), f"{c['name']}: {name} changed outside the destination"
    return after["out"][G:G + M, off:off + co].reshape(c["B"], Ho, Wo, co)


def _held(o, got, what):
    """The bound, and the outputs with no tap inside the image bit for bit; prints the RATIO line."""
    c = o.c
    assert tuple(got.shape) == tuple(o.out.shape)
    print(f"RATIO {what} {o.ratio(got):.3f} of {o.K}")
    assert not o.violates(got), f"{what}: |error| / unit {o.ratio(got):.3f} above {o.K}"
    if bool(o.no_tap.any()):
        assert c["geom"] in gc.RINGS + ("over",)
        assert torch.equal(got.double()[o.no_tap], o.out[o.no_tap]), f"{what}: an output with no tap inside the image is not the epilogue of an exact 0"


@pytest.mark.parametrize("arith,c", [(a, c) for a, c in gc.geom_cases() if a != "bf16"], ids=gc.FP32_IDS + gc.F16_IDS)
def test_fp32_and_fp16_convolution_off_same_padding_against_float64(cuda, arith, c):
    o = gc.oracle(arith, c)
    host = fc.buffers(c, gc.f16_tensors(c) if arith == "fp16" else None)
    split = len(c["plan"]) == 6 and c["plan"][4] > 1
    ws = torch.zeros((fc.WS_BYTES,), dtype=torch.uint8, device="cuda") if c["extra"].get("ws") else None
    after = _launch(c, host, ws)
    got = _output(c, host, after, fc.out_off_of(c))
    _held(o, got, f"{c['name']} {c['plan']}")
    if arith == "fp32":
        fc.check(o.r, got, c["name"])
    for n in range(2 if split else 1):                                   # split-K: on the workspace as the kernel left it
        if split:
            assert not bool(ws[:65536].any()), f"{c['name']}: arrival counters not back at zero"
        again = _launch(c, host, ws)
        assert all(torch.equal(bits(after[k]), bits(again[k])) for k in after), f"{c['name']}: launch {n + 2} differs"
    if split:
        assert not bool(ws[:65536].any()) and bool(ws[65536:].any())     # the partial tiles went through the workspace
    _raw[c["name"]] = got


def _launch_bf16(c, prec, host):
    from sd_animation_optical_flow_amd import ops
    dev = {k: v.cuda() for k, v in host.items()}
    ops.conv2d_desc(bc.descriptor(c, prec, lambda name: dev[name].data_ptr()))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dev.items()}


@pytest.mark.parametrize("precision", list(bc.PRECISIONS))
@pytest.mark.parametrize("c", gc.BF16, ids=gc.BF16_IDS)
def test_split_bf16_convolution_off_same_padding_against_the_products_it_forms(cuda, c, precision):
    from sd_animation_optical_flow_amd import _lib
    prec = bc.PRECISIONS[precision]
    o = gc.oracle("bf16", c, prec)
    p = _lib.ConvPlan()
    assert _lib.lib().ofx_conv2d_plan(C.byref(bc.descriptor(c, prec, lambda name: 0x10000)), 0, 0, C.byref(p)) == 0
    assert (p.path, p.prec, p.bm, p.bn, p.bk, p.mode) == (0, prec, *c["plan"][prec][:3], gc.GATHER)
    host = bc.buffers(c, prec)
    after = _launch_bf16(c, prec, host)
    got = _output(c, host, after)
    _held(o, got, f"{c['name']} {precision} {bc.signature(c, prec)}")
    bc.check(o.r, got, bc.K_of(prec), f"{c['name']} {precision}")
    again = _launch_bf16(c, prec, host)
    assert all(torch.equal(bits(after[k]), bits(again[k])) for k in after), f"{c['name']}: a repeat differs"
    _raw[(c["name"], prec)] = got
    if precision.endswith("_w") and bc.same_plan(c) and (c["name"], prec - 1) in _raw:   # the pre-split format: the same bits
        assert torch.equal(bits(got), bits(_raw[(c["name"], prec - 1)])), f"{c['name']}: {precision} differs from {precision[:-2]}"


@pytest.mark.parametrize("arith,name,precision", [("fp32", "g-model-fp32", "fp32"), ("fp16", "g-f16-model-fp16", "fp16")])
def test_the_downsample_as_the_model_calls_it(cuda, arith, name, precision):
    """ops.conv2d_nhwc(x, w, 3, 3, cout, stride=2, shift=bias, pad=(0, 0), out_hw=(H / 2, W / 2), precision=...), the call of
    vae.py's encoder.down.N.downsample.conv: inside the bound, and the bits of the raw guarded launch of the same descriptor."""
    from sd_animation_optical_flow_amd import ops
    c = next(x for a, x in gc.geom_cases() if x["name"] == name)
    o = gc.oracle(arith, c)
    t = gc.f16_tensors(c) if arith == "fp16" else fc.inputs(name)
    x = t["x"].cuda()
    got = ops.conv2d_nhwc(x, ops.pack_conv_weight(t["w"]).cuda(), 3, 3, c["cout"], stride=2, shift=t["shift"].cuda(), pad=(0, 0),
                          out_hw=(x.shape[1] // 2, x.shape[2] // 2), precision=precision).cpu()
    _held(o, got, f"{name} through ops.conv2d_nhwc")
    if name not in _raw:
        host = fc.buffers(c, t if arith == "fp16" else None)
        _raw[name] = _output(c, host, _launch(c, host, None))
    assert torch.equal(bits(got), bits(_raw[name]))


def test_a_negative_pad_is_rejected_on_the_device_with_nothing_written(cuda):
    from sd_animation_optical_flow_amd import _lib, ops
    c = fc.case("g-down-64x64-scalar")
    host = fc.buffers(c)
    dev = {k: v.cuda() for k, v in host.items()}
    for pad in ((-1, 0), (0, -1)):
        d = fc.descriptor(c, lambda name: dev[name].data_ptr() + 4 * G * dev[name].shape[1])
        d.padH, d.padW = pad
        assert _lib.lib().ofx_conv2d(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == EINVAL
        out = torch.full((c["B"], *fc.out_hw(c), c["cout"]), 7.25, device="cuda")
        with pytest.raises(RuntimeError, match="pad must be >= 0"):
            ops.conv2d_nhwc(dev["in0"][G:-G].view(c["B"], c["H"], c["W"], c["c0"]), dev["w"][G:-G], 3, 3, c["cout"], stride=2, pad=pad,
                            out_hw=fc.out_hw(c), out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.25).all())
    assert all(torch.equal(bits(dev[k].cpu()), bits(host[k])) for k in host)
