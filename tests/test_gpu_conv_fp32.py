"""The fp32 direct convolutions with the plain epilogue on the device: every case of tests/fp32_check.py as a raw ConvDesc launch
through ofx_conv2d (no Winograd operand: nothing leaves the direct kernels).  The oracle, the case table (with the plan every case
reaches and its coverage of kTiles, held on the CPU by test_fp32_check_host.py) and the bound are fp32_check.py's.

Per case: the plan, asked again of the device build; every buffer the descriptor names -- in0, in1, w, scale, shift, res, addend,
nmean / nrstd, out -- between GUARD rows of NaN, the addend's columns past Cout NaN, the output NaN over its full ldo; the result
inside |out - ref| <= slope K_DIRECT 2^-24 M + extra (the worst ratio is printed as a RATIO line; the table of them is in the header
of wino_check.py); every byte outside columns [out_off, out_off + Cout) of rows [0, M) of `out` unchanged bit for bit, guards
included, and no input changed; a second launch bit for bit.  Split-K cases run on one workspace that is zeroed once: its 64 KiB of
arrival counters read zero after every launch and three launches agree bit for bit (the reduction order is fixed: the last arriver
sums the partial tiles in split order); that the split ran is the plan's ksplit > 1, which sizes the grid.

Measured on MI355X: all 94 cases pass; the worst |err| / (slope 2^-24 M) is 4.51 (`p-256x64-patch-over`, 3x3 on overhanging 16x16
patches) against K_DIRECT = 11.0; split-K at most 2.65, paired pipelines 3.31, norm on load 3.83, tanh / sigmoid 2.17.  No kernel
defect found; the table per case is in the header of wino_check.py."""
import ctypes as C

import pytest
import torch

import fp32_check as fc

pytestmark = pytest.mark.gpu

G = fc.GUARD
EINVAL = -1
bits = lambda t: t.contiguous().view(torch.int32)


def _launch(c, host, ws, expect=0, **override):
    """One ofx_conv2d of case c on fresh device copies of the guarded host buffers -> {name: the buffer afterwards, on the CPU}."""
    from sd_animation_optical_flow_amd import _lib
    dev = {k: v.cuda() for k, v in host.items()}
    d = fc.descriptor(c, lambda name: dev[name].data_ptr() + 4 * G * dev[name].shape[1], ws.data_ptr() if ws is not None else 0)
    for k, v in override.items():
        setattr(d, k, v)
    p = _lib.ConvPlan()
    st = _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 0, C.byref(p))
    if expect == 0:
        assert st == 0 and p.path == 0 and (p.bm, p.bn, p.bk, p.ks, p.ksplit, p.mode) == c["plan"], (c["name"], st)
    st = _lib.lib().ofx_conv2d(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == expect, (c["name"], st)
    return {k: v.cpu() for k, v in dev.items()}


def _output(c, host, after):
    """Everything but rows [0, M) x columns [out_off, out_off + cout) of `out` unchanged -> those, [B, Ho, Wo, cout]."""
    Ho, Wo = fc.out_hw(c)
    M, co, off = fc.rows_of(c), c["cout"], fc.out_off_of(c)
    for name, before in host.items():
        a, b = bits(after[name]).clone(), bits(before)
        if name == "out":
            a[G:G + M, off:off + co] = b[G:G + M, off:off + co]
        assert torch.equal(a, b), f"{c['name']}: {name} changed outside the destination"
    return after["out"][G:G + M, off:off + co].reshape(c["B"], Ho, Wo, co)


@pytest.mark.parametrize("c", fc.CASES, ids=fc.IDS)
def test_fp32_convolution_against_float64(cuda, c):
    r = fc.reference(c["name"])
    host = fc.buffers(c)
    split = c["plan"][4] > 1
    ws = torch.zeros((fc.WS_BYTES,), dtype=torch.uint8, device="cuda") if c["extra"].get("ws") else None
    after = _launch(c, host, ws)
    got = _output(c, host, after)
    assert tuple(got.shape) == tuple(r.out.shape)
    print(f"RATIO {c['name']} {c['plan']} {fc.ratio(r, got):.3f}")
    fc.check(r, got, c["name"])
    for n in range(2 if split else 1):                                   # split-K: on the workspace as the kernel left it
        if split:
            assert not bool(ws[:65536].any()), f"{c['name']}: arrival counters not back at zero"
        again = _launch(c, host, ws)
        assert all(torch.equal(bits(after[k]), bits(again[k])) for k in after), f"{c['name']}: launch {n + 2} differs"
    if split:
        assert not bool(ws[:65536].any())
        assert bool(ws[65536:].any())                                    # the partial tiles went through the workspace


def test_the_norm_on_load_with_a_transcendental_activation_is_rejected_with_nothing_written(cuda):
    c = fc.case("n-128x128-patch")
    host = fc.buffers(c)
    after = _launch(c, host, None, expect=EINVAL, act=fc.ACTS["tanh"])
    assert all(torch.equal(bits(after[k]), bits(host[k])) for k in host)
