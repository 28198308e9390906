"""The F(4x4,3x3) kernels' epilogue (conv_wino44_body.inl): a lane stores four adjacent channels of a pixel, as 16 bytes where the
destination allows it (base pointer, channel offset and ldo aligned: the vector path) and channel by channel otherwise (the
fallback path, and on either path a quad that straddles Cout).

Every case is forced with TILE_WINOGRAD4 (wino44_check.make / run; the launches that need a destination, a residual or
statistics run() cannot express go through _launch, the same call) and checked elementwise against float64 with wino_check's
bound at K_F43, the constant of wino44_check; no tolerance of this file's own.  Shapes: one to four 16x32 patches, Cin 16 - 48.
The statistics' bounds are those of test_gpu_conv_winograd44_fused.py.  GPU tests are marked -m gpu.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino44_check as w4  # noqa: E402
import wino_check as wc  # noqa: E402

NAN = float("nan")


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


_CACHE = {}


def _case(case):
    """make() once per case (tensors and float64 reference, never modified) with its device operands"""
    if case[0] not in _CACHE:
        c = w4.make(case, 500 + sum(map(ord, case[0])))
        _CACHE[case[0]] = (c, w4.operands(_ops(), c["w"]))
    return _CACHE[case[0]]


def _launch(ops, c, opw, ld=None, off=0, skew=0, res=None, part=None):
    """The launch of w4.run into a NaN-filled destination [B, H, W, ld] whose base pointer is `skew` floats off a 16-byte boundary,
    channels [off, off + co); -> (NCHW cpu result, the flat destination with its `skew` leading floats, its [B, H, W, ld] view,
    rows of statistics or None)."""
    wp, u2, u4 = opw
    B, H, W = c["shape"]
    co = c["co"]
    ld = co if ld is None else ld
    kw = dict(act="relu" if c["relu"] else None, wino_w=u2, wino4_w=u4, tile=ops.TILE_WINOGRAD4)
    if c["scale"] is not None:
        kw.update(scale=c["scale"].cuda(), shift=c["shift"].cuda())
    if c["x1"] is not None:
        kw["x2"] = w4.nhwc(c["x1"])
    if res is not None:
        kw["res"] = res
    if part is not None:
        kw["stats_part"] = part
    flat = torch.full((skew + B * H * W * ld,), NAN, device="cuda")
    dst = flat[skew:].view(B, H, W, ld)
    assert dst.data_ptr() % 16 == 4 * skew % 16
    out = ops.conv2d_nhwc(w4.nhwc(c["x0"]), wp, 3, 3, co, out=dst, out_off=off, **kw)
    rows = out[1] if part is not None else None
    return w4.nchw(dst[..., off:off + co]), flat, dst, rows


def _untouched(flat, dst, skew, off, co):
    assert bool(torch.isnan(flat[:skew]).all()), "written before the destination"
    assert bool(torch.isnan(dst[..., :off]).all()) and bool(torch.isnan(dst[..., off + co:]).all()), "neighbours written"
    assert not bool(torch.isnan(dst[..., off:off + co]).any())


def _bound(got, c, what):
    ratio = wc.worst_ratio(got, c["ref"], c["mag"])
    print(f"{what}: worst ratio {ratio:.3g} (K_F43 = {w4.K_F43})")
    wc.check(got, c["ref"], c["mag"], w4.K_F43, what)


# (name, B, H, W, (c0, c1), Cout, distribution, relu, scale/shift, (ldo, offset) or None): the rows of wino44_check.CASES
FULL = [
    ("full_co64", 1, 16, 32, (16, 0), 64, "normal", True, True, None),
    ("full_co192", 1, 16, 64, (32, 0), 192, "relu", False, True, None),
]
PARTIAL = [
    # the engine's conv: 126 channels into hx, the two flow channels right behind
    ("conv_126_in_256", 1, 16, 32, (32, 16), 126, "relu", True, True, (256, 128)),
    ("partial_co33", 1, 16, 32, (16, 0), 33, "normal", True, False, (36, 0)),
    ("partial_co65", 1, 16, 32, (16, 0), 65, "tanh", False, True, (68, 0)),
    # the second 64-block's second half is empty, and its waves store nothing
    ("partial_co96", 1, 16, 32, (48, 0), 96, "normal", True, True, None),
]
# (case, skew of the base pointer in floats)
FALLBACK = [
    (("fallback_off33_ld192", 1, 16, 32, (16, 0), 126, "tanh", True, True, (192, 33)), 0),
    (("fallback_ld190", 1, 16, 32, (16, 0), 126, "normal", False, True, (190, 32)), 0),
    (("fallback_base_skew", 1, 16, 32, (32, 0), 64, "relu", True, True, (64, 0)), 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FULL + PARTIAL, ids=[c[0] for c in FULL + PARTIAL])
def test_vector_path_against_float64(cuda, case):
    ops = _ops()
    c, opw = _case(case)
    got, dst = w4.run(ops, c, ops.TILE_WINOGRAD4, opw)
    _bound(got, c, case[0])
    ld, off = c["dst"] if c["dst"] else (c["co"], 0)
    assert ld % 4 == 0 and off % 4 == 0   # the vector path's conditions (torch's allocations are 16-byte aligned)
    if dst is not None:
        assert dst.data_ptr() % 16 == 0
        _untouched(dst.view(-1), dst, 0, off, c["co"])
    again, _ = w4.run(ops, c, ops.TILE_WINOGRAD4, opw)
    assert torch.equal(got, again), "not bit-identical on a second call"


@pytest.mark.gpu
@pytest.mark.parametrize("case,skew", FALLBACK, ids=[c[0][0] for c in FALLBACK])
def test_fallback_path_against_float64(cuda, case, skew):
    ops = _ops()
    c, opw = _case(case)
    ld, off = c["dst"]
    assert ld % 4 or off % 4 or skew % 4   # not the vector path
    if skew == 0:   # run()'s own destination
        got, dst = w4.run(ops, c, ops.TILE_WINOGRAD4, opw)
        flat = dst.view(-1)
    else:
        got, flat, dst, _ = _launch(ops, c, opw, ld, off, skew)
    _bound(got, c, case[0])
    _untouched(flat, dst, skew, off, c["co"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [FULL[0], PARTIAL[0], PARTIAL[3]], ids=[FULL[0][0], PARTIAL[0][0], PARTIAL[3][0]])
def test_the_two_paths_agree_to_the_bit(cuda, case):
    """The same convolution into an aligned destination, into one at an odd channel offset and into two whose base pointers are
    one and two floats off a 16-byte boundary"""
    ops = _ops()
    c, opw = _case(case)
    co = c["co"]
    ld = 256
    vec, flat, dst, _ = _launch(ops, c, opw, ld, 128)
    _untouched(flat, dst, 0, 128, co)
    _bound(vec, c, case[0])
    for off, skew in ((129, 0), (128, 1), (128, 2)):
        got, flat, dst, _ = _launch(ops, c, opw, ld, off, skew)
        _untouched(flat, dst, skew, off, co)
        assert torch.equal(vec, got), (off, skew)


@pytest.mark.gpu
@pytest.mark.parametrize("co", [64, 96])
def test_residual_merge_on_both_paths(cuda, co):
    """RES with ldres > Cout: relu(y + res) after the activation; a misaligned destination, a misaligned residual and a residual
    row that is no multiple of four floats each take the fallback path, to the same bits."""
    ops = _ops()
    case = (f"res_co{co}", 2, 16, 32, (32, 0), co, "normal", True, True, None)
    c, opw = _case(case)
    B, H, W = c["shape"]
    g = torch.Generator().manual_seed(77 + co)
    res = torch.randn((B, co, H, W), generator=g)
    ref = torch.relu(c["ref"] + res.double())
    cr = dict(c, ref=ref, mag=c["mag"] + res.double().abs())

    def residual(ldres, skew):
        flat = torch.full((skew + B * H * W * ldres,), NAN, device="cuda")
        r = flat[skew:].view(B, H, W, ldres)
        r[..., :co] = w4.nhwc(res)
        return r

    vec, flat, dst, _ = _launch(ops, c, opw, co + 4, 0, res=residual(co + 8, 0))
    _untouched(flat, dst, 0, 0, co)
    _bound(vec, cr, case[0])
    for (ld, off, skew), (ldres, rskew) in (((co + 4, 1, 0), (co + 8, 0)), ((co + 4, 0, 0), (co + 8, 1)), ((co + 4, 0, 0), (co + 6, 0))):
        got, flat, dst, _ = _launch(ops, c, opw, ld, off, skew, res=residual(ldres, rskew))
        _untouched(flat, dst, skew, off, co)
        assert torch.equal(vec, got), (ld, off, skew, ldres, rskew)


@pytest.mark.gpu
@pytest.mark.parametrize("co", [64, 96])
def test_statistics_on_both_paths(cuda, co):
    ops = _ops()
    case = (f"stats_co{co}", 2, 32, 64, (16, 0), co, "normal", False, True, None)
    c, opw = _case(case)
    B, H, W = c["shape"]
    rows = (H // 16) * (W // 32)
    need = B * rows * co * 2
    outs, parts = [], []
    for off, skew in ((0, 0), (0, 0), (1, 0), (0, 3)):   # vector, its repeat, two fallbacks
        part = torch.full((need + 256,), NAN, device="cuda")
        got, flat, dst, got_rows = _launch(ops, c, opw, co + 4, off, skew, part=part)
        assert got_rows == rows
        _untouched(flat, dst, skew, off, co)
        assert bool(torch.isfinite(part[:need]).all()) and bool(torch.isnan(part[need:]).all())
        outs.append(got)
        parts.append(part[:need].clone())
    _bound(outs[0], c, case[0])
    assert torch.equal(parts[0], parts[1]), "partials differ on a repeat"
    for k in (1, 2, 3):
        assert torch.equal(outs[0], outs[k]), k
    # each row is its patch's own sums: against float64 sums of the kernel's output over that 16x32 patch, on either path
    o = outs[0].double().view(B, co, H // 16, 16, W // 32, 32)
    for part in (parts[0], parts[2], parts[3]):
        ps = part.double().cpu().view(B, H // 16, W // 32, co, 2)
        assert torch.allclose(ps[..., 0], o.sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3)
        assert torch.allclose(ps[..., 1], (o * o).sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("skew", [0, 1], ids=["vector", "fallback"])
def test_borders_and_the_xcd_remap(cuda, skew):
    """Two images of 2x2 patches with ReLU and scale / shift: every border, the seams between patches, eight workgroups"""
    ops = _ops()
    case = ("borders_2x2x2", 2, 32, 64, (32, 0), 64, "relu", True, True, None)
    c, opw = _case(case)
    got, flat, dst, _ = _launch(ops, c, opw, 64, 0, skew)
    _untouched(flat, dst, skew, 0, 64)
    _bound(got, c, case[0])
    for name, sl in (("top", (..., 0, slice(None))), ("bottom", (..., -1, slice(None))), ("left", (..., 0)), ("right", (..., -1))):
        wc.check(got[sl], c["ref"][sl], c["mag"][sl], w4.K_F43, f"{case[0]} {name}")
