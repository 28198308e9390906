"""The F(2x2,3x3) slab loop's prefetches at the slab counts where their clamps act (conv_wino.hip, wino3x3_slabs).

The weights run one 8-channel step ahead and the last step reloads itself; the halo is issued two slabs ahead, the first two
before the loop, and the last slabs re-issue the last one.  With one to four slabs (Cin = 16, 32, 48, 64) the loop runs from
"prologue only" to "every clamp and both halo buffers twice"; a clamp that is off by one pairs a slab with the wrong weights or
the wrong halo, an O(1) error.  Cout = 64 and 128 (one and two output blocks per patch), a map of one patch (8x16: every pixel
on a border) and of 2 x 2 patches, batch 1 and 2, through all six <NORM, RES, STATS> variants, forced onto the fused kernel as
in test_gpu_conv_winograd_rows.py.

Reference: float64, with the operand-scaled bound of wino_check.py at its K for this kernel (K_F23).  The magnitude M takes the
normalised operand (NORM) and the residual (RES) as the kernel's arithmetic sees them.  Every launch is repeated and must
reproduce itself bit for bit.  GPU tests are marked -m gpu.
"""
import itertools

import pytest
import torch

import wino_check as wc

VARIANTS = [(False, False, False), (False, False, True), (False, True, False), (True, False, False), (True, False, True),
            (True, True, False)]
SHAPES = list(itertools.product([64, 128], [(8, 16), (16, 32)], [1, 2]))   # Cout, map, batch


def nhwc(x):  # NCHW cpu -> NHWC cuda
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):  # NHWC cuda -> NCHW cpu
    return x.permute(0, 3, 1, 2).contiguous().cpu()


def _case(ops, cin, cout, H, W, B, norm, res, stats):
    g = torch.Generator().manual_seed(((cin * 131 + cout) * 7 + H + B) * 8 + 4 * norm + 2 * res + stats)
    w = torch.randn((cout, cin, 3, 3), generator=g) / (cin * 9) ** 0.5
    scale = 0.5 + torch.rand((cout,), generator=g)
    shift = torch.randn((cout,), generator=g) * 0.1
    x = torch.randn((B, cin, H, W), generator=g)
    xin = x.double()
    kw = dict(scale=scale.cuda(), shift=shift.cuda())
    if norm:   # the reference normalises with the float32 mean and rstd the kernel is given
        mean = x.double().mean(dim=(2, 3)).float()
        rstd = (1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)).float()
        xin = torch.relu((xin - mean.double().view(B, cin, 1, 1)) * rstd.double().view(B, cin, 1, 1))
        kw.update(nmean=mean.cuda(), nrstd=rstd.cuda())
    ref, mag = wc.reference(xin, w, 3, 3, scale=scale, shift=shift, relu=res)
    if res:
        r = torch.randn((B, cout, H, W), generator=g)
        ref, mag = torch.relu(ref + r.double()), mag + r.double().abs()
        kw.update(act="relu", res=nhwc(r))
    xd, wp, u = nhwc(x), ops.pack_conv_weight(w).cuda(), ops.wino_conv_weight(w).cuda()
    rows = (H // 8) * (W // 16)

    def launch():
        if not stats:
            return ops.conv2d_nhwc(xd, wp, 3, 3, cout, wino_w=u, tile=ops.TILE_WINOGRAD, **kw), None
        part = torch.full((B * rows * cout * 2,), float("nan"), device="cuda")
        out, got_rows = ops.conv2d_nhwc(xd, wp, 3, 3, cout, wino_w=u, tile=ops.TILE_WINOGRAD, stats_part=part, **kw)
        assert got_rows == rows
        return out, part

    what = f"cin {cin} cout {cout} map {H}x{W} batch {B} norm {norm} res {res} stats {stats}"
    out, part = launch()
    ratio = wc.check(nchw(out), ref, mag, wc.K_F23, what)
    if stats:   # each row is the patch's own sums of the stored values
        o = nchw(out).double().view(B, cout, H // 8, 8, W // 16, 16)
        ps = part.double().cpu().view(B, H // 8, W // 16, cout, 2)
        assert torch.allclose(ps[..., 0], o.sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3), what
        assert torch.allclose(ps[..., 1], (o * o).sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3), what
    out2, part2 = launch()
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), what
    if stats:
        assert torch.equal(part.view(torch.int32), part2.view(torch.int32)), what
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("cin", [16, 32, 48, 64], ids=lambda c: f"slabs{c // 16}")
@pytest.mark.parametrize("norm,res,stats", VARIANTS)
def test_one_to_four_slabs_through_the_six_variants(cuda, cin, norm, res, stats):
    from sd_animation_optical_flow_amd import ops
    worst = 0.0
    for cout, (H, W), B in SHAPES:
        worst = max(worst, _case(ops, cin, cout, H, W, B, norm, res, stats))
    print(f"cin {cin} norm {norm} res {res} stats {stats}: worst |err| / (2^-24 M) {worst:.3g} (K {wc.K_F23})")
