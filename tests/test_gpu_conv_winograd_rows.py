"""The F(2x2,3x3) kernel's operand path (conv_wino.hip): each wave forms its own row of B^T d B in registers from two rows of the
halo, so a wrong row pair, sign or column would be a wrong pairing of whole input pixels with weights.

Impulse inputs make that an O(1) error: one non-zero pixel, in one channel, per image.  Every pixel of a 16x32 map (2 x 2
patches) takes its turn, so every tile -- on all four image borders, on the patch seams and inside -- sees the pixel at each of
the 16 positions of its 4x4 window, and with it every wave's two rows and four columns.  The channels cover the four k-groups of
a 16-channel slab (channels 4 g .. 4 g + 3 of it, which feed different lanes and MFMA steps) and all three slabs of the layer,
that is both halo buffers.  Reference: float64 F.conv2d, as in the other Winograd tests.

The six <NORM, RES, STATS> variants then run unit-normal data under the bound the existing Winograd tests use, 2e-5 absolute.
GPU tests are marked -m gpu.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def nhwc(x):  # NCHW cpu -> NHWC cuda
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):  # NHWC cuda -> NCHW cpu
    return x.permute(0, 3, 1, 2).contiguous().cpu()


IMP_H, IMP_W, IMP_CIN, IMP_COUT = 16, 32, 48, 64
# Bound of the impulse cases, from the arithmetic alone.  The pixel is 1.0 and |w| <= 1, so the transformed input is exactly 0 or
# +-1 and every product is exactly +-U, U = fl(G g G^T), |U| <= 2.25 (G's rows sum to at most 1.5 in magnitude) with a rounding
# error of at most 2^-24 * 2.25.  An output is A^T (.) A over the 16 products: 9 terms, 8 additions, each addition rounding a
# partial sum of at most 9 * 2.25.  |error| <= 2^-24 (9 * 2.25 + 8 * 9 * 2.25) = 1.1e-5 < 2e-5, the bound of the random cases too.
IMP_BOUND = 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("chan", [1, 6, 11, 12, 16 + 5, 32 + 10], ids=lambda c: f"slab{c // 16}-kgroup{c % 16 // 4}-ch{c}")
def test_one_pixel_at_every_window_position_of_every_tile(cuda, chan):
    ops = _ops()
    g = torch.Generator().manual_seed(100 + chan)
    w = torch.rand((IMP_COUT, IMP_CIN, 3, 3), generator=g) * 2.0 - 1.0
    B = IMP_H * IMP_W
    x = torch.zeros((B, IMP_CIN, IMP_H, IMP_W))
    b = torch.arange(B)
    x[b, chan, b // IMP_W, b % IMP_W] = 1.0                      # image b: pixel (b / W, b % W)
    ref = F.conv2d(x[:, chan:chan + 1].double(), w[:, chan:chan + 1].double(), padding=1)
    got = nchw(ops.conv2d_nhwc(nhwc(x), ops.pack_conv_weight(w).cuda(), 3, 3, IMP_COUT, wino_w=ops.wino_conv_weight(w).cuda(),
                               tile=ops.TILE_WINOGRAD)).double()
    err = (got - ref).abs()
    per_pixel = err.amax(dim=(1, 2, 3)).view(IMP_H, IMP_W)       # by the position of the input pixel
    worst = int(per_pixel.argmax())
    print(f"channel {chan}: max |err| {float(err.max()):.3g} (pixel {worst // IMP_W}, {worst % IMP_W}); "
          f"smallest response {float(ref.abs()[ref != 0].min()):.3g}")
    assert float(err.max()) <= IMP_BOUND, (chan, float(err.max()), (worst // IMP_W, worst % IMP_W))
    # outside the pixel's 3x3 reach the tiles that do not hold it in their window see zeros only
    far = torch.ones((B, 1, IMP_H, IMP_W), dtype=torch.bool)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            yy, xx = b // IMP_W + dy, b % IMP_W + dx
            ok = (yy >= 0) & (yy < IMP_H) & (xx >= 0) & (xx < IMP_W)
            far[b[ok], 0, yy[ok], xx[ok]] = False
    assert float(got.abs()[far.expand_as(got)].max()) == 0.0


def _weights(ci, co, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((co, ci, 3, 3), generator=g) / np.sqrt(ci * 9)
    scale = 0.5 + torch.rand((co,), generator=g)
    shift = torch.randn((co,), generator=g) * 0.1
    return g, w, scale, shift


VARIANTS = [(False, False, False), (False, False, True), (False, True, False), (True, False, False), (True, False, True),
            (True, True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("c,H,W", [(64, 32, 64), (96, 24, 48), (128, 16, 32)])
@pytest.mark.parametrize("norm,res,stats", VARIANTS)
def test_unit_normal_data_through_the_six_variants(cuda, c, H, W, norm, res, stats):
    """<NORM, RES, STATS> as ofx_conv_wino_launch selects them: fused relu(norm(.)) on the operand, the residual merge, the epilogue
    statistics (raw outputs: identity activation).  |out - float64| <= 2e-5 everywhere, borders included."""
    ops = _ops()
    B = 2
    g, w, scale, shift = _weights(c, c, 7 * c + H + 4 * norm + 2 * res + stats)
    x = torch.randn((B, c, H, W), generator=g)
    xin = x.double()
    kw = dict(scale=scale.cuda(), shift=shift.cuda())
    if norm:   # the reference normalises with the float32 mean and rstd the kernel is given
        mean = x.double().mean(dim=(2, 3)).float()
        rstd = (1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)).float()
        xin = torch.relu((xin - mean.double().view(B, c, 1, 1)) * rstd.double().view(B, c, 1, 1))
        kw.update(nmean=mean.cuda(), nrstd=rstd.cuda())
    ref = F.conv2d(xin, w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if res:
        r = torch.randn((B, c, H, W), generator=g)
        ref = torch.relu(torch.relu(ref) + r.double())
        kw.update(act="relu", res=nhwc(r))
    wp, u = ops.pack_conv_weight(w).cuda(), ops.wino_conv_weight(w).cuda()
    if stats:
        rows = (H // 8) * (W // 16)
        part = torch.full((B * rows * c * 2,), float("nan"), device="cuda")
        out, got_rows = ops.conv2d_nhwc(nhwc(x), wp, 3, 3, c, wino_w=u, tile=ops.TILE_WINOGRAD, stats_part=part, **kw)
        assert got_rows == rows
        o = nchw(out).double().view(B, c, H // 8, 8, W // 16, 16)   # each row is the patch's own sums of the stored values
        ps = part.double().cpu().view(B, H // 8, W // 16, c, 2)
        assert torch.allclose(ps[..., 0], o.sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3)
        assert torch.allclose(ps[..., 1], (o * o).sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3)
    else:
        out = ops.conv2d_nhwc(nhwc(x), wp, 3, 3, c, wino_w=u, tile=ops.TILE_WINOGRAD, **kw)
    got = nchw(out).double()
    for name, sl in (("all", np.s_[:]), ("top", np.s_[:, :, 0]), ("bottom", np.s_[:, :, -1]), ("left", np.s_[:, :, :, 0]),
                     ("right", np.s_[:, :, :, -1])):
        e = (got[sl] - ref[sl]).abs().max().item()
        print(f"c {c} norm {norm} res {res} stats {stats} {name}: max |err| {e:.3g}")
        assert e < 2e-5, (name, e)
