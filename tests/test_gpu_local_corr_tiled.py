"""-m gpu: the LDS-tiled volume-free lookup (csrc/corr_local_tiled.hip, `ops.local_corr_rows`) against a float64 evaluation of
AlternateCorrBlock (`oracle.raft_oracle.local_corr_level` on double inputs, level by level).

Bound: max abs 1e-4 on unit-variance features with the engine's 1/sqrt(C) scale -- the bound test_local_corr_* hold the per-pixel
kernel to.  fp32 products of C <= 256 unit-variance terms, scaled to unit variance, carry ~C * 2^-24 / sqrt(C) ~ 1e-6 of rounding:
the bound leaves two orders of margin and catches any wrong tap, weight or channel (those are O(1)).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import raft_oracle as RO

NETS = {"basic": (256, 4), "small": (128, 3)}     # (C, radius)


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def _maps(seed, n1, n2, h, w, C, levels):
    g = torch.Generator().manual_seed(seed)
    f1 = torch.randn((n1, h, w, C), generator=g)
    f2 = torch.randn((n2, h, w, C), generator=g)
    lv = [f2.cuda()]
    for _ in range(1, levels):
        lv.append(_ops().avgpool2_nhwc(lv[-1]))
    return f1, f2, lv, g


def _grid(B, h, w):
    return torch.stack(torch.meshgrid(torch.arange(w).float(), torch.arange(h).float(), indexing="xy"), -1)[None].repeat(B, 1, 1, 1)


def _ref(f1, f2, coords, levels, r, idx1=None, idx2=None):
    """float64 rows [B*h*w, levels*(2r+1)^2]: AlternateCorrBlock.__call__ (corr.py:74-91) level by level on the oracle's
    `local_corr_level`.  (`RO.alternate_corr_lookup` is this loop, but pools once more after the last level and so refuses maps whose
    last level is one pixel wide -- the cases this file is about.)"""
    a = (f1 if idx1 is None else f1[idx1]).double()
    b = (f2 if idx2 is None else f2[idx2]).double()
    B, h, w, _ = coords.shape
    a, b = a[:B].contiguous(), b[:B].permute(0, 3, 1, 2)
    outs = []
    for l in range(levels):
        c = (coords.double() / 2 ** l).reshape(B, 1, h, w, 2)
        outs.append(RO.local_corr_level(a, b.permute(0, 2, 3, 1).contiguous(), c, r).squeeze(1))       # [B, (2r+1)^2, h, w]
        if l + 1 < levels:
            b = F.avg_pool2d(b, 2, stride=2)
    out = torch.stack(outs, 1).reshape(B, -1, h, w) / a.shape[-1] ** 0.5
    return out.permute(0, 2, 3, 1).reshape(B * h * w, -1)


def _check(tag, got, ref, bound=1e-4):
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"{tag}: max abs err {err:.3e} (bound {bound:.0e}), ref max {ref.abs().max().item():.2f}")
    assert err < bound, tag


@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("shape", [(2, 16, 24), (1, 13, 19), (2, 8, 8), (1, 9, 30)])
def test_coherent_coordinates_against_float64(cuda, net, shape):
    """Whole and ragged tile grids; 8x8 maps pool down to 1x1 at level 3.  Smooth sub-pixel motion: every tile stages its box."""
    ops = _ops()
    C, r = NETS[net]
    B, h, w = shape
    f1, f2, lv, g = _maps(3 + h, B, B, h, w, C, 4)
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    flow = torch.stack([1.7 + 0.8 * torch.sin(yy / 5.0), -2.3 + 0.6 * torch.cos(xx / 7.0)], -1)
    coords = (_grid(B, h, w) + flow[None] + torch.rand((B, h, w, 2), generator=g) * 0.5).contiguous()
    rows = ops.local_corr_rows(f1.cuda(), lv, coords.cuda(), r)
    assert tuple(rows.shape) == (B * h * w, 4 * (2 * r + 1) ** 2)
    _check(f"{net} {shape} coherent", rows, _ref(f1, f2, coords, 4, r))


@pytest.mark.parametrize("net", sorted(NETS))
def test_random_and_outside_coordinates_against_float64(cuda, net):
    """Uniformly random coordinates over (and a margin around) a 40x48 map: every level-0 tile's box exceeds the LDS budget and takes
    the per-pixel fallback; then coordinates far outside the map (every tap is zero) and straddling its border."""
    ops = _ops()
    C, r = NETS[net]
    B, h, w = 1, 40, 48
    f1, f2, lv, g = _maps(11, B, B, h, w, C, 4)
    rnd = torch.rand((B, h, w, 2), generator=g) * torch.tensor([w + 12.0, h + 12.0]) - 6.0
    _check(f"{net} random", ops.local_corr_rows(f1.cuda(), lv, rnd.contiguous().cuda(), r), _ref(f1, f2, rnd, 4, r))
    far = _grid(B, h, w) + torch.tensor([500.0, -300.0])
    out = ops.local_corr_rows(f1.cuda(), lv, far.contiguous().cuda(), r)
    assert float(out.abs().max()) == 0.0
    edge = (_grid(B, h, w) + torch.tensor([-(r + 2.5), h - 3.25])).contiguous()      # windows hang over the left and bottom borders
    _check(f"{net} border", ops.local_corr_rows(f1.cuda(), lv, edge.cuda(), r), _ref(f1, f2, edge, 4, r))


@pytest.mark.parametrize("net", sorted(NETS))
def test_non_finite_and_huge_coordinates_follow_the_per_pixel_kernel(cuda, net):
    """NaN, +-inf and 1e8 coordinates: those pixels come out exactly as the per-pixel kernel writes them (zeros), the other pixels of
    the same tiles stay within the float64 bound."""
    ops = _ops()
    C, r = NETS[net]
    B, h, w = 1, 16, 24
    f1, f2, lv, g = _maps(17, B, B, h, w, C, 4)
    coords = (_grid(B, h, w) + (torch.rand((B, h, w, 2), generator=g) - 0.5) * 3).contiguous()
    clean = coords.clone()
    bad = [(0, 0, float("nan"), 1.0), (3, 5, 2.0, float("inf")), (7, 7, float("-inf"), float("nan")), (8, 8, 1e8, 4.0), (15, 23, 3.0, -1e8),
           (9, 17, 3.0e7, 3.0e7)]
    mask = torch.zeros((h, w), dtype=torch.bool)
    for y, x, cx, cy in bad:
        coords[0, y, x] = torch.tensor([cx, cy])
        clean[0, y, x] = torch.tensor([-1000.0, -1000.0])
        mask[y, x] = True
    new = ops.local_corr_rows(f1.cuda(), lv, coords.cuda(), r).cpu()
    old = ops.local_corr_rows(f1.cuda(), lv, coords.cuda(), r, tiled=False).cpu()
    m = mask.reshape(-1)
    assert torch.equal(new[m], old[m]) and float(new[m].abs().max()) == 0.0
    assert torch.isfinite(new).all()
    _check(f"{net} non-finite neighbours", new, _ref(f1, f2, clean, 4, r))
    _check(f"{net} per-pixel kernel, same input", old, _ref(f1, f2, clean, 4, r))


@pytest.mark.parametrize("net", sorted(NETS))
def test_shared_and_indexed_images(cuda, net):
    ops = _ops()
    C, r = NETS[net]
    B, h, w, n = 5, 16, 16, 3
    f1, f2, lv, g = _maps(23, n, n, h, w, C, 4)
    coords = (_grid(B, h, w) + (torch.rand((B, h, w, 2), generator=g) - 0.5) * 5).contiguous()
    i1 = torch.tensor([2, 0, 1, 1, 2])
    i2 = torch.tensor([0, 2, 2, 1, 0])
    got = ops.local_corr_rows(f1.cuda(), lv, coords.cuda(), r, idx1=i1.cuda(), idx2=i2.cuda())
    _check(f"{net} indexed", got, _ref(f1, f2, coords, 4, r, i1, i2))
    zero = torch.zeros(B, dtype=torch.int64)
    f1b = torch.randn((B, h, w, C), generator=g)
    got = ops.local_corr_rows(f1b.cuda(), lv, coords.cuda(), r, idx2=zero.cuda())           # all zeros: one key frame for the batch
    _check(f"{net} shared fmap2", got, _ref(f1b, f2, coords, 4, r, None, zero))
    got = ops.local_corr_rows(f1.cuda(), [t[:1].repeat(B, 1, 1, 1).contiguous() for t in lv], coords.cuda(), r, idx1=zero.cuda())
    _check(f"{net} shared fmap1", got, _ref(f1, f2[:1].repeat(B, 1, 1, 1), coords, 4, r, zero, None))
    with pytest.raises(RuntimeError):
        ops.local_corr_rows(f1.cuda(), lv, coords.cuda(), r, idx2=torch.tensor([0, 1, 2, 3, 0]).cuda())     # image 3 of 3
    with pytest.raises(RuntimeError):
        ops.local_corr_rows(f1.cuda(), lv, coords.cuda(), r)                                               # 3 images, 5 pairs, no indices


@pytest.mark.parametrize("net,ld", [("basic", 336), ("small", 224)])
def test_deterministic_and_pad_columns_untouched(cuda, net, ld):
    """Two runs are bit-identical (staged and fallback tiles alike), and of rows poisoned beforehand only the feature columns are
    written: the engine zeroes the pad columns of its lookup rows once per forward and relies on nobody touching them."""
    ops = _ops()
    C, r = NETS[net]
    B, h, w = 2, 33, 27
    f1, f2, lv, g = _maps(29, B, B, h, w, C, 4)
    coords = _grid(B, h, w) + (torch.rand((B, h, w, 2), generator=g) - 0.5) * 4
    coords[1] = torch.rand((h, w, 2), generator=g) * torch.tensor([float(w), float(h)])          # pair 1: incoherent, fallback tiles
    c = coords.contiguous().cuda()
    n_out = 4 * (2 * r + 1) ** 2
    rows = torch.full((B * h * w, ld), float("nan"), device="cuda")
    ops.local_corr_rows(f1.cuda(), lv, c, r, rows=rows)
    assert torch.isfinite(rows[:, :n_out]).all() and torch.isnan(rows[:, n_out:]).all()
    again = torch.full((B * h * w, ld), float("nan"), device="cuda")
    ops.local_corr_rows(f1.cuda(), lv, c, r, rows=again)
    assert torch.equal(rows[:, :n_out], again[:, :n_out])
    _check(f"{net} padded rows", rows[:, :n_out], _ref(f1, f2, coords, 4, r))
    fewer = ops.local_corr_rows(f1.cuda(), lv[:2], c, r)                                             # two levels only
    assert torch.equal(fewer, rows[:, : n_out // 2])


def test_preconditions(cuda):
    ops = _ops()
    f = torch.zeros((1, 8, 8, 24)).cuda()
    c = torch.zeros((1, 8, 8, 2)).cuda()
    from sd_animation_optical_flow_amd._lib import OfxError
    with pytest.raises(OfxError):
        ops.local_corr_rows(f, [f], c, 4)                      # C % 16
    f = torch.zeros((1, 8, 8, 32)).cuda()
    with pytest.raises(OfxError):
        ops.local_corr_rows(f, [f], c, 2)                      # radius 3 or 4 only
    with pytest.raises(RuntimeError):
        ops.local_corr_rows(f, [f, f], c, 4)                   # level 1 must be 4x4
    with pytest.raises(RuntimeError):
        ops.local_corr_rows(f, [f], c, 4, rows=torch.zeros((64, 80)).cuda())      # 81 columns needed
