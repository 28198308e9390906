"""The fused Winograd F(2x2,3x3) convolution (conv_wino.hip) on the encoders' stride-1 3x3 layers: the residual merge of the
context encoder's blocks, instance norm + ReLU fused into the operand, and the epilogue statistics of the feature encoder.

Checked against float64 F.conv2d (forced route) and, end to end, against the direct kernels (OFX_CONV_NO_WINOGRAD_ENC /
OFX_CONV_NO_WINOGRAD are read once per process, hence child processes).  GPU tests are marked -m gpu.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def nhwc(x):  # NCHW cpu -> NHWC cuda
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):  # NHWC cuda -> NCHW cpu
    return x.permute(0, 3, 1, 2).contiguous().cpu()


def _weights(ci, co, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((co, ci, 3, 3), generator=g) / np.sqrt(ci * 9)
    scale = 0.5 + torch.rand((co,), generator=g)
    shift = torch.randn((co,), generator=g) * 0.1
    return g, w, scale, shift


# (Cin = Cout, map per image): the three residual stages of a 512x768 frame, and a map that is no bench size
STAGES = [(64, 384, 256), (96, 192, 128), (128, 96, 64), (96, 40, 48)]


@pytest.mark.gpu
@pytest.mark.parametrize("c,H,W", STAGES)
def test_residual_epilogue_with_folded_scale_and_shift(cuda, c, H, W):
    """cnet's conv2: y = relu(acc * scale + shift), then relu(y + res)."""
    ops = _ops()
    g, w, scale, shift = _weights(c, c, c + H)
    x = torch.relu(torch.randn((1, c, H, W), generator=g))
    res = torch.randn((1, c, H, W), generator=g)
    y = torch.relu(F.conv2d(x.double(), w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    ref = torch.relu(y + res.double())
    wp, u = ops.pack_conv_weight(w).cuda(), ops.wino_conv_weight(w).cuda()
    kw = dict(scale=scale.cuda(), shift=shift.cuda(), act="relu", res=nhwc(res))
    got = ops.conv2d_nhwc(nhwc(x), wp, 3, 3, c, wino_w=u, tile=ops.TILE_WINOGRAD, **kw)
    direct = ops.conv2d_nhwc(nhwc(x), wp, 3, 3, c, **kw)
    e_win = (nchw(got).double() - ref).abs().max().item()
    e_dir = (nchw(direct).double() - ref).abs().max().item()
    assert e_win < 2e-5 and e_win < 8 * e_dir + 1e-6, (e_win, e_dir)
    assert not torch.equal(got, direct)                                 # the fused kernel ran


@pytest.mark.gpu
@pytest.mark.parametrize("c,H,W", STAGES)
def test_norm_and_relu_on_load_pads_after_normalising(cuda, c, H, W):
    """fnet's conv2: the operand is relu((x - mean) * rstd) per image and channel; the zero padding is that of the normalised
    map, so the border pixels see zeros, not relu(-mean * rstd)."""
    ops = _ops()
    B = 2
    g, w, _, shift = _weights(c, c, 3 * c + W)
    # channel means of either sign: where the mean is negative, normalising the padding instead of zeroing it would feed
    # relu(-mean * rstd) ~ 0.75 into every border tap
    off = torch.where(torch.arange(c) % 2 == 0, 1.5, -1.5).view(1, c, 1, 1)
    x = torch.randn((B, c, H, W), generator=g) * 2.0 + off
    mean = x.double().mean(dim=(2, 3))
    rstd = 1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)
    xn = torch.relu((x.double() - mean.view(B, c, 1, 1)) * rstd.view(B, c, 1, 1))
    ref = F.conv2d(xn, w.double(), padding=1) + shift.double().view(1, -1, 1, 1)
    wp, u = ops.pack_conv_weight(w).cuda(), ops.wino_conv_weight(w).cuda()
    kw = dict(shift=shift.cuda(), nmean=mean.float().cuda(), nrstd=rstd.float().cuda())
    got = nchw(ops.conv2d_nhwc(nhwc(x), wp, 3, 3, c, wino_w=u, tile=ops.TILE_WINOGRAD, **kw)).double()
    direct = nchw(ops.conv2d_nhwc(nhwc(x), wp, 3, 3, c, **kw)).double()
    e_dir = (direct - ref).abs().max().item()
    for name, sl in (("all", np.s_[:]), ("top", np.s_[:, :, 0]), ("bottom", np.s_[:, :, -1]), ("left", np.s_[:, :, :, 0]),
                     ("right", np.s_[:, :, :, -1])):
        e = (got[sl] - ref[sl]).abs().max().item()
        assert e < 3e-5 and e < 8 * e_dir + 1e-6, (name, e, e_dir)


@pytest.mark.gpu
@pytest.mark.parametrize("c,H,W", STAGES)
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
def test_epilogue_statistics_against_float64_and_on_a_repeat(cuda, c, H, W, norm):
    """ofx_conv2d_stats on the fused kernel: one row per 8x16 patch, nothing written past [B][rows][Cout][2] (the 96-channel
    layers' second block computes 32 channels that do not exist), finalised mean / rstd against float64 of the reference output,
    and the partials bit-identical on a repeat."""
    ops = _ops()
    B = 2
    g, w, _, shift = _weights(c, c, 5 * c + H)
    x = torch.randn((B, c, H, W), generator=g) + 0.5
    kw = dict(shift=shift.cuda())
    xin = x.double()
    if norm:
        mean = x.double().mean(dim=(2, 3))
        rstd = 1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)
        xin = torch.relu((xin - mean.view(B, c, 1, 1)) * rstd.view(B, c, 1, 1))
        kw.update(nmean=mean.float().cuda(), nrstd=rstd.float().cuda())
    ref = F.conv2d(xin, w.double(), padding=1) + shift.double().view(1, -1, 1, 1)
    rows = (H // 8) * (W // 16)
    need = B * rows * c * 2
    wp, u = ops.pack_conv_weight(w).cuda(), ops.wino_conv_weight(w).cuda()
    parts = []
    for _ in range(2):
        part = torch.full((need + 4096,), float("nan"), device="cuda")
        out, got_rows = ops.conv2d_nhwc(nhwc(x), wp, 3, 3, c, wino_w=u, tile=ops.TILE_WINOGRAD, stats_part=part, **kw)
        assert got_rows == rows
        assert torch.isfinite(part[:need]).all() and torch.isnan(part[need:]).all()
        parts.append(part[:need].clone())
    assert torch.equal(parts[0], parts[1])
    # each row is the patch's own sums: check against float64 sums of the kernel's output over that patch
    o = nchw(out).double().view(B, c, H // 8, 8, W // 16, 16)
    ps = parts[0].double().cpu().view(B, H // 8, W // 16, c, 2)
    assert torch.allclose(ps[..., 0], o.sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3)
    assert torch.allclose(ps[..., 1], (o * o).sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3)
    mean, rstd = ops.inorm_finalize(parts[0], B, rows, H * W, c)
    rmean = ref.mean(dim=(2, 3))
    rrstd = 1.0 / torch.sqrt(ref.var(dim=(2, 3), unbiased=False) + 1e-5)
    assert (mean.double().cpu() - rmean).abs().max().item() < 2e-5
    assert ((rstd.double().cpu() - rrstd) / rrstd).abs().max().item() < 1e-4
    with pytest.raises(RuntimeError):   # a residual merge: statistics are of raw outputs only, so the forced route is refused
        ops.conv2d_nhwc(nhwc(x), wp, 3, 3, c, wino_w=u, tile=ops.TILE_WINOGRAD, stats_part=part, res=out, **kw)


@pytest.mark.gpu
def test_fused_norm_with_a_residual_and_the_mask_head_shape(cuda):
    """The combinations the engine does not use today still compute the documented epilogue; mask.0 (128 -> 256, ReLU) too."""
    ops = _ops()
    g, w, scale, shift = _weights(64, 64, 5)
    x = torch.randn((1, 64, 16, 32), generator=g)
    res = torch.randn((1, 64, 16, 32), generator=g)
    mean = x.double().mean(dim=(2, 3))
    rstd = 1.0 / x.double().std(dim=(2, 3))
    xn = torch.relu((x.double() - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1))
    ref = torch.relu(torch.relu(F.conv2d(xn, w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
                     + res.double())
    got = ops.conv2d_nhwc(nhwc(x), ops.pack_conv_weight(w).cuda(), 3, 3, 64, scale=scale.cuda(), shift=shift.cuda(), act="relu",
                          res=nhwc(res), nmean=mean.float().cuda(), nrstd=rstd.float().cuda(), wino_w=ops.wino_conv_weight(w).cuda(),
                          tile=ops.TILE_WINOGRAD)
    assert (nchw(got).double() - ref).abs().max().item() < 3e-5

    g, w, _, shift = _weights(128, 256, 6)
    x = torch.randn((1, 128, 64, 96), generator=g)
    ref = torch.relu(F.conv2d(x.double(), w.double(), padding=1) + shift.double().view(1, -1, 1, 1))
    got = ops.conv2d_nhwc(nhwc(x), ops.pack_conv_weight(w).cuda(), 3, 3, 256, shift=shift.cuda(), act="relu",
                          wino_w=ops.wino_conv_weight(w).cuda(), tile=ops.TILE_WINOGRAD)
    assert (nchw(got).double() - ref).abs().max().item() < 2e-5


@pytest.mark.gpu
def test_layers_that_do_not_qualify_are_still_rejected(cuda):
    ops = _ops()
    g, w, _, shift = _weights(64, 64, 7)
    x = nhwc(torch.randn((1, 64, 32, 64), generator=g))
    wp, u = ops.pack_conv_weight(w).cuda(), ops.wino_conv_weight(w).cuda()
    with pytest.raises(RuntimeError):   # stride 2 (the strided blocks' conv1)
        ops.conv2d_nhwc(x, wp, 3, 3, 64, stride=2, wino_w=u, tile=ops.TILE_WINOGRAD)
    m = torch.zeros((1, 64), device="cuda")
    w2 = torch.randn((64, 80, 3, 3), generator=g) / 30.0
    with pytest.raises(RuntimeError):   # fused norm over two input segments
        ops.conv2d_nhwc(x, ops.pack_conv_weight(w2).cuda(), 3, 3, 64, x2=nhwc(torch.randn((1, 16, 32, 64))), nmean=m, nrstd=m,
                        wino_w=ops.wino_conv_weight(w2).cuda(), tile=ops.TILE_WINOGRAD)
    with pytest.raises(RuntimeError):   # 1x5: no fused norm there
        w15 = torch.randn((128, 64, 1, 5), generator=g) / 20.0
        ops.conv2d_nhwc(x, ops.pack_conv_weight(w15).cuda(), 1, 5, 128, nmean=m, nrstd=m, wino_w=ops.wino15_conv_weight(w15).cuda(),
                        tile=ops.TILE_WINOGRAD)


_ROUTE_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd import ops
g = torch.Generator().manual_seed(3)
x = torch.relu(torch.randn((4, 384, 256, 64), generator=g)).cuda()
res = torch.randn((4, 384, 256, 64), generator=g).cuda()
w = torch.randn((64, 64, 3, 3), generator=g) / 24.0
sc, sh = (0.5 + torch.rand(64, generator=g)).cuda(), (0.1 * torch.randn(64, generator=g)).cuda()
y = ops.conv2d_nhwc(x, ops.pack_conv_weight(w).cuda(), 3, 3, 64, scale=sc, shift=sh, act="relu", res=res,
                    wino_w=ops.wino_conv_weight(w).cuda())
np.save(sys.argv[2], y.cpu().numpy())
"""


@pytest.mark.gpu
def test_no_winograd_switch_restores_the_direct_result_bit_for_bit(cuda, tmp_path):
    """A layer1-sized residual layer (4 images: 3072 workgroups) takes the fused kernel on its own; OFX_CONV_NO_WINOGRAD gives back
    exactly what the direct kernel computes."""
    def run(tag, extra):
        env = {k: v for k, v in os.environ.items() if not k.startswith("OFX_CONV_NO_WINOGRAD")}
        env.update(extra)
        path = str(tmp_path / f"{tag}.npy")
        out = subprocess.run([sys.executable, "-c", _ROUTE_SCRIPT, ROOT, path], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return np.load(path)

    ops = _ops()
    auto, off = run("auto", {}), run("off", {"OFX_CONV_NO_WINOGRAD": "1"})
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn((4, 384, 256, 64), generator=g)).cuda()
    res = torch.randn((4, 384, 256, 64), generator=g).cuda()
    w = torch.randn((64, 64, 3, 3), generator=g) / 24.0
    sc, sh = (0.5 + torch.rand(64, generator=g)).cuda(), (0.1 * torch.randn(64, generator=g)).cuda()
    direct = ops.conv2d_nhwc(x, ops.pack_conv_weight(w).cuda(), 3, 3, 64, scale=sc, shift=sh, act="relu", res=res)   # no operand: the direct route
    assert np.array_equal(off, direct.cpu().numpy())
    assert not np.array_equal(auto, off) and np.abs(auto - off).max() < 1e-4


_ENGINE_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd.raft import RaftEngine
from sd_animation_optical_flow_amd.weights import random_state_dict
B, H, W = 8, 512, 768
g = torch.Generator().manual_seed(5)
base = torch.rand((1, 3, H + 32, W + 32), generator=g)
base = torch.nn.functional.conv2d(base, torch.ones((3, 1, 5, 5)) / 25.0, padding=2, groups=3)
base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)[0].permute(1, 2, 0)
key = base[16:16 + H, 16:16 + W].contiguous().cuda()
frames = torch.stack([base[16 + (b % 5) - 2:16 + (b % 5) - 2 + H, 16 + (3 * b % 7) - 3:16 + (3 * b % 7) - 3 + W] for b in range(B)])
frames = frames.contiguous().cuda()
out = []
for norm in ("eval", "batch"):
    eng = RaftEngine(random_state_dict(0), "cuda", cnet_norm=norm)
    a = eng.forward(frames, key, iters=6).cpu().numpy()
    b = eng.forward(frames, key, iters=6).cpu().numpy()
    assert np.array_equal(a, b), norm   # the epilogue statistics are deterministic: a repeat is bit-identical
    out.append(a)
np.save(sys.argv[2], np.stack(out))
"""


@pytest.mark.gpu
def test_engine_flow_with_and_without_the_encoder_route(cuda, tmp_path):
    """Eight 512x768 pairs (layer1 / layer2 take the fused kernel, with norm-on-load and epilogue statistics in fnet and cnetb and
    the residual merge in cnet), in both cnet_norm modes, against the engine built without the encoders' Winograd operands."""
    def run(tag, extra):
        env = {k: v for k, v in os.environ.items() if not k.startswith("OFX_CONV_NO_WINOGRAD")}
        env.update(extra)
        path = str(tmp_path / f"{tag}.npy")
        out = subprocess.run([sys.executable, "-c", _ENGINE_SCRIPT, ROOT, path], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return np.load(path)

    wino = run("wino", {})
    direct = run("direct", {"OFX_CONV_NO_WINOGRAD_ENC": "1"})
    assert np.isfinite(wino).all()
    for k, norm in enumerate(("eval", "batch")):
        d = np.abs(wino[k] - direct[k]).max()
        assert 0 < d < 1e-4, (norm, d)
