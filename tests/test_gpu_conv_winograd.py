"""The fused Winograd F(2x2,3x3) convolution (conv_wino.hip) of the update block's 3x3 layers.

GPU tests are marked -m gpu; the host weight transform is checked without a GPU.
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


def _wino_reference(w):
    """U = G g G^T in float64, in the documented operand order of ofx_wino_conv_weight."""
    co, ci = w.shape[:2]
    G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
    u = np.einsum("ir,ocrs,js->ijoc", G, w.astype(np.float64), G)        # [4][4][co][ci]
    nb = 2 * ((co + 63) // 64)
    full = np.zeros((16, nb * 32, ci), dtype=np.float64)
    full[:, :co, :] = u.reshape(16, co, ci)
    # [16][nb][32 n][ci / 8][2 h][4 e] -> [16][nb][ci / 8][2 h][32 n][4 e]
    blk = full.reshape(16, nb, 32, ci // 8, 2, 4).transpose(0, 1, 3, 4, 2, 5)
    return blk.reshape(-1)


@pytest.mark.parametrize("co,ci", [(192, 256), (126, 32), (64, 16)])
def test_host_weight_transform_against_numpy_float64(co, ci):
    ops = _ops()
    rng = np.random.default_rng(co + ci)
    w = (rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci)).astype(np.float32)
    got = ops.wino_conv_weight(torch.from_numpy(w)).numpy()
    ref = _wino_reference(w)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref.astype(np.float32))                 # one rounding of the float64 transform
    with pytest.raises(Exception):
        ops.wino_conv_weight(torch.zeros((8, 12, 3, 3)))              # Cin must be whole 16-channel slabs


def _case(B, H, W, ci, co, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, ci, H, W), generator=g)
    w = torch.randn((co, ci, 3, 3), generator=g) / np.sqrt(ci * 9)
    sh = torch.randn((co,), generator=g) * 0.1
    ref = torch.relu(F.conv2d(x.double(), w.double(), padding=1) + sh.double().view(1, -1, 1, 1))
    return x, w, sh, ref


# the update block's four 3x3 layers: convc2, flow_head.conv1, conv, convf2
SHAPES = [(256, 192), (128, 256), (256, 126), (128, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("ci,co", SHAPES)
def test_winograd_matches_float64_and_stays_near_the_direct_error(cuda, ci, co):
    ops = _ops()
    x, w, sh, ref = _case(2, 16, 32, ci, co, ci + co)
    wp, u = ops.pack_conv_weight(w).cuda(), ops.wino_conv_weight(w).cuda()
    kw = dict(shift=sh.cuda(), act="relu")
    win = ops.conv2d_nhwc(nhwc(x), wp, 3, 3, co, wino_w=u, tile=ops.TILE_WINOGRAD, **kw)
    direct = ops.conv2d_nhwc(nhwc(x), wp, 3, 3, co, tile=16128128, **kw)
    e_win = (nchw(win).double() - ref).abs().max().item()
    e_dir = (nchw(direct).double() - ref).abs().max().item()
    assert e_win < 2e-5, (e_win, e_dir)
    assert e_win <= 3 * e_dir, (e_win, e_dir)
    assert not torch.equal(win, direct)                                # the fused kernel really ran
    assert torch.equal(win, ops.conv2d_nhwc(nhwc(x), wp, 3, 3, co, wino_w=u, tile=ops.TILE_WINOGRAD, **kw))   # repeats bit for bit


@pytest.mark.gpu
def test_two_input_segments_and_identity_activation(cuda):
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    xa, xb = torch.randn((1, 192, 8, 16), generator=g), torch.randn((1, 64, 8, 16), generator=g)
    w = torch.randn((126, 256, 3, 3), generator=g) / 48.0
    sc, sh = torch.rand((126,), generator=g) + 0.5, torch.randn((126,), generator=g)
    ref = F.conv2d(torch.cat([xa, xb], 1).double(), w.double(), padding=1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    out = ops.conv2d_nhwc(nhwc(xa), ops.pack_conv_weight(w).cuda(), 3, 3, 126, x2=nhwc(xb), scale=sc.cuda(), shift=sh.cuda(),
                          wino_w=ops.wino_conv_weight(w).cuda(), tile=ops.TILE_WINOGRAD)
    assert (nchw(out).double() - ref).abs().max().item() < 2e-5


@pytest.mark.gpu
def test_strided_destination_with_a_channel_offset_leaves_the_neighbours_alone(cuda):
    ops = _ops()
    x, w, sh, ref = _case(1, 16, 16, 128, 126, 7)
    ld, off = 300, 130
    dst = torch.full((1, 16, 16, ld), 7.5, device="cuda")
    ops.conv2d_nhwc(nhwc(x), ops.pack_conv_weight(w).cuda(), 3, 3, 126, shift=sh.cuda(), act="relu",
                    wino_w=ops.wino_conv_weight(w).cuda(), tile=ops.TILE_WINOGRAD, out=dst, out_off=off)
    assert (nchw(dst[..., off:off + 126].contiguous()).double() - ref).abs().max().item() < 2e-5
    assert bool((dst[..., :off] == 7.5).all()) and bool((dst[..., off + 126:] == 7.5).all())


@pytest.mark.gpu
def test_maps_of_partial_patches_take_the_direct_kernel(cuda):
    """Automatic routing: a batch large enough for the fused kernel takes it on a map of whole 8x16 patches and keeps the direct
    kernel (bit for bit the launch without the Winograd operand) when the width is not whole patches; forcing the fused kernel
    there is rejected."""
    ops = _ops()
    for (H, W, whole) in ((64, 96, True), (64, 88, False)):
        x, w, sh, ref = _case(24, H, W, 128, 64, H + W)
        wp, u = ops.pack_conv_weight(w).cuda(), ops.wino_conv_weight(w).cuda()
        kw = dict(shift=sh.cuda(), act="relu")
        auto = ops.conv2d_nhwc(nhwc(x), wp, 3, 3, 64, wino_w=u, **kw)
        direct = ops.conv2d_nhwc(nhwc(x), wp, 3, 3, 64, **kw)
        assert (nchw(auto).double() - ref).abs().max().item() < 2e-5
        assert torch.equal(auto, direct) != whole, (H, W)
        if not whole:
            with pytest.raises(RuntimeError):
                ops.conv2d_nhwc(nhwc(x), wp, 3, 3, 64, wino_w=u, tile=ops.TILE_WINOGRAD, **kw)


_BENCH_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd.raft import RaftEngine
from sd_animation_optical_flow_amd.weights import random_state_dict
eng = RaftEngine(random_state_dict(0), "cuda")
B, H, W = 64, 512, 768
g = torch.Generator().manual_seed(11)
base = torch.rand((1, 3, H + 32, W + 32), generator=g)
base = torch.nn.functional.conv2d(base, torch.ones((3, 1, 5, 5)) / 25.0, padding=2, groups=3)
base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)[0].permute(1, 2, 0)
key = base[16:16 + H, 16:16 + W].contiguous()
frames = torch.stack([base[16 + (b % 5) - 2:16 + (b % 5) - 2 + H, 16 + (3 * b % 7) - 3:16 + (3 * b % 7) - 3 + W] for b in range(B)])
up = eng.forward(frames.contiguous().cuda(), key.cuda(), iters=20)
np.save(sys.argv[2], up.cpu().numpy())
"""


@pytest.mark.gpu
def test_bench_size_flow_with_and_without_the_winograd_route(cuda, tmp_path):
    """The bench configuration (64 pairs of 512x768, 20 iterations) takes the fused kernel for its four 3x3 update-block layers;
    OFX_CONV_NO_WINOGRAD (read once per process, hence child processes) keeps the direct kernels.  The flows must differ (the
    route was taken) by less than 1e-4 px."""
    def run(tag, extra):
        env = {k: v for k, v in os.environ.items() if k != "OFX_CONV_NO_WINOGRAD"}
        env.update(extra)
        path = str(tmp_path / f"{tag}.npy")
        out = subprocess.run([sys.executable, "-c", _BENCH_SCRIPT, ROOT, path], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        return np.load(path)

    wino = run("wino", {})
    direct = run("direct", {"OFX_CONV_NO_WINOGRAD": "1"})
    d = np.abs(wino - direct).max()
    assert np.isfinite(wino).all() and 0 < d < 1e-4, d
