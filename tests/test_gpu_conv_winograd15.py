"""The fused 1D Winograd F(4,5) convolution (conv_wino.hip) of the SepConvGRU's 1x5 and 5x1 layers.

GPU tests are marked -m gpu; the host weight transform is checked without a GPU.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI_ZR, EPI_Q = 1, 2


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def nhwc(x):  # NCHW cpu -> NHWC cuda
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):  # NHWC cuda -> NCHW cpu
    return x.permute(0, 3, 1, 2).contiguous().cpu()


# G of F(4,5) over the points 0, 1, -1, 2, -2, 1/2, -1/2, inf (row 0 sign-flipped), as the host transform writes it
_G = np.array([
    [1, 0, 0, 0, 0],
    [-2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9, -2.0 / 9],
    [-2.0 / 9, 2.0 / 9, -2.0 / 9, 2.0 / 9, -2.0 / 9],
    [1.0 / 90, 1.0 / 45, 2.0 / 45, 4.0 / 45, 8.0 / 45],
    [1.0 / 90, -1.0 / 45, 2.0 / 45, -4.0 / 45, 8.0 / 45],
    [32.0 / 45, 16.0 / 45, 8.0 / 45, 4.0 / 45, 2.0 / 45],
    [32.0 / 45, -16.0 / 45, 8.0 / 45, -4.0 / 45, 2.0 / 45],
    [0, 0, 0, 0, 1],
], dtype=np.float64)


def _wino15_reference(w):
    """U = G g in float64 (taps summed in order), in the documented operand order of ofx_wino15_conv_weight."""
    co, ci = w.shape[:2]
    g = w.reshape(co, ci, 5).astype(np.float64)
    u = np.zeros((8, co, ci), dtype=np.float64)
    for t in range(5):
        u = u + _G[:, t].reshape(8, 1, 1) * g[None, :, :, t]
    nb = 4 * ((co + 127) // 128)
    full = np.zeros((8, nb * 32, ci), dtype=np.float64)
    full[:, :co, :] = u
    # [8][nb][32 n][ci / 8][2 h][4 e] -> [8][nb][ci / 8][2 h][32 n][4 e]
    return full.reshape(8, nb, 32, ci // 8, 2, 4).transpose(0, 1, 3, 4, 2, 5).reshape(-1)


def test_transform_reproduces_a_five_tap_correlation():
    """y = A^T [(G g) (.) (B^T d)] is the correlation of d with g (the matrices of the kernel, in float64)."""
    BT = np.array([
        [1, 0, -5.25, 0, 5.25, 0, -1, 0],
        [0, 1, 1, -4.25, -4.25, 1, 1, 0],
        [0, -1, 1, 4.25, -4.25, -1, 1, 0],
        [0, 0.5, 0.25, -2.5, -1.25, 2, 1, 0],
        [0, -0.5, 0.25, 2.5, -1.25, -2, 1, 0],
        [0, 2, 4, -2.5, -5, 0.5, 1, 0],
        [0, -2, 4, 2.5, -5, -0.5, 1, 0],
        [0, -1, 0, 5.25, 0, -5.25, 0, 1],
    ])
    AT = np.array([
        [1, 1, 1, 1, 1, 1, 1, 0],
        [0, 1, -1, 2, -2, 0.5, -0.5, 0],
        [0, 1, 1, 4, 4, 0.25, 0.25, 0],
        [0, 1, -1, 8, -8, 0.125, -0.125, 1],
    ])
    rng = np.random.default_rng(0)
    d, g = rng.standard_normal(8), rng.standard_normal(5)
    y = AT @ ((_G @ g) * (BT @ d))
    assert np.allclose(y, [d[i:i + 5] @ g for i in range(4)], rtol=0, atol=1e-12)


@pytest.mark.parametrize("co,ci,kh,kw", [(256, 256, 1, 5), (128, 256, 5, 1), (64, 16, 1, 5), (200, 32, 5, 1)])
def test_host_weight_transform_against_numpy_float64(co, ci, kh, kw):
    ops = _ops()
    rng = np.random.default_rng(co + ci + kh)
    w = (rng.standard_normal((co, ci, kh, kw)) * 0.02).astype(np.float32)
    got = ops.wino15_conv_weight(torch.from_numpy(w)).numpy()
    ref = _wino15_reference(w)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref.astype(np.float32))                 # one rounding of the float64 transform


@pytest.mark.parametrize("shape", [(8, 12, 1, 5), (8, 24, 5, 1), (8, 16, 3, 3), (8, 16, 1, 3), (8, 16, 5, 5)])
def test_host_weight_transform_refuses_other_shapes(shape):
    with pytest.raises(Exception):
        _ops().wino15_conv_weight(torch.zeros(shape))                # whole 16-channel slabs, 1x5 or 5x1 only


def test_the_3x3_transform_keeps_refusing_1d_weights():
    with pytest.raises(RuntimeError):
        _ops().wino_conv_weight(torch.zeros((8, 16, 1, 5)))


def _pad(kh):
    return (0, 2) if kh == 1 else (2, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
@pytest.mark.parametrize("co,segs", [(256, 1), (128, 2), (64, 1)])
def test_plain_epilogue_matches_float64_and_stays_near_the_direct_error(cuda, kh, kw, co, segs):
    ops = _ops()
    g = torch.Generator().manual_seed(co + kh + segs)
    x = torch.randn((2, 256, 16, 32), generator=g)
    w = torch.randn((co, 256, kh, kw), generator=g) / np.sqrt(256 * 5)
    sh = torch.randn((co,), generator=g) * 0.1
    add = torch.randn((2, co, 16, 32), generator=g) * 0.5
    ref = torch.relu(F.conv2d(x.double(), w.double(), padding=_pad(kh)) + sh.double().view(1, -1, 1, 1) + add.double())
    xa, xb = (x, None) if segs == 1 else (x[:, :128], x[:, 128:])
    kw_ = dict(x2=None if xb is None else nhwc(xb), shift=sh.cuda(), act="relu", addend=nhwc(add))
    wp, u = ops.pack_conv_weight(w).cuda(), ops.wino15_conv_weight(w).cuda()
    win = ops.conv2d_nhwc(nhwc(xa), wp, kh, kw, co, wino_w=u, tile=ops.TILE_WINOGRAD, **kw_)
    direct = ops.conv2d_nhwc(nhwc(xa), wp, kh, kw, co, **kw_)
    e_win = (nchw(win).double() - ref).abs().max().item()
    e_dir = (nchw(direct).double() - ref).abs().max().item()
    # F(4,5)'s transforms (|B^T| <= 5.25, |A^T| <= 8) cost a few times the direct kernel's largest error on unit-normal inputs
    # (1.5e-5 against 3.7e-6 here; a float32 host emulation of the same arithmetic: 1.3e-5 max, 2x the RMS of a sequential fp32
    # sum): the gate is the same scale, not the same bound
    assert e_win < 2e-5, (e_win, e_dir)
    assert e_win <= 6 * e_dir, (e_win, e_dir)
    assert not torch.equal(win, direct)                                # the fused kernel really ran
    assert torch.equal(win, ops.conv2d_nhwc(nhwc(xa), wp, kh, kw, co, wino_w=u, tile=ops.TILE_WINOGRAD, **kw_))   # bit for bit


@pytest.mark.gpu
def test_strided_destination_with_a_channel_offset_leaves_the_neighbours_alone(cuda):
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    x = torch.randn((1, 64, 8, 16), generator=g)
    w = torch.randn((96, 64, 5, 1), generator=g) / np.sqrt(64 * 5)
    ref = F.conv2d(x.double(), w.double(), padding=(2, 0))
    ld, off = 300, 130
    dst = torch.full((1, 8, 16, ld), 7.5, device="cuda")
    ops.conv2d_nhwc(nhwc(x), ops.pack_conv_weight(w).cuda(), 5, 1, 96, wino_w=ops.wino15_conv_weight(w).cuda(),
                    tile=ops.TILE_WINOGRAD, out=dst, out_off=off)
    assert (nchw(dst[..., off:off + 96].contiguous()).double() - ref).abs().max().item() < 2e-5
    assert bool((dst[..., :off] == 7.5).all()) and bool((dst[..., off + 96:] == 7.5).all())


# ---- the GRU gate epilogues through a raw descriptor, laid out as the engine launches them (raft_engine.cpp, run_recurrence):
# hx rows [h 128 | motion 128 | inp 128], gadd rows [zr1 256 | q1 128 | zr2 256 | q2 128], z / rh rows of 128
B, H, W = 2, 16, 32
M = B * H * W


def _gru_state(seed):
    g = torch.Generator().manual_seed(seed)
    hx = torch.cat([torch.tanh(torch.randn((M, 128), generator=g)), torch.relu(torch.randn((M, 128), generator=g)),
                    torch.randn((M, 128), generator=g)], 1)
    gadd = torch.randn((M, 768), generator=g) * 0.3
    z = torch.rand((M, 128), generator=g)
    wzr = torch.randn((256, 256, 1, 5), generator=g) * 0.02
    wq = torch.randn((128, 256, 1, 5), generator=g) * 0.02
    return hx, gadd, z, wzr, wq


def _conv64(rows, w, kh, kw):   # [M][C] float64 rows -> conv -> [M][Cout]
    x = rows.double().view(B, H, W, -1).permute(0, 3, 1, 2)
    return F.conv2d(x, w.double().view(w.shape[0], w.shape[1], kh, kw), padding=_pad(kh)).permute(0, 2, 3, 1).reshape(M, -1)


def _launch(kh, kw, epi, cout, w, u, in0, ld0, c0, hx, z, rh, gadd, goff, in1=None, ld1=0, c1=0, wino=True):
    from sd_animation_optical_flow_amd import _lib, ops
    d = _lib.ConvDesc()
    d.in0, d.ld0, d.c0 = in0, ld0, c0
    if in1 is not None:
        d.in1, d.ld1, d.c1 = in1, ld1, c1
    wp = ops.pack_conv_weight(w).cuda()
    d.w = wp.data_ptr()
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, H, W, H, W, cout
    d.KH, d.KW, d.stride, d.padH, d.padW = kh, kw, 1, kh // 2, kw // 2
    d.act, d.epi = 0, epi
    d.aux_z, d.aux_rh, d.aux_h, d.ldh = z.data_ptr(), rh.data_ptr(), hx.data_ptr(), 384
    d.addend, d.ldadd = gadd.data_ptr() + 4 * goff, 768
    if wino:
        d.wino_w, d.tile = u.data_ptr(), ops.TILE_WINOGRAD
    lib = _lib.lib()
    st = lib.ofx_conv2d(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, st


def _zr(kh, kw, wino, seed=1):
    ops = _ops()
    hx, gadd, z0, wzr, _ = _gru_state(seed)
    wzr = wzr.view(256, 256, kh, kw)
    u = ops.wino15_conv_weight(wzr).cuda()
    dhx, dg = hx.cuda(), gadd.cuda()
    z, rh = torch.full((M, 128), 3.0, device="cuda"), torch.full((M, 128), 3.0, device="cuda")
    _launch(kh, kw, EPI_ZR, 256, wzr, u, dhx.data_ptr(), 384, 256, dhx, z, rh, dg, 0, wino=wino)
    v = _conv64(hx[:, :256], wzr, kh, kw) + gadd[:, :256].double()
    zr = torch.sigmoid(v)
    assert torch.equal(dhx.cpu(), hx)                                   # the input rows are only read
    return z.cpu(), rh.cpu(), zr[:, :128], zr[:, 128:] * hx[:, :128].double()


def _q(kh, kw, wino, seed=2):
    ops = _ops()
    hx, gadd, z, _, wq = _gru_state(seed)
    wq = wq.view(128, 256, kh, kw)
    u = ops.wino15_conv_weight(wq).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    rh = torch.tanh(torch.randn((M, 128), generator=g)) * 0.5
    dhx, dg, dz, drh = hx.cuda(), gadd.cuda(), z.cuda(), rh.cuda()
    _launch(kh, kw, EPI_Q, 128, wq, u, drh.data_ptr(), 128, 128, dhx, dz, drh, dg, 256, in1=dhx.data_ptr() + 4 * 128, ld1=384,
            c1=128, wino=wino)
    v = _conv64(torch.cat([rh, hx[:, 128:256]], 1), wq, kh, kw) + gadd[:, 256:384].double()
    hn = (1 - z.double()) * hx[:, :128].double() + z.double() * torch.tanh(v)
    out = dhx.cpu()
    assert torch.equal(out[:, 128:], hx[:, 128:])                       # only the h channels are written
    return out[:, :128], hn


@pytest.mark.gpu
@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
def test_gru_zr_epilogue_matches_float64(cuda, kh, kw):
    z, rh, z_ref, rh_ref = _zr(kh, kw, True)
    zd, rhd, _, _ = _zr(kh, kw, False)
    e = max((z.double() - z_ref).abs().max().item(), (rh.double() - rh_ref).abs().max().item())
    e_dir = max((zd.double() - z_ref).abs().max().item(), (rhd.double() - rh_ref).abs().max().item())
    assert e < 2e-6 and e <= 6 * e_dir + 2e-7, (e, e_dir)
    assert not torch.equal(z, zd)                                       # the fused kernel really ran
    z2, rh2, _, _ = _zr(kh, kw, True)
    assert torch.equal(z, z2) and torch.equal(rh, rh2)                  # repeats bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
def test_gru_q_epilogue_updates_h_in_place_as_float64(cuda, kh, kw):
    h, h_ref = _q(kh, kw, True)
    hd, _ = _q(kh, kw, False)
    e, e_dir = (h.double() - h_ref).abs().max().item(), (hd.double() - h_ref).abs().max().item()
    assert e < 5e-6 and e <= 6 * e_dir + 2e-7, (e, e_dir)
    assert not torch.equal(h, hd)
    assert torch.equal(h, _q(kh, kw, True)[0])


def _routing_case(Bn, Wd, co=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((Bn, 256, 64, Wd), generator=g)
    w = torch.randn((co, 256, 1, 5), generator=g) / np.sqrt(256 * 5)
    return x, w


@pytest.mark.gpu
def test_partial_patches_and_small_grids_take_the_direct_kernel(cuda):
    """Automatic routing: a grid that fills the chip takes the fused kernel on a map of whole 8x16 patches; a map that is not whole
    patches, or a small grid (one pair), keeps the direct kernel bit for bit.  Forcing the fused kernel on a map that does not
    qualify is rejected."""
    ops = _ops()
    for (Bn, Wd, fused) in ((8, 96, True), (8, 88, False), (1, 96, False)):
        x, w = _routing_case(Bn, Wd, seed=Bn + Wd)
        wp, u = ops.pack_conv_weight(w).cuda(), ops.wino15_conv_weight(w).cuda()
        ref = F.conv2d(x.double(), w.double(), padding=(0, 2))
        auto = ops.conv2d_nhwc(nhwc(x), wp, 1, 5, 256, wino_w=u)
        direct = ops.conv2d_nhwc(nhwc(x), wp, 1, 5, 256)
        assert (nchw(auto).double() - ref).abs().max().item() < 2e-5
        assert torch.equal(auto, direct) != fused, (Bn, Wd)
        if Wd % 16:
            with pytest.raises(RuntimeError):
                ops.conv2d_nhwc(nhwc(x), wp, 1, 5, 256, wino_w=u, tile=ops.TILE_WINOGRAD)


_SWITCH_SCRIPT = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd import ops
g = torch.Generator().manual_seed(0)
def same(kh, kw, u_of):
    x = torch.randn((8, 64, 96, 256), generator=g).cuda()
    w = torch.randn((256, 256, kh, kw), generator=g) * 0.02
    wp = ops.pack_conv_weight(w).cuda()
    return torch.equal(ops.conv2d_nhwc(x, wp, kh, kw, 256, wino_w=u_of(w).cuda()), ops.conv2d_nhwc(x, wp, kh, kw, 256))
print(int(same(1, 5, ops.wino15_conv_weight)), int(same(3, 3, ops.wino_conv_weight)))
"""


@pytest.mark.gpu
def test_switches_turn_off_the_1d_route_alone_or_both(cuda):
    """OFX_CONV_NO_WINOGRAD15 keeps the direct kernel for 1x5 / 5x1 layers only; OFX_CONV_NO_WINOGRAD for both Winograd routes
    (each read once per process, hence child processes).  Output: 1 = the direct kernel's result bit for bit."""
    def run(extra):
        env = {k: v for k, v in os.environ.items() if k not in ("OFX_CONV_NO_WINOGRAD", "OFX_CONV_NO_WINOGRAD15")}
        env.update(extra)
        out = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout.split()[-2:]

    assert run({}) == ["0", "0"]
    assert run({"OFX_CONV_NO_WINOGRAD15": "1"}) == ["1", "0"]
    assert run({"OFX_CONV_NO_WINOGRAD": "1"}) == ["1", "1"]


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
def test_bench_size_flow_with_and_without_the_1d_winograd_route(cuda, tmp_path):
    """The bench configuration (64 pairs of 512x768, 20 iterations) takes the fused F(4,5) kernel for its four per-iteration GRU
    layers; OFX_CONV_NO_WINOGRAD15 keeps the direct kernels for them.  The flows must differ (the route was taken) by less than
    1e-4 px."""
    def run(tag, extra):
        env = {k: v for k, v in os.environ.items() if k not in ("OFX_CONV_NO_WINOGRAD", "OFX_CONV_NO_WINOGRAD15")}
        env.update(extra)
        path = str(tmp_path / f"{tag}.npy")
        out = subprocess.run([sys.executable, "-c", _BENCH_SCRIPT, ROOT, path], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        return np.load(path)

    wino = run("wino15", {})
    direct = run("direct", {"OFX_CONV_NO_WINOGRAD15": "1"})
    d = np.abs(wino - direct).max()
    assert np.isfinite(wino).all() and 0 < d < 1e-4, d
