"""The F(4,5) kernels' slab loop (conv_wino.hip, wino_slabs_staged) at the shapes where its pipeline can go wrong.

The loop keeps each weight fragment one slab ahead in registers (reloaded behind the MFMAs that consumed it), the A operands two
fragments ahead, and the halo of the next slab in flight under the products.  The shapes are the smallest that reach every state
of that pipeline: one slab (Cin = 16: the loop re-issues its own slab as "next"), two slabs (Cin = 32: the first real prefetch),
sixteen slabs in two segments of 128 + 128 channels (the q layer's operand; the segment switch falls on a slab boundary); a map
of one 8x16 patch (every halo pixel outside the map comes from the buffer range check) and one of four; one image and three; one
and two blocks of 128 output channels.  Both orientations, the three epilogues, forced onto the fused route through a raw
descriptor as tests/test_gpu_conv_winograd15.py does, against a float64 convolution of the same fp32 weights with that file's
bounds (plain 2e-5, z | r 2e-6, q 5e-6) as they are.  The inputs are unit-normal.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

EPI_PLAIN, EPI_ZR, EPI_Q = 0, 1, 2
ACT_RELU = 1
BOUND = {EPI_PLAIN: 2e-5, EPI_ZR: 2e-6, EPI_Q: 5e-6}
# The bounds belong to the scale of the sums they were set for, and the kernel's rounding error grows with that scale, so the
# weights here give unit-normal inputs the same sums at every Cin.  Plain: a sum of unit variance (weights of 1 / sqrt(5 Cin), as
# there).  Gates: there, weights of 0.02 on 256 channels of tanh / ReLU of unit normals (mean squares 0.39 / 0.5, 0.45 together):
# pre-activations of rms 0.02 sqrt(5 * 256 * 0.45) = 0.48.
GATE_RMS = 0.02 * np.sqrt(5 * 256 * 0.45)

# (segments of input channels, H, W, B, Cout of the plain / q layer); the z | r layer has Cout = 256 throughout (its split falls
# on a 128-channel block), the q layer 128
SHAPES = [
    ((16,), 8, 16, 1, 128),
    ((16,), 16, 32, 3, 256),
    ((32,), 8, 16, 3, 256),
    ((32,), 16, 32, 1, 128),
    ((128, 128), 16, 32, 1, 128),
    ((128, 128), 8, 16, 3, 256),
]


def _conv64(rows, w, B, H, W):   # [M][C] rows -> float64 conv -> [M][Cout]
    kh, kw = w.shape[2:]
    x = rows.double().view(B, H, W, -1).permute(0, 3, 1, 2)
    return F.conv2d(x, w.double(), padding=(kh // 2, kw // 2)).permute(0, 2, 3, 1).reshape(B * H * W, -1)


def _run(kh, kw, epi, segs, H, W, B, cout, seed):
    """-> (largest error against float64, the kernel's outputs)"""
    from sd_animation_optical_flow_amd import _lib, ops
    M, cin = B * H * W, sum(segs)
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn((M, c), generator=g) for c in segs]
    x = torch.cat(xs, 1)
    w = torch.randn((cout, cin, kh, kw), generator=g) * ((1.0 if epi == EPI_PLAIN else GATE_RMS) / np.sqrt(cin * 5))
    add = torch.randn((M, cout), generator=g) * 0.5
    v = _conv64(x, w, B, H, W) + add.double()

    d = _lib.ConvDesc()
    dx = [t.cuda() for t in xs]
    d.in0, d.ld0, d.c0 = dx[0].data_ptr(), segs[0], segs[0]
    if len(segs) == 2:
        d.in1, d.ld1, d.c1 = dx[1].data_ptr(), segs[1], segs[1]
    wp, u = ops.pack_conv_weight(w).cuda(), ops.wino15_conv_weight(w).cuda()
    d.w, d.wino_w, d.tile = wp.data_ptr(), u.data_ptr(), ops.TILE_WINOGRAD
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, H, W, H, W, cout
    d.KH, d.KW, d.stride, d.padH, d.padW = kh, kw, 1, kh // 2, kw // 2
    d.epi = epi
    dadd = add.cuda()
    d.addend, d.ldadd = dadd.data_ptr(), cout

    if epi == EPI_PLAIN:
        sh = torch.randn((cout,), generator=g) * 0.1
        dsh, out = sh.cuda(), torch.full((M, cout), 7.5, device="cuda")
        d.shift, d.act, d.out, d.ldo = dsh.data_ptr(), ACT_RELU, out.data_ptr(), cout
        ref = [torch.relu(v + sh.double())]
        outs = lambda: [out.cpu()]
    elif epi == EPI_ZR:
        hd = cout // 2
        h = torch.tanh(torch.randn((M, hd), generator=g))
        dh = h.cuda()
        z, rh = torch.full((M, hd), 3.0, device="cuda"), torch.full((M, hd), 3.0, device="cuda")
        d.aux_z, d.aux_rh, d.aux_h, d.ldh = z.data_ptr(), rh.data_ptr(), dh.data_ptr(), hd
        s = torch.sigmoid(v)
        ref = [s[:, :hd], s[:, hd:] * h.double()]
        outs = lambda: [z.cpu(), rh.cpu()]
    else:
        h = torch.tanh(torch.randn((M, cout), generator=g))
        zg = torch.rand((M, cout), generator=g)
        dh, dz = h.cuda(), zg.cuda()
        d.aux_z, d.aux_h, d.ldh = dz.data_ptr(), dh.data_ptr(), cout
        d.aux_rh = dx[0].data_ptr()
        ref = [(1 - zg.double()) * h.double() + zg.double() * torch.tanh(v)]
        outs = lambda: [dh.cpu()]

    st = _lib.lib().ofx_conv2d(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, st
    got = outs()
    for t, x0 in zip(dx, xs):
        assert torch.equal(t.cpu(), x0)                                    # the operands are only read
    return max((a.double() - r).abs().max().item() for a, r in zip(got, ref)), got


@pytest.mark.gpu
@pytest.mark.parametrize("segs,H,W,B,cout", SHAPES, ids=lambda v: "+".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("epi", [EPI_PLAIN, EPI_ZR, EPI_Q], ids=["plain", "zr", "q"])
@pytest.mark.parametrize("kh,kw", [(1, 5), (5, 1)])
def test_slab_pipeline_matches_float64(cuda, kh, kw, epi, segs, H, W, B, cout):
    cout = 256 if epi == EPI_ZR else 128 if epi == EPI_Q else cout
    seed = 1000 * kh + 100 * epi + sum(segs) + H + B
    e, got = _run(kh, kw, epi, segs, H, W, B, cout, seed)
    print(f"{kh}x{kw} epi {epi} cin {segs} map {H}x{W} B {B} Cout {cout}: max error {e:.3e} (bound {BOUND[epi]:.0e})")
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert e < BOUND[epi], e
    _, again = _run(kh, kw, epi, segs, H, W, B, cout, seed)
    assert all(torch.equal(a, b) for a, b in zip(got, again))              # repeats bit for bit
