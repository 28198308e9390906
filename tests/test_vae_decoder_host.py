"""Host side of the first-stage decoder (no GPU): the state-dict layout against the reference module's own key list, the float64
restatement against the real `Decoder`'s output, and the parity-folded weights of the fused upsample convolution."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_decoder_check as VC   # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vae_dec_ref_8x6.npz")


def test_decoder_tensors_are_the_reference_modules_keys_and_shapes():
    from sd_animation_optical_flow_amd import vae
    g = np.load(GOLD)
    names = [str(n) for n in g["names"]]
    shapes = [tuple(int(v) for v in row[:nd]) for row, nd in zip(g["shapes"], g["ndims"])]
    mine = vae.decoder_tensors()
    assert [k for k, _ in mine] == names                       # module order, decoder.* then post_quant_conv.*
    assert [tuple(s) for _, s in mine] == shapes
    sd = vae.random_vae_decoder_state_dict(0)
    assert list(sd.keys()) == names and all(tuple(sd[k].shape) == s for k, s in zip(names, shapes))


def test_decoder_weights_have_their_own_generator():
    """The encoder's seeded tensors are what they were (the encoder golden depends on them) whether or not decoder weights are drawn,
    and the decoder's differ from seed to seed."""
    from sd_animation_optical_flow_amd import vae
    from oracle import vae_oracle as VO
    a = vae.random_vae_state_dict(0)
    d0 = vae.random_vae_decoder_state_dict(0)
    b = vae.random_vae_state_dict(0)
    ref = VO.init_vae_state_dict(0)
    assert list(a.keys()) == list(ref.keys())
    assert all(torch.equal(a[k], ref[k]) and torch.equal(b[k], ref[k]) for k in ref)
    d1 = vae.random_vae_decoder_state_dict(1)
    assert torch.equal(d0["decoder.conv_in.weight"], vae.random_vae_decoder_state_dict(0)["decoder.conv_in.weight"])
    assert not torch.equal(d0["decoder.conv_in.weight"], d1["decoder.conv_in.weight"])


def test_float64_restatement_against_the_reference_decoder():
    """The restatement on the golden latent against the REAL `Decoder`'s fp32 image: within a quarter of the GPU tests' bar (what
    the golden script asserted when it ran), and the byte frame by decode_latent's expression reproduces the stored one."""
    from sd_animation_optical_flow_amd import vae
    g = np.load(GOLD)
    ref = torch.from_numpy(g["image"])
    out = VC.decode64(VC.to64(vae.random_vae_decoder_state_dict(0)), torch.from_numpy(g["z"]))
    assert tuple(out.shape) == tuple(ref.shape) == (1, 3, 64, 48)
    bar = 2e-4 * max(1.0, ref.abs().max().item())
    dist = (out - ref.double()).abs().max().item()
    assert dist <= bar / 4, (dist, bar)
    assert abs(dist - float(g["ref_vs_f64"][0])) <= 1e-6       # the figure the fixture recorded (thread counts move the last bits)
    assert np.array_equal(VC.to_u8_bgr(ref), g["frame_bgr"])
    assert g["frame_bgr"].shape == (64, 48, 3) and g["frame_bgr"].dtype == np.uint8


def test_upconv2x_weight_folds_the_taps_per_parity():
    """ofx_upconv2x_weight through the library: the four folded 2x2 convolutions on the low-resolution map equal interpolate +
    conv2d in float64.  The folded weights are float64 sums rounded once to fp32, so each differs from the exact sum by at most
    2^-24 of its magnitude; the outputs then differ by at most 2^-24 * conv(|x|, |w folded|) (1 + 1e-6: |exact| <= |folded| /
    (1 - 2^-24), and the float64 roundings of two 4-to-9-term sums, ~1e-15 relative)."""
    from sd_animation_optical_flow_amd import ops
    g = torch.Generator().manual_seed(5)
    for (co, ci, H, W) in ((8, 4, 5, 7), (3, 12, 1, 1), (16, 8, 2, 9)):
        w = torch.randn((co, ci, 3, 3), generator=g)
        x = torch.randn((2, ci, H, W), generator=g).double()
        wf = ops.upconv2x_weight(w)
        assert tuple(wf.shape) == (4, co, 4, ci) and wf.dtype == torch.float32
        # the exact folds, in float64
        w64 = w.double()
        rows = {0: (w64[:, :, 0:1], w64[:, :, 1:2] + w64[:, :, 2:3]), 1: (w64[:, :, 0:1] + w64[:, :, 1:2], w64[:, :, 2:3])}
        ref = VC.upconv64(x, w)
        out = torch.zeros_like(ref)
        bound = torch.zeros_like(ref)
        for py in (0, 1):
            for px in (0, 1):
                r = torch.cat(rows[py], dim=2)                                              # [co, ci, 2, 3]
                exact = torch.cat([r[..., 0:1], r[..., 1:2] + r[..., 2:3]] if px == 0 else [r[..., 0:1] + r[..., 1:2], r[..., 2:3]], dim=3)
                k = wf[2 * py + px].reshape(co, 2, 2, ci).permute(0, 3, 1, 2).double()       # OIHW 2x2, tap = 2 ty + tx
                assert (k - exact).abs().le(exact.abs() * 2.0 ** -24).all()                  # rounded once
                # taps over low-resolution rows y - 1 + py + {0, 1}: pad one row / column on the side the parity looks at
                xp = F.pad(x, (1 - px, px, 1 - py, py))
                out[:, :, py::2, px::2] = F.conv2d(xp, k)
                bound[:, :, py::2, px::2] = F.conv2d(xp.abs(), k.abs())
        assert (out - ref).abs().le(bound * 2.0 ** -24 * (1 + 1e-6)).all()
    L = ops._lib.lib()
    assert L.ofx_upconv2x_weight(None, 5, 7, None) == 16 * 5 * 7
    assert L.ofx_upconv2x_weight(None, 0, 4, None) < 0
