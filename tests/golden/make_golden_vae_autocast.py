#!/usr/bin/env python3
"""The reference's own arithmetic for the first stage, measured: its VAE under torch.autocast, run by the REAL reference code on the
CPU in the build container:

    python tests/golden/make_golden_vae_autocast.py

The reference runs its whole diffusion stage under `torch.autocast(enabled=True, device_type='cuda')` (ofgen.py:104,
ofgen_keyframe_inpaint.py:212,273): the VAE encode before the sampler and the VAE decodes after it take half operands and give half
results.  This script loads `random_vae_decoder_state_dict(0)` into the reference's `Decoder` and
`oracle.vae_oracle.init_vae_state_dict(0)` into its `Encoder` exactly as make_golden_vae_decoder.py / make_golden_vae.py do (nothing
of the reference is copied), and runs them, with `post_quant_conv` / `quant_conv`, under
`torch.autocast(device_type="cpu", dtype=torch.float16)`, the same casting policy on the device this container has.

Cases: the stored inputs of vae_dec_ref_8x6.npz (z [1,4,8,6]) and vae_ref_64x48.npz (image [1,3,64,48]), and one second case each
with B = 2 and sides that are no multiple of a tile: z [2,4,6,10] and an image [2,3,40,56], stored here.

Stored in tests/golden/vae_ref_autocast.npz, per case:
    autocast_vs_f64   max |reference under autocast - float64|; the float64 side is `vae_decoder_check.decode64` for the decoder and
                      `vae_oracle.encode_moments` on a float64 state dict for the encoder.  The yardstick of
                      `VaeDecoder(precision="fp16")` / `VaeEncoder(precision="fp16")`: the device performs a subset of autocast's
                      roundings (the operands of the convolutions only), so it is held to twice that distance
                      (tests/test_gpu_vae_f16.py), the bar of tests/test_gpu_unet_precision.py.
    emulated_vs_f64   the same network in fp32 on the CPU with only the convolutions' operands rounded to half: what the device's
                      arithmetic alone costs.  A quarter of it is the floor that shows the half arithmetic ran.
    fp32_vs_f64       the same network in plain fp32, for scale.
The script asserts emulated / autocast <= 1.5 for every case, so the device bar (2 x autocast) has margin from the reference alone.
"""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

import vae_decoder_check as VC   # noqa: E402
from oracle import vae_oracle as VO   # noqa: E402
from sd_animation_optical_flow_amd.vae import random_vae_decoder_state_dict   # noqa: E402

CASES = ("dec_8x6", "dec_b2_6x10", "enc_64x48", "enc_b2_40x56")
RATIO_CAP = 1.5
DD = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4], num_res_blocks=2,
          attn_resolutions=[], dropout=0.0)


@contextlib.contextmanager
def half_operand_convs():
    """Inside: every F.conv2d of the functional restatements rounds its input and its weight to half (nearest even) and contracts
    them in fp32 with an fp32 bias -- the arithmetic of the device's "fp16" convolutions up to the order of the fp32 sums."""
    real = F.conv2d

    def conv2d(x, w, b=None, *args, **kw):
        return real(x.half().float(), w.half().float(), None if b is None else b.float(), *args, **kw)

    F.conv2d = conv2d
    try:
        yield
    finally:
        F.conv2d = real


def second_inputs():
    z2 = torch.randn((2, 4, 6, 10), generator=torch.Generator().manual_seed(32))
    g = torch.Generator().manual_seed(13)
    H, W = 40, 56
    base = F.avg_pool2d(torch.rand((2, 3, H + 8, W + 8), generator=g), 5, 1, 2)[:, :, 4:4 + H, 4:4 + W]
    return z2, (base - base.min()) / (base.max() - base.min()) * 2 - 1


def main():
    from ldm.modules.diffusionmodules.model import Decoder, Encoder
    dsd = random_vae_decoder_state_dict(0)
    dec = Decoder(**DD).eval()
    dec.load_state_dict({k[len("decoder."):]: v for k, v in dsd.items() if k.startswith("decoder.")}, strict=True)
    esd = VO.init_vae_state_dict(0)
    enc = Encoder(**DD).eval()
    enc.load_state_dict({k[len("encoder."):]: v for k, v in esd.items() if k.startswith("encoder.")}, strict=True)
    dsd64, esd64 = VC.to64(dsd), {k: v.double() for k, v in esd.items()}
    z2, image2 = second_inputs()
    inputs = {"dec_8x6": torch.from_numpy(np.load(os.path.join(HERE, "vae_dec_ref_8x6.npz"))["z"]), "dec_b2_6x10": z2,
              "enc_64x48": torch.from_numpy(np.load(os.path.join(HERE, "vae_ref_64x48.npz"))["image"]), "enc_b2_40x56": image2}

    def decode_ref(z):
        return dec(F.conv2d(z, dsd["post_quant_conv.weight"], dsd["post_quant_conv.bias"]))

    def encode_ref(image):
        return F.conv2d(enc(image), esd["quant_conv.weight"], esd["quant_conv.bias"])

    auto, emu, f32 = [], [], []
    with torch.no_grad():
        for name in CASES:
            x = inputs[name]
            is_dec = name.startswith("dec")
            ref64 = VC.decode64(dsd64, x) if is_dec else VO.encode_moments(esd64, x.double())
            module = decode_ref if is_dec else encode_ref
            with torch.autocast(device_type="cpu", dtype=torch.float16):
                got = module(x)
            assert got.dtype == torch.float16, got.dtype              # the last convolution ran under autocast
            plain = module(x)
            with half_operand_convs():
                em = VC.decode64(dsd, x.float()) if is_dec else VO.encode_moments(esd, x)
            assert em.dtype == torch.float32 and tuple(em.shape) == tuple(ref64.shape) == tuple(got.shape)
            d = lambda t: float((t.double() - ref64).abs().max())
            auto.append(d(got)), emu.append(d(em)), f32.append(d(plain))
            print(f"  {name:14s} autocast {auto[-1]:.3e}   emulated {emu[-1]:.3e}   ratio {emu[-1] / auto[-1]:.2f}   fp32 module {f32[-1]:.3e}"
                  f"   max |ref| {float(ref64.abs().max()):.3f}")
            assert emu[-1] / auto[-1] <= RATIO_CAP, (name, emu[-1], auto[-1])
            assert f32[-1] < 0.05 * emu[-1], (name, f32[-1])             # the half roundings, not fp32's, are what is measured
    path = os.path.join(HERE, "vae_ref_autocast.npz")
    np.savez_compressed(path, cases=np.array(CASES), autocast_vs_f64=np.array(auto), emulated_vs_f64=np.array(emu),
                        fp32_vs_f64=np.array(f32), ratio_cap=np.array([RATIO_CAP]), z_b2_6x10=z2.numpy(), image_b2_40x56=image2.numpy())
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
