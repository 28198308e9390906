#!/usr/bin/env python3
"""Golden vectors of the first-stage decoder, produced by the REAL reference code in the build container:

    python tests/golden/make_golden_vae_decoder.py

Imports `ldm.modules.diffusionmodules.model.Decoder` from /root/reference (imported from where it lies, nothing copied), builds
the SD-v1 decoder of guided_ldm_inpaint4_v15.yaml, loads `random_vae_decoder_state_dict(0)` into it with strict key matching (so
keys and shapes are the reference's), applies `post_quant_conv` like AutoencoderKL.decode and stores in
tests/golden/vae_dec_ref_8x6.npz: the latent z [1,4,8,6], the fp32 image [1,3,64,48], the BGR byte frame by decode_latent's
expression (ofgen_keyframe_inpaint.py:234-235), the key names and shapes in the module's order, and the measured distance between
the fp32 module and the float64 restatement (tests/vae_decoder_check.py), which must stay within a quarter of the tests' bar
2e-4 * max(1, max|ref|).  The weights (198 MB) are regenerated from the seed, never stored.  xformers is not installed here, so
the reference takes its `AttnBlock` (vanilla attention).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

import vae_decoder_check as VC   # noqa: E402
from sd_animation_optical_flow_amd.vae import random_vae_decoder_state_dict   # noqa: E402


def main():
    from ldm.modules.diffusionmodules.model import Decoder
    dd = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
              num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    dec = Decoder(**dd).eval()
    sd = random_vae_decoder_state_dict(0)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=True)
    names = ["decoder." + k for k in dec.state_dict().keys()] + ["post_quant_conv.weight", "post_quant_conv.bias"]
    shapes = [tuple(sd[k].shape) for k in names]
    assert sorted(names) == sorted(sd.keys())
    z = torch.randn((1, 4, 8, 6), generator=torch.Generator().manual_seed(31))
    with torch.no_grad():
        image = dec(torch.nn.functional.conv2d(z, sd["post_quant_conv.weight"], sd["post_quant_conv.bias"]))
    frame = VC.to_u8_bgr(image)
    ref64 = VC.decode64(VC.to64(sd), z)
    dist = float((image.double() - ref64).abs().max())
    bar = 2e-4 * max(1.0, float(image.abs().max()))
    print(f"reference fp32 vs float64 restatement: max |d| = {dist:.3e}; bar {bar:.3e}; max |image| = {float(image.abs().max()):.3f}")
    assert dist <= bar / 4, (dist, bar)
    shp = np.zeros((len(names), 4), dtype=np.int64)
    for i, s in enumerate(shapes):
        shp[i, :len(s)] = s
    np.savez_compressed(os.path.join(HERE, "vae_dec_ref_8x6.npz"), z=z.numpy(), image=image.numpy(), frame_bgr=frame,
                        names=np.array(names), shapes=shp, ndims=np.array([len(s) for s in shapes], dtype=np.int64),
                        ref_vs_f64=np.array([dist]))


if __name__ == "__main__":
    main()
