#!/usr/bin/env python3
"""The reference's own arithmetic for the diffusion stage, measured: its UNet under torch.autocast, run by the REAL reference code
on the CPU in the build container:

    python tests/golden/make_golden_unet_autocast.py

The reference runs its whole Stable Diffusion stage under `torch.autocast(enabled=True, device_type='cuda')` (ofgen.py:104,
ofgen_keyframe_inpaint.py:212,273, ofgen_pixel_inpaint.py:193,234): convolutions and Linears take half operands and give half
results, attention runs in half.  This script loads `random_unet_state_dict(0, U0)` into the reference's `UNetModel` exactly as
make_golden_unet.py does (its `run` and its stand-ins are reused, nothing of the reference is copied) and runs the five stored
scenarios of unet_ref_u0.npz -- plain, reference K/V of batch B and of batch B - 1 (frames rebuilt from the stored fp32 history, as
the GPU tests rebuild them), `control` with only_mid_control False and True -- under
`torch.autocast(device_type="cpu", dtype=torch.float16)`, the same casting policy on the device this container has.

Stored in tests/golden/unet_ref_u0_autocast.npz, per output (the five `out*` and the seven (k, v) of the plain run):
    the autocast output as float32, and its distance (max |difference|) from the float64 restatement `unet_check.unet64`.
That distance is the yardstick of `UNetModel(precision="fp16")`: the reference's own mode for this stage against the truth.  The
device performs a subset of autocast's roundings (operands of the contractions only; activations, attention and every output stay
fp32), so it is held to twice that distance (tests/test_gpu_unet_precision.py).
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_unet as MG   # noqa: E402  (puts the repository, tests/ and the reference on sys.path)
import transformer_check as TC   # noqa: E402
import unet_check as UC   # noqa: E402
from make_golden_transformer import _register_xformers   # noqa: E402
from sd_animation_optical_flow_amd.unet import random_unet_state_dict, unet_layout   # noqa: E402

OUT_KEYS = ("out", "out_refall", "out_refpos", "out_ctl", "out_ctl_mid")


def main():
    _register_xformers()
    MG._register_omegaconf()
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    cfg = UC.U0
    sd = random_unet_state_dict(0, cfg)
    mod = UNetModel(image_size=32, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"], out_channels=cfg["out_channels"],
                    num_res_blocks=cfg["num_res_blocks"], attention_resolutions=list(cfg["attention_resolutions"]),
                    channel_mult=list(cfg["channel_mult"]), num_heads=cfg["num_heads"], use_spatial_transformer=True,
                    transformer_depth=1, context_dim=cfg["context_dim"], use_checkpoint=False, legacy=False).eval()
    mod.load_state_dict(sd, strict=True)
    gold = np.load(os.path.join(HERE, "unet_ref_u0.npz"))
    lay = unet_layout(cfg)
    heads = UC.transformer_heads(lay)
    x, t, context = (torch.from_numpy(gold[n]) for n in ("x", "timesteps", "context"))
    ctl = UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)
    hist32 = [(torch.from_numpy(gold[f"k{i}"]), torch.from_numpy(gold[f"v{i}"])) for i in range(len(heads))]
    sd64 = TC.to64(sd)
    store, dist = {}, {}

    def keep(name, got, ref64):
        got = got.detach().float()
        store[name] = got.numpy().copy()
        dist[name] = float((got.double() - ref64).abs().max())

    def auto(**kw):
        with torch.no_grad(), torch.autocast(device_type="cpu", dtype=torch.float16):
            return MG.run(mod, x, t, context, **kw)

    out, hist = auto()
    assert out.dtype == torch.float16, out.dtype                  # the last convolution ran under autocast
    ref, hist64 = UC.unet64(sd64, lay, x, t, context)
    keep("out", out, ref)
    for i, ((k, v), (k64, v64), h) in enumerate(zip(hist, hist64, heads)):
        keep(f"k{i}", k, TC.heads_first(k64, h))
        keep(f"v{i}", v, TC.heads_first(v64, h))
    for mode, tag in (("all", "out_refall"), ("positive", "out_refpos")):
        frames = UC.reference_frames(hist32, heads, mode)
        f64 = [[(TC.heads_last(k, h).double(), TC.heads_last(v, h).double()) for (k, v), h in zip(frames[0], heads)]]
        keep(tag, auto(reference_kv=frames)[0], UC.unet64(sd64, lay, x, t, context, reference_kv=f64)[0])
    for mid, tag in ((False, "out_ctl"), (True, "out_ctl_mid")):
        keep(tag, auto(control=ctl, only_mid_control=mid)[0], UC.unet64(sd64, lay, x, t, context, control=ctl, only_mid_control=mid)[0])
    keys = sorted(dist)
    for k_ in keys:
        print(f"  {k_:12s} reference under autocast vs float64 restatement {dist[k_]:.3e}   fp32 module {float(gold['ref_vs_f64'][list(gold['dist_keys']).index(k_)]):.3e}"
              f"   max |ref| {float(np.abs(store[k_]).max()):.3f}")
    path = os.path.join(HERE, "unet_ref_u0_autocast.npz")
    np.savez_compressed(path, dist_keys=np.array(keys), autocast_vs_f64=np.array([dist[k_] for k_ in keys]), **store)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
