#!/usr/bin/env python3
"""Golden vectors of the UNet, produced by the REAL reference code on the CPU in the build container:

    python tests/golden/make_golden_unet.py

Imports `ldm.modules.diffusionmodules.openaimodel.UNetModel` from /root/reference (imported from where it lies, nothing copied),
builds configuration `u0` (tests/unet_check.U0: in 9, out 4, model_channels 64, channel_mult [1, 2, 3], one ResBlock per level,
attention at ds 1 and 2, one head, context 64, legacy False, use_checkpoint False; 8.7 M parameters in 326 tensors, seven
transformers with heads of 64, 128 and 192, ResBlock inputs of 384, 320, 192 and 128 channels), loads
`random_unet_state_dict(0, U0)` into it with strict key matching (so keys and shapes are the reference's) and stores in
tests/golden/unet_ref_u0.npz, for B = 2, an 8 x 12 latent, 9 context tokens and timesteps (981, 17):
    the inputs; the output and all seven (k, v) of a plain run; the output with reference K/V of batch B (the plain run's history
    with the two images swapped); the output with reference K/V of batch B - 1 (image 0's history); the output with seeded `control`
    residuals for only_mid_control False and True; the outputs of three ResBlocks run alone (unet_check.RESBLOCK_CASES); the key
    names and shapes; and, per output, the measured distance between the reference's fp32 module and the float64 restatement
    (tests/unet_check.py): the yardstick of which the device's bar is four times.
Weights, reference K/V, control residuals and the ResBlocks' inputs are regenerated from seeds or from stored arrays, never stored.

Two stand-ins are registered before the import: `xformers.ops` (not installed; a few-line CPU softmax attention, as
make_golden_transformer.py does) and an empty `omegaconf.listconfig.ListConfig` (not installed; the class is only compared by type at
openaimodel.py:482).  controlnet.py cannot be imported here (cv2, k_diffusion and pytorch_lightning are absent), so `run` below drives
the reference's own `input_blocks` / `middle_block` / `output_blocks` (`TimestepEmbedSequential`, whose forward does the
`reference_kv` routing, openaimodel.py:79-90) and restates the loop of `ControlledUnetModel.forward`, controlnet.py:33-62, line by
line -- including its pops: the lists are rebuilt for every run.

On the CPU `k.cpu()` (attention.py:353) is the tensor itself, so in the batch B - 1 run `k[nhead:] = k2` also overwrites the returned
kv_hist: only the plain run's history is stored.
"""
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True      # importing make_golden_transformer must not leave a cache directory under tests/golden
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

import transformer_check as TC   # noqa: E402
import unet_check as UC   # noqa: E402
from make_golden_transformer import _register_xformers   # noqa: E402
from sd_animation_optical_flow_amd.unet import random_unet_state_dict, unet_layout, unet_tensors   # noqa: E402


def _register_omegaconf():
    oc, lc = types.ModuleType("omegaconf"), types.ModuleType("omegaconf.listconfig")
    lc.ListConfig = type("ListConfig", (), {})
    oc.listconfig = lc
    sys.modules["omegaconf"], sys.modules["omegaconf.listconfig"] = oc, lc


def run(mod, x, timesteps, context, control=None, only_mid_control=False, reference_kv=()):
    """ControlledUnetModel.forward (controlnet.py:33-62) over the reference's own blocks; with control None the additions are
    skipped, which is UNetModel.forward (openaimodel.py:769-793) with reference_kv passed on."""
    from ldm.modules.diffusionmodules.util import timestep_embedding
    reference_kv = [[(k, v) for k, v in f] for f in reference_kv]                 # popped below (openaimodel.py:86)
    control = None if control is None else [c.clone() for c in control]
    hs, kv_hists = [], []
    t_emb = timestep_embedding(timesteps, mod.model_channels, repeat_only=False)    # :36
    emb = mod.time_embed(t_emb)                                                     # :37
    h = x.type(mod.dtype)                                                           # :38
    for module in mod.input_blocks:                                                 # :39-44
        h, cur = module(h, emb, context, reference_kv=reference_kv)
        kv_hists.extend(cur)
        hs.append(h)
    h, cur = mod.middle_block(h, emb, context, reference_kv=reference_kv)           # :46
    kv_hists.extend(cur)
    if control is not None:
        h = h + control.pop()                                                       # :50
    for module in mod.output_blocks:                                                # :52-59
        if only_mid_control or control is None:
            h = torch.cat([h, hs.pop()], dim=1)
        else:
            h = torch.cat([h, hs.pop() + control.pop()], dim=1)
        h, cur = module(h, emb, context, reference_kv=reference_kv)
        kv_hists.extend(cur)
    return mod.out(h), kv_hists                                                     # :62


def main():
    _register_xformers()
    _register_omegaconf()
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from ldm.modules.diffusionmodules.util import timestep_embedding
    cfg = UC.U0
    sd = random_unet_state_dict(0, cfg)
    mod = UNetModel(image_size=32, in_channels=cfg["in_channels"], model_channels=cfg["model_channels"], out_channels=cfg["out_channels"],
                    num_res_blocks=cfg["num_res_blocks"], attention_resolutions=list(cfg["attention_resolutions"]),
                    channel_mult=list(cfg["channel_mult"]), num_heads=cfg["num_heads"], use_spatial_transformer=True,
                    transformer_depth=1, context_dim=cfg["context_dim"], use_checkpoint=False, legacy=False).eval()
    mod.load_state_dict(sd, strict=True)
    names = list(mod.state_dict().keys())
    assert names == list(sd.keys()) == [k for k, _ in unet_tensors(cfg)]
    print(f"u0: {sum(v.numel() for v in sd.values()) / 1e6:.2f} M parameters in {len(names)} tensors")
    lay = unet_layout(cfg)
    heads = UC.transformer_heads(lay)
    x, t, context = UC.u0_inputs()
    ctl = UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)
    sd64 = TC.to64(sd)
    store, dist = {}, {}

    def keep(name, got, ref64):
        store[name] = got.numpy()
        dist[name] = float((got.double() - ref64).abs().max())

    with torch.no_grad():
        out, hist = run(mod, x, t, context)
        hist = [(k.clone(), v.clone()) for k, v in hist]
        assert len(hist) == len(heads) == 7
        ref, hist64 = UC.unet64(sd64, lay, x, t, context)
        keep("out", out, ref)
        for i, ((k, v), (k64, v64), h) in enumerate(zip(hist, hist64, heads)):
            keep(f"k{i}", k, TC.heads_first(k64, h))
            keep(f"v{i}", v, TC.heads_first(v64, h))
        for mode, tag in (("all", "out_refall"), ("positive", "out_refpos")):
            frames = UC.reference_frames(hist, heads, mode)
            got, _ = run(mod, x, t, context, reference_kv=frames)
            f64 = [[(TC.heads_last(k, h).double(), TC.heads_last(v, h).double()) for (k, v), h in zip(frames[0], heads)]]
            keep(tag, got, UC.unet64(sd64, lay, x, t, context, reference_kv=f64)[0])
            assert not torch.equal(got, out)
        for mid, tag in ((False, "out_ctl"), (True, "out_ctl_mid")):
            got, _ = run(mod, x, t, context, control=ctl, only_mid_control=mid)
            keep(tag, got, UC.unet64(sd64, lay, x, t, context, control=ctl, only_mid_control=mid)[0])
            assert not torch.equal(got, out)
        assert not np.array_equal(store["out_ctl"], store["out_ctl_mid"])
        # ResBlocks alone, the reference's own modules of the same model
        emb = mod.time_embed(timestep_embedding(t, mod.model_channels, repeat_only=False))
        emb64 = UC.time_embed64(sd64, t, cfg["model_channels"])
        for ci, (tag, name, _, up) in enumerate(UC.RESBLOCK_CASES):
            xb, skip = UC.resblock_inputs(ci)
            xin = xb if skip is None else torch.cat([xb, skip], dim=1)
            blocks = getattr(mod, name.split(".")[0])[int(name.split(".")[1])]
            got = blocks[int(name.split(".")[2])](xin, emb)
            r64 = UC.resblock64(sd64, name, xin.double(), emb64)
            if up is not None:
                got = blocks[int(up.split(".")[2])](got)
                r64 = UC.upsample64(sd64, up, r64)
            keep(f"rb{ci}", got, r64)
    for k_, d in dist.items():
        print(f"  {k_:12s} reference fp32 vs float64 restatement {d:.3e}   max |ref| {float(np.abs(store[k_]).max()):.3f}")
    shapes = [tuple(sd[n].shape) for n in names]
    shp = np.zeros((len(names), 4), dtype=np.int64)
    for i, s in enumerate(shapes):
        shp[i, :len(s)] = s
    keys = sorted(dist)
    path = os.path.join(HERE, "unet_ref_u0.npz")
    np.savez_compressed(path, x=x.numpy(), timesteps=t.numpy(), context=context.numpy(), names=np.array(names), shapes=shp,
                        ndims=np.array([len(s) for s in shapes], dtype=np.int64), dist_keys=np.array(keys),
                        ref_vs_f64=np.array([dist[k_] for k_ in keys]), **store)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
