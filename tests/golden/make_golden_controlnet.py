#!/usr/bin/env python3
"""Golden vectors of ControlNet, produced by the REAL reference code on the CPU in the build container:

    python tests/golden/make_golden_controlnet.py

Imports `controlnet.ControlNet` and `controlnet.apply_multi_controlnet` from /root/reference (imported from where they lie, nothing
copied), builds configuration `c0` (tests/controlnet_check.C0, the ControlNet twin of unet_check.U0: in 4, hint 3, model_channels
64, channel_mult [1, 2, 3], one ResBlock per level, attention at ds 1 and 2, one head, context 64, legacy False, use_checkpoint
False; 4.50 M parameters in 172 tensors), loads `random_controlnet_state_dict(0, C0)` into it with strict key matching (so keys and
shapes are the reference's) and stores in tests/golden/controlnet_ref_c0.npz, for B = 2, an 8 x 12 latent, a 64 x 96 hint, 9
context tokens and timesteps (981, 17):
    the inputs (the hint as the seed of `controlnet_check.c0_inputs` and its float64 sum: uniform noise does not compress);
    `guided_hint`; the seven residuals with a hint of batch 2 and again with a hint of batch 1 (image 0's map); the key
    names and shapes; the residuals of a second net (seed 1) on the same inputs; for the two nets (weights 0.7 / 0.3, windows
    [0, 1] and [0, 0.9]) the output of the reference's own
    `apply_multi_controlnet` at denoise_percentage 0.5 and 0.95, with `c.net` and `c.result` preset from the modules' outputs, so its
    mixing code runs but its loaders and cv2 do not; and, per stored output, the measured distance between the reference's fp32
    module and the float64 restatement (tests/controlnet_check.py): the yardstick of which the device's bar is four times.
Weights are regenerated from seeds, never stored.

controlnet.py imports more than it needs to build the module.  Stand-ins are registered in sys.modules before the import for what
is not installed: `cv2`, `omegaconf(.listconfig)`, `torchvision(.utils)`, `pytorch_lightning(.utilities.distributed)` with
LightningModule = nn.Module, `k_diffusion(.sampling)`, `controlnet_models(.hed)`, and the `xformers.ops` CPU attention of
make_golden_transformer.py.  None of them is called on the paths run here.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

sys.dont_write_bytecode = True      # importing make_golden_transformer must not leave a cache directory under tests/golden
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

import controlnet_check as CC   # noqa: E402
import transformer_check as TC   # noqa: E402
from make_golden_transformer import _register_xformers   # noqa: E402
from sd_animation_optical_flow_amd.controlnet import controlnet_layout, controlnet_tensors, random_controlnet_state_dict   # noqa: E402


def _module(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _unused(*a, **k):
    raise RuntimeError("a stand-in of make_golden_controlnet.py was called: this path is not meant to run")


def _register_stand_ins():
    _register_xformers()
    _module("cv2", Canny=_unused, imwrite=_unused)
    ListConfig = type("ListConfig", (), {})
    lc = _module("omegaconf.listconfig", ListConfig=ListConfig)
    _module("omegaconf", listconfig=lc, ListConfig=ListConfig, OmegaConf=type("OmegaConf", (), {}))
    tvu = _module("torchvision.utils", make_grid=_unused)
    _module("torchvision", utils=tvu)
    dist = _module("pytorch_lightning.utilities.distributed", rank_zero_only=lambda fn: fn)
    util = _module("pytorch_lightning.utilities", distributed=dist)
    _module("pytorch_lightning", LightningModule=nn.Module, utilities=util)
    kds = _module("k_diffusion.sampling")
    _module("k_diffusion", sampling=kds)
    hed = _module("controlnet_models.hed", apply_hed=_unused)
    _module("controlnet_models", hed=hed)


def build(ref, seed):
    cfg = CC.C0
    sd = random_controlnet_state_dict(seed, cfg)
    mod = ref.ControlNet(image_size=32, in_channels=cfg["in_channels"], hint_channels=cfg["hint_channels"],
                         model_channels=cfg["model_channels"], num_res_blocks=cfg["num_res_blocks"],
                         attention_resolutions=list(cfg["attention_resolutions"]), channel_mult=list(cfg["channel_mult"]),
                         num_heads=cfg["num_heads"], use_spatial_transformer=True, transformer_depth=1, context_dim=cfg["context_dim"],
                         use_checkpoint=False, legacy=False).eval()
    mod.load_state_dict(sd, strict=True)
    names = list(mod.state_dict().keys())
    assert names == list(sd.keys()) == [k for k, _ in controlnet_tensors(cfg)]
    return sd, mod


def main():
    _register_stand_ins()
    import controlnet as ref
    cfg = CC.C0
    lay = controlnet_layout(cfg)
    x, hint, t, context = CC.c0_inputs()
    store, dist = {}, {}

    def keep(name, got, ref64):
        store[name] = got.numpy()
        dist[name] = float((got.double() - ref64).abs().max())

    results, results64 = [], []
    with torch.no_grad():
        for seed, _, _, _ in CC.MIX_NETS:
            sd, mod = build(ref, seed)
            sd64 = TC.to64(sd)
            outs = [o.clone() for o in mod(x, hint, t, context)]
            outs64, guided64 = CC.controlnet64(sd64, lay, x, hint, t, context)
            results.append((mod, outs))
            results64.append(outs64)
            if seed != 0:                                                          # the second net of the mixes: its residuals only
                for i, (o, o64) in enumerate(zip(outs, outs64)):
                    keep(f"net{seed}_out{i}", o, o64)
                continue
            names = list(sd.keys())
            shapes = [tuple(sd[n].shape) for n in names]
            print(f"c0: {sum(v.numel() for v in sd.values()) / 1e6:.2f} M parameters in {len(names)} tensors")
            assert [tuple(o.shape) for o in outs] == CC.C0_SHAPES
            guided, _ = mod.input_hint_block(hint, None, None)
            keep("guided_hint", guided, guided64)
            for i, (o, o64) in enumerate(zip(outs, outs64)):
                keep(f"out{i}", o, o64)
            outs1 = mod(x, hint[:1], t, context)                                   # a hint of batch 1 broadcasts in h += guided_hint
            outs1_64, _ = CC.controlnet64(sd64, lay, x, hint[:1], t, context)
            for i, (o, o64) in enumerate(zip(outs1, outs1_64)):
                keep(f"out{i}_hint1", o, o64)
            assert not torch.equal(outs1[0], outs[0])
        # the reference's own mixing: c.net and c.result preset, so :414-419 (the loaders, cv2) are skipped and :420-432 run
        for p in CC.MIX_P:
            nets = [ref.SingleControlNet(weight=w, model="canny", args={}, condition=None, guidance_start=gs, guidance_end=ge,
                                         result=[o.clone() for o in outs], net=mod)
                    for (_, w, gs, ge), (mod, outs) in zip(CC.MIX_NETS, results)]
            mixed = ref.apply_multi_controlnet(x, t, context, p, nets)
            for i, (m, m64) in enumerate(zip(mixed, CC.mix64(results64, p))):
                keep(f"mix{int(round(p * 100))}_{i}", m, m64)
    for k_, d in dist.items():
        print(f"  {k_:14s} reference fp32 vs float64 restatement {d:.3e}   max |ref| {float(np.abs(store[k_]).max()):.3f}")
    shp = np.zeros((len(names), 4), dtype=np.int64)
    for i, s in enumerate(shapes):
        shp[i, :len(s)] = s
    keys = sorted(dist)
    path = os.path.join(HERE, "controlnet_ref_c0.npz")
    np.savez_compressed(path, x=x.numpy(), hint_seed=np.array(CC.C0_SEED), hint_sum=np.array(float(hint.double().sum())), timesteps=t.numpy(), context=context.numpy(), names=np.array(names),
                        shapes=shp, ndims=np.array([len(s) for s in shapes], dtype=np.int64), dist_keys=np.array(keys),
                        ref_vs_f64=np.array([dist[k_] for k_ in keys]), **store)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
