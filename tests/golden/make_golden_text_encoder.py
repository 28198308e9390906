#!/usr/bin/env python3
"""Golden vectors of the CLIP text encoder, produced by the REAL reference code on the CPU in the build container:

    python tests/golden/make_golden_text_encoder.py

Imports `ldm.modules.encoders.modules.FrozenCLIPEmbedder` and `hack._hacked_clip_forward` from /root/reference (imported from where
they lie, nothing copied) and runs the reference's forward on configuration `t0` (tests/text_encoder_check.T0: vocabulary 512,
width 128, two heads of 64, three layers, MLP 512, 77 positions) for the two prompts of `text_encoder_check.t0_inputs` (100 and 5
raw ids) with clip_skip 0, 2 and 3.  Stored in tests/golden/clip_text_ref_t0.npz:
    the prompts' raw ids; the [2,3,77] token tensor the reference actually fed its transformer, captured at the call; the three
    [2,231,128] outputs; the key names and shapes of the transformer's state dict; and per output `ref_dist`, the max abs distance
    between the reference's fp32 output and the float64 restatement (tests/text_encoder_check.py): the yardstick of which the
    device's bar is four times.
Weights are regenerated from the seed (`random_clip_text_state_dict(0, T0)`), never stored.

How the embedder is built without a download.  `FrozenCLIPEmbedder.__init__` calls `from_pretrained` twice, so the instance is
made with `FrozenCLIPEmbedder.__new__` + `nn.Module.__init__`; `.transformer` is transformers' `CLIPTextModel(CLIPTextConfig(...t0...,
hidden_act="quick_gelu"))` loaded strictly from the seeded state dict (so keys and shapes are the library's), `.tokenizer` a stub
that parses space-separated integers and carries the three special ids (the second prompt is written with '_' between its ids, so
the reference's `replace('_', ' ')` runs).  With clip_skip 0 the reference's forward runs as it is.  With clip_skip > 1 it reads
`self.transformer.text_model.final_layer_norm` (hack.py:45), and the CLIPTextModel of the transformers installed here (5.15) has no
`.text_model`: the instance is given a `text_model` stand-in whose `final_layer_norm` is the model's own -- the model itself, set
with `object.__setattr__`, because a plain assignment would register the module as its own child.

Stand-ins registered in sys.modules before the import for what is not installed: `open_clip` (imported by
ldm/modules/encoders/modules.py, used only by FrozenOpenCLIPEmbedder) and the `xformers.ops` CPU attention of
make_golden_transformer.py (hack.py imports ldm.modules.attention).  Neither is called on the paths run here.
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

import text_encoder_check as XC   # noqa: E402
from make_golden_transformer import _register_xformers   # noqa: E402
from sd_animation_optical_flow_amd.text_encoder import clip_text_tensors, random_clip_text_state_dict   # noqa: E402


def _unused(*a, **k):
    raise RuntimeError("a stand-in of make_golden_text_encoder.py was called: this path is not meant to run")


class _Tokenizer:
    """Space-separated integers are the ids; the interface hack.py:33-40 uses."""
    bos_token_id, eos_token_id, pad_token_id = XC.T0_BOS, XC.T0_EOS, XC.T0_PAD

    def __call__(self, texts, truncation=False, add_special_tokens=False):
        assert truncation is False and add_special_tokens is False
        return {"input_ids": [[int(s) for s in t.split()] for t in texts]}


def main():
    _register_xformers()
    oc = types.ModuleType("open_clip")
    oc.create_model_and_transforms = _unused
    sys.modules["open_clip"] = oc
    from transformers import CLIPTextConfig, CLIPTextModel
    import hack
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder

    cfg = XC.T0
    sd = random_clip_text_state_dict(0, cfg)
    model = CLIPTextModel(CLIPTextConfig(vocab_size=cfg["vocab"], hidden_size=cfg["width"], intermediate_size=cfg["intermediate"],
                                         num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                                         max_position_embeddings=cfg["positions"], hidden_act="quick_gelu", bos_token_id=XC.T0_BOS,
                                         eos_token_id=XC.T0_EOS, pad_token_id=XC.T0_PAD)).eval()
    model.load_state_dict(sd, strict=True)
    names = [k for k, _ in model.named_parameters()]
    assert names == list(sd.keys()) == [k for k, _ in clip_text_tensors(cfg)]
    shapes = [tuple(sd[n].shape) for n in names]
    object.__setattr__(model, "text_model", model)                 # hack.py:45 (docstring)

    emb = FrozenCLIPEmbedder.__new__(FrozenCLIPEmbedder)
    nn.Module.__init__(emb)
    emb.transformer, emb.tokenizer, emb.device, emb.max_length = model, _Tokenizer(), "cpu", 77
    fed = []
    model.register_forward_pre_hook(lambda m, args, kwargs: fed.append(kwargs["input_ids"].clone()), with_kwargs=True)

    raw = XC.t0_inputs()
    texts = [" ".join(str(v) for v in raw[0]), "_".join(str(v) for v in raw[1])]
    sd64 = XC.to64(sd)
    store, dist = {}, {}
    with torch.no_grad():
        for skip in XC.T0_SKIPS:
            emb.clip_skip = skip
            z = hack._hacked_clip_forward(emb, texts)
            assert tuple(z.shape) == (2, 231, cfg["width"]) and z.dtype == torch.float32
            tokens = fed[-1].reshape(2, 3, 77)
            z64 = XC.forward_tokens64(sd64, cfg, tokens, skip)
            store[f"out_skip{skip}"] = z.numpy()
            dist[f"out_skip{skip}"] = float((z.double() - z64).abs().max())
            print(f"  clip_skip {skip}: reference fp32 vs float64 restatement {dist[f'out_skip{skip}']:.3e}   max |ref| {float(z.abs().max()):.3f}")
    assert all(torch.equal(f, fed[0]) for f in fed) and fed[0].dtype == torch.int32
    assert not np.array_equal(store["out_skip0"], store["out_skip2"]) and not np.array_equal(store["out_skip2"], store["out_skip3"])
    shp = np.zeros((len(names), 2), dtype=np.int64)
    for i, s in enumerate(shapes):
        shp[i, :len(s)] = s
    raw_pad = np.full((len(raw), max(len(r) for r in raw)), -1, dtype=np.int64)
    for i, r in enumerate(raw):
        raw_pad[i, :len(r)] = r
    keys = sorted(dist)
    path = os.path.join(HERE, "clip_text_ref_t0.npz")
    np.savez_compressed(path, raw_ids=raw_pad, raw_len=np.array([len(r) for r in raw], dtype=np.int64),
                        tokens=fed[0].reshape(2, 3, 77).numpy(), names=np.array(names), shapes=shp,
                        ndims=np.array([len(s) for s in shapes], dtype=np.int64), dist_keys=np.array(keys),
                        ref_dist=np.array([dist[k] for k in keys]), **store)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
