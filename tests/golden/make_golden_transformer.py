#!/usr/bin/env python3
"""Golden vectors of `SpatialTransformer`, produced by the REAL reference code on the CPU in the build container:

    python tests/golden/make_golden_transformer.py

Imports `ldm.modules.attention.SpatialTransformer` from /root/reference (imported from where it lies, nothing copied), builds it
with use_checkpoint=False, loads `random_spatial_transformer_state_dict(0, ...)` into it with strict key matching (so keys and shapes
are the reference's) and stores in tests/golden/spatial_transformer_ref_{c0,c1}.npz (one file per configuration: together they
would pass the repository's size limit for one file), for
    c0: C = 320, 8 heads of 40, context 768, a 6x5 map, B = 2, 77 context tokens
    c1: C = 128, 2 heads of 64, context 64, a 12x11 map, B = 2, 9 context tokens
the input, the context, the output and kv_hist of a plain run; the output of a run with reference_kv of batch B; the output of a
run with reference_kv of batch B - 1; the key names and shapes in the module's order; and the measured distance between the fp32
module and the float64 restatement (tests/transformer_check.py), which must stay within a quarter of the tests' bar
2e-4 * max(1, max|ref|).  The weights are regenerated from the seed, never stored, and neither are the reference K/V, which are
taken from the stored kv_hist: for batch B the plain run's own history with the two images swapped (`reference_all`: every image
attends to the other image's keys), for batch B - 1 the history of image 0 (`reference_positive`; a batch-1 run of that image is
made as well and must record the same history to 1e-5).

xformers is not installed here and the project's own `memory_efficient_attention` needs a GPU, so a few-line CPU stand-in (softmax
attention in the input's own precision) is registered as `xformers.ops` before the import.  On the CPU `k.cpu()` (:353) is the
tensor itself, so in the batch B - 1 run `k[nhead:] = k2` (:365) also overwrites the returned kv_hist: only the plain run's kv_hist
is stored (on a GPU the reference's history is a copy made before the replacement, which is what the project returns).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

import transformer_check as TC   # noqa: E402
from sd_animation_optical_flow_amd.transformer import random_spatial_transformer_state_dict   # noqa: E402

CONFIGS = {
    "c0": dict(C=320, heads=8, d=40, ctx=768, h=6, w=5, B=2, M=77),
    "c1": dict(C=128, heads=2, d=64, ctx=64, h=12, w=11, B=2, M=9),
}


def _cpu_attention(q, k, v, attn_bias=None, op=None):
    s = torch.einsum("bqd,bkd->bqk", q, k) * (q.shape[-1] ** -0.5)
    if attn_bias is not None:
        s = s + attn_bias
    return torch.einsum("bqk,bkd->bqd", torch.softmax(s, -1), v)


def _register_xformers():
    xf, xops = types.ModuleType("xformers"), types.ModuleType("xformers.ops")
    xops.memory_efficient_attention = _cpu_attention
    xf.ops = xops
    sys.modules["xformers"], sys.modules["xformers.ops"] = xf, xops


def main():
    _register_xformers()
    from ldm.modules.attention import SpatialTransformer
    for tag, c in CONFIGS.items():
        sd = random_spatial_transformer_state_dict(0, c["C"], c["heads"], c["d"], c["ctx"])
        mod = SpatialTransformer(c["C"], c["heads"], c["d"], depth=1, context_dim=c["ctx"], use_checkpoint=False).eval()
        mod.load_state_dict(sd, strict=True)
        names = list(mod.state_dict().keys())
        assert names == list(sd.keys())
        g = torch.Generator().manual_seed(77 + c["C"])
        x = torch.randn((c["B"], c["C"], c["h"], c["w"]), generator=g)
        context = torch.randn((c["B"], c["M"], c["ctx"]), generator=g)
        H = c["heads"]
        with torch.no_grad():
            out, hist = mod(x, context=context)
            k, v = (t.clone() for t in hist[0])
            ko, vo = TC.reference_all(k, v, H)
            out_all, _ = mod(x, context=context, reference_kv=[(ko, vo, 0)])
            k1, v1 = TC.reference_positive(k, v, H)
            _, hist_1 = mod(x[:1], context=context[:1])                            # the batch-1 run records the same history
            assert float((hist_1[0][0] - k1).abs().max()) <= 1e-5 and float((hist_1[0][1] - v1).abs().max()) <= 1e-5
            out_pos, _ = mod(x, context=context, reference_kv=[(k1.clone(), v1.clone(), 0)])
        # the float64 restatement on the same inputs
        sd64 = TC.to64(sd)
        ref, hist64 = TC.spatial_transformer64(sd64, x, H, context)
        ref_all, _ = TC.spatial_transformer64(sd64, x, H, context, [(TC.heads_last(ko, H), TC.heads_last(vo, H))])
        ref_pos, _ = TC.spatial_transformer64(sd64, x, H, context, [(TC.heads_last(k1, H), TC.heads_last(v1, H))])
        dist = max(float((a.double() - b).abs().max()) for a, b in ((out, ref), (out_all, ref_all), (out_pos, ref_pos)))
        dist_kv = max(float((k.double() - TC.heads_first(hist64[0][0], H)).abs().max()),
                      float((v.double() - TC.heads_first(hist64[0][1], H)).abs().max()))
        bar = min(TC.bar_of(t) for t in (out, out_all, out_pos, k, v))
        print(f"{tag}: reference fp32 vs float64 restatement: outputs {dist:.3e}, kv_hist {dist_kv:.3e}; bar {bar:.3e}; "
              f"max |out| {float(out.abs().max()):.3f}")
        assert max(dist, dist_kv) <= bar / 4, (dist, dist_kv, bar)
        assert not torch.equal(out, out_all) and not torch.equal(out, out_pos)
        shapes = [tuple(sd[n].shape) for n in names]
        shp = np.zeros((len(names), 4), dtype=np.int64)
        for i, s in enumerate(shapes):
            shp[i, :len(s)] = s
        path = os.path.join(HERE, f"spatial_transformer_ref_{tag}.npz")
        np.savez_compressed(path, cfg=np.array([c[n] for n in ("C", "heads", "d", "ctx", "h", "w", "B", "M")], dtype=np.int64),
                            x=x.numpy(), context=context.numpy(), out=out.numpy(), k=k.numpy(), v=v.numpy(),
                            out_refall=out_all.numpy(), out_refpos=out_pos.numpy(), names=np.array(names), shapes=shp,
                            ndims=np.array([len(s) for s in shapes], dtype=np.int64), ref_vs_f64=np.array([dist, dist_kv]))
        print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
