"""Host side of `SpatialTransformer` (no GPU): the float64 restatement against the real reference module's stored outputs, the
state-dict layout against the module's own key list, the new C entry points in the built library, and the reference_kv batch
rules, which are decided from shapes alone."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import transformer_check as TC   # noqa: E402

TAGS = ("c0", "c1")


def gold(tag):
    return np.load(os.path.join(HERE, "golden", f"spatial_transformer_ref_{tag}.npz"))


def references(g, heads):
    """The reference K/V of the two stored runs, from the stored kv_hist (tests/golden/make_golden_transformer.py)."""
    k, v = torch.from_numpy(g["k"]), torch.from_numpy(g["v"])
    return TC.reference_all(k, v, heads), TC.reference_positive(k, v, heads)


@pytest.mark.parametrize("tag", TAGS)
def test_float64_restatement_against_the_reference_module(tag):
    """Every stored output of the REAL module within a quarter of the GPU tests' bar, and the distances the fixture recorded."""
    from sd_animation_optical_flow_amd import transformer as T
    g = gold(tag)
    C, heads, d, ctx, h, w, B, M = (int(v) for v in g["cfg"])
    sd64 = TC.to64(T.random_spatial_transformer_state_dict(0, C, heads, d, ctx))
    x, context = torch.from_numpy(g["x"]), torch.from_numpy(g["context"])
    assert tuple(x.shape) == (B, C, h, w) and tuple(context.shape) == (B, M, ctx)
    (ka, va), (kp, vp) = references(g, heads)
    out, hist = TC.spatial_transformer64(sd64, x, heads, context)
    out_all, hist_all = TC.spatial_transformer64(sd64, x, heads, context, [(TC.heads_last(ka, heads), TC.heads_last(va, heads))])
    out_pos, _ = TC.spatial_transformer64(sd64, x, heads, context, [(TC.heads_last(kp, heads), TC.heads_last(vp, heads))])
    worst = 0.0
    for mine, name in ((out, "out"), (out_all, "out_refall"), (out_pos, "out_refpos")):
        ref = torch.from_numpy(g[name])
        dist = float((mine - ref.double()).abs().max())
        worst = max(worst, dist)
        assert dist <= TC.bar_of(ref) / 4, (name, dist)
    worst_kv = 0.0
    for mine, name in ((hist[0][0], "k"), (hist[0][1], "v")):
        ref = torch.from_numpy(g[name])
        assert tuple(ref.shape) == (B * heads, h * w, d)
        dist = float((TC.heads_first(mine, heads) - ref.double()).abs().max())
        worst_kv = max(worst_kv, dist)
        assert dist <= TC.bar_of(ref) / 4, (name, dist)
    assert abs(worst - float(g["ref_vs_f64"][0])) <= 1e-6 and abs(worst_kv - float(g["ref_vs_f64"][1])) <= 1e-6
    # the history is the block's own K/V whatever it attends to, and image 0 keeps its own K/V in the batch B - 1 run
    assert torch.equal(hist_all[0][0], hist[0][0])
    assert torch.equal(out_pos[0], out[0]) and not torch.equal(out_pos[1], out[1]) and not torch.equal(out_all[0], out[0])


@pytest.mark.parametrize("tag", TAGS)
def test_spatial_transformer_tensors_are_the_reference_modules_keys_and_shapes(tag):
    from sd_animation_optical_flow_amd import transformer as T
    g = gold(tag)
    C, heads, d, ctx = (int(v) for v in g["cfg"][:4])
    names = [str(n) for n in g["names"]]
    shapes = [tuple(int(v) for v in row[:nd]) for row, nd in zip(g["shapes"], g["ndims"])]
    mine = T.spatial_transformer_tensors(C, heads, d, ctx)
    assert len(mine) == 26
    assert [k for k, _ in mine] == names and [tuple(s) for _, s in mine] == shapes
    sd = T.random_spatial_transformer_state_dict(0, C, heads, d, ctx)
    assert list(sd.keys()) == names and all(tuple(sd[k].shape) == s for k, s in zip(names, shapes))
    assert float(sd["proj_out.weight"].abs().max()) > 0                       # not the zero-initialised identity
    two = T.spatial_transformer_tensors(C, heads, d, ctx, depth=2)
    assert len(two) == 4 + 2 * 20 + 2 and two[24][0] == "transformer_blocks.1.attn1.to_q.weight"
    assert dict(T.spatial_transformer_tensors(C, heads, d, None))["transformer_blocks.0.attn2.to_k.weight"] == (heads * d, heads * d)


def test_library_exports_the_transformer_entry_points():
    from sd_animation_optical_flow_amd import _lib
    lib = _lib.lib()
    for name in ("ofx_layernorm", "ofx_geglu", "ofx_attention_bnhd_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # validation happens on the host before any launch: no device is needed to be turned away
    assert lib.ofx_layernorm(None, 4, None, None, None, 4, 1, 4, 1e-5, None) == TC.SC.EINVAL
    assert lib.ofx_geglu(None, 8, None, 4, 1, 4, None) == TC.SC.EINVAL
    assert lib.ofx_attention_bnhd_f32(None, 40, None, 40, None, 40, None, 0, None, 40, 1, 1, 1, 1, 40, 1.0, None) == TC.SC.EINVAL


def test_reference_kv_batch_rules():
    """attention.py:358-369 by shapes: batch B -> every image attends to the references alone; batch B - 1 with exactly N tokens ->
    images 1.. take them; everything else raises ValueError."""
    from sd_animation_optical_flow_amd.transformer import plan_reference_kv as plan
    B, N, H, D = 2, 30, 8, 40
    ours = lambda b, n: ((b, n, H * D), (b, n, H * D))
    theirs = lambda b, n: ((b * H, n, D), (b * H, n, D))
    assert plan([ours(2, 30)], B, N, H, D) == ("all", 30, [False])
    assert plan([theirs(2, 17), ours(2, 30)], B, N, H, D) == ("all", 47, [True, False])          # concatenated along tokens
    assert plan([theirs(1, 30)], B, N, H, D) == ("positive", 30, [True])
    assert plan([ours(1, 10), ours(1, 20)], B, N, H, D) == ("positive", 30, [False, False])
    assert plan([ours(1, 30)], 1, N, H, D) == ("all", 30, [False])                               # B = 1: batch B
    bad = [
        [],                                                    # nothing
        [ours(1, 29)],                                         # batch B - 1 but not N tokens
        [ours(1, 30), ours(1, 30)],                            # batch B - 1, 2 N tokens
        [ours(3, 30)],                                         # neither B nor B - 1
        [ours(2, 30), ours(1, 30)],                            # mixed batches
        [((2, 30, 64), (2, 30, 64))],                          # last dimension neither inner nor d_head
        [((12, 30, D), (12, 30, D))],                          # [(b h), n, d] whose first dimension is no multiple of the heads
        [((2, 30, H * D), (2, 31, H * D))],                    # k and v differ
        [((2, 30 * H * D), (2, 30 * H * D))],                  # not 3-D
    ]
    for shapes in bad:
        with pytest.raises(ValueError):
            plan(shapes, B, N, H, D)
    with pytest.raises(ValueError):
        plan([ours(1, 30)], 3, N, H, D)                        # B = 3 wants batch 2 or 3


def test_layout_helpers_round_trip():
    from sd_animation_optical_flow_amd import transformer as T
    t = torch.randn((2, 5, 24), generator=torch.Generator().manual_seed(1))
    r = T.to_reference_layout(t, 3)
    assert tuple(r.shape) == (6, 5, 8) and torch.equal(r, TC.heads_first(t, 3)) and r.is_contiguous()
    assert torch.equal(T.from_reference_layout(r, 3), t)
    assert torch.equal(r[4], t[1, :, 8:16])                                   # (b = 1, h = 1)
