"""`attention_precision="fp16"` on the device at the level of the modules: SpatialTransformer at the configurations of
tests/test_gpu_transformer.py (c0, c1) and UNetModel at configuration u0 with the five scenarios of tests/test_gpu_unet_precision.py.
The restatements with the roundings put in, the bars and their reasoning, and what the arithmetic alone does (measured on the CPU
before any device was asked) are in attn_f16_model_check.py.  Every test prints its distances before it judges them (-s).

u0 has one head size outside the fused five (the 192-wide middle head): UNetModel keeps that one transformer at fp32 attention and
warns (unet.py), which these tests assert; a SpatialTransformer built directly with such a head raises (test_attn_f16_host.py).

Measured on an MI355X (gfx950), the run that accompanied the kernel: see the end of attn_f16_model_check.py's header."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import attn_f16_model_check as MC   # noqa: E402
import transformer_check as TC      # noqa: E402
import unet_check as UC             # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "unet_ref_u0.npz")
GOLD_AUTOCAST = os.path.join(HERE, "golden", "unet_ref_u0_autocast.npz")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6: SpatialTransformer

@pytest.mark.parametrize("tag", ["c0", "c1"])
def test_spatial_transformer_with_fp16_attention(cuda, tag):
    from sd_animation_optical_flow_amd import transformer as T
    g = np.load(os.path.join(HERE, "golden", f"spatial_transformer_ref_{tag}.npz"))
    Cn, heads, d, ctx = (int(v) for v in g["cfg"][:4])
    sd = T.random_spatial_transformer_state_dict(0, Cn, heads, d, ctx)
    half = T.SpatialTransformer(sd, heads, d, attention_precision="fp16")
    plain = T.SpatialTransformer(sd, heads, d)
    assert half.attention_precision == "fp16" and plain.attention_precision == "fp32" and half.fused_attention and half.precision == "fp32"
    x, c = torch.from_numpy(g["x"]), torch.from_numpy(g["context"])
    k, v = torch.from_numpy(g["k"]), torch.from_numpy(g["v"])
    sd64 = TC.to64(sd)
    runs = {"plain": ({}, {}),
            "reference_kv of batch B": (dict(reference_kv=[(*TC.reference_all(k, v, heads), 0)]),
                                        dict(reference_kv=[tuple(TC.heads_last(t, heads) for t in TC.reference_all(k, v, heads))])),
            "reference_kv of batch B - 1": (dict(reference_kv=[(*TC.reference_positive(k, v, heads), 0)]),
                                            dict(reference_kv=[tuple(TC.heads_last(t, heads) for t in TC.reference_positive(k, v, heads))]))}
    dist = {}
    for name, (kw, kw64) in runs.items():
        out, hist = half(x.cuda(), c.cuda(), **kw)
        out32, hist32 = plain(x.cuda(), c.cuda(), **kw)
        ref, _ = MC.spatial_transformer64_r(sd64, x, heads, c, attn="half", **kw64)
        dist[name] = (float((out.cpu().double() - ref).abs().max()), MC.bar_st(ref), float((out32.cpu().double() - ref).abs().max()))
        # kv_hists are recorded before the attention: fp32, and exactly what they are without the argument
        assert len(hist) == len(hist32) == 1
        for a, b in zip(hist[0], hist32[0]):
            assert a.dtype == torch.float32 and torch.equal(a, b), name
        assert not torch.equal(out, out32), name                           # the fp16 kernel ran
    for name, (d16, bar, d32) in dist.items():
        print(f"{tag} {name}: fp16 attention vs the half restatement {d16:.3e}; bar {bar:.3e}; (the fp32 module against it {d32:.3e})")
    for name, (d16, bar, _) in dist.items():
        assert d16 <= bar, (tag, name, d16, bar)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7: UNetModel

@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def yard16():
    g = np.load(GOLD_AUTOCAST)
    return {str(k): float(v) for k, v in zip(g["dist_keys"], g["autocast_vs_f64"])}


def bar2(yardstick):
    """The bar of tests/test_gpu_unet_precision.py: twice the distance of the reference under autocast from float64."""
    return 2.0 * float(yardstick)


@pytest.fixture(scope="module")
def setup(cuda, gold):
    from sd_animation_optical_flow_amd import unet as UN
    sd = UN.random_unet_state_dict(0, UC.U0)
    lay = UN.unet_layout(UC.U0)
    heads = UC.transformer_heads(lay)
    hist = [(torch.from_numpy(gold[f"k{i}"]), torch.from_numpy(gold[f"v{i}"])) for i in range(len(heads))]
    return dict(UN=UN, sd=sd, lay=lay, heads=heads, hist=hist, runs={})


@pytest.fixture(scope="module")
def refs64(gold, setup):
    """unet_check.unet64 of the five stored runs, computed once and left unchanged."""
    sd64, lay, heads = TC.to64(setup["sd"]), setup["lay"], setup["heads"]
    x, t, ctx = (torch.from_numpy(gold[n]) for n in ("x", "timesteps", "context"))
    ctl = UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)
    f64 = lambda mode: [[(TC.heads_last(k, h).double(), TC.heads_last(v, h).double())
                         for (k, v), h in zip(UC.reference_frames(setup["hist"], heads, mode)[0], heads)]]
    r = {"out": UC.unet64(sd64, lay, x, t, ctx)[0]}
    r["out_refall"] = UC.unet64(sd64, lay, x, t, ctx, reference_kv=f64("all"))[0]
    r["out_refpos"] = UC.unet64(sd64, lay, x, t, ctx, reference_kv=f64("positive"))[0]
    r["out_ctl"] = UC.unet64(sd64, lay, x, t, ctx, control=ctl)[0]
    r["out_ctl_mid"] = UC.unet64(sd64, lay, x, t, ctx, control=ctl, only_mid_control=True)[0]
    return r


def _build(setup, **kw):
    """UNetModel at u0.  With attention_precision="fp16" the construction must warn about the one head size without an fp16 kernel;
    without the argument it must not warn at all."""
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        model = setup["UN"].UNetModel(setup["sd"], UC.U0, prefix="", **kw)
    mine = [w for w in caught if "attention_precision" in str(w.message)]
    assert len(mine) == (1 if kw.get("attention_precision", "fp32") == "fp16" else 0), [str(w.message) for w in caught]
    assert all("middle_block" in str(w.message) for w in mine)
    return model


def _runs(setup, gold, precision, attention_precision):
    """The five scenarios and the plain run's K/V history of one model, run once."""
    key = (precision, attention_precision)
    if key in setup["runs"]:
        return setup["runs"][key]
    kw = {} if attention_precision is None else dict(attention_precision=attention_precision)
    model = _build(setup, precision=precision, **kw)
    want = attention_precision or "fp32"
    assert model.attention_precision == want and len(model.st) == len(setup["heads"])
    # u0's middle transformer has a 192-wide head, which the fused kernel does not take: it keeps fp32 attention, loudly (_build)
    assert all(st.precision == precision and st.attention_precision == (want if st.fused_attention else "fp32") for st in model.st.values())
    assert [st.d_head for st in model.st.values() if not st.fused_attention] == [192]
    assert model.attention_precision_of == {n: st.attention_precision for n, st in model.st.items()}
    heads, lay = setup["heads"], setup["lay"]
    x, t, ctx = (torch.from_numpy(gold[n]).cuda() for n in ("x", "timesteps", "context"))
    ctl = [c.cuda() for c in UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)]
    fa, fp = UC.reference_frames(setup["hist"], heads, "all"), UC.reference_frames(setup["hist"], heads, "positive")
    out, hist = model(x, t, ctx)
    res = {"out": out, "hist": hist}
    res["out_refall"], res["hist_refall"] = model(x, t, ctx, reference_kv=fa)
    res["out_refpos"] = model(x, t, ctx, reference_kv=fp)[0]
    res["out_ctl"] = model(x, t, ctx, control=ctl)[0]
    res["out_ctl_mid"] = model(x, t, ctx, control=ctl, only_mid_control=True)[0]
    setup["runs"][key] = res
    return res


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_unet_with_fp16_attention_against_float64(setup, gold, refs64, yard16, precision):
    """UNetModel(precision=, attention_precision="fp16") against unet_check.unet64 under the bar of test_gpu_unet_precision.py,
    2 x autocast_vs_f64 per output, at all five scenarios; the K/V history of every transformer is bit for bit that of the model
    built without the argument."""
    res = _runs(setup, gold, precision, "fp16")
    base = _runs(setup, gold, precision, None)
    dist = {name: (float((res[name].cpu().double() - refs64[name]).abs().max()), float((base[name].cpu().double() - refs64[name]).abs().max()))
            for name in sorted(refs64)}
    for name, (d16, d32) in dist.items():
        print(f"precision={precision} attention_precision=fp16 {name}: device vs float64 {d16:.3e}; bar {bar2(yard16[name]):.3e}; "
              f"(fp32 attention {d32:.3e})")
    for name, (d16, _) in dist.items():
        assert d16 <= bar2(yard16[name]), (precision, name, d16, bar2(yard16[name]))
        assert not torch.equal(res[name], base[name]), name                # the fp16 attention kernel ran
    # the plain run: every transformer's own K/V depends on what the attentions before it computed, except the first one's, which
    # precedes every attention and is bit for bit the same; all of them are fp32 [B, N, inner] tensors of the same shapes
    assert len(res["hist"]) == len(base["hist"]) == len(setup["heads"])
    assert torch.equal(res["hist"][0][0], base["hist"][0][0]) and torch.equal(res["hist"][0][1], base["hist"][0][1])
    for (k, v), (kb, vb) in zip(res["hist"], base["hist"]):
        assert k.dtype == v.dtype == torch.float32 and k.shape == kb.shape and v.shape == vb.shape


def test_every_transformer_records_the_kv_history_of_the_model_without_the_argument(setup, gold):
    """Transformer by transformer on the SAME input: each SpatialTransformer of the fp16-attention model and its twin of the model
    built without the argument record bit-identical (k, v) -- the history is taken before the attention and is fp32."""
    kw16 = dict(precision="fp16", attention_precision="fp16")
    m16, m0 = _build(setup, **kw16), _build(setup, precision="fp16")
    assert sorted(m16.st) == sorted(m0.st) and len(m0.st) == len(setup["heads"])
    g = torch.Generator().manual_seed(7)
    ctx = torch.from_numpy(gold["context"]).cuda()
    for name in sorted(m0.st):
        a, b = m16.st[name], m0.st[name]
        x = torch.randn((UC.U0_B, a.in_channels, 4, 6), generator=g).cuda()
        (oa, ha), (ob, hb) = a(x, ctx), b(x, ctx)
        assert len(ha) == len(hb) >= 1
        for (ka, va), (kb, vb) in zip(ha, hb):
            assert ka.dtype == torch.float32 and torch.equal(ka, kb) and torch.equal(va, vb), name
        assert torch.equal(oa, ob) == (a.attention_precision == "fp32"), name      # the fp16 kernel ran wherever it exists
