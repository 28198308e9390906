"""-m gpu: `weight_dtype="fp16"` on the SD models against `precision="fp16"` with fp32 weights, at the seeded test configurations
(UNet u0 at B = 2 on an 8x12 latent, ControlNet c0, SpatialTransformer c0 / c1, the VAE's golden cases).

The half operands are the halves the fp16 kernels round every weight to on every launch, so nothing may move: every output, every
recorded K/V entry and every ControlNet residual is compared bit for bit, a call with `control` and `reference_kv` included.  And the
memory claim is held: every entry of `model.w` that `_conv` / `_gemm` (or the VAE decoder's fused Upsample) read is float16 of the
same shape, exactly half the bytes of its fp32 twin, and every other entry -- biases, norm scales, the timestep path, ControlNet's hint
stem, the UNet's own Upsample weights -- is the same fp32 tensor."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import controlnet_check as CC   # noqa: E402
import transformer_check as TC   # noqa: E402
import unet_check as UC   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.dtype == torch.float16 else t.dtype)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b)), what


def _held_bytes(half, full, want_half, what):
    """`half.w` against `full.w` (the fp32-weight twin): the entries named `want_half` are float16 at exactly half the bytes, every
    other entry is identical; -> (bytes of fp32 weights, bytes with weight_dtype="fp16")."""
    assert half.weight_dtype == "fp16" and full.weight_dtype == "fp32" and not full.half_keys
    assert sorted(half.w) == sorted(full.w) and half.half_keys == set(want_half), (what, sorted(half.half_keys ^ set(want_half)))
    nb = lambda t: t.numel() * t.element_size()
    for key, t in full.w.items():
        h = half.w[key]
        if key in want_half:
            assert t.dtype == torch.float32 and h.dtype == torch.float16 and h.shape == t.shape and 2 * nb(h) == nb(t), (what, key)
            assert torch.equal(h, t.half()), (what, key)                     # the halves the kernel would round to
        else:
            _same(h, t, (what, key))
    return sum(nb(t) for t in full.w.values()), sum(nb(t) for t in half.w.values())


def _models(full, half):
    """-> [(name, fp32-weight model, half-weight model)] of a UNet trunk and its transformers."""
    assert sorted(full.st) == sorted(half.st)
    return [("trunk", full, half)] + [(n, full.st[n], half.st[n]) for n in sorted(full.st)]


def _trunk_bytes(full, half, sd, what, fp32_prefixes=()):
    tot = [0, 0]
    for name, f, h in _models(full, half):
        if name == "trunk":
            st_names = tuple(n + "." for n in full.st)
            want = {k for k, t in sd.items() if t.dim() == 4 and not k.startswith(st_names) and not k.endswith(".conv.weight")
                    and not k.startswith(fp32_prefixes)}
        else:
            want = {k for k, t in f.w.items() if t.dim() == 2}              # every Linear and 1x1 of a transformer is a GEMM operand
            assert want and all(k.endswith(".weight") for k in want)
        a, b = _held_bytes(h, f, want, f"{what} {name}")
        tot[0] += a
        tot[1] += b
    print(f"{what}: weights on the device {tot[0]} bytes in fp32, {tot[1]} with weight_dtype='fp16' ({tot[1] / tot[0]:.3f})")
    assert tot[1] < tot[0]       # (how far below depends on the configuration: the timestep path and the UNet's Upsample stay fp32)
    return tot


def test_unet_outputs_and_kv_history_are_bit_identical(cuda):
    from sd_animation_optical_flow_amd import unet as UN
    gold = np.load(os.path.join(GOLDEN, "unet_ref_u0.npz"))
    sd = UN.random_unet_state_dict(0, UC.U0)
    full = UN.UNetModel(sd, UC.U0, prefix="", precision="fp16")
    half = UN.UNetModel(sd, UC.U0, prefix="", precision="fp16", weight_dtype="fp16")
    assert half.precision == "fp16" and all(st.weight_dtype == "fp16" and st.precision == "fp16" for st in half.st.values())
    _trunk_bytes(full, half, sd, "UNetModel u0")
    # the UNet's own Upsample operands stay fp32 (ofx_upconv2x runs in fp32 in every precision)
    ups = [k for k in half.w if k.endswith(".conv.weight") or k.endswith(".conv.weight.folded")]
    assert ups and all(half.w[k].dtype == torch.float32 for k in ups)
    assert all(half.w[k].dtype == torch.float32 for k in half.w if k.startswith(("time_embed.", "emb_layers.", "freqs")))
    lay = UN.unet_layout(UC.U0)
    heads = UC.transformer_heads(lay)
    x, t, ctx = (torch.from_numpy(gold[n]).cuda() for n in ("x", "timesteps", "context"))
    assert tuple(x.shape) == (2, x.shape[1], 8, 12)
    hist = [(torch.from_numpy(gold[f"k{i}"]), torch.from_numpy(gold[f"v{i}"])) for i in range(len(heads))]
    ctl = [c.cuda() for c in UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)]
    calls = {"plain": {}, "control + reference_kv of batch B": dict(control=ctl, reference_kv=UC.reference_frames(hist, heads, "all")),
             "reference_kv of batch B - 1": dict(reference_kv=UC.reference_frames(hist, heads, "positive")),
             "only_mid_control": dict(control=ctl, only_mid_control=True)}
    for name, kw in calls.items():
        (of, hf), (oh, hh) = full(x, t, ctx, **kw), half(x, t, ctx, **kw)
        _same(oh, of, name)
        assert len(hh) == len(hf) == len(heads)
        for i, ((kf, vf), (kh, vh)) in enumerate(zip(hf, hh)):
            _same(kh, kf, (name, "k", i))
            _same(vh, vf, (name, "v", i))
    # and the arithmetic is the fp16 one, not the default's
    plain32 = UN.UNetModel(sd, UC.U0, prefix="")(x, t, ctx)[0]
    assert not torch.equal(plain32, half(x, t, ctx)[0])


def test_controlnet_residuals_are_bit_identical(cuda):
    from sd_animation_optical_flow_amd import controlnet as CN
    sd = CN.random_controlnet_state_dict(0, CC.C0)
    full = CN.ControlNet(sd, CC.C0, prefix="", precision="fp16")
    half = CN.ControlNet(sd, CC.C0, prefix="", precision="fp16", weight_dtype="fp16")
    _trunk_bytes(full, half, sd, "ControlNet c0", fp32_prefixes=("input_hint_block.",))
    stem = [k for k in half.w if k.startswith("input_hint_block.")]
    assert stem and all(half.w[k].dtype == torch.float32 for k in stem)     # the hint stem is exact fp32 in every mode
    x, hint, t, context = (v.cuda() for v in CC.c0_inputs())
    _same(half.hint_stem(hint), full.hint_stem(hint), "guided_hint")
    for h in (hint, hint[:1]):                                               # a hint per image, and one for the whole batch
        of, oh = full(x, h, t, context), half(x, h, t, context)
        assert len(of) == len(oh) > 1
        for i, (a, b) in enumerate(zip(of, oh)):
            _same(b, a, ("residual", i, h.shape[0]))


@pytest.mark.parametrize("tag", ["c0", "c1"])
def test_spatial_transformer_is_bit_identical(cuda, tag):
    from sd_animation_optical_flow_amd import transformer as T
    g = np.load(os.path.join(GOLDEN, f"spatial_transformer_ref_{tag}.npz"))
    Cn, heads, d, ctx = (int(v) for v in g["cfg"][:4])
    sd = T.random_spatial_transformer_state_dict(0, Cn, heads, d, ctx)
    full = T.SpatialTransformer(sd, heads, d, precision="fp16")
    half = T.SpatialTransformer(sd, heads, d, precision="fp16", weight_dtype="fp16")
    a, b = _held_bytes(half, full, {k for k, t in full.w.items() if t.dim() == 2}, f"SpatialTransformer {tag}")
    print(f"SpatialTransformer {tag}: weights on the device {a} bytes in fp32, {b} with weight_dtype='fp16' ({b / a:.3f})")
    x, c = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["context"]).cuda()
    k, v = torch.from_numpy(g["k"]), torch.from_numpy(g["v"])
    for name, kw in {"plain": {}, "reference_kv of batch B": dict(reference_kv=[(*TC.reference_all(k, v, heads), 0)]),
                     "reference_kv of batch B - 1": dict(reference_kv=[(*TC.reference_positive(k, v, heads), 0)])}.items():
        (of, hf), (oh, hh) = full(x, c, **kw), half(x, c, **kw)
        _same(oh, of, name)
        assert len(hf) == len(hh) >= 1
        for (kf, vf), (kh, vh) in zip(hf, hh):
            _same(kh, kf, name)
            _same(vh, vf, name)


def _vae_want(model):
    return {k for k, t in model.w.items() if k.endswith(".weight") and t.dim() == 2} | {k for k in model.w if k.endswith(".folded")}


def test_vae_decoder_is_bit_identical(cuda):
    from sd_animation_optical_flow_amd.vae import VaeDecoder, random_vae_decoder_state_dict
    sd = random_vae_decoder_state_dict(0)
    full, half = VaeDecoder(sd, precision="fp16"), VaeDecoder(sd, precision="fp16", weight_dtype="fp16")
    folded = [k for k in half.w if k.endswith(".folded")]
    assert len(folded) == 3 and all(half.w[k].dtype == torch.float16 and half.w[k].dim() == 4 for k in folded)   # the three Upsample layers
    a, b = _held_bytes(half, full, _vae_want(full), "VaeDecoder")
    print(f"VaeDecoder: weights on the device {a} bytes in fp32, {b} with weight_dtype='fp16' ({b / a:.3f})")
    assert b < 0.51 * a
    z = torch.from_numpy(np.load(os.path.join(GOLDEN, "vae_ref_autocast.npz"))["z_b2_6x10"]).cuda()
    assert all(full.fused_upsample.values()) and all(half.fused_upsample.values())
    _same(half.decode(z), full.decode(z), "decode")
    _same(half.decode_latent(z), full.decode_latent(z), "decode_latent")
    assert not torch.equal(half.decode(z), VaeDecoder(sd).decode(z))         # the fp16 arithmetic, not the default's
    # the unfused pair reads the packed 3x3 operand of the same layers, half as well
    for m in (full, half):
        m.fused_upsample = {lvl: False for lvl in m.fused_upsample}
    _same(half.decode(z), full.decode(z), "decode, unfused Upsample")


def test_vae_encoder_is_bit_identical(cuda):
    from oracle import vae_oracle as VO
    from sd_animation_optical_flow_amd.vae import VaeEncoder
    sd = VO.init_vae_state_dict(0)
    full, half = VaeEncoder(sd, precision="fp16"), VaeEncoder(sd, precision="fp16", weight_dtype="fp16")
    a, b = _held_bytes(half, full, _vae_want(full), "VaeEncoder")
    print(f"VaeEncoder: weights on the device {a} bytes in fp32, {b} with weight_dtype='fp16' ({b / a:.3f})")
    assert b < 0.51 * a
    image = torch.from_numpy(np.load(os.path.join(GOLDEN, "vae_ref_autocast.npz"))["image_b2_40x56"]).cuda()
    _same(half.encode_moments(image), full.encode_moments(image), "encode_moments")
