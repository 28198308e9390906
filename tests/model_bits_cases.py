"""The model runs whose output bits are recorded (tools/model_bits.py, tests/test_gpu_model_bits.py) and the seeded state dicts whose
bits are recorded (tests/test_model_weights_host.py): the five SD-stage models on the inputs of their own goldens, through public
names only.  A change of how the models load, pack or call their layers keeps these bits; a change of a kernel's arithmetic records
new ones.  Plain data and input construction: importing this module needs no GPU."""
import functools
import hashlib
import os
import warnings

import numpy as np
import torch

import controlnet_check as CC
import text_encoder_check as XC
import unet_check as UC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "model_bits", "sha256.json")
WEIGHTS_GOLDEN = os.path.join(HERE, "golden", "model_bits", "weights_sha256.json")
VAE_SMALL = dict(ch=32, ch_mult=(1, 2), num_res_blocks=1, in_channels=3, z_channels=4, double_z=True, embed_dim=4)


def gold(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def sha256(tensors):
    """SHA-256 over dtype, shape and bytes (C order) of every tensor, in order."""
    h = hashlib.sha256()
    for t in tensors:
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def state_dict_sha256(sd):
    """SHA-256 over keys, shapes and bytes of a state dict, in its own order."""
    h = hashlib.sha256()
    for key, t in sd.items():
        a = np.ascontiguousarray(t.numpy())
        assert a.dtype == np.float32
        h.update(f"{key}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------------------------
# the seeded state dicts

def st_cfg(tag):
    """(in_channels, heads, d_head, context_dim) of a stored SpatialTransformer configuration."""
    return tuple(int(v) for v in gold(f"spatial_transformer_ref_{tag}")["cfg"][:4])


def weight_cases():
    """[(name, make)]: make() -> the state dict, on the small configurations of the goldens at seeds 0 and 3, the two VAE dicts on
    a two-level ch = 32 ddconfig at both seeds and on SD_V1_CONFIG at seed 0."""
    from sd_animation_optical_flow_amd import controlnet, text_encoder, transformer, unet, vae
    out = []
    for seed in (0, 3):
        out += [(f"unet/u0/seed{seed}", lambda s=seed: unet.random_unet_state_dict(s, UC.U0)),
                (f"controlnet/c0/seed{seed}", lambda s=seed: controlnet.random_controlnet_state_dict(s, CC.C0)),
                (f"clip_text/t0/seed{seed}", lambda s=seed: text_encoder.random_clip_text_state_dict(s, XC.T0)),
                (f"vae_encoder/ch32/seed{seed}", lambda s=seed: vae.random_vae_state_dict(s, VAE_SMALL)),
                (f"vae_decoder/ch32/seed{seed}", lambda s=seed: vae.random_vae_decoder_state_dict(s, VAE_SMALL))]
        out += [(f"spatial_transformer/{tag}/seed{seed}",
                 lambda s=seed, tag=tag: transformer.random_spatial_transformer_state_dict(s, *st_cfg(tag))) for tag in ("c0", "c1")]
    out += [("vae_encoder/sd_v1/seed0", lambda: vae.random_vae_state_dict(0)),
            ("vae_decoder/sd_v1/seed0", lambda: vae.random_vae_decoder_state_dict(0))]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the device runs; every model is built once per process

@functools.lru_cache(maxsize=None)
def _unet(**kw):
    from sd_animation_optical_flow_amd import unet as UN
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)               # u0's 192-wide middle head keeps fp32 attention and says so
        return UN.UNetModel(UN.random_unet_state_dict(0, UC.U0), UC.U0, prefix="", **kw)


@functools.lru_cache(maxsize=None)
def _controlnet():
    from sd_animation_optical_flow_amd import controlnet as CN
    return CN.ControlNet(CN.random_controlnet_state_dict(0, CC.C0), CC.C0, prefix="")


@functools.lru_cache(maxsize=None)
def _transformer(tag, **kw):
    from sd_animation_optical_flow_amd import transformer as T
    Cn, heads, d, ctx = st_cfg(tag)
    return T.SpatialTransformer(T.random_spatial_transformer_state_dict(0, Cn, heads, d, ctx), heads, d, **kw)


@functools.lru_cache(maxsize=None)
def _clip(clip_skip):
    from sd_animation_optical_flow_amd import text_encoder as TE
    return TE.ClipTextEncoder(TE.random_clip_text_state_dict(0, XC.T0), XC.T0, prefix="", clip_skip=clip_skip)


@functools.lru_cache(maxsize=None)
def _vae(which):
    from sd_animation_optical_flow_amd import vae
    return vae.VaeEncoder(vae.random_vae_state_dict(0)) if which == "encoder" else vae.VaeDecoder(vae.random_vae_decoder_state_dict(0))


def _flat(out, hist):
    return [out] + [t for kv in hist for t in kv]


def _unet_run(kind, **kw):
    def make():
        g = gold("unet_ref_u0")
        x, t, ctx = (torch.from_numpy(g[n]).cuda() for n in ("x", "timesteps", "context"))
        model = _unet(**kw)
        if kind == "control":
            heads = UC.transformer_heads(model.layout)
            hist = [(torch.from_numpy(g[f"k{i}"]), torch.from_numpy(g[f"v{i}"])) for i in range(len(heads))]
            ref = UC.reference_frames(hist, heads, "all")            # batch B
            ctl = [c.cuda() for c in UC.control_residuals(model.layout, UC.U0_B, UC.U0_H, UC.U0_W)]
            return lambda: [model(x, t, ctx, control=ctl, reference_kv=ref)[0]]
        if kind == "padded":                                         # the sampler's path: the first convolution's own operand
            xp = torch.zeros((UC.U0_B, UC.U0_H, UC.U0_W, model.in_pad), device="cuda")
            xp[..., :model.in_channels] = x.permute(0, 2, 3, 1)
            return lambda: _flat(*model.forward_nhwc(xp, t, ctx, padded=True))
        return lambda: _flat(*model(x, t, ctx))
    return make


def _controlnet_run(hint_batch):
    def make():
        x, hint, t, ctx = (v.cuda() for v in CC.c0_inputs())
        net = _controlnet()
        return lambda: net(x, hint[:hint_batch].contiguous(), t, ctx)
    return make


def _transformer_run(tag, **kw):
    def make():
        g = gold(f"spatial_transformer_ref_{tag}")
        x, ctx = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["context"]).cuda()
        mod = _transformer(tag, **kw)
        return lambda: _flat(*mod(x, ctx))
    return make


def _clip_run(kind):
    def make():
        tokens = torch.from_numpy(gold("clip_text_ref_t0")["tokens"])
        if kind == "conditioning":
            return lambda: list(_clip(0).conditioning(tokens[:1], tokens[1:]))
        if kind == "hidden_states":
            def launch():
                out, hs = _clip(0).encode_ids(tokens.reshape(-1, tokens.shape[2]), hidden_states=True)
                return [out] + list(hs)
            return launch
        return lambda: [_clip(2).forward_tokens(tokens)]
    return make


def _vae_run(kind):
    def make():
        if kind == "encode_moments":
            image = torch.from_numpy(gold("vae_ref_64x48")["image"]).cuda()
            return lambda: [_vae("encoder").encode_moments(image)]
        z = torch.from_numpy(gold("vae_dec_ref_8x6")["z"]).cuda()
        return lambda: [getattr(_vae("decoder"), kind)(z)]
    return make


def runs():
    """[(name, make)]: make() builds the model (once per process) and the inputs and returns launch(), which runs the case once and
    returns its outputs as a list of device tensors."""
    return [("unet/plain", _unet_run("plain")),
            ("unet/control-reference_kv", _unet_run("control")),
            ("unet/precision-fp16", _unet_run("plain", precision="fp16")),
            ("unet/attention_precision-fp16", _unet_run("plain", attention_precision="fp16")),
            ("unet/forward_nhwc-padded", _unet_run("padded")),
            ("controlnet/hint-batch2", _controlnet_run(2)),
            ("controlnet/hint-batch1", _controlnet_run(1)),
            ("spatial_transformer/c0", _transformer_run("c0")),
            ("spatial_transformer/c1", _transformer_run("c1")),
            ("spatial_transformer/c0-attention_precision-fp16", _transformer_run("c0", attention_precision="fp16")),
            ("clip_text/conditioning", _clip_run("conditioning")),
            ("clip_text/encode_ids-hidden_states", _clip_run("hidden_states")),
            ("clip_text/clip_skip2", _clip_run("clip_skip2")),
            ("vae_encoder/encode_moments", _vae_run("encode_moments")),
            ("vae_decoder/decode", _vae_run("decode")),
            ("vae_decoder/decode_latent", _vae_run("decode_latent"))]
