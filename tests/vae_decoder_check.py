"""Float64 CPU restatement of the first-stage decoder (not a conftest: imported by name).

    AutoencoderKL.decode       ldm/models/autoencoder.py: post_quant_conv, then Decoder.forward
    Decoder.forward            ldm/modules/diffusionmodules/model.py:619-652
      ResnetBlock.forward      :129-149      Upsample.forward :52-58      AttnBlock.forward :179-203
      Normalize / nonlinearity :35-41
    decode_first_stage         ldm/models/diffusion/ddpm.py:820-828  (z / scale_factor first)
    decode_latent              ofgen_keyframe_inpaint.py:234-235      (clip, * 127.5 + 127.5, uint8, RGB -> BGR)

Every tensor is float64, so the restatement's own rounding is ~1e-16 of the activations: what it differs from the real fp32
`Decoder` by is that module's fp32 rounding (measured when the golden is made, tests/golden/make_golden_vae_decoder.py).
PINNED by tests/test_vae_decoder_host.py against tests/golden/vae_dec_ref_8x6.npz, the output of the reference's own module.
"""
import numpy as np
import torch
import torch.nn.functional as F

SCALE_FACTOR = 0.18215


def _norm(sd, name, x):
    return F.group_norm(x, 32, sd[f"{name}.weight"], sd[f"{name}.bias"], eps=1e-6)


def _silu(x):
    return x * torch.sigmoid(x)


def _conv(sd, name, x, padding=0):
    return F.conv2d(x, sd[f"{name}.weight"], sd[f"{name}.bias"], padding=padding)


def _resblock(sd, name, x):
    h = _conv(sd, f"{name}.conv1", _silu(_norm(sd, f"{name}.norm1", x)), padding=1)
    h = _conv(sd, f"{name}.conv2", _silu(_norm(sd, f"{name}.norm2", h)), padding=1)
    if f"{name}.nin_shortcut.weight" in sd:
        x = _conv(sd, f"{name}.nin_shortcut", x)
    return x + h


def _attn(sd, name, x):
    hn = _norm(sd, f"{name}.norm", x)
    q, k, v = (_conv(sd, f"{name}.{n}", hn) for n in ("q", "k", "v"))
    b, c, h, w = q.shape
    w_ = torch.bmm(q.reshape(b, c, h * w).permute(0, 2, 1), k.reshape(b, c, h * w)) * (int(c) ** (-0.5))
    w_ = torch.softmax(w_, dim=2)
    h_ = torch.bmm(v.reshape(b, c, h * w), w_.permute(0, 2, 1)).reshape(b, c, h, w)
    return x + _conv(sd, f"{name}.proj_out", h_)


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


@torch.no_grad()
def decode64(sd64, z, n_levels=4, num_res_blocks=2):
    """sd64: the state dict in float64 (to64, made once and shared); z [B,4,h,w] -> image float64 [B,3,8h,8w]."""
    h = _conv(sd64, "post_quant_conv", z.double())
    h = _conv(sd64, "decoder.conv_in", h, padding=1)
    h = _resblock(sd64, "decoder.mid.block_1", h)
    h = _attn(sd64, "decoder.mid.attn_1", h)
    h = _resblock(sd64, "decoder.mid.block_2", h)
    for lvl in reversed(range(n_levels)):
        for j in range(num_res_blocks + 1):
            h = _resblock(sd64, f"decoder.up.{lvl}.block.{j}", h)
        if lvl != 0:
            h = _conv(sd64, f"decoder.up.{lvl}.upsample.conv", F.interpolate(h, scale_factor=2.0, mode="nearest"), padding=1)
    return _conv(sd64, "decoder.conv_out", _silu(_norm(sd64, "decoder.norm_out", h)), padding=1)


def to_u8_bgr(image_f32):
    """decode_latent's expression on an fp32 image [1,3,H,W] (torch clip, numpy fp32 multiply and add, astype, channel swap)."""
    a = image_f32.clip(-1, 1)[0].permute(1, 2, 0).cpu().numpy()
    return np.ascontiguousarray((a * 127.5 + 127.5).astype(np.uint8)[:, :, ::-1])


def upconv64(x, w):
    """x NCHW, w OIHW 3x3 -> conv3x3(pad 1)(nearest 2x(x)) in float64."""
    return F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), padding=1)
