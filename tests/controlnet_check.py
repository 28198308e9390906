"""Float64 restatement of ControlNet and of `ofx_conv3x3_silu`, with the derived error bounds and the GPU case table.
Not a conftest: imported by name, and importable without a device.

    ControlNet.forward          controlnet.py:301-322
    input_hint_block            controlnet.py:164-180
    apply_multi_controlnet      controlnet.py:412-432
The model is restated in NCHW float64 on `unet_check`'s blocks (`time_embed64`, `resblock64`, `_conv`) and
`transformer_check.spatial_transformer64`.  PINNED by tests/test_controlnet_host.py against tests/golden/controlnet_ref_c0.npz, the
output of the reference's own module.

ofx_conv3x3_silu (u = 2^-24).  The pre-activation is an fp32 sum of D = 9 Cin products (Cin the kernel's padded channel count; fused
multiply-add chains per channel chunk, then the chunk sums) and the bias addition.  Every term passes through at most D
roundings whatever the order, the bias addition one more; with the slack `sd_ops_check.py` keeps in its dot products this is its (D + 4) u sum |q k| form:
    |y - y64| <= (9 Cin + 4) u (sum |x w| + |bias|)
With SiLU, `sd_ops_check`'s own line (the sigmoid is `ofx_sigmoid`, the function GroupNorm's SiLU uses): the slope of y sigmoid(y)
is at most SILU_SLOPE = 1.1, the evaluation is expf (E_EXP u), the addition (u) and the division (E_DIV u):
    |out - silu(y64)| <= 1.1 bound(y) + (E_EXP + 1 + E_DIV) u |silu(y64)| + FLOOR
No constant is defined here: E_EXP, E_DIV, FLOOR and SILU_SLOPE are sd_ops_check's.

The bar for `ControlNet.forward` and the mixes is `unet_check.bar4`: four times the distance of the reference's fp32 module from
this restatement, stored per output by tests/golden/make_golden_controlnet.py.
"""
import torch
import torch.nn.functional as F

import sd_ops_check as SC
import transformer_check as TC
import unet_check as UC

U = SC.U

# the ControlNet twin of unet_check.U0: the same trunk, in_channels 4, a 3-channel hint
C0 = dict(in_channels=4, hint_channels=3, model_channels=64, channel_mult=(1, 2, 3), num_res_blocks=1, attention_resolutions=(1, 2),
          num_heads=1, context_dim=64, legacy=False, transformer_depth=1)
C0_B, C0_H, C0_W, C0_M, C0_T = UC.U0_B, UC.U0_H, UC.U0_W, UC.U0_M, UC.U0_T
C0_SHAPES = [(2, 64, 8, 12), (2, 64, 8, 12), (2, 64, 4, 6), (2, 128, 4, 6), (2, 128, 2, 3), (2, 192, 2, 3), (2, 192, 2, 3)]
# the two nets of the stored mixes: (seed of random_controlnet_state_dict, weight, guidance_start, guidance_end)
MIX_NETS = ((0, 0.7, 0.0, 1.0), (1, 0.3, 0.0, 0.9))
MIX_P = (0.5, 0.95)
C0_SEED = 3030


def c0_inputs():
    """x [2,4,8,12], hint [2,3,64,96] in [0, 1] (two different maps), timesteps, context [2,9,64]."""
    g = torch.Generator().manual_seed(C0_SEED)
    x = torch.randn((C0_B, C0["in_channels"], C0_H, C0_W), generator=g)
    context = torch.randn((C0_B, C0_M, C0["context_dim"]), generator=g)
    hint = torch.rand((C0_B, C0["hint_channels"], 8 * C0_H, 8 * C0_W), generator=g)
    return x, hint, torch.tensor(C0_T), context


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the model in float64

@torch.no_grad()
def hint_stem64(sd64, layout, hint):
    """`input_hint_block` (:164-180): SiLU after every layer but the last."""
    g = hint.double()
    for i, (name, _, _, stride) in enumerate(layout["hint"]):
        g = UC._conv(sd64, name, g, stride=stride)
        if i != len(layout["hint"]) - 1:
            g = UC.silu64(g)
    return g


@torch.no_grad()
def controlnet64(sd64, layout, x, hint, timesteps, context):
    """sd64: float64 state dict without prefix; layout: `controlnet.controlnet_layout(cfg)`; x [B,C,H,W]; hint [B or 1,3,8H,8W] ->
    (the len(input_blocks) + 1 residuals, guided_hint), float64 NCHW."""
    cfg = layout["cfg"]
    emb = UC.time_embed64(sd64, timesteps, int(cfg["model_channels"]))
    ctx = None if context is None else context.double()
    guided = hint_stem64(sd64, layout, hint)

    def block(layers, h):
        for l in layers:
            kind, name = l[0], l[1]
            if kind == "conv":
                h = UC._conv(sd64, name, h)
            elif kind == "res":
                h = UC.resblock64(sd64, name, h, emb)
            elif kind == "st":
                sub = {k[len(name) + 1:]: v for k, v in sd64.items() if k.startswith(name + ".")}
                h, _ = TC.spatial_transformer64(sub, h, l[3], ctx, [], depth=int(cfg["transformer_depth"]))
            else:
                assert kind == "down", kind
                h = UC._conv(sd64, f"{name}.op", h, stride=2)
        return h

    outs = []
    h = x.double()
    for i, blk in enumerate(layout["input"]):
        h = block(blk, h)
        if i == 0:
            h = h + guided                                        # :313, a batch-1 hint broadcasts
        outs.append(UC._conv(sd64, layout["zero"][i][0], h, pad=0))
    h = block(layout["middle"], h)
    outs.append(UC._conv(sd64, layout["zero"][-1][0], h, pad=0))
    return outs, guided


def mix_weights(p):
    """The weights apply_multi_controlnet gives MIX_NETS at denoise_percentage p (:423, both window ends inclusive)."""
    return [0.0 if p < gs or p > ge else w for _, w, gs, ge in MIX_NETS]


def mix64(results, p):
    """results: per net, the list of residuals -> sum_n weight_n(p) result_n[i] in float64."""
    ws = mix_weights(p)
    return [sum(w * r[i].double() for w, r in zip(ws, results)) for i in range(len(results[0]))]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. ofx_conv3x3_silu: cases, reference, bound, planted bugs

def _kc(name, cin, cout, stride, H, W, B=1, silu=True, ldx=None, ldo=None, kind="plain"):
    cp = (cin + 3) // 4 * 4
    return dict(name=name, cin=cin, cin_pad=cp, cout=cout, stride=stride, H=H, W=W, B=B, silu=silu, ldx=ldx or cp, ldo=ldo or cout, kind=kind)


# The smallest shapes that reach every path: channel chunks of 4 (Cin % 8 != 0) and of 8, one to many chunks; 1, 2, 4 and 6 channel
# blocks of 16 per workgroup (Cout 16 / 32 / 256, 320 / 96) and Cout 48 (three workgroups of one block); both strides; images
# smaller than, equal to and not a whole number of 8 x 16 tiles, odd sizes under stride 2; several images; strided rows.
CONV_CASES = [
    _kc("hint3-16-s1-17x23", 3, 16, 1, 17, 23),                             # channel 3 of x is data, its weights are zero
    _kc("hint3-16-s2-1x1", 3, 16, 2, 1, 1),
    _kc("16-16-s1-9x11-b3", 16, 16, 1, 9, 11, B=3),
    _kc("16-16-s2-3x5-nosilu", 16, 16, 2, 3, 5, silu=False),
    _kc("16-32-s2-17x23", 16, 32, 2, 17, 23),
    _kc("32-32-s1-16x32", 32, 32, 1, 16, 32),
    _kc("32-96-s2-16x32-b3", 32, 96, 2, 16, 32, B=3),
    _kc("96-96-s1-3x5", 96, 96, 1, 3, 5),
    _kc("96-256-s2-9x11", 96, 256, 2, 9, 11),
    _kc("256-320-s1-17x23-nosilu", 256, 320, 1, 17, 23, silu=False),
    _kc("256-320-s1-1x1-b3", 256, 320, 1, 1, 1, B=3),
    _kc("12-48-s1-9x11", 12, 48, 1, 9, 11),                                 # three chunks of 4; three workgroups along Cout
    _kc("16-32-s1-9x11-slack", 16, 32, 1, 9, 11, B=3, ldx=24, ldo=40, kind="slack"),
    _kc("32-32-s2-17x23-slack", 32, 32, 2, 17, 23, ldx=36, ldo=36, kind="slack"),
    _kc("32-32-s1-17x23-beyond90", 32, 32, 1, 17, 23, kind="big"),          # pre-activations beyond +-90: both ends of expf
]
SENTINEL = 12345.0


def conv_input(c):
    """-> x [B,H,W,ldx] (channels cin.. of a row hold finite junk the kernel must not use, or skip), w OIHW [cout,cin,3,3], bias."""
    g = SC._gen("cn-" + c["name"])
    x = torch.randn((c["B"], c["H"], c["W"], c["ldx"]), generator=g)
    w = torch.randn((c["cout"], c["cin"], 3, 3), generator=g) * (1.0 / (9 * c["cin"]) ** 0.5)
    bias = 0.5 * torch.randn((c["cout"],), generator=g)
    if c["kind"] == "big":
        x = x * 60.0
    return x, w, bias


def _conv64(x, w, bias, c, stride=None):
    xin = x[..., :c["cin"]].permute(0, 3, 1, 2).double()
    return F.conv2d(xin, w.double(), None if bias is None else bias.double(), stride=stride or c["stride"], padding=1).permute(0, 2, 3, 1)


def conv_reference(x, w, bias, c):
    """-> (ref64 [B,Ho,Wo,cout], bound, y64): the float64 output, its bound (header) and the float64 pre-activation."""
    y = _conv64(x, w, bias, c)
    mag = _conv64(x.abs(), w.abs(), bias.abs(), c)
    by = (9 * c["cin_pad"] + 4) * U * mag
    if not c["silu"]:
        return y, by, y
    s = UC.silu64(y)
    return s, SC.SILU_SLOPE * by + (SC.E_EXP + 1 + SC.E_DIV) * U * s.abs() + SC.FLOOR, y


def conv_planted(x, w, bias, c):
    """Wrong results a kernel could plausibly give, from the float64 data (nothing faulty is launched): name -> [B,Ho,Wo,cout]."""
    act = UC.silu64 if c["silu"] else (lambda t: t)
    out = {"dropped-bias": act(_conv64(x, w, None, c))}
    shifted = torch.zeros_like(x)
    shifted[:, :, 1:] = x[:, :, :-1]                               # every tap reads one column to the left
    out["tap-shifted-a-column"] = act(_conv64(shifted, w, bias, c))
    if c["stride"] == 2 and c["H"] > 1 and c["W"] > 1:
        full = _conv64(x, w, bias, c, stride=1)
        odd = full[:, 1::2, 1::2]
        Ho, Wo = (c["H"] - 1) // 2 + 1, (c["W"] - 1) // 2 + 1
        pad = torch.zeros((c["B"], Ho, Wo, c["cout"]), dtype=torch.float64)
        pad[:, :odd.shape[1], :odd.shape[2]] = odd
        out["stride-2-odd-phase"] = act(pad)
    return out


def worst_ratio(got, ref, bound):
    return SC._worst((got.double() - ref).abs(), bound)
