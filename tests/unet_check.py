"""Float64 restatements of the UNet and of the three kernels of csrc/unet.hip, with derived error bounds and the GPU case tables.
Not a conftest: imported by name, and importable without a device.

    UNetModel.forward                 ldm/modules/diffusionmodules/openaimodel.py:757-793
    ControlledUnetModel.forward       controlnet.py:29-62
    TimestepEmbedSequential.forward   openaimodel.py:79-90
    ResBlock._forward                 openaimodel.py:257-277
    timestep_embedding                ldm/modules/diffusionmodules/util.py:154-174
The model is restated from the formulas in NCHW float64 (F.group_norm / F.conv2d / F.interpolate on float64 tensors) on top of
`transformer_check.spatial_transformer64`.  PINNED by tests/test_unet_host.py against tests/golden/unet_ref_u0.npz, the output of the
reference's own modules.

u = 2^-24, u64 = 2^-53 (sd_ops_check.U, U64).  Bounds are first order, relative to the OPERANDS.

ofx_groupnorm_cat.  z = cat(x0, x1) + e is normalised; the kernel evaluates y = x scale + shift', shift' = beta - (mean_z - e) scale,
with scale and shift' formed in float64 and rounded once each.  sd_ops_check's GroupNorm bound is K_GN u (|x scale| + |shift|) for the
three fp32 roundings (scale, shift, the fused multiply-add); here the operand magnitude is |x| + |e| (the magnitude of z's two
parts, which may cancel: |z| can be far below either), and the folded shift takes one more rounding of its e-part:
    |y - y64| <= K_GN u ((|x| + |e|) |scale| + |shift|) + u |e scale|,            shift = beta - mean_z scale
The f64 statistics add what sd_ops_check derives, with the summation chain L of `gn_layout` (the kernels keep ofx_groupnorm's
order) grown by L_E = 6 roundings for S + n e and Q + 2 e S + n e^2 (two products and an addition, twice), and with the moments of
|x| + |e| in place of those of |x|:
    rho <= 1.5 (L + 1 + L_E) u64 E[(|x| + |e|)^2] / (var + eps) + 2 u64,      d mean <= (L + 1 + L_E) u64 mean(|x| + |e|)
    |d scale| <= rho |scale|,       |d shift'| <= rho (|mean_z| + |e|) |scale| + d mean |scale|
SiLU on top as in sd_ops_check (`gn_ratios` is used as it stands).

ofx_emb_linear.  out = sum_k s(x_k) w_k + bias: every term passes through at most K roundings whatever the order of the additions
(the kernel's chain is K / 256 + 4 fused multiply-adds in a lane, six butterfly levels and the bias: far fewer), its own product
and the bias addition two more; with SiLU in front, s~ = s (1 + (E_EXP + 1 + E_DIV) u) (expf, the addition, the division:
sd_ops_check's measured E_EXP, E_DIV):
    |out - ref| <= (K + 2) u sum_k |s(x_k)| |w_k| + [silu] (E_EXP + 1 + E_DIV) u sum_k |s(x_k)| |w_k| + FLOOR

ofx_timestep_embedding.  a~ = fl(t f) = t f (1 + u) moves cos / sin by at most u |t f| (their slopes are at most 1); the device's
cosf / sinf add E_SINCOS u, absolute (|cos|, |sin| <= 1):
    |out - ref| <= u |t f| + E_SINCOS u
Measured term.  Y_SINCOS: the worst |cosf(a) - cos64(a)|, |sinf(a) - sin64(a)| of the device in units of u over the arguments
a = fl(t f) of the test grid (t in TS_T, the frequency tables of dims 320 and 65, and a sweep of 0..1000 rad), by
tools/sincos_probe.hip run by tools/unet_rate.py --sincos-probe and recorded in profiles/r20_unet_rate.txt: 1.143 u (cosf, at a = 569.39)
and 1.146 u (sinf, at a = 591.42) over 1 049 344 arguments (torch's float32 cos / sin on the host: 0.601); Y_SINCOS = 1.2.
As sd_ops_check does for E_EXP, the kernel may use up to twice that: E_SINCOS = 2 Y_SINCOS.  No other constant is measured.

The bar for a ResBlock run alone and for the whole model is not derived but measured against a yardstick, the reference's own fp32
CPU module against the float64 restatement, per output (tests/golden/make_golden_unet.py stores it): the device gets FOUR times
that distance (`bar4`), the ratio make_golden_transformer.py asserts between a reference fp32 run and the device's bar; it allows
for a second fp32 evaluation with another summation order in every layer.
"""
import math

import torch
import torch.nn.functional as F

import sd_ops_check as SC
import transformer_check as TC

U, U64, FLOOR = SC.U, SC.U64, SC.FLOOR
GN_EPS = 1e-5                 # nn.GroupNorm's default: `normalization` = GroupNorm32(32, channels) (util.py:202-208)
L_E = 6
Y_SINCOS = 1.2                # measured 1.146 on an MI355X, rounded up: header, profile file
E_SINCOS = 2.0 * Y_SINCOS
TS_T = (0.0, 1.0, 17.5, 999.0)
TS_DIMS = (320, 65)

U0 = dict(in_channels=9, out_channels=4, model_channels=64, channel_mult=(1, 2, 3), num_res_blocks=1, attention_resolutions=(1, 2),
          num_heads=1, context_dim=64, legacy=False, transformer_depth=1)
U0_B, U0_H, U0_W, U0_M, U0_T = 2, 8, 12, 9, (981.0, 17.0)


def bar4(yardstick):
    """The device's bar: four times the measured distance between the reference's fp32 module and the float64 restatement."""
    return 4.0 * float(yardstick)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. groupnorm_cat

def _nc(name, B, HW, C0, C1, e=True, silu=True, kind="plain"):
    return dict(name=name, B=B, HW=HW, C0=C0, C1=C1, e=e, silu=silu, kind=kind, groups=32)


GNC_CASES = [
    _nc("seam-192+128", 2, 96, 192, 128),                        # a group across the seam, 10 channels per group
    _nc("wide-1280+1280", 1, 6, 1280, 1280),                     # 640 float4 columns: three channel passes, the last partial; 256 slices, 6 pixels
    _nc("b4-128+64", 4, 35, 128, 64),                            # 64 slices; 6 channels per group; odd HW
    _nc("b5-640+320", 5, 24, 640, 320),                          # 30 channels per group
    _nc("single-64-e", 2, 96, 64, 0),
    _nc("single-64", 2, 96, 64, 0, e=False),
    _nc("single-64-nosilu", 2, 96, 64, 0, e=False, silu=False),
    _nc("slices-of-nan", 2, 96, 192, 128, kind="nan_slices"),    # x0, x1 channel slices of wider tensors whose other columns are NaN
    _nc("constant-group", 2, 96, 64, 64, kind="constant"),
    _nc("e-1e3", 2, 96, 192, 128, kind="big_e"),                 # e = 1e3 on one channel of N(0, 1) data: the cancellation in the statistics
    _nc("inplace-64", 2, 96, 64, 0, kind="alias"),
]


def gnc_input(c):
    """-> x0 [B,HW,C0], x1 [B,HW,C1] or None, e [B,C] or None, gamma, beta (float32, CPU)."""
    g = SC._gen("gnc-" + c["name"])
    B, HW, C0, C1 = c["B"], c["HW"], c["C0"], c["C1"]
    C = C0 + C1
    x0 = torch.randn((B, HW, C0), generator=g) * 1.5 + 0.25
    x1 = torch.randn((B, HW, C1), generator=g) * 0.7 - 0.5 if C1 else None
    e = torch.randn((B, C), generator=g) if c["e"] else None
    if c["kind"] == "constant":                                  # group 1 of every image: one value in x0, e constant over the group
        cpg = C // c["groups"]
        x0[:, :, cpg:2 * cpg] = 0.75
        e[:, cpg:2 * cpg] = -0.25
    if c["kind"] == "big_e":
        x0 = torch.randn((B, HW, C0), generator=g)
        x1 = torch.randn((B, HW, C1), generator=g)
        e = torch.zeros((B, C))
        e[:, 7] = 1e3
        e[1, C0 + 3] = -1e3
    gamma = torch.randn((C,), generator=g) * 0.5 + torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    beta = torch.randn((C,), generator=g)
    return x0, x1, e, gamma, beta


def gnc_reference(x0, x1, e, gamma, beta, groups, eps=GN_EPS):
    """-> (x [B,HW,C] float32, the concatenation; ref) with ref the dict `sd_ops_check.gn_ratios` takes: float64 scale and the
    folded shift [B,C], and the coefficients of |y - y64| <= coef_a |x scale| + coef_b (header)."""
    x = x0 if x1 is None else torch.cat([x0, x1], dim=2)
    B, HW, C = x.shape
    cpg = C // groups
    ed = torch.zeros((B, C), dtype=torch.float64) if e is None else e.double()
    z = (x.double() + ed.view(B, 1, C)).view(B, HW, groups, cpg)
    mag = (x.double().abs() + ed.abs().view(B, 1, C)).view(B, HW, groups, cpg)
    mean = z.mean(dim=(1, 3))
    var = ((z - mean.view(B, 1, groups, 1)) ** 2).mean(dim=(1, 3))
    absmean, sq = mag.mean(dim=(1, 3)), (mag * mag).mean(dim=(1, 3))
    e32 = SC._eps32(eps)
    rstd = 1.0 / torch.sqrt(var + e32)
    L = SC.gn_layout(B, HW, C, groups)["chain"] + 1 + (L_E if e is not None else 0)
    rho = 1.5 * L * U64 * sq / (var + e32) + 2 * U64
    assert float(rho.max()) <= SC.FIRST_ORDER_LIMIT, f"case outside the first-order range of the statistics' bound: {float(rho.max()):.3g}"
    dmean = L * U64 * absmean
    ga, be = SC._affine64(gamma, beta, C)
    ex = lambda t: t.repeat_interleave(cpg, dim=1)
    scale = ex(rstd) * ga
    shift0 = be - ex(mean) * scale
    shift = be - (ex(mean) - ed) * scale
    es = (ed * scale).abs()
    coef_a = SC.K_GN * U + ex(rho)
    coef_b = SC.K_GN * U * (es + shift0.abs()) + U * es + ex(rho) * (ex(mean).abs() + ed.abs()) * scale.abs() + ex(dmean) * scale.abs()
    return x, dict(scale=scale, shift=shift, coef_a=coef_a, coef_b=coef_b)


def gnc_simulate(x0, x1, e, gamma, beta, groups, silu, eps=GN_EPS):
    """The kernels' arithmetic in kernel order on the host: float64 partial sums per slice, the e-shift of every (slice, channel) pair
    of sums, the group statistics, scale and the folded shift rounded to float32, one fused multiply-add (evaluated in float64 and
    rounded once), SiLU in float32.  [B,HW,C] float32."""
    import numpy as np
    x = (x0 if x1 is None else torch.cat([x0, x1], dim=2)).numpy()
    B, HW, C = x.shape
    lay = SC.gn_layout(B, HW, C, groups)
    slices, per, cpg = lay["slices"], lay["per"], C // groups
    out = np.empty_like(x)
    e32 = np.float64(np.float32(eps))
    ga = np.ones(C, np.float32) if gamma is None else gamma.numpy()
    be = np.zeros(C, np.float32) if beta is None else beta.numpy()
    for b in range(B):
        s, q = np.zeros(C), np.zeros(C)
        for sl in range(slices):
            blk = x[b, sl * per:min(HW, (sl + 1) * per)].astype(np.float64)
            S, Q, n = blk.sum(0), (blk * blk).sum(0), float(blk.shape[0])
            if e is not None:
                ec = e[b].numpy().astype(np.float64)
                S, Q = S + n * ec, Q + 2.0 * ec * S + n * ec * ec
            s, q = s + S, q + Q
        n = float(HW * cpg)
        mu = s.reshape(groups, cpg).sum(1) / n
        var = np.maximum(q.reshape(groups, cpg).sum(1) / n - mu * mu, 0.0)
        r = np.repeat(1.0 / np.sqrt(var + e32), cpg) * ga.astype(np.float64)
        ec = np.zeros(C) if e is None else e[b].numpy().astype(np.float64)
        scale = r.astype(np.float32)
        shift = (be.astype(np.float64) - (np.repeat(mu, cpg) - ec) * r).astype(np.float32)
        y = (x[b].astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(np.float32)
        if silu:
            y = y / (np.float32(1.0) + np.exp(-y, dtype=np.float32))
        out[b] = y
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. emb_linear, timestep_embedding

def silu64(x):
    return x * torch.sigmoid(x)


def emb_linear_reference(x, w, bias, silu_in):
    """x [B,K], w [N,K], bias [N] or None (float32) -> (ref64, bound) [B,N] (header)."""
    K = x.shape[1]
    s = silu64(x.double()) if silu_in else x.double()
    ref = s @ w.double().T + (0.0 if bias is None else bias.double())
    mag = s.abs() @ w.double().abs().T
    bound = (K + 2) * U * mag + ((SC.E_EXP + 1 + SC.E_DIV) * U * mag if silu_in else 0.0) + FLOOR
    return ref, bound


def timestep_freqs(dim, max_period=10000):
    """util.py:165-167 verbatim in spirit: the fp32 CPU table."""
    half = dim // 2
    return torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)


def timestep_embedding_reference(t, dim):
    """t [B] float32 -> (ref64, bound) [B, dim] (header)."""
    f = timestep_freqs(dim)
    a = t.double()[:, None] * f.double()[None]
    ref = torch.cat([torch.cos(a), torch.sin(a)], dim=-1)
    bound = torch.cat([U * a.abs() + E_SINCOS * U] * 2, dim=-1)
    if dim % 2:
        ref = torch.cat([ref, torch.zeros_like(ref[:, :1])], dim=-1)
        bound = torch.cat([bound, torch.zeros_like(bound[:, :1])], dim=-1)
    return ref, bound


def sincos_arguments():
    """The float32 arguments the kernel hands to cosf / sinf over the test grid, and a sweep of 0..1000 rad."""
    parts = [(torch.tensor(TS_T)[:, None] * timestep_freqs(d)[None]).flatten() for d in TS_DIMS]
    parts.append(torch.linspace(0.0, 1000.0, 1 << 20))
    return torch.cat(parts).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the model in float64

def _gn_silu(sd, name, x):
    return silu64(F.group_norm(x, 32, sd[f"{name}.weight"], sd[f"{name}.bias"], eps=GN_EPS))


def _conv(sd, name, x, stride=1, pad=1):
    return F.conv2d(x, sd[f"{name}.weight"], sd[f"{name}.bias"], stride=stride, padding=pad)


def time_embed64(sd, t, model_channels):
    """emb = time_embed(timestep_embedding(t)) (:770-771); the table and t are the fp32 values, everything after them float64."""
    te = timestep_embedding_reference(t.float(), model_channels)[0]
    h = te @ sd["time_embed.0.weight"].T + sd["time_embed.0.bias"]
    return silu64(h) @ sd["time_embed.2.weight"].T + sd["time_embed.2.bias"]


def resblock64(sd, name, x, emb):
    """ResBlock._forward (:257-277), use_scale_shift_norm False, no up / down: x [B,C,H,W] (already concatenated), emb [B, 4 mc]."""
    h = _conv(sd, f"{name}.in_layers.2", _gn_silu(sd, f"{name}.in_layers.0", x))
    e = silu64(emb) @ sd[f"{name}.emb_layers.1.weight"].T + sd[f"{name}.emb_layers.1.bias"]
    h = h + e[:, :, None, None]
    h = _conv(sd, f"{name}.out_layers.3", _gn_silu(sd, f"{name}.out_layers.0", h))
    skip = _conv(sd, f"{name}.skip_connection", x, pad=0) if f"{name}.skip_connection.weight" in sd else x
    return skip + h


def upsample64(sd, name, x):
    return _conv(sd, f"{name}.conv", F.interpolate(x, scale_factor=2, mode="nearest"))


@torch.no_grad()
def unet64(sd64, layout, x, timesteps, context, control=None, only_mid_control=False, reference_kv=()):
    """sd64: float64 state dict without prefix; layout: `unet.unet_layout(cfg)`; x [B,C,H,W]; reference_kv: frames of one (k, v)
    [b, n, inner] per transformer; control: NCHW residuals (not consumed) -> (eps float64, [(k, v)] as [B, N, inner])."""
    cfg = layout["cfg"]
    emb = time_embed64(sd64, timesteps, int(cfg["model_channels"]))
    ctx = None if context is None else context.double()
    hists = []

    def block(layers, h):
        for l in layers:
            kind, name = l[0], l[1]
            if kind == "conv":
                h = _conv(sd64, name, h)
            elif kind == "res":
                h = resblock64(sd64, name, h, emb)
            elif kind == "st":
                sub = {k[len(name) + 1:]: v for k, v in sd64.items() if k.startswith(name + ".")}
                ref = [f[len(hists)] for f in reference_kv]
                h, kv = TC.spatial_transformer64(sub, h, l[3], ctx, ref, depth=int(cfg["transformer_depth"]))
                hists.extend(kv)
            elif kind == "down":
                h = _conv(sd64, f"{name}.op", h, stride=2)
            else:
                h = upsample64(sd64, name, h)
        return h

    hs = []
    h = x.double()
    for blk in layout["input"]:
        h = block(blk, h)
        hs.append(h)
    h = block(layout["middle"], h)
    ctl = None if control is None else [c.double() for c in control]
    if ctl is not None:
        h = h + ctl[-1]
    for i, blk in enumerate(layout["output"]):
        skip = hs.pop()
        if ctl is not None and not only_mid_control:
            skip = skip + ctl[-2 - i]
        h = block(blk, torch.cat([h, skip], dim=1))
    return _conv(sd64, "out.2", _gn_silu(sd64, "out.0", h)), hists


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. what the fixture script and the tests regenerate from seeds

def control_residuals(layout, B, H, W, seed=4242):
    """Seeded `control` of ControlledUnetModel.forward: one NCHW residual per input block and one for the middle block."""
    g = torch.Generator().manual_seed(seed)
    out, ds = [], 1
    for blk, ch in zip(layout["input"], layout["skip"]):
        ds = ds * 2 if blk[0][0] == "down" else ds
        out.append(0.1 * torch.randn((B, ch, H // ds, W // ds), generator=g))
    out.append(0.1 * torch.randn(tuple(out[-1].shape), generator=g))
    return out


def transformer_heads(layout):
    return [l[3] for blk in layout["input"] + [layout["middle"]] + layout["output"] for l in blk if l[0] == "st"]


def reference_frames(kv, heads, mode):
    """One reference frame from the stored plain-run history `kv` ([(k, v)] in the reference's [(b h), n, d] layout): mode "all" --
    the two images swapped (batch B), "positive" -- image 0's history (batch B - 1).  -> [[(k, v)] per transformer]."""
    fn = TC.reference_all if mode == "all" else TC.reference_positive
    return [[fn(k, v, h) for (k, v), h in zip(kv, heads)]]


# ResBlocks run alone: name, (channels of x, channels of the skip half or 0), followed by this Upsample or None
RESBLOCK_CASES = [
    ("identity", "input_blocks.1.0", (64, 0), None),
    ("skip1x1-two-segments", "output_blocks.3.0", (128, 64), None),
    ("then-upsample", "output_blocks.1.0", (192, 128), "output_blocks.1.1"),
]
RB_H, RB_W = 5, 7              # odd sizes: neither is a multiple of a tile


def resblock_inputs(case_index, B=U0_B):
    _, _, (c0, c1), _ = RESBLOCK_CASES[case_index]
    g = torch.Generator().manual_seed(9000 + case_index)
    x = torch.randn((B, c0, RB_H, RB_W), generator=g)
    skip = torch.randn((B, c1, RB_H, RB_W), generator=g) * 0.8 + 0.1 if c1 else None
    return x, skip


def u0_inputs():
    g = torch.Generator().manual_seed(2020)
    x = torch.randn((U0_B, U0["in_channels"], U0_H, U0_W), generator=g)
    context = torch.randn((U0_B, U0_M, U0["context_dim"]), generator=g)
    return x, torch.tensor(U0_T), context
