"""Float64 restatement of the CLIP text encoder as hack.py drives it, the test configuration and its inputs, and float64 references
with derived bounds for `ofx_clip_embed` and `ofx_quick_gelu`.  Not a conftest: imported by name, and importable without a device.

    _hacked_clip_forward        hack.py:32-70       (chunks of 75, [bos] + piece + [eos] padded to 77, clip_skip, the rearranges)
    FrozenCLIPEmbedder          ldm/modules/encoders/modules.py   (transformers' CLIPTextModel, hidden_act quick_gelu)
The forward is restated from those lines and from the formulas of CLIP's text tower: token + position embedding; per layer
x += out_proj(softmax(q k^T d^-0.5 + triu(-inf, 1)) v) on LayerNorm(x), x += fc2(quick_gelu(fc1(LayerNorm(x)))), quick_gelu(m) =
m sigmoid(1.702 m), every LayerNorm with eps 1e-5 and the biased variance; final_layer_norm on the last layer's output, or on
hidden_states[-clip_skip] (the embedding output and every layer output, layers + 1 entries) when clip_skip > 1.  PINNED by
tests/test_text_encoder_host.py against tests/golden/clip_text_ref_t0.npz, the output of the reference's own embedder.

ofx_clip_embed.  One fp32 addition per element: the reference is `tok[ids] + pos[arange(rows) % T]` in fp32, and the bar is
bit-identity.  A row whose id is outside [0, vocab) must be all NaN and every other row bit-identical.

ofx_quick_gelu (u = 2^-24).  The kernel evaluates x / (1 + expf(-(c x))), c = fl(1.702).  Against r = x sigma(t), t = 1.702 x,
sigma(t) = 1 / (1 + e^-t), per element:
  * the argument: c differs from 1.702 by at most u relative and the product c x is rounded once, so the exponent is off by at
    most 2 u |t| and e = expf(.) carries a relative error of 2 u |t| + E_EXP u (E_EXP: sd_ops_check's measured allowance for the
    device's expf);
  * the sum s = 1 + e: e's error enters s with the weight e / (1 + e) = 1 - sigma(t), the addition adds u;
  * the division adds E_DIV u (sd_ops_check's allowance for a division).
    |out - r| <= ((2 |t| + E_EXP) (1 - sigma(t)) + 1 + E_DIV) u |r| (1 + SECOND_ORDER) + FLOOR + |x| 2^-128
SECOND_ORDER = 1e-3 covers the products of the terms above (the largest, 2 u |t|, is 2e-5 at |x| = 100).  FLOOR = 4 * 2^-126
(sd_ops_check's) covers results below the normal range, flushed or denormal.  |x| 2^-128 covers the overflow of the exponential:
once e > FLT_MAX < 2^128 (x < -52.1) the sum is +inf and the quotient -0, where r = x / (1 + e) is smaller than |x| 2^-128 in
magnitude.  No constant is measured here: E_EXP, E_DIV and FLOOR are sd_ops_check's.

The bar for the encoder is `unet_check.bar4`, the factor ControlNet's parity test uses: four times the distance of the
reference's fp32 module from this restatement, stored per output by tests/golden/make_golden_text_encoder.py (`ref_dist`).  The
bar of a hidden state, and of inputs the golden file does not hold (T = 20, the causality probe), is four times the distance of
this restatement run in torch fp32 from itself in float64 on the same input (`fp32_yardsticks`).
"""
import torch

import sd_ops_check as SC
import unet_check as UC

U = SC.U
SECOND_ORDER = 1e-3
SENTINEL = 12345.0

# Head size 64 is the production head size; two heads make the head indexing matter; three layers make clip_skip 2 and 3 differ
# from each other and from the default.
T0 = dict(vocab=512, width=128, heads=2, layers=3, intermediate=512, positions=77)
T0_BOS, T0_EOS, T0_PAD = 510, 511, 511
T0_SEED = 4040
T0_SKIPS = (0, 2, 3)
PLANTED = ("mask-dropped", "gelu-1.0", "positions-shifted", "clip-skip-off-by-one")
PLANTED_FACTOR = 100.0


def t0_inputs():
    """Two prompts as raw id lists: 100 ids (spills into chunk 2) and 5 ids (chunks 2 and 3 are empty); ids in [0, 510)."""
    g = torch.Generator().manual_seed(T0_SEED)
    return [torch.randint(0, T0_BOS, (n,), generator=g).tolist() for n in (100, 5)]


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the model in float64 (or, for the yardsticks, the same statements in fp32)

def _ln(x, g, b, eps=1e-5):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g + b


@torch.no_grad()
def clip_text64(sd, cfg, ids, clip_skip=0, hidden_states=False, dtype=torch.float64, plant=None):
    """sd: state dict without prefix (keys of `text_encoder.clip_text_tensors`); ids integer [S,T] -> final_layer_norm(h) [S,T,width]
    in `dtype`, h chosen by clip_skip as hack.py:42-47 does; with hidden_states, (that, [embedding output, layer outputs...]).
    plant: one of PLANTED, a deliberate mistake (tests only)."""
    assert plant is None or plant in PLANTED
    W, H, L = int(cfg["width"]), int(cfg["heads"]), int(cfg["layers"])
    d = W // H
    ids = torch.as_tensor(ids).long()
    S, T = ids.shape
    p = lambda k: sd[k].to(dtype)
    lin = lambda x, name: x @ p(f"{name}.weight").t() + p(f"{name}.bias")
    positions = torch.arange(T)
    if plant == "positions-shifted":
        positions = (positions + 1) % int(cfg["positions"])
    x = p("embeddings.token_embedding.weight")[ids] + p("embeddings.position_embedding.weight")[positions]
    mask = torch.full((T, T), float("-inf"), dtype=dtype).triu(1)
    if plant == "mask-dropped":
        mask = torch.zeros((T, T), dtype=dtype)
    alpha = 1.0 if plant == "gelu-1.0" else 1.702
    k = int(clip_skip) + (1 if plant == "clip-skip-off-by-one" else 0)
    run = L if k <= 1 else L + 1 - k
    hs = [x]
    for i in range(run):
        l = f"encoder.layers.{i}"
        h = _ln(x, p(f"{l}.layer_norm1.weight"), p(f"{l}.layer_norm1.bias"))
        q, kk, v = (lin(h, f"{l}.self_attn.{n}").view(S, T, H, d).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        prob = torch.softmax(q @ kk.transpose(-1, -2) * d ** -0.5 + mask, dim=-1)
        x = x + lin((prob @ v).transpose(1, 2).reshape(S, T, W), f"{l}.self_attn.out_proj")
        m = lin(_ln(x, p(f"{l}.layer_norm2.weight"), p(f"{l}.layer_norm2.bias")), f"{l}.mlp.fc1")
        x = x + lin(m * torch.sigmoid(alpha * m), f"{l}.mlp.fc2")
        hs.append(x)
    out = _ln(x, p("final_layer_norm.weight"), p("final_layer_norm.bias"))
    return (out, hs) if hidden_states else out


@torch.no_grad()
def forward_tokens64(sd, cfg, tokens, clip_skip=0, plant=None):
    """hack.py:64-70: tokens [B,F,T] -> [B, F*T, width] float64."""
    tokens = torch.as_tensor(tokens)
    B, Fn, T = tokens.shape
    return clip_text64(sd, cfg, tokens.reshape(B * Fn, T), clip_skip, plant=plant).reshape(B, Fn * T, int(cfg["width"]))


@torch.no_grad()
def fp32_yardsticks(sd, cfg, ids, clip_skip=0):
    """(distance of the output, [distance per hidden state]): max |fp32 run - float64 run| of this restatement on `ids`; sd fp32."""
    o32, h32 = clip_text64(sd, cfg, ids, clip_skip, hidden_states=True, dtype=torch.float32)
    o64, h64 = clip_text64(to64(sd), cfg, ids, clip_skip, hidden_states=True)
    return float((o32.double() - o64).abs().max()), [float((a.double() - b).abs().max()) for a, b in zip(h32, h64)]


bar4 = UC.bar4


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. ofx_clip_embed: cases, inputs, reference

def _ec(rows, T, C, ldo, vocab, bad=False):
    return dict(name=f"r{rows}-t{T}-c{C}-ld{ldo}" + ("-bad-ids" if bad else ""), rows=rows, T=T, C=C, ldo=ldo, vocab=vocab, bad=bad)


# one row of one float4; one 77-token sequence; the production shape of six sequences; T < 77 with slack columns (rows 5..9 reuse
# positions 0..4); rows past 65535 (more float4 than one trip of the largest grid needs is not required: the row index passes 2^16)
EMBED_CASES = [_ec(1, 1, 4, 4, 97), _ec(77, 77, 128, 128, 97), _ec(462, 77, 768, 768, 97), _ec(10, 5, 128, 160, 97),
               _ec(70000, 77, 4, 4, 97), _ec(77, 77, 128, 128, 97, bad=True)]
EMBED_BAD_ROWS = {5: -1, 40: None}            # row -> id; None: `vocab`, the first id past the table


def embed_input(c):
    """-> ids int32 [rows] (id vocab - 1 in the last row, 0 in the first when there are two), tok [vocab,C], pos [T + 3, C]."""
    g = SC._gen("ce-" + c["name"])
    ids = torch.randint(0, c["vocab"], (c["rows"],), generator=g).to(torch.int32)
    ids[0] = 0
    ids[-1] = c["vocab"] - 1
    if c["bad"]:
        for r, v in EMBED_BAD_ROWS.items():
            ids[r] = c["vocab"] if v is None else v
    return ids, torch.randn((c["vocab"], c["C"]), generator=g), torch.randn((c["T"] + 3, c["C"]), generator=g)


def embed_reference(ids, tok, pos, c):
    """fp32 `tok[ids] + pos[arange(rows) % T]`; rows with an id out of range are NaN."""
    ok = (ids >= 0) & (ids < c["vocab"])
    ref = tok[ids.long().clamp(0, c["vocab"] - 1)] + pos[torch.arange(c["rows"]) % c["T"]]
    ref[~ok] = float("nan")
    return ref, ok


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. ofx_quick_gelu: cases, input sets, reference and bound

QGELU_CASES = [dict(name=f"r{r}-n{n}-ldx{lx}-ldo{lo}", rows=r, n=n, ldx=lx, ldo=lo)
               for r, n, lx, lo in ((1, 4, 4, 4), (77, 512, 512, 512), (462, 3072, 3072, 3072), (33, 128, 192, 160))]
QGELU_SETS = ("normal", "zeros", "tiny", "sweep")


def qgelu_input(c, kind):
    """x [rows, n] fp32: normal (sigma 3); +-0; +-1e-30; a sweep over [-100, 100] (both ends of expf, -80 among the overflows)."""
    rows, n = c["rows"], c["n"]
    g = SC._gen(f"qg-{c['name']}-{kind}")
    sign = torch.where(torch.rand((rows, n), generator=g) < 0.5, -1.0, 1.0)
    if kind == "normal":
        return 3.0 * torch.randn((rows, n), generator=g)
    if kind == "zeros":
        return sign * 0.0
    if kind == "tiny":
        return sign * 1e-30
    assert kind == "sweep"
    x = torch.linspace(-100.0, 100.0, rows * n).reshape(rows, n).clone()
    x.view(-1)[1] = -80.0                                          # the ends stay -100 and 100
    return x


def qgelu_reference(x):
    """-> (ref64, bound) per element (header)."""
    x = x.double()
    t = 1.702 * x
    one_minus_sigma = 1.0 / (1.0 + torch.exp(t))
    r = x / (1.0 + torch.exp(-t))
    rel = ((2.0 * t.abs() + SC.E_EXP) * one_minus_sigma + 1.0 + SC.E_DIV) * U
    return r, rel * r.abs() * (1.0 + SECOND_ORDER) + SC.FLOOR + x.abs() * 2.0 ** -128


def worst_ratio(got, ref, bound):
    return SC._worst((got.double() - ref).abs(), bound)
