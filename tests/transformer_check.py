"""Float64 restatement of `SpatialTransformer`, and float64 references with derived error bounds for ofx_layernorm and ofx_geglu
(csrc/transformer.hip).  Not a conftest: imported by name, and importable without a device.

    SpatialTransformer.forward               ldm/modules/attention.py:515-537
      BasicTransformerBlock._forward         :464-469
      MemoryEfficientCrossAttention.forward  :326-436   (kv_hist :353, ref_kv_hists :358-369, use_attn_bias = False)
      FeedForward / GEGLU                    :49-76
The restatement is written from the formulas (x + proj_out(blocks(proj_in(GroupNorm(x)))), a block = three pre-norm residual
sub-blocks) on [B, N, inner] tokens with einsum attention, every tensor float64.  PINNED by tests/test_transformer_host.py against
tests/golden/spatial_transformer_ref_c0.npz / _c1.npz, the output of the reference's own module.

u = 2^-24 (sd_ops_check.U).  Bounds are first order, relative to the OPERANDS, with named constants per rounding.

ofx_layernorm.  One wave per row; lane l holds float4 l, l + 64, ... (NV = ln_nv(C) of them).  An element passes through at most
    L_SUM = 2 + NV + 6        additions: (x + y) + (z + w), NV accumulations in the lane, 6 levels of the wave reduction
so the sum is off by at most L_SUM u sum|x| and the mean, one division later, by
    dm <= (L_SUM + LN_DIV) u mean|x|.
The centred value d~ = fl(x - m~) = (x - mu - dm)(1 + u).  Since sum(x - mu) = 0, the mean square of the shifted centred values is
var + dm^2: the shift enters the variance in second order, but relative to var + eps it is dm^2 / (var + eps), which at a row of
mean 1e3 and unit spread is of the order of u and is kept.  The squares carry 2 u (of d~) + 1 u (the product), their sum L_SUM u,
then the division, the addition of eps, the square root and the reciprocal (both correctly rounded: 1 u each; the relative error of
var + eps halves through the root):
    rho = (LN_SQ + L_SUM + LN_DIV + LN_EPS) u / 2 + dm^2 / (2 (var + eps)) + (LN_SQRT + LN_RCP) u
The output (x - m~) rstd~ gamma + beta takes the rounding of d~, two products and the addition (LN_OUT = 4 roundings, of which the
last is relative to |y| <= A + |beta|), with A = |gamma| |x - mu| rstd:
    |y - y64| <= (LN_OUT u + rho) A + |gamma| rstd dm + u |beta|                      (times LN_SLACK for the second-order terms)
The dm term is what makes the bound relative to the operands: a constant row has y = beta up to |gamma| rstd dm, rstd = eps^-1/2.
A variance formed as E[x^2] - mean^2 would be off by ~ C u E[x^2] instead, 1e6 times more at a row of mean 1e3 and unit spread.
eps is the float the ABI receives.

ofx_geglu.  out = x * (0.5 g) * (1 + erff(fl(g k))), k = fl(2^-1/2).  t~ = g / sqrt 2 (1 + 2 u) (the constant and the product), which
moves erf by at most GG_T u |t| erf'(t), erf'(t) = 2 / sqrt(pi) e^(-t^2); erff itself is off by E_ERF u |erf t| (the measured term,
below); 1 + e is rounded (u |1 + erf t|); 0.5 g is exact; the two products add GG_MUL = 2 roundings of the result:
    |out - ref| <= |x| |g| / 2 (GG_T u |t| erf'(t) + E_ERF u |erf t| + u |1 + erf t|) + GG_MUL u |ref| + FLOOR
The bound is relative to the operands: for g <= -4 the result is |x g| / 2 erfc(|t|) ~ 1e-5 |x g| while the error of 1 + erff(t) is
an absolute ~u (the cancellation F.gelu's own formula has).  The reference uses erfc in float64 and so keeps that tail.

Measured term.  Y_ERF: the worst error of the device's erff against float64 erf over the arguments t~ of the GEGLU test grid, in
units of u |erf t| (tools/erff_probe.hip run by tools/spatial_transformer_rate.py --erff-probe, recorded in
profiles/r17_spatial_transformer_rate.txt: 1.970 over 2^21 arguments, the worst at t = 0.0139; Y_ERF = 2.0).  As sd_ops_check does
for its measured E_EXP, the kernel may use up to twice that: E_ERF = 2 Y_ERF = 4.
Worst ratios |error| / bound measured on an MI355X over tests/test_gpu_transformer.py (printed by the tests, -s to re-measure):
LayerNorm 0.93 (37x640 in place; 0.15 at mean 1e3, 0 at the constant rows), GEGLU @@GG@@.
"""
import math

import torch
import torch.nn.functional as F

import sd_ops_check as SC

U = SC.U
FLOOR = SC.FLOOR
LN_EPS_DEFAULT = 1e-5
LN_DIV, LN_SQ, LN_EPS, LN_SQRT, LN_RCP, LN_OUT = 1, 3, 1, 1, 1, 4
LN_SLACK = 1.001
GG_T, GG_MUL = 2, 2
Y_ERF = 2.0           # measured 1.970 on an MI355X (torch's float32 erf on the host: 1.180), rounded up: header, profile file
E_ERF = 2.0 * Y_ERF

INV_SQRT2_F32 = float(torch.tensor(0.70710678118654752440, dtype=torch.float32).double())


def bar_of(ref):
    """The project's bar for whole networks in fp32 (tests/test_gpu_vae.py)."""
    return 2e-4 * max(1.0, float(ref.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the module in float64

def to64(sd):
    return {k: v.double() for k, v in sd.items()}


def _ln(sd, name, x):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + LN_EPS_DEFAULT) * sd[f"{name}.weight"] + sd[f"{name}.bias"]


def _heads(t, h):
    B, N, inner = t.shape
    return t.reshape(B, N, h, inner // h).permute(0, 2, 1, 3)              # [B, h, N, d]


def _attend(q, k, v, h):
    """q [B,Nq,inner], k / v [B,Nk,inner] -> softmax(q k^T d^-1/2) v per head, [B,Nq,inner]."""
    qh, kh, vh = _heads(q, h), _heads(k, h), _heads(v, h)
    p = torch.softmax(torch.einsum("bhqd,bhkd->bhqk", qh, kh) * (qh.shape[-1] ** -0.5), -1)
    o = torch.einsum("bhqk,bhkd->bhqd", p, vh)
    return o.permute(0, 2, 1, 3).reshape(q.shape)


def heads_first(t, h):
    """[B, N, h*d] -> [(b h), n, d], the layout of the reference's kv_hist."""
    B, N, inner = t.shape
    return _heads(t, h).reshape(B * h, N, inner // h)


def heads_last(t, h):
    BH, N, d = t.shape
    return t.reshape(BH // h, h, N, d).permute(0, 2, 1, 3).reshape(BH // h, N, h * d)


def reference_all(k, v, heads):
    """The batch-B references of the stored runs: a [(b h), n, d] history of a batch of 2 with the two images swapped."""
    sw = lambda t: t.reshape(2, heads, *t.shape[1:]).flip(0).reshape(t.shape).contiguous()
    return sw(k), sw(v)


def reference_positive(k, v, heads):
    """The batch B - 1 references of the stored runs: the history of image 0 alone (B = 2)."""
    return k[:heads].clone(), v[:heads].clone()


@torch.no_grad()
def spatial_transformer64(sd64, x, heads, context=None, reference_kv=(), depth=1):
    """sd64: the state dict in float64; x [B,C,h,w]; context [B,M,ctx], a list of one per block, or None; reference_kv: (k, v) pairs
    [b, n, inner] in float64 -> (out float64 [B,C,h,w], [(k, v)] per block as [B, N, inner])."""
    x = x.double()
    B, C, h, w = x.shape
    t = F.group_norm(x, 32, sd64["norm.weight"], sd64["norm.bias"], eps=1e-6)
    t = F.conv2d(t, sd64["proj_in.weight"], sd64["proj_in.bias"])
    inner = t.shape[1]
    t = t.reshape(B, inner, h * w).permute(0, 2, 1)
    N = h * w
    ctxs = list(context) if isinstance(context, (list, tuple)) else [context] * depth
    hists = []
    for i in range(depth):
        b = f"transformer_blocks.{i}"
        lin = lambda name, z, bias=False: z @ sd64[f"{b}.{name}.weight"].T + (sd64[f"{b}.{name}.bias"] if bias else 0.0)
        hn = _ln(sd64, f"{b}.norm1", t)
        q, k, v = lin("attn1.to_q", hn), lin("attn1.to_k", hn), lin("attn1.to_v", hn)
        hists.append((k, v))
        if reference_kv:
            k2 = torch.cat([e[0].double() for e in reference_kv], 1)
            v2 = torch.cat([e[1].double() for e in reference_kv], 1)
            if k2.shape[0] == B:
                k, v = k2, v2
            else:
                assert k2.shape[0] == B - 1 and k2.shape[1] == N
                k, v = torch.cat([k[:1], k2]), torch.cat([v[:1], v2])
        t = lin("attn1.to_out.0", _attend(q, k, v, heads), True) + t
        hn = _ln(sd64, f"{b}.norm2", t)
        src = hn if ctxs[i] is None else ctxs[i].double()
        t = lin("attn2.to_out.0", _attend(lin("attn2.to_q", hn), lin("attn2.to_k", src), lin("attn2.to_v", src), heads), True) + t
        a = lin("ff.net.0.proj", _ln(sd64, f"{b}.norm3", t), True)
        half = a.shape[-1] // 2
        gate = a[..., half:]
        t = lin("ff.net.2", a[..., :half] * (0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0)))), True) + t
    t = t.permute(0, 2, 1).reshape(B, inner, h, w)
    return F.conv2d(t, sd64["proj_out.weight"], sd64["proj_out.bias"]) + x, hists


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm

def ln_nv(C):
    """float4 per lane of layernorm_kernel for a row of C floats (the instantiations of ofx_layernorm)."""
    need = -(-C // 256)
    return next(nv for nv in (1, 2, 3, 5, 8, 16) if need <= nv)


def ln_reference(x, gamma, beta, eps=LN_EPS_DEFAULT):
    """x [rows, C] float32, gamma / beta [C] or None -> (y64, bound) [rows, C] (header)."""
    rows, C = x.shape
    xd = x.double()
    e = SC._eps32(eps)
    ga = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    mu = xd.mean(1, keepdim=True)
    d = xd - mu
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + e)
    y = d * rstd * ga + be
    l_sum = 2 + ln_nv(C) + 6
    dm = (l_sum + LN_DIV) * U * xd.abs().mean(1, keepdim=True)
    rho = (LN_SQ + l_sum + LN_DIV + LN_EPS) * U / 2 + dm * dm / (2 * (var + e)) + (LN_SQRT + LN_RCP) * U
    A = ga.abs() * d.abs() * rstd
    bound = LN_SLACK * ((LN_OUT * U + rho) * A + ga.abs() * rstd * dm + U * be.abs())
    return y, bound


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. GEGLU

def gelu64(g):
    """g/2 (1 + erf(g / sqrt 2)) in float64 with the negative tail kept: 1 + erf(t) = erfc(-t)."""
    return 0.5 * g * torch.special.erfc(-g / math.sqrt(2.0))


def geglu_reference(a, inner):
    """a [rows, >= 2*inner] float32 -> (ref64, bound) [rows, inner] (header)."""
    x, g = a[:, :inner].double(), a[:, inner:2 * inner].double()
    ref = x * gelu64(g)
    t = g / math.sqrt(2.0)
    erf = torch.erf(t)
    dterm = GG_T * U * t.abs() * (2.0 / math.sqrt(math.pi)) * torch.exp(-t * t) + E_ERF * U * erf.abs() + U * torch.special.erfc(-t)
    bound = x.abs() * g.abs() * 0.5 * dterm + GG_MUL * U * ref.abs() + FLOOR
    return ref, bound


def geglu_gates(n, gen):
    """n gate values: random ones of unit scale, and the special ones -- +-20 (erf saturated: the product with a negative gate must
    round to +-0, not NaN), +-0.0, values around +-1e-4, and the range -6..-3 where 1 + erf cancels."""
    special = torch.tensor([20.0, -20.0, 0.0, -0.0, 1e-4, -1e-4, 1.3e-4, -0.7e-4, -3.0, -4.0, -5.0, -5.5, -6.0, 3.0, 5.0, 0.5, -0.5])
    g = torch.randn((n,), generator=gen) * 1.5
    m = min(n, special.numel())
    idx = torch.randperm(n, generator=gen)[:m]
    g[idx] = special[:m]
    return g


def erff_arguments(g):
    """The float32 arguments the kernel hands to erff for float32 gates g: fl(g * fl(2^-1/2))."""
    return (g.float() * torch.tensor(0.70710678118654752440, dtype=torch.float32))
