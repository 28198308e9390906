"""Float64 restatements, derived error bounds and case tables for ofx_groupnorm, ofx_softmax_rows and the unfused branch of
ofx_attention_f32 (csrc/sd_ops.hip).  Not a conftest: imported by name, and importable without a device.

u = 2^-24 is the fp32 unit round-off (a correctly rounded operation is off by at most u times its result), u64 = 2^-53.

ofx_groupnorm.  The statistics are f64 sums, so with scale = rstd gamma and shift = beta - mean rstd gamma taken in float64, the fp32
roundings are three: scale (u |scale|), shift (u |shift|) and the fused multiply-add (u |y|, |y| <= |x scale| + |shift|):
    |y - y64| <= u |x scale| + u |shift| + u (|x scale| + |shift|) = K_GN u (|x scale| + |shift|),    K_GN = 2
(2.001 carries the second-order terms and the f64 roundings of the products.)  The bound is relative to the OPERANDS of the
multiply-add, not to its result: a constant group has y = beta exactly while |x scale| = |shift| = |x| / sqrt(eps).
To this the f64 statistics add their own error, which the summation order bounds: an element passes through at most
    L = ceil(per / rws) + rws + cpg ceil(slices / tpg) + tpg
additions (the strided loop of a thread row, the thread rows of a slice, a finalize thread's share of the slices, the shares of a
group), so the sums S, Q are off by at most L u64 sum|x| and L u64 sum x^2.  With var = Q/n - mean^2 (|mean| mean|x| <= E[x^2]):
    d mean <= (L + 1) u64 mean|x|,     d var <= 3 (L + 1) u64 E[x^2],     rho = |d rstd / rstd| <= 1.5 (L + 1) u64 E[x^2] / (var + eps) + 2 u64
    |d scale| <= rho |scale|,           |d shift| <= rho |mean scale| + d mean |scale|
first order in rho, which `gn_reference` asserts stays below FIRST_ORDER_LIMIT.  (E[x^2] / (var + eps) is 5e5 for a constant group
and 1e6 for |mean| / std = 1e3: there rho reaches a few u and is no longer negligible, which is why it is spelt out.)
eps is the float the ABI receives: the reference uses float32(eps), not the decimal literal.

ofx_softmax_rows.  The logit v = x scale + bias is formed with two roundings (one if the compiler contracts it):
    |dv| <= u |x scale| + u |v|,        and the subtraction of the maximum adds u |v - max|:       Delta_j = u (|x scale| + |v| + |v - max|)
A softmax whose logits move by at most Delta_i has p~_j = p_j e^(d_j) / sum_i p_i e^(d_i), |d_i| <= Delta_i, and since
(sum p_i e^-Delta_i)(sum p_i e^Delta_i) >= 1:          |p~_j / p_j - 1| <= e^(Delta_j) S+ - 1,      S+ = sum_i p_i e^(Delta_i).
The sum of the exponentials takes ceil(n / 256) sequential additions per thread and 8 tree levels, the product with the reciprocal
one more rounding: K_SUM(n) = ceil(n / 256) + 9 roundings of u each, relative to positive partial sums.  What cannot be derived is
the device's expf (once in the numerator, and through the sum, where a relative error of every term is at most that of the sum)
and its reciprocal: E_EXP and E_DIV below.  In all
    |p~_j - p_j| <= p_j (e^(Delta_j) S+ - 1 + (K_SUM(n) + 2 E_EXP + E_DIV) u) + FLOOR
FLOOR = 4 * 2^-126 covers exponentials below the normal range (flushed or denormal: absolute error 2^-126, the sum is >= 1).

Unfused attention.  A score is a sum of D products on the fp32 matrix cores: every term passes through at most D roundings
(its product, then at most D - 1 additions, in any order), then the scaling and the bias addition as above:
    Delta_j = (D + 4) u sum_d |q_d k_d| |scale| + 2 u |bias_j| + u |v_j - max|            (2 of the 4: the scaling and the addition;
                                                                                           2: second-order slack up to D = 512)
The probabilities carry r_j = e^(Delta_j) S+ - 1 + (K_SUM(Nk) + 2 E_EXP + E_DIV) u, and the second product adds (Nk + 4) u of its
terms (Nk roundings, zero padding adds none):
    |out_d - ref_d| <= sum_j p_j r_j |v_jd| + (Nk + 4) u sum_j p_j (1 + r_j) |v_jd| + FLOOR sum_j |v_jd|

SiLU after GroupNorm: y / (1 + expf(-y)).  d/dy of y sigmoid(y) is at most 1.1, so the error of y enters as 1.1 |dy|; the evaluation
itself is expf (relative E_EXP u e / (1 + e) <= E_EXP u), the addition (u) and the division (E_DIV u):
    |out - silu(y64)| <= 1.1 bound(y) + (E_EXP + 1 + E_DIV) u |silu(y64)| + FLOOR

Measured term (expf and the division).  Yardstick: the error of a CPU fp32 evaluation (torch, float32) of the same formula on the
same inputs against float64, in units of u of the result -- `exp_yardstick`, `div_yardstick`; the CPU test
test_the_cpu_yardstick_is_where_the_header_says re-measures them over the tables' own inputs.
    Y_EXP = 1.1 (measured 1.02 over the softmax and attention tables and the SiLU arguments, rounded up)
    Y_DIV = 1.0 (IEEE division: correctly rounded, measured 1.00)
The kernel may use up to twice that, for a different but equally accurate expf:  E_EXP = 2 Y_EXP = 2.2,  E_DIV = 2 Y_DIV = 2.
Worst ratios measured on an MI355X (gfx950) over tests/test_gpu_sd_ops.py, 2026-10-18, with the NaN-row fix of
ofx_attention_f32 in place (the tests print every ratio, run with -s to re-measure).  A ratio is |error| / bound over the elements,
inside when <= 1; "measured-term use" is the part of the error beyond the derived terms over the measured allowance (0: the derived
terms alone cover the error); margin = 1 / ratio.
    test_groupnorm_against_float64, no SiLU                    0.928  (c512-g32-hw4099)                   margin 1.08
    test_groupnorm_against_float64, SiLU                       0.493  (c1280-g32-hw4099)                  margin 2.03
        measured-term use                                      0.080  (c1280-g32-hw4099; 0 in five of the seven SiLU cases)
    test_groupnorm_apply_takes_its_grid_stride_trip            0.963 without SiLU, 0.503 with             margin 1.04 / 1.99
    test_softmax_rows_against_float64                          0.479  (n256-wide-row)                     margin 2.09
    test_unfused_attention_against_float64, exact workspace    0.064  (d4-nk33-last-row-of-last-head)     margin 15.7
        one batch-head at a time                               0.064  (the same case; equal in every case) margin 15.7
  In every softmax and attention case the NaN rows are exactly the planted ones.  (The GroupNorm ratios sit near 1 because the
  bound is the worst case of three roundings, K_GN = 2, and tensors of 1e6 to 7e7 elements come close to it; the attention bound is
  a worst case over D + Nk roundings, which random data stays far inside.)
"""
import math

import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 1e-300
FLOOR = 4 * 2.0 ** -126
K_GN = 2.001
FIRST_ORDER_LIMIT = 2e-4
Y_EXP, Y_DIV = 1.1, 1.0
E_EXP, E_DIV = 2.0 * Y_EXP, 2.0 * Y_DIV
SILU_SLOPE = 1.1
GN_EPS = 1e-6

EINVAL, EALIGN, ENOMEM = -1, -2, -3          # include/ofx.h


def _cdiv(a, b):
    return -(-a // b)


def _round_up(a, m):
    return _cdiv(a, m) * m


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


def _worst(err, bound):
    """max err / bound with NaN (and inf) counted as infinite."""
    r = err / bound.clamp_min(TINY)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def exp_yardstick(t):
    """float32 t -> the worst error of torch's float32 exp against float64 in units of u exp(t), over the arguments whose
    exponential is a normal number."""
    t = t.float().flatten()
    t = t[torch.isfinite(t) & (t > -87.0) & (t < 88.0)]
    ref = torch.exp(t.double())
    return _worst((torch.exp(t).double() - ref).abs(), U * ref)


def div_yardstick(a, b):
    """float32 a / b against float64, in units of u |a / b|, over the quotients that are normal numbers."""
    ref = a.double() / b.double()
    ok = torch.isfinite(ref) & (ref.abs() >= 2.0 ** -126)
    return _worst(((a / b).double() - ref).abs()[ok], U * ref.abs()[ok])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. GroupNorm

KINDS = ("plain", "constant", "bigmean", "tinyvar", "large")


def _gc(name, B, HW, C, groups, data="mixed", affine="both", silu=False, alias=False):
    return dict(name=name, B=B, HW=HW, C=C, groups=groups, data=data, affine=affine, silu=silu, alias=alias)


# layout reached (gn_layout): ncg/rws per channel pass, slices, per, tpg, cpg, finalize passes
GN_CASES = [
    # ncg 1, rws 256 (one thread column); 256 slices of one pixel, 193 of them empty; ONE group: tpg 256, every data kind
    _gc("c4-g1-plain", 3, 63, 4, 1, data="plain"),
    _gc("c4-g1-constant", 3, 63, 4, 1, data="constant", silu=True),
    _gc("c4-g1-bigmean", 3, 63, 4, 1, data="bigmean"),
    _gc("c4-g1-tinyvar", 3, 63, 4, 1, data="tinyvar", silu=True),
    _gc("c4-g1-large", 3, 63, 4, 1, data="large"),
    # one pixel, groups = C (cpg 1, tpg 64): every group is a single value
    _gc("c4-gC-hw1", 1, 1, 4, 4, data="plain"),
    # B = 5: 64 slices, 63 empty; gamma NULL
    _gc("c32-g1-hw1-b5", 5, 1, 32, 1, data="plain", affine="no_gamma", silu=True),
    # ncg 8, rws 32; per 1, every slice full; groups = C = 32: cpg 1, tpg 8
    _gc("c32-gC-hw256", 1, 256, 32, 32),
    # ncg 16, rws 16; per 2: 128 full slices, one of a single pixel, 127 empty; in place
    _gc("c64-g32-hw257-inplace", 3, 257, 64, 32, silu=True, alias=True),
    # B = 4: 64 slices, per 5 (51 full, one of 2 pixels, 12 empty); ncg 32, rws 8; beta NULL
    _gc("c128-g32-hw257-b4", 4, 257, 128, 32, affine="no_beta"),
    # ncg 80, rws 3 (16 idle threads), per 4 > rws: a second trip of the strided loop; 250 full slices and 6 empty; cpg 10
    _gc("c320-g32-hw1000", 1, 1000, 320, 32, silu=True),
    # 5 groups of 12 channels: tpg 51 (one idle finalize thread), ncg 15, rws 17 (one idle thread)
    _gc("c60-g5-hw1000", 3, 1000, 60, 5),
    # ncg 128, rws 2, per 17: nine trips
    _gc("c512-g32-hw4099", 1, 4099, 512, 32),
    # ncg 256, rws 1; 512 groups: tpg 1, two finalize passes, cpg 2; B = 4
    _gc("c1024-g512-hw63-b4", 4, 63, 1024, 512, silu=True),
    # groups = C = 1024: four finalize passes, cpg 1
    _gc("c1024-gC-hw257", 1, 257, 1024, 1024),
    # C = 1280: a second channel pass with ncg 64, rws 4; no affine parameters at all
    _gc("c1280-g32-hw63", 3, 63, 1280, 32, affine="none"),
    # the second channel pass with multi-pixel slices (per 17 > rws 4)
    _gc("c1280-g32-hw4099", 1, 4099, 1280, 32, silu=True),
    # B = 5 with per 65 > rws 8; in place
    _gc("c128-g32-hw4099-b5-inplace", 5, 4099, 128, 32, alias=True),
    # one thread column whose strided loop makes a second trip: per 313 > rws 256 (B = 4: 64 slices)
    _gc("c4-g1-hw20000-b4", 4, 20000, 4, 1, data="plain"),
]
GN_LARGE = _gc("apply-grid-stride", 2, 66000, 512, 32, data="plain")         # B HW C / 4 = 16 896 000 > 65536 * 256


def gn_layout(B, HW, C, groups):
    """The thread layouts of gn_partial_kernel / gn_finalize_kernel / gn_apply_kernel for a shape, restated."""
    cg = C // 4
    passes = [(min(256, cg - c0), 256 // min(256, cg - c0)) for c0 in range(0, cg, 256)]
    slices = 64 if B >= 4 else 256
    per = _cdiv(HW, slices)
    tpg = 1 if groups >= 256 else 256 // groups
    cpg = C // groups
    return dict(passes=passes, ncg=[p[0] for p in passes], rws=[p[1] for p in passes], slices=slices, per=per,
                full=HW // per, nonempty=_cdiv(HW, per), tpg=tpg, cpg=cpg, fin_passes=_cdiv(groups, 256 // tpg),
                idle=any(n * r < 256 for n, r in passes), trips=max(_cdiv(per, r) for _, r in passes),
                chain=max(_cdiv(per, r) + r for _, r in passes) + cpg * _cdiv(slices, tpg) + tpg,
                apply_trips=_cdiv(B * HW * cg, 65536 * 256))


def gn_input(c):
    """x [B, HW, C] float32, gamma, beta ([C] or None): the data kind of group g of image b is c['data'], or for 'mixed'
    KINDS[(g + b) % 5]; values distinct per image and channel wherever the kind allows it."""
    g = _gen(c["name"])
    B, HW, C, G = c["B"], c["HW"], c["C"], c["groups"]
    cpg = C // G
    base = torch.randn((B, HW, C), generator=g)
    bi = torch.arange(B, dtype=torch.float32).view(B, 1, 1)
    ci = torch.arange(C, dtype=torch.float32).view(1, 1, C)
    gi = (torch.arange(C) // cpg).view(1, 1, C)
    if c["data"] == "mixed":
        kind = (gi + torch.arange(B).view(B, 1, 1)) % len(KINDS)
    else:
        kind = torch.full((B, 1, C), KINDS.index(c["data"]))
    gf = gi.float()
    x = base * 2.0 + 0.5 + 0.25 * bi + 0.01 * (ci % 32)
    x = torch.where(kind == 1, (0.75 + 0.125 * bi + 0.0625 * (gf % 8)).expand_as(x), x)
    x = torch.where(kind == 2, (100.0 + bi + gf % 7) + 0.1 * base, x)
    x = torch.where(kind == 3, (0.5 + 0.03125 * (gf % 4)) + 1e-5 * base, x)
    x = torch.where(kind == 4, torch.where(base < 0, -1.0, 1.0) * 1e4 * (1.0 + 0.01 * bi + 0.001 * (ci % cpg)), x)
    gamma = torch.randn((C,), generator=g) * 0.5 + torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    beta = torch.randn((C,), generator=g)
    if c["affine"] in ("no_gamma", "none"):
        gamma = None
    if c["affine"] in ("no_beta", "none"):
        beta = None
    return x.contiguous(), gamma, beta


def _affine64(gamma, beta, C):
    ga = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(C, dtype=torch.float64) if beta is None else beta.double()
    return ga, be


def _eps32(eps):
    return float(torch.tensor(eps, dtype=torch.float32).double())


def gn_reference(x, gamma, beta, groups, eps=GN_EPS, layout=None):
    """float64 scale, shift [B, C] and the per-(image, channel) coefficients of the bound on y = x scale + shift:
    |y - y64| <= coef_a |x scale| + coef_b  (header).  Two-pass variance: the reference does not share the kernel's cancellation."""
    B, HW, C = x.shape
    cpg = C // groups
    lay = layout or gn_layout(B, HW, C, groups)
    xd = x.double().view(B, HW, groups, cpg)
    mean = xd.mean(dim=(1, 3))
    var = ((xd - mean.view(B, 1, groups, 1)) ** 2).mean(dim=(1, 3))
    absmean, sq = xd.abs().mean(dim=(1, 3)), (xd * xd).mean(dim=(1, 3))
    e = _eps32(eps)
    rstd = 1.0 / torch.sqrt(var + e)
    L = lay["chain"] + 1
    rho = 1.5 * L * U64 * sq / (var + e) + 2 * U64
    assert float(rho.max()) <= FIRST_ORDER_LIMIT, f"case outside the first-order range of the statistics' bound: {float(rho.max()):.3g}"
    dmean = L * U64 * absmean
    ga, be = _affine64(gamma, beta, C)
    ex = lambda t: t.repeat_interleave(cpg, dim=1)                   # [B, groups] -> [B, C]
    scale = ex(rstd) * ga
    shift = be - ex(mean) * scale
    coef_a = K_GN * U + ex(rho)
    coef_b = K_GN * U * shift.abs() + ex(rho) * (ex(mean) * scale).abs() + ex(dmean) * scale.abs()
    return dict(scale=scale, shift=shift, coef_a=coef_a, coef_b=coef_b)


def gn_apply64(x, scale, shift):
    B, HW, C = x.shape
    return x.double() * scale.view(B, 1, C) + shift.view(B, 1, C)


def gn_ratios(out, x, ref, silu):
    """out, x [B, HW, C] (out: float32 from the kernel, or a float64 simulation) -> (worst |error| / bound, worst use of the measured
    allowance).  Image by image, so that the large case stays within memory."""
    worst, used = 0.0, 0.0
    B, HW, C = x.shape
    step = max(1, (1 << 22) // C)
    for b in range(B):
        for r0 in range(0, HW, step):
            xs = x[b, r0:r0 + step].double() * ref["scale"][b].view(1, -1)
            y = xs + ref["shift"][b].view(1, -1)
            bound = ref["coef_a"][b].view(1, -1) * xs.abs() + ref["coef_b"][b].view(1, -1)
            o = out[b, r0:r0 + step].double()
            if silu:
                y = y * torch.sigmoid(y)
                derived = SILU_SLOPE * bound + U * y.abs() + FLOOR
                measured = (E_EXP + E_DIV) * U * y.abs()
                err = (o - y).abs()
                worst = max(worst, _worst(err, derived + measured))
                used = max(used, _worst((err - derived).clamp_min(0), measured.clamp_min(FLOOR)))
            else:
                worst = max(worst, _worst((o - y).abs(), bound))
    return worst, used


def gn_partials(x, lay):
    """float64 per-slice sums S, Q [B, slices, C] of gn_partial_kernel, and the same sums as a slice loop that never makes its
    second trip would leave them (thread row tr adds pixel beg + tr only)."""
    B, HW, C = x.shape
    slices, per = lay["slices"], lay["per"]
    xd = torch.zeros((B, slices * per, C), dtype=torch.float64)
    xd[:, :HW] = x.double()
    v = xd.view(B, slices, per, C)
    S, Q = v.sum(2), (v * v).sum(2)
    S1, Q1 = S.clone(), Q.clone()
    c0 = 0
    for ncg, rws in lay["passes"]:
        w = v[:, :, :rws, c0:c0 + 4 * ncg]
        S1[:, :, c0:c0 + 4 * ncg], Q1[:, :, c0:c0 + 4 * ncg] = w.sum(2), (w * w).sum(2)
        c0 += 4 * ncg
    return (S, Q), (S1, Q1)


def gn_finalize64(S, Q, HW, gamma, beta, groups, eps=GN_EPS, clamp=True, group_shift=0, neg_var=None):
    """gn_finalize_kernel in float64 from the partials: scale, shift [B, C].  clamp=False with neg_var: the variance of a group
    whose sums give var <= 0 (a constant group) is taken as `neg_var` unclamped; group_shift: the statistics of group g + shift."""
    B, _, C = S.shape
    cpg = C // groups
    n = float(HW * cpg)
    s, q = S.sum(1).view(B, groups, cpg).sum(2), Q.sum(1).view(B, groups, cpg).sum(2)
    mu = s / n
    var = q / n - mu * mu
    if clamp:
        var = var.clamp_min(0)
    elif neg_var is not None:
        var = torch.where(var <= n * U64 * q / n, torch.full_like(var, neg_var), var)
    rstd = 1.0 / torch.sqrt(var + _eps32(eps))
    if group_shift:
        mu, rstd = mu.roll(-group_shift, 1), rstd.roll(-group_shift, 1)
    ga, be = _affine64(gamma, beta, C)
    scale = rstd.repeat_interleave(cpg, dim=1) * ga
    return scale, be - mu.repeat_interleave(cpg, dim=1) * scale


# "unclamped_variance" plants var = -2 eps in the constant groups, so it shows only that the checker counts the resulting NaN as
# a violation.  It does NOT show that the GPU cases would notice a missing `var < 0` clamp: with float64 sums the cancellation
# error of Q/n - mean^2 is ~1e-16 E[x^2] against eps = 1e-6, far inside the bound, and a constant group's mean and squares are
# mostly exact, so the kernel's clamp is not observable through these cases (what they do hold is the constant groups' output).
GN_BUGS = ("slice_dropped", "first_pixel_only", "group_off_by_one", "unclamped_variance", "image_swapped", "channel_swapped")


def gn_bugged(bug, x, gamma, beta, c, lay):
    """The float64 output [B, HW, C] of a GroupNorm with one simulated bug (before SiLU)."""
    HW, G = c["HW"], c["groups"]
    (S, Q), (S1, Q1) = gn_partials(x, lay)
    kw = {}
    if bug == "slice_dropped":
        S, Q = S.clone(), Q.clone()
        S[:, lay["nonempty"] - 1] = 0
        Q[:, lay["nonempty"] - 1] = 0
    elif bug == "first_pixel_only":
        S, Q = S1, Q1
    elif bug == "group_off_by_one":
        kw = dict(group_shift=1)
    elif bug == "unclamped_variance":
        kw = dict(clamp=False, neg_var=-2.0 * GN_EPS)
    scale, shift = gn_finalize64(S, Q, HW, gamma, beta, G, **kw)
    if bug == "image_swapped":
        scale, shift = scale.roll(1, 0), shift.roll(1, 0)
    elif bug == "channel_swapped":
        scale, shift = scale.roll(1, 1), shift.roll(1, 1)
    return gn_apply64(x, scale, shift)


def gn_bug_visible(bug, c, lay):
    """Whether the simulated bug changes anything at this case (a loop that never makes a second trip is right when there is none)."""
    has_const = c["data"] in ("mixed", "constant") or c["HW"] * lay["cpg"] == 1
    return {"slice_dropped": True, "first_pixel_only": lay["trips"] > 1, "group_off_by_one": c["groups"] > 1,
            "unclamped_variance": has_const, "image_swapped": c["B"] > 1, "channel_swapped": True}[bug]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. row softmax

def _sm(name, rows, n, ldk, scale, bias, bias_rows=0):
    ld = {"n": n, "up4": _round_up(n, 4), "n+37": n + 37}[ldk]
    return dict(name=name, rows=rows, n=n, ld=ld, ldk=ldk, scale=scale, bias=bias, bias_rows=bias_rows if bias == "shared" else (rows if bias == "row" else 0),
                ld_bias=n + (5 if bias else 0))


SM_SCALE = 0.158
SM_CASES = [
    _sm("n1-ld-n", 1, 1, "n", 1.0, None),
    _sm("n1-up4-shared", 7, 1, "up4", SM_SCALE, "shared", 3),
    _sm("n1-wide-row", 64, 1, "n+37", 1.0, "row"),
    _sm("n3-ld-n-row", 300, 3, "n", SM_SCALE, "row"),
    _sm("n3-up4", 5, 3, "up4", 1.0, None),
    _sm("n3-wide-shared", 64, 3, "n+37", 1.0, "shared", 5),
    _sm("n255-ld-n-shared", 130, 255, "n", 1.0, "shared", 65),
    _sm("n255-up4-row", 4, 255, "up4", SM_SCALE, "row"),
    _sm("n255-wide", 64, 255, "n+37", SM_SCALE, None),
    _sm("n256-ld-n", 200, 256, "n", SM_SCALE, None),
    _sm("n256-up4-shared", 9, 256, "up4", 1.0, "shared", 4),
    _sm("n256-wide-row", 33, 256, "n+37", 1.0, "row"),
    _sm("n257-ld-n-row", 64, 257, "n", 1.0, "row"),
    _sm("n257-up4", 300, 257, "up4", 1.0, None),
    _sm("n257-wide-shared", 20, 257, "n+37", SM_SCALE, "shared", 7),
    _sm("n1000-ld-n-shared", 260, 1000, "n", SM_SCALE, "shared", 130),
    _sm("n1000-up4-row", 64, 1000, "up4", 1.0, "row"),          # (1000 is a multiple of 4: ld = n again, with a bias per row)
    _sm("n1000-wide", 6, 1000, "n+37", 1.0, None),
]
SM_GUARD = 64


def planted_rows(rows):
    """The fully masked rows of a case: the first, a middle and the last one."""
    return sorted({0, rows // 2, rows - 1}) if rows >= 3 else []


def sm_input(c):
    """The buffer [rows * ld + SM_GUARD] (pad columns NaN, sentinels 12345.0), the bias [bias_rows, ld_bias] or None (its pad
    columns NaN: they are never to be read) and the planted rows.  Logits reach +-80 after scaling; -inf entries are sprinkled over
    the columns >= 1 (of the bias where there is one), so that only the planted rows are masked entirely."""
    g = _gen(c["name"])
    rows, n, ld = c["rows"], c["n"], c["ld"]
    x = torch.full((rows, ld), float("nan"))
    x[:, :n] = (torch.rand((rows, n), generator=g) * 2 - 1) * (78.0 / c["scale"])
    bias = None
    holes = lambda r: torch.rand((r, n), generator=g) < 0.2
    if c["bias"]:
        bias = torch.full((c["bias_rows"], c["ld_bias"]), float("nan"))
        bias[:, :n] = (torch.rand((c["bias_rows"], n), generator=g) * 2 - 1) * 2.0
        m = holes(c["bias_rows"])
        m[:, 0] = False
        bias[:, :n][m] = float("-inf")
    else:
        m = holes(rows)
        m[:, 0] = False
        x[:, :n][m] = float("-inf")
    planted = planted_rows(rows)
    for r in planted:
        x[r, :n] = float("-inf")
    buf = torch.cat([x.flatten(), torch.full((SM_GUARD,), 12345.0)])
    return buf, bias, planted


def _softmax_bound(v, xs_abs, extra_k):
    """v [.., n] float64 logits (-inf allowed), xs_abs the magnitude u multiplies in their error beyond u |v - max| -> p, the
    relative error bound r of every p (header)."""
    p = torch.softmax(v, -1)
    fin = torch.isfinite(v)
    mx = torch.where(fin, v, torch.full_like(v, -1e300)).max(-1, keepdim=True).values
    delta = torch.where(fin, xs_abs + U * (v - mx).abs(), torch.zeros_like(v))
    splus = (p * torch.exp(delta)).sum(-1, keepdim=True)
    k_sum = _cdiv(v.shape[-1], 256) + 9
    return p, torch.exp(delta) * splus - 1.0 + (k_sum + extra_k) * U


def sm_reference(buf, bias, c, bias_row=None):
    """float64 softmax p [rows, n] and its absolute bound.  bias_row: the rule that picks the bias row of row r (default r % bias_rows)."""
    rows, n, ld = c["rows"], c["n"], c["ld"]
    x = buf[:rows * ld].view(rows, ld)[:, :n].double()
    s = float(torch.tensor(c["scale"], dtype=torch.float32).double())
    xs = x * s
    v = xs.clone()
    if bias is not None:
        idx = torch.arange(rows) % c["bias_rows"] if bias_row is None else bias_row
        v = xs + bias[:, :n].double()[idx]
    p, r = _softmax_bound(v, U * (xs.abs() + v.abs()), 2 * E_EXP + E_DIV)
    return p, p * r + FLOOR


def rows_report(out, ref, bound, planted):
    """out, ref, bound [R, n] and the planted row indices -> dict(nan_rows: rows that are NaN in every column, partial_nan: rows
    with some but not all columns NaN, ratio: worst |error| / bound over the rows that are not planted)."""
    nan = torch.isnan(out)
    full = nan.all(1)
    keep = torch.ones(out.shape[0], dtype=torch.bool)
    keep[planted] = False
    ratio = _worst((out[keep].double() - ref[keep]).abs(), bound[keep]) if bool(keep.any()) else 0.0
    return dict(nan_rows=full.nonzero().flatten().tolist(), partial_nan=(nan.any(1) & ~full).nonzero().flatten().tolist(), ratio=ratio)


def rows_violations(out, ref, bound, planted):
    """The names of what is wrong with the rows (empty: they pass): 'count' -- the number of NaN rows is not the number planted;
    'which' -- other rows than the planted ones are NaN (a row leaking into its neighbour); 'bound' -- a row that is not planted is
    outside its bound (a NaN in it counts)."""
    rep = rows_report(out, ref, bound, planted)
    bad = set()
    if len(rep["nan_rows"]) + len(rep["partial_nan"]) != len(planted):
        bad.add("count")
    if rep["nan_rows"] != sorted(planted) or rep["partial_nan"]:
        bad.add("which")
    if not rep["ratio"] <= 1.0:
        bad.add("bound")
    return bad


def sm_violations(after, c, ref, bound, planted):
    """`after`: the whole buffer as the kernel left it (CPU).  rows_violations plus 'pad' (a column n..ld-1 that is not exactly 0.0,
    masked rows included) and 'sentinel' (a float behind rows * ld changed)."""
    rows, n, ld = c["rows"], c["n"], c["ld"]
    body = after[:rows * ld].view(rows, ld)
    bad = rows_violations(body[:, :n], ref, bound, planted)
    if ld > n and not bool((body[:, n:] == 0.0).all()):
        bad.add("pad")
    if not bool((after[rows * ld:] == 12345.0).all()) or after.numel() != rows * ld + SM_GUARD:
        bad.add("sentinel")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. unfused attention

def _at(name, BH, Nq, Nk, D, bias, scale=None, mag=1.0, planted=()):
    return dict(name=name, BH=BH, Nq=Nq, Nk=Nk, D=D, bias=bias, scale=scale, mag=mag, planted=list(planted))


# planted: (batch-head, row) pairs whose every key is masked; with a shared bias the row is masked in every batch-head (z = None)
AT_CASES = [
    _at("one-of-everything", 1, 1, 1, 4, None),
    # a fully masked row BETWEEN two valid rows, Nk % 32 = 7: the second GEMM's A rows are 8 floats, its weights padded to 32 --
    # a read past lds multiplies the next row's (NaN) scores by zero weights
    _at("kpad-beside-nan-nk7", 2, 65, 7, 36, "shared", planted=[(None, 0), (None, 31), (None, 64)]),
    _at("kpad-beside-nan-nk33", 1, 65, 33, 96, "shared", planted=[(None, 32)]),
    _at("kpad-beside-nan-nk77-per-head", 5, 130, 77, 48, "per", scale=0.3, mag=6.0, planted=[(0, 0), (0, 129), (2, 64), (4, 129)]),
    _at("vae-mid-block-512", 2, 130, 130, 512, "per", mag=6.0, planted=[(0, 5), (1, 129)]),
    _at("single-query-nk31", 5, 1, 31, 4, "per", planted=[(3, 0)]),
    _at("nk32-no-bias", 2, 65, 32, 36, None, mag=6.0),
    _at("nk130-explicit-scale", 1, 130, 130, 48, None, scale=0.05, mag=6.0),
    _at("single-key", 2, 65, 1, 96, "per", planted=[(1, 3)]),
    _at("d512-nk77-shared", 5, 65, 77, 512, "shared", planted=[(None, 0), (None, 64)]),
    _at("d4-nk33-last-row-of-last-head", 2, 130, 33, 4, "per", scale=1.0, planted=[(1, 129), (1, 64)]),
]
AT_GUARD = 256


def at_planted(c):
    """The planted (z, row) pairs with a shared bias expanded over the batch-heads, as flat row indices z * Nq + row."""
    out = []
    for z, r in c["planted"]:
        out += [zz * c["Nq"] + r for zz in (range(c["BH"]) if z is None else [z])]
    return sorted(out)


def at_input(c):
    g = _gen(c["name"])
    BH, Nq, Nk, D = c["BH"], c["Nq"], c["Nk"], c["D"]
    q = torch.randn((BH, Nq, D), generator=g) * c["mag"]
    k = torch.randn((BH, Nk, D), generator=g) * c["mag"]
    v = torch.randn((BH, Nk, D), generator=g) * 1.5 + 0.25
    bias = None
    if c["bias"]:
        shape = (Nq, Nk) if c["bias"] == "shared" else (BH, Nq, Nk)
        bias = torch.randn(shape, generator=g) * 2.0
        m = torch.rand(shape, generator=g) < 0.3
        m[..., 0] = False
        bias[m] = float("-inf")
        for z, r in c["planted"]:
            if c["bias"] == "shared":
                bias[r] = float("-inf")
            else:
                bias[z, r] = float("-inf")
    return q, k, v, bias


def at_scale(c):
    return float(c["D"]) ** -0.5 if c["scale"] is None else float(c["scale"])


def at_reference(q, k, v, bias, scale):
    """float64 softmax(q k^T scale + bias) v [BH, Nq, D] and its bound (header)."""
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    s = abs(float(torch.tensor(scale, dtype=torch.float32).double()))
    qd, kd, vd = q.double(), k.double(), v.double()
    sc = torch.einsum("zqd,zkd->zqk", qd, kd) * float(torch.tensor(scale, dtype=torch.float32).double())
    mag = torch.einsum("zqd,zkd->zqk", qd.abs(), kd.abs()) * s
    dv = (D + 4) * U * mag
    if bias is not None:
        bd = bias.double().expand(BH, Nq, Nk)
        sc = sc + bd
        dv = dv + 2 * U * torch.where(torch.isfinite(bd), bd.abs(), torch.zeros_like(bd))
    p, r = _softmax_bound(sc, dv, 2 * E_EXP + E_DIV)
    ref = torch.einsum("zqk,zkd->zqd", p, vd)
    va = vd.abs()
    bound = (torch.einsum("zqk,zkd->zqd", p * r, va) + (Nk + 4) * U * torch.einsum("zqk,zkd->zqd", p * (1 + r), va)
             + FLOOR * va.sum(1, keepdim=True))
    return ref, bound


def at_workspace_bytes(BH, Nq, Nk, D):
    """ofx_attention_workspace_bytes for a head size the fused kernel does not take, restated."""
    kp, lds, vp = _round_up(D, 32), _round_up(Nk, 4), _round_up(Nk, 32)
    return BH * (Nk * kp + Nq * lds + D * vp) * 4 + 1024


FLASH_D = (40, 64, 80, 128, 160)
