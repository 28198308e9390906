"""Float64 references and derived error bounds for the encoders' instance-norm path (not a conftest: imported by name).

Five kernels and one epilogue branch are held to the bounds below (u = 2^-24, the fp32 unit round-off).  Every reference of a
statistic is computed in float64 from the values the kernel under test stored in fp32, so the rounding of the convolution that
produced them is checked on its own (wino_check.py, K_DIRECT).

f64 statistics pass (ofx_inorm_stats) and ofx_inorm_finalize: the sums run in f64 and the result is rounded once to fp32.
    |mean - ref|     <= u |ref| + 2^-52 HW mean|x|
    |rstd / ref - 1| <= 2u + 2^-51 HW E[x^2] / (var + eps)
  (a sequential f64 sum of HW terms is off by at most 2^-53 HW sum|x| to first order; var = E[x^2] - mean^2 inherits the error of
  E[x^2] and twice that of the mean, |mean| mean|x| <= E[x^2]; rstd = (var + eps)^-1/2 halves the relative error of var + eps; one
  u for the fp32 rounding, one for sqrt / divide and the second-order terms.)  For ofx_inorm_finalize, HW in the bound is the
  number of partial rows and x the partials.

Epilogue partials (conv.hip, the `do_stats` branch): a lane adds the 16 * TM = WM / 2 values of its column in fp32 (fmaf for the
squares: one rounding per step), then one add with the other lane half.  WM / 2 + 1 <= 33 roundings, each relative to a partial
sum that is at most sum|v| of the wave's column.  With S, Q the stored pair of one wave row (or the f64 sums of the rows of an
image):
    |S - sum v|   <= K_STATS u sum|v|
    |Q - sum v^2| <= K_STATS u sum v^2          K_STATS = 64 (33 roundings, first order, rounded up to the next power of two)
After ofx_inorm_finalize (f64 sums of the partials, one rounding to fp32):
    |mean - ref|     <= K_STATS u mean|v| + u |ref|
    |rstd / ref - 1| <= 2u + 1.5 K_STATS u E[v^2] / (var + eps)
  (d var <= d E[v^2] + 2 |mean| d mean <= 3 K_STATS u E[v^2], using |mean| mean|v| <= E[v^2]; rstd halves it.)  The rstd bounds
  are first order in x = (the last term): they hold while 1.5 x^2 <= u, i.e. x <= 2e-4, which `finalized_ratios` asserts of the case.

ofx_inorm_apply: compared as floats, element for element, with a float32 restatement in the kernel's operation order (`apply_f32`):
a subtract, a multiply, fmaxf, (the same for the residual,) the residual add, fmaxf.  The source leaves the compiler nothing to
contract -- `(v - mu) * rs` is a subtract followed by a multiply and a fmaxf sits between it and the residual add -- except on one
path: a normalised residual that is not ReLU'd (`res_mean` given, bit 1 of `relu` clear) feeds `(r - m2) * s2` straight into
`r + y`, which -ffp-contract=fast may fuse.  The ISA of inorm_apply_kernel for gfx950 (hipcc --save-temps) holds no v_fma / v_fmac
at all: v_pk_add_f32 (negated operand), v_pk_mul_f32, v_max_f32, one v_pk_add_f32 shared by every residual path, v_max_f32.  So the
restatement is plain float32 throughout, and a compiler that starts fusing that path shows up as a one-ulp mismatch in the
"normalised residual" cases.  (Equality is of values: the sign of a zero that fmaxf returns is not compared.)  A float64 evaluation
(`apply_f64`) with the bound K_APPLY u (|x - mu| rs + |r - m2| s2 + |out|) is kept as a second, looser check, so that a wrong
restatement cannot hide a wrong kernel.

Largest ratios measured on an MI355X (gfx950) over tests/test_gpu_encoder_norm.py, 2026-10-16 (the tests print each ratio; run
them with -s to re-measure).  For the partials a ratio is |error| / (u magnitude), inside when <= K_STATS; for the finalised
statistics it is |error| / bound, inside when <= 1.
    partials, per row                        S 4.55   Q 5.67     (K_STATS = 64)
    partials, per-image totals               S 1.98   Q 2.60     (K_STATS = 64)
    finalised from epilogue partials         mean 0.043   rstd 0.023
    f64 pass (ofx_inorm_stats)               mean 0.998   rstd 0.498     (the mean's is the fp32 rounding itself)
    ofx_inorm_finalize, synthetic partials   mean 0.988   rstd 0.493
    ofx_inorm_apply against float64          1.92     (K_APPLY = 4); against the float32 restatement: equal
    direct convolution output of the cases   3.95     (K_DIRECT = 11)
    norm on load, all / top / bottom / left / right    4.82 / 4.33 / 4.82 / 4.43 / 4.50     (K_DIRECT = 11)
"""
import torch

U = 2.0 ** -24
TINY = 1e-30
K_STATS = 64.0
EPS_NORM = 1e-5
FIRST_ORDER_LIMIT = 2e-4

# ---------------------------------------------------------------------------------------------------------------------------------
# the launcher's rule, restated (conv.hip: conv_plan -- tile selection, halo-patch test, statistics rows).  The library answers the
# same question itself (ofx_conv2d_plan, include/ofx.h); tests/test_conv_plan_host.py holds the two against each other on the host.

# tile code (tile = pair * 2e9 + BK * 1e6 + BM * 1e3 + BN) -> WM, the output rows of a tile one wave owns
WAVE_ROWS = {(256, 64): 64, (128, 128): 64, (128, 64): 64, (128, 192): 64, (128, 96): 32, (128, 32): 32, (64, 64): 32}
# setup_stats: waves per tile along M, i.e. partial rows per tile
WAVES_M = {(256, 64): 4, (128, 128): 2, (128, 64): 2, (128, 192): 2, (128, 96): 4, (128, 32): 4, (64, 64): 2}
K_FILL = 768                # workgroups that fill the chip three per CU
PATCH_MAX_WASTE = 1.09


def _cdiv(a, b):
    return -(-a // b)


def out_size(H, W, kh, kw, stride):
    return (H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1


def auto_tile(M, cout, norm, precision="fp32"):
    """The automatic (BM, BN) of a plain-epilogue layer."""
    fp32 = precision == "fp32"          # (the pre-split-weight modes "bf16x3_w" / "bf16x6_w" choose like their families)
    waste = lambda t: _cdiv(cout, t) * t / cout
    if cout <= 32:
        bn = 32
    elif waste(128) <= 1.13 and not (waste(192) <= 1.0 and waste(128) > 1.05 and fp32 and not norm):
        bn = 128
    elif waste(192) <= 1.05 and fp32 and not norm:
        bn = 192
    elif waste(96) <= 1.05 and fp32:
        bn = 96
    elif waste(64) <= 1.13:
        bn = 64
    elif waste(32) < waste(64) - 0.1:
        bn = 32
    else:
        bn = 64
    bm = 128
    blocks_of = lambda t: _cdiv(M, 128) * _cdiv(cout, t)
    if bn >= 64 and blocks_of(bn) < K_FILL:
        if bn == 192 and blocks_of(96) >= K_FILL:
            bn = 96
        elif bn >= 128 and blocks_of(64) >= K_FILL:
            bn = 64
        elif bn == 96:
            bn = 32
        else:
            bm, bn = 64, 64
    return bm, bn


def split_k(tiles, kpad):
    """The number of K splits a 64x64 small-grid launch with a workspace takes (1: none)."""
    nk32, S = kpad // 32, 1
    if tiles <= 2048 and nk32 >= 12:
        base = best = float(_cdiv(tiles, 256))
        for c in (2, 3, 4):
            if nk32 // c < 6:
                break
            span = _cdiv(tiles * c, 256) / c
            if span < best - 1e-9 and span < base * (1.0 - 0.04 * c) + 1e-9:
                best, S = span, c
    return S


def plan(B, H, W, cin, cout, kh, kw, stride=1, tile=0, norm=False, precision="fp32", act=None, res=False, splitk=False):
    """What the direct-kernel launcher does with a single-segment plain-epilogue layer: the tile, the A-side schedule
    ('general', 'scalar' or 'patch'), the patch size, the K splits (`splitk`: a workspace of any size is offered) and the partial
    rows per image ofx_conv2d_stats reports (0: none).  An independent restatement: the authority is the launcher's own
    answer, ofx_conv2d_plan (include/ofx.h), which tests/test_conv_plan_host.py compares this with field by field; `bk` is the
    chunk length of the kernel that runs."""
    Ho, Wo = out_size(H, W, kh, kw, stride)
    M = B * Ho * Wo
    fp32 = precision == "fp32"
    if tile:
        bm, bn, tile_bk = (tile % 1000000) // 1000, tile % 1000, (tile % 1000000000) // 1000000
    else:
        (bm, bn), tile_bk = auto_tile(M, cout, norm, precision), 0
    bk = tile_bk if tile_bk else (32 if (bn == 32 or bm == 64) else 16)
    ukm = 32 if tile else bk
    uk = fp32 and cin % ukm == 0
    shape_ok = (kh, kw) in ((3, 3), (1, 5), (5, 1))
    same = stride == 1 and (Ho, Wo) == (H, W)
    ph, pw = 8, 16
    if fp32:
        big = (bm == 128 or (bm, bn) == (256, 64)) and bk == 16
        small = (bm, bn) == (64, 64) and bk == 32
        pw, ph = (16 if big else 8), (16 if bm == 256 else 8)
        whole = H % ph == 0 and W % pw == 0
        cover = (_cdiv(H, ph) * ph) * (_cdiv(W, pw) * pw) / (H * W)
        patch = (not (not whole and tile == 0 and cover > PATCH_MAX_WASTE) and shape_ok and same and (whole or big) and cin % bk == 0
                 and (big or small) and bn in (64, 96, 128, 192))
        if patch and (bm, bn) == (128, 64) and tile == 0 and H % 16 == 0 and W % 16 == 0 and M // 256 >= K_FILL:
            bm, ph = 256, 16
    else:
        # the split-bf16 modes map every choice onto three tiles and re-derive the patch test for 8x16 patches
        bn = 64 if bm == 64 else (bn if bn == 64 else 128)
        whole = H % 8 == 0 and W % 16 == 0
        cover = (_cdiv(H, 8) * 8) * (_cdiv(W, 16) * 16) / (H * W)
        patch = ((whole or tile != 0 or cover <= PATCH_MAX_WASTE) and shape_ok and same and cin % 16 == 0 and bm == 128 and tile_bk != 32)
        # ... which exist with 16-wide chunks only, but for the 128x128 tile of the on-the-fly bf16x3 split (a forced BK = 32)
        bk = 32 if (precision == "bf16x3" and (bm, bn) == (128, 128) and tile_bk == 32) else 16
    mt_img = _cdiv(H, ph) * _cdiv(W, pw) if patch else None
    waves_m = WAVES_M.get((bm, bn), 0)
    hw = Ho * Wo
    ok = waves_m and act in (None, "none") and not res and (patch or hw % bm == 0)
    rows = ((mt_img if patch else hw // bm) * waves_m) if ok else 0
    # the 64x64 BK = 32 tile: split-K when a workspace is offered and it pays, else two paired K pipelines on grids of up to 320
    # workgroups (or when the tile code asks for them); the paired kernel has no halo-patch form
    splits, paired = 1, False
    if fp32 and (bm, bn, bk) == (64, 64, 32):
        kpad = _cdiv(kh * kw * cin, 32) * 32
        tiles = (B * mt_img if patch else _cdiv(M, 64)) * _cdiv(cout, 64)
        if splitk and tile == 0:
            splits = split_k(tiles, kpad)
        if splits == 1:
            paired = tile >= 2000000000 or (tile < 1000000 and tiles <= 320 and kpad >= 256)
    on_patch = patch and not paired
    kind = "patch" if on_patch else "scalar" if (uk and bn != 192) else "general"
    return dict(bm=bm, bn=bn, bk=bk, wm=WAVE_ROWS.get((bm, bn)), kind=kind, ph=ph, pw=pw, whole=whole if on_patch else None,
                rows=rows, Ho=Ho, Wo=Wo, splits=splits, paired=paired)


def row_labels(p):
    """[Ho * Wo] int64: the partial row of an image that each output pixel is summed into.  General kernels: row r covers the WM
    consecutive output rows [r WM, (r + 1) WM) of the [Ho * Wo, Cout] matrix.  Patch kernels: the tiles are the ph x pw patches in
    raster order (the last ones may hang over the map) and wave w of a tile owns the patch rows [w WM / pw, (w + 1) WM / pw)."""
    Ho, Wo = p["Ho"], p["Wo"]
    pix = torch.arange(Ho * Wo)
    if p["kind"] != "patch":
        return pix // p["wm"]
    y, x = pix // Wo, pix % Wo
    tile = (y // p["ph"]) * _cdiv(Wo, p["pw"]) + x // p["pw"]
    return tile * (p["bm"] // p["wm"]) + (y % p["ph"]) // (p["wm"] // p["pw"])


# ---------------------------------------------------------------------------------------------------------------------------------
# epilogue partials

def row_sums(v, labels, rows):
    """v [B, C, Ho, Wo] (any float dtype) -> float64 (sum v, sum v^2, sum |v|), each [B, rows, C], over the pixels of each row."""
    B, C = v.shape[:2]
    flat = v.double().reshape(B, C, -1).permute(0, 2, 1)              # [B, HW, C]
    out = []
    for t in (flat, flat * flat, flat.abs()):
        acc = torch.zeros((B, rows, C), dtype=torch.float64)
        acc.index_add_(1, labels, t)
        out.append(acc)
    return out


def _ratio(err, bound):
    """max err / bound, NaN (an unwritten partial) counted as infinite."""
    r = err / bound.clamp_min(TINY)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def partial_ratios(part, v, labels, rows):
    """part [B, rows, C, 2] as stored, v the kernel's own output [B, C, Ho, Wo] -> the worst |error| / (u times the magnitude)
    of the four quantities the bound K_STATS applies to: every row's S and Q, and the per-image totals of S and Q."""
    S, Q, A = row_sums(v, labels, rows)
    p = part.double()
    return {
        "row_S": _ratio((p[..., 0] - S).abs(), U * A),
        "row_Q": _ratio((p[..., 1] - Q).abs(), U * Q),
        "total_S": _ratio((p[..., 0].sum(1) - S.sum(1)).abs(), U * A.sum(1)),
        "total_Q": _ratio((p[..., 1].sum(1) - Q.sum(1)).abs(), U * Q.sum(1)),
    }


def partial_violations(part, v, labels, rows, K=K_STATS):
    """The names of the quantities outside the bound (empty: the partials pass)."""
    return {k for k, r in partial_ratios(part, v, labels, rows).items() if not r <= K}


def stats64(v, eps=EPS_NORM):
    """v [B, C, ...] -> float64 per (b, c): mean, rstd, mean|v|, E[v^2], var."""
    f = v.double().reshape(v.shape[0], v.shape[1], -1)
    mean = f.mean(2)
    var = ((f - mean[..., None]) ** 2).mean(2)
    return dict(mean=mean, rstd=1.0 / torch.sqrt(var + eps), absmean=f.abs().mean(2), sq=(f * f).mean(2), var=var)


def stat_ratios(mean, rstd, r, k_u, c, eps=EPS_NORM):
    """mean, rstd [B, C] against the float64 reference r (mean, rstd, absmean, sq, var: see stats64): the ratios of
        |mean - ref| to k_u mean|v| + u |ref|       and       |rstd / ref - 1| to 2u + c k_u E[v^2] / (var + eps)."""
    x = c * k_u * r["sq"] / (r["var"] + eps)
    assert float(x.max()) <= FIRST_ORDER_LIMIT, f"case outside the first-order range of the rstd bound: {float(x.max()):.3g}"
    m = _ratio((mean.double() - r["mean"]).abs(), k_u * r["absmean"] + U * r["mean"].abs())
    s = _ratio((rstd.double() / r["rstd"] - 1.0).abs(), 2 * U + x)
    return {"mean": m, "rstd": s}


def finalized_ratios(mean, rstd, v, k_u, eps=EPS_NORM):
    """mean, rstd [B, C] from a finalize kernel, v the values they are statistics of; k_u = the error of the sums relative to
    mean|v| and E[v^2] (K_STATS u for the epilogue partials, 2^-52 HW for an f64 pass).  Returns the ratios of
        |mean - ref| to k_u mean|v| + u |ref|       and       |rstd / ref - 1| to 2u + c k_u E[v^2] / (var + eps)
    with c = 1.5 for fp32 partials and 2 for the f64 pass (the 2^-51 of the header): <= 1 means inside the bound."""
    return stat_ratios(mean, rstd, stats64(v, eps), k_u, 1.5 if k_u >= U else 2.0, eps)


def partials_reference(part, HW, eps=EPS_NORM):
    """[B, rows, C, 2] partials (any values with sum Q / HW >= (sum S / HW)^2) -> the reference dictionary of stat_ratios: the sums
    of ofx_inorm_finalize in float64, with mean|v| and E[v^2] standing for sum|S| / HW and sum|Q| / HW."""
    p = part.double()
    mean = p[..., 0].sum(1) / HW
    var = (p[..., 1].sum(1) / HW - mean * mean).clamp_min(0)
    return dict(mean=mean, rstd=1.0 / torch.sqrt(var + eps), absmean=p[..., 0].abs().sum(1) / HW, sq=p[..., 1].abs().sum(1) / HW, var=var)


def finalize64(part, HW, eps=EPS_NORM):
    """[B, rows, C, 2] partials -> float64 (mean, rstd): the sums of ofx_inorm_finalize in float64."""
    p = part.double()
    mean = p[..., 0].sum(1) / HW
    var = (p[..., 1].sum(1) / HW - mean * mean).clamp_min(0)
    return mean, 1.0 / torch.sqrt(var + eps)


# ---------------------------------------------------------------------------------------------------------------------------------
# ofx_inorm_apply

def _bc(s, x):
    return s.view(s.shape[0], s.shape[1], *([1] * (x.dim() - 2)))


def apply_f32(x, mean, rstd, res=None, res_mean=None, res_rstd=None, relu=1):
    """The kernel's arithmetic in float32, operation by operation.  x, res [B, C, ...] float32, statistics [B, C] float32."""
    assert x.dtype == torch.float32 and mean.dtype == torch.float32 and rstd.dtype == torch.float32
    y = (x - _bc(mean, x)) * _bc(rstd, x)
    if (relu & 1) or res is not None:
        y = torch.clamp_min(y, 0.0)
    if res is None:
        return y
    if res_mean is None:
        return torch.clamp_min(res + y, 0.0)
    d = res - _bc(res_mean, x)
    r = d * _bc(res_rstd, x)
    if relu & 2:
        r = torch.clamp_min(r, 0.0)
    return torch.clamp_min(r + y, 0.0)


def apply_f64(x, mean, rstd, res=None, res_mean=None, res_rstd=None, relu=1):
    """The documented formula in float64 and the magnitude its float32 evaluation error scales with."""
    y = (x.double() - _bc(mean, x).double()) * _bc(rstd, x).double()
    mag = y.abs()
    if (relu & 1) or res is not None:
        y = torch.relu(y)
    if res is not None:
        r = res.double()
        if res_mean is not None:
            r = (r - _bc(res_mean, x).double()) * _bc(res_rstd, x).double()
            mag = mag + r.abs()
            if relu & 2:
                r = torch.relu(r)
        y = torch.relu(r + y)
    return y, mag + y.abs()


K_APPLY = 4.0      # sub, mul, (sub, mul,) add: each at most u of a quantity bounded by the magnitude above
