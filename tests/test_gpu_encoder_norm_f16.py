"""The encoder path of `RaftEngine(precision="fp16")`, kernel by kernel: the instance norm + ReLU the direct kernels apply to their
operand on load, and the statistics their epilogue leaves behind, both in the fp16 arithmetic (OFX_PREC_F16_EPI, `ops.conv2d_nhwc(precision="fp16_epi")`).  The pattern, the
statistics bounds (K_STATS, the finalised mean / rstd) and the row labelling are inorm_check.py's; the convolution bound is
f16_check.py's derived one, (K + 2) 2^-24 sum |x_h| |w_h| + 2 2^-24 |ref| + FLOOR.  Nothing is measured into a bound.

Norm on load.  The staging code (conv.hip: a_commit on the halo patch, norm_a off it) forms fmaxf((v - mu) * rs, 0) in fp32 -- a
subtract, a multiply, a max; a padding tap is zeroed AFTER it -- and THAT value is rounded to half (v_cvt_pk_f16_f32, nearest even).
The source leaves nothing to contract: (v - mu) * rs is no a * b + c.  The gfx950 ISA of the NORM = true, PREC = 5 instantiations
(hipcc -S --cuda-device-only; read for the 128x128, 128x64 and 64x64 tiles on the patch, the scalar and the general schedule)
agrees: every v_cvt_pk_f16_f32 of the A side takes two v_max_f32 results whose operands are v_mul_f32 products of v_sub_f32
differences, zeroed under exec for a padding tap, and the code ahead of a kernel's last conversion holds no v_fma / v_fmac /
v_pk_fma at all (they begin with the epilogue).  So the oracle restates the operand bit for bit -- torch.clamp_min((x - mean) * rstd, 0) in float32, then .half() -- the
half rounding is deterministic and the bound stays the derived one, with no half-ulp flip term.  A compiler that starts fusing that
expression shows up as a ratio far above 1 (one flipped half rounding is 2^-11 |x| |w| against a bound of K 2^-24 per unit).
Checked on the smallest maps of test_gpu_encoder_norm's "all / top / bottom / left / right" cases (16x32: whole patches; 13x22: every
patch hangs over), channel means alternating in sign so that a normalised padding would show on every border.

Epilogue statistics.  Computed from the fp32 accumulators exactly as in fp32: every row's (sum, sum of squares) and the per-image
totals are held to K_STATS against the float64 sums of the stored fp32 values, the finalised mean / rstd to their bounds.

Every case states the plan it must reach, asserted through ofx_conv2d_plan."""
import ctypes as C

import numpy as np
import pytest
import torch

import f16_check as FC
import inorm_check as ic

gpu = pytest.mark.gpu
PTR = 0x10000
PREC_F16_EPI = FC.PREC_F16 | 256          # include/ofx.h: the fp16 arithmetic with nmean / ofx_conv2d_stats served (OFX_PREC_F16 rejects both)


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def nhwc(x):  # NCHW cpu -> NHWC cuda
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def _plan_of(B, H, W, cin, cout, k, stride, tile, norm, stats_cap=0):
    from sd_animation_optical_flow_amd import _lib
    d = _lib.ConvDesc()
    d.in0, d.ld0, d.c0, d.w, d.out, d.ldo = PTR, cin, cin, PTR, PTR, cout
    d.B, d.Hin, d.Win = B, H, W
    d.Hout, d.Wout = ic.out_size(H, W, k, k, stride)
    d.Cout, d.KH, d.KW, d.stride, d.padH, d.padW = cout, k, k, stride, k // 2, k // 2
    d.tile, d.precision = tile, PREC_F16_EPI
    if norm:
        d.nmean = d.nrstd = PTR
    p = _lib.ConvPlan()
    assert _lib.lib().ofx_conv2d_plan(C.byref(d), stats_cap, 0, C.byref(p)) == 0
    assert p.path == 0 and p.prec == FC.PREC_F16 and p.ks == 1 and p.ksplit == 1
    return (p.bm, p.bn, p.bk, p.mode), p.stats_rows


def _reference(x_operand, w, shift, k, stride):
    """f16_check.reference on an NCHW operand that is already what the kernel rounds: -> (ref, bound), NHWC float64."""
    c = dict(name="norm-f16", k=k, stride=stride, extra={})
    t = dict(x=x_operand.permute(0, 2, 3, 1).contiguous(), x2=None, w=w, scale=None, shift=shift, addend=None, res=None)
    return FC.reference(c, t)


# ---------------------------------------------------------------------------------------------------------------------------------
# norm + ReLU on load

# (tile, channels) -> the plan per map: the halo patch for the forced BK 16 tiles (and the automatic choice on the whole map), the
# scalar-coordinate schedule for whole 32-channel chunks at BK 32, the general gather for 48 channels at BK 32 (the two 128-row arms
# there are the ones compiled one workgroup per CU lower)
NORM_CASES = [
    (16128128, 64, {(16, 32): (128, 128, 16, 2), (13, 22): (128, 128, 16, 2)}),
    (16128064, 64, {(16, 32): (128, 64, 16, 2), (13, 22): (128, 64, 16, 2)}),
    (16064064, 64, {(16, 32): (64, 64, 16, 2), (13, 22): (64, 64, 16, 2)}),
    (32128128, 64, {(16, 32): (128, 128, 32, 1), (13, 22): (128, 128, 32, 1)}),
    (32128064, 64, {(16, 32): (128, 64, 32, 1), (13, 22): (128, 64, 32, 1)}),
    (32064064, 64, {(16, 32): (64, 64, 32, 1), (13, 22): (64, 64, 32, 1)}),
    (32128128, 48, {(16, 32): (128, 128, 32, 0), (13, 22): (128, 128, 32, 0)}),
    (32128064, 48, {(16, 32): (128, 64, 32, 0), (13, 22): (128, 64, 32, 0)}),
    (0, 64, {(16, 32): (128, 128, 16, 2), (13, 22): (128, 128, 32, 1)}),   # 13x22 in 8x16 patches: a cover of 1.79, off the patch
]
NORM_MAPS = [(16, 32), (13, 22)]


@gpu
@pytest.mark.parametrize("tile,c,plans", NORM_CASES, ids=[f"t{t}-c{c}" for t, c, _ in NORM_CASES])
@pytest.mark.parametrize("H,W", NORM_MAPS)
def test_fp16_kernels_round_the_normalised_operand_and_pad_after_normalising(cuda, tile, c, plans, H, W):
    ops = _ops()
    B, co = 3, 96
    assert _plan_of(B, H, W, c, co, 3, 1, tile, True)[0] == plans[(H, W)]
    g = torch.Generator().manual_seed(tile % 1000 + H + c)
    w = torch.randn((co, c, 3, 3), generator=g) / np.sqrt(c * 9)
    shift = torch.randn((co,), generator=g) * 0.1
    off = torch.where(torch.arange(c) % 2 == 0, 1.5, -1.5).view(1, c, 1, 1) * (1.0 + 0.5 * torch.arange(B).view(B, 1, 1, 1))
    x = torch.randn((B, c, H, W), generator=g) * 2.0 + off
    mean = x.double().mean(dim=(2, 3)).float()
    rstd = (1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)).float()
    xn = torch.clamp_min((x - mean.view(B, c, 1, 1)) * rstd.view(B, c, 1, 1), 0.0)      # float32, the staging code's order
    assert xn.dtype == torch.float32
    ref, bound = _reference(xn, w, shift, 3, 1)
    kw = dict(shift=shift.cuda(), nmean=mean.cuda(), nrstd=rstd.cuda(), tile=tile)
    out = ops.conv2d_nhwc(nhwc(x), ops.pack_conv_weight(w).cuda(), 3, 3, co, precision="fp16_epi", **kw)
    again = ops.conv2d_nhwc(nhwc(x), ops.pack_conv_weight(w).cuda(), 3, 3, co, precision="fp16_epi", **kw)
    exact = ops.conv2d_nhwc(nhwc(x), ops.pack_conv_weight(w).cuda(), 3, 3, co, **kw)
    assert torch.equal(out, again) and not torch.equal(out, exact)       # repeats; the fp16 arithmetic ran, not the fp32 kernel
    out = out.cpu()
    for name, sl in (("all", np.s_[:]), ("top", np.s_[:, 0]), ("bottom", np.s_[:, -1]), ("left", np.s_[:, :, 0]), ("right", np.s_[:, :, -1])):
        r = FC.worst_ratio(out[sl], ref[sl], bound[sl])
        print(f"ratio norm on load fp16, tile {tile} c {c} {H}x{W} {name}: |error| / bound {r:.4f}")
        assert r <= 1.0, (tile, c, H, W, name, r)


# ---------------------------------------------------------------------------------------------------------------------------------
# epilogue statistics

def _sc(name, B, H, W, cin, cout, k, stride, tile, plan, rows, norm=False):
    return dict(name=name, B=B, H=H, W=W, cin=cin, cout=cout, k=k, stride=stride, tile=tile, plan=plan, rows=rows, norm=norm)


# plan = (bm, bn, bk, mode), rows = partial rows per image (tiles per image x the two wave rows of every fp16 tile)
STATS_CASES = [
    _sc("patch128x128", 1, 16, 32, 32, 128, 3, 1, 16128128, (128, 128, 16, 2), 8),
    _sc("patch128x64-norm", 3, 16, 32, 64, 64, 3, 1, 16128064, (128, 64, 16, 2), 8, norm=True),
    _sc("patch64x64", 2, 16, 24, 64, 70, 3, 1, 16064064, (64, 64, 16, 2), 12),
    _sc("over128x64-ragged-norm", 2, 7, 5, 32, 70, 3, 1, 16128064, (128, 64, 16, 2), 2, norm=True),
    _sc("over64x64", 2, 13, 22, 32, 64, 3, 1, 16064064, (64, 64, 16, 2), 12),
    _sc("scalar128x128-bk16-s2", 2, 32, 32, 64, 128, 3, 2, 16128128, (128, 128, 16, 1), 4),
    _sc("general128x64-bk32-s2-norm", 1, 32, 64, 48, 64, 3, 2, 32128064, (128, 64, 32, 0), 8, norm=True),
    _sc("scalar128x128-bk32-s2-norm", 1, 32, 32, 64, 128, 3, 2, 32128128, (128, 128, 32, 1), 4, norm=True),
    _sc("stem-auto", 2, 64, 96, 4, 64, 7, 2, 0, (64, 64, 32, 0), 48),
    _sc("down-auto", 2, 32, 32, 96, 128, 1, 2, 0, (64, 64, 32, 1), 8),
]


def _labels_plan(c):
    """The dictionary inorm_check.row_labels reads, from the case's literal plan."""
    bm, bn, bk, mode = c["plan"]
    Ho, Wo = ic.out_size(c["H"], c["W"], c["k"], c["k"], c["stride"])
    return dict(bm=bm, bn=bn, wm=ic.WAVE_ROWS[(bm, bn)], kind="patch" if mode == 2 else "direct", ph=8, pw=16 if bm == 128 else 8,
                Ho=Ho, Wo=Wo, rows=c["rows"])


@gpu
@pytest.mark.parametrize("c", STATS_CASES, ids=[c["name"] for c in STATS_CASES])
def test_fp16_epilogue_statistics(cuda, c):
    ops = _ops()
    B, H, W, cin, cout, k, stride = (c[n] for n in ("B", "H", "W", "cin", "cout", "k", "stride"))
    need = B * c["rows"] * cout * 2
    assert _plan_of(B, H, W, cin, cout, k, stride, c["tile"], c["norm"], stats_cap=need) == (c["plan"], c["rows"])
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c["name"]))
    off = torch.where(torch.arange(cin) % 2 == 0, 1.5, -1.5).view(1, cin, 1, 1) + 0.25 * torch.arange(B).view(B, 1, 1, 1)
    x = torch.randn((B, cin, H, W), generator=g) * 2.0 + off
    w = torch.randn((cout, cin, k, k), generator=g) / np.sqrt(cin * k * k)
    shift = torch.randn((cout,), generator=g) * 0.5
    kw = dict(stride=stride, shift=shift.cuda(), tile=c["tile"], precision="fp16_epi")
    operand = x
    if c["norm"]:
        mean = x.double().mean(dim=(2, 3)).float()
        rstd = (1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)).float()
        kw.update(nmean=mean.cuda(), nrstd=rstd.cuda())
        operand = torch.clamp_min((x - mean.view(B, -1, 1, 1)) * rstd.view(B, -1, 1, 1), 0.0)
    ref, bound = _reference(operand, w, shift, k, stride)
    wp = ops.pack_conv_weight(w).cuda()
    parts, outs = [], []
    for _ in range(2):
        part = torch.full((need + 4096,), float("nan"), device="cuda")
        out, rows = ops.conv2d_nhwc(nhwc(x), wp, k, k, cout, stats_part=part, **kw)
        assert rows == c["rows"]
        parts.append(part.cpu())
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(parts[0][:need], parts[1][:need])
    r = FC.worst_ratio(outs[0], ref, bound)
    print(f"ratio conv output fp16 {c['name']}: |error| / bound {r:.4f}")
    assert r <= 1.0
    part = parts[0]
    assert bool(torch.isfinite(part[:need]).all()), "a partial the host counted was never written"
    assert bool(torch.isnan(part[need:]).all()), "written past [B][rows][Cout][2]"
    p = _labels_plan(c)
    v = outs[0].permute(0, 3, 1, 2)                                      # the stored fp32 values, NCHW
    pr = part[:need].view(B, c["rows"], cout, 2)
    labels = ic.row_labels(p)
    ratios = ic.partial_ratios(pr, v, labels, c["rows"])
    for name, val in ratios.items():
        print(f"ratio partials fp16 {c['name']} {name} {val:.4g}  (K_STATS = {ic.K_STATS:g})")
    assert not ic.partial_violations(pr, v, labels, c["rows"]), (c["name"], ratios)
    mean_d, rstd_d = ops.inorm_finalize(part[:need].cuda(), B, c["rows"], p["Ho"] * p["Wo"], cout)
    fr = ic.finalized_ratios(mean_d.cpu(), rstd_d.cpu(), v, ic.K_STATS * ic.U)
    for name, val in fr.items():
        print(f"ratio finalised fp16 {c['name']} {name} {val:.4g}")
    assert fr["mean"] <= 1.0 and fr["rstd"] <= 1.0, (c["name"], fr)
