"""The encoders' instance-norm path against float64, kernel by kernel: the statistics the direct convolution epilogue leaves behind
(ofx_conv2d_stats without a Winograd operand), the f64 statistics pass (ofx_inorm_stats), ofx_inorm_finalize, ofx_inorm_apply in
every residual mode, and the norm + ReLU the direct kernels apply to their operand on load.

Bounds and references live in inorm_check.py and are derived there, not measured.  The case tables are plain data: CPU tests assert
what they cover (every entry of the launcher's waves-per-tile table, every A-side schedule, both strides, whole and overhanging
patches, both sides of B = 8) and that the checker catches the statistics bugs it is meant to catch at every map size of the table.
GPU tests are marked -m gpu; the CPU self-tests carry no marker.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inorm_check as ic
import wino_check as wc

gpu = pytest.mark.gpu


def _note(name, ratio):
    """Print a measured ratio (pytest -s shows them; the worst ones are recorded in the header of inorm_check.py)."""
    print(f"ratio {name} {float(ratio):.4g}")


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def nhwc(x):  # NCHW cpu -> NHWC cuda
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):  # NHWC cuda -> NCHW cpu
    return x.permute(0, 3, 1, 2).contiguous().cpu()


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the case table of the direct kernels' epilogue statistics

def _sc(name, B, H, W, cin, cout, k, stride, tile, norm=False, stem=False, splitk=False, precision="fp32", auto=None):
    """auto = (BM, BN, rows): what the launcher's heuristics choose today for a tile = 0 case, as literal values.  The statistics
    tests follow inorm_check.plan(); test_automatic_choices_are_where_the_table_says compares the two, so that a retuned
    threshold fails THERE, reading 'the heuristic moved', before any statistics check reports a row-count mismatch."""
    return dict(name=name, B=B, H=H, W=W, cin=cin, cout=cout, kh=k, kw=k, stride=stride, tile=tile, norm=norm, stem=stem,
                splitk=splitk, precision=precision, auto=auto)


STATS_CASES = [
    # the halo patch on whole maps: every tile that carries it
    _sc("patch256x64", 2, 32, 32, 64, 64, 3, 1, 16256064),
    _sc("patch128x128", 1, 16, 32, 32, 128, 3, 1, 16128128),
    _sc("patch128x64-norm", 3, 16, 32, 64, 64, 3, 1, 16128064, norm=True),
    _sc("patch128x192", 2, 8, 32, 32, 96, 3, 1, 16128192),
    _sc("patch128x96-norm", 2, 16, 16, 32, 96, 3, 1, 16128096, norm=True),
    _sc("patch128x128-ragged", 3, 8, 16, 16, 70, 3, 1, 16128128),
    # the 8x8-patch small tile; the paired tile code keeps the small tile but has no patch form
    _sc("small-patch", 3, 16, 24, 64, 70, 3, 1, 32064064),
    _sc("small-patch-norm", 1, 8, 8, 32, 64, 3, 1, 32064064, norm=True),
    _sc("paired", 2, 16, 24, 64, 96, 3, 1, 2032064064),
    _sc("paired-norm-s2", 1, 32, 32, 48, 64, 3, 2, 2032064064, norm=True),
    # the halo patch on overhanging maps (a forced tile keeps the patch kernel there)
    _sc("over128x64", 3, 13, 22, 64, 64, 3, 1, 16128064),
    _sc("over128x128-norm", 1, 65, 97, 32, 128, 3, 1, 16128128, norm=True),
    _sc("over128x96", 2, 13, 22, 32, 96, 3, 1, 16128096),
    _sc("over128x192", 1, 9, 40, 16, 128, 3, 1, 16128192),
    _sc("over256x64", 2, 40, 25, 64, 64, 3, 1, 16256064),
    _sc("over128x64-ragged-norm", 2, 7, 5, 32, 70, 3, 1, 16128064, norm=True),
    # the scalar-coordinate schedule (whole 32-channel chunks) and the general gather, stride 1 and 2
    _sc("scalar128x128-s2", 2, 32, 32, 64, 128, 3, 2, 16128128),
    _sc("general128x64-s2-norm", 1, 32, 64, 48, 64, 3, 2, 16128064, norm=True),
    _sc("general128x192-s2", 2, 32, 32, 32, 96, 3, 2, 16128192),
    _sc("scalar128x96-s2", 3, 32, 32, 64, 96, 3, 2, 16128096),
    _sc("scalar128x32-s2", 2, 32, 32, 64, 70, 3, 2, 32128032),
    _sc("scalar128x32-s1-norm", 1, 16, 24, 64, 64, 3, 1, 32128032, norm=True),
    _sc("general64x64bk16", 2, 8, 24, 16, 64, 3, 1, 16064064),
    _sc("scalar64x64bk16-s2", 1, 16, 32, 32, 128, 3, 2, 16064064),
    _sc("scalar256x64-s2", 1, 32, 32, 32, 64, 3, 2, 16256064),
    _sc("general64x64bk32", 3, 8, 8, 16, 96, 3, 1, 32064064),
    # the 7x7 stride-2 stem on the 4-channel output of preprocess_u8
    _sc("stem-auto", 2, 64, 96, 4, 64, 7, 2, 0, stem=True, auto=(64, 64, 48)),
    _sc("stem128x128", 1, 32, 64, 4, 96, 7, 2, 16128128, stem=True),
    _sc("stem128x64", 3, 32, 32, 4, 64, 7, 2, 16128064, stem=True),
    _sc("stem128x32", 1, 32, 32, 4, 70, 7, 2, 32128032, stem=True),
    # the 1x1 stride-2 downsample
    _sc("down128x128", 2, 32, 32, 64, 128, 1, 2, 16128128),
    _sc("down128x96", 1, 32, 32, 64, 96, 1, 2, 16128096),
    _sc("down128x32", 3, 32, 32, 64, 70, 1, 2, 32128032),
    _sc("down-auto", 2, 32, 32, 96, 128, 1, 2, 0, auto=(64, 64, 8)),
    # the automatic choice: a strided 96-channel layer (128x32), a small grid (paired 64x64), a split-K small grid on the patch
    # and on the scalar schedule (the last workgroup to arrive writes the statistics), and one chip-filling stage (256x64)
    _sc("auto128x32-s2", 3, 48, 64, 64, 96, 3, 2, 0, auto=(128, 32, 24)),
    _sc("auto-small-paired-norm", 1, 16, 16, 64, 64, 3, 1, 0, norm=True, auto=(64, 64, 8)),
    _sc("auto-splitk-patch", 2, 16, 16, 128, 128, 3, 1, 0, splitk=True, auto=(64, 64, 8)),
    _sc("auto-splitk-scalar-s2-norm", 1, 32, 32, 128, 128, 3, 2, 0, norm=True, splitk=True, auto=(64, 64, 8)),
    _sc("auto-stage-256x64", 2, 384, 256, 64, 64, 3, 1, 0, auto=(256, 64, 1536)),
]

# b. the split-bf16 precisions: the tile is remapped (128x96 / 128x32 / 128x192 -> 128x128) before the statistics are set up
BF16_CASES = [
    _sc("bf16x3-patch128x128", 2, 16, 32, 64, 128, 3, 1, 16128128, precision="bf16x3"),
    _sc("bf16x3-over128x64-norm", 3, 13, 22, 64, 64, 3, 1, 16128064, norm=True, precision="bf16x3"),
    _sc("bf16x3-remap96", 2, 32, 32, 64, 96, 3, 2, 16128096, precision="bf16x3"),
    _sc("bf16x3-remap32", 1, 32, 32, 64, 70, 1, 2, 32128032, precision="bf16x3"),
    _sc("bf16x3-auto-small", 2, 16, 16, 64, 64, 3, 1, 0, precision="bf16x3", auto=(64, 64, 8)),
    _sc("bf16x6-patch128x64", 2, 16, 32, 64, 64, 3, 1, 16128064, precision="bf16x6"),
    _sc("bf16x6-remap192-s2-norm", 1, 32, 32, 32, 128, 3, 2, 16128192, norm=True, precision="bf16x6"),
    # the pre-split-weight forms (what an engine that uploads split weights once runs): other instantiations, the same statistics
    _sc("bf16x3_w-over128x128", 2, 13, 22, 64, 96, 3, 1, 16128128, precision="bf16x3_w"),
    _sc("bf16x3_w-remap96-s2-norm", 1, 32, 32, 64, 96, 3, 2, 16128096, norm=True, precision="bf16x3_w"),
    _sc("bf16x6_w-patch128x64-norm", 3, 16, 32, 64, 64, 3, 1, 16128064, norm=True, precision="bf16x6_w"),
    _sc("bf16x6_w-small-s2", 2, 32, 32, 64, 70, 3, 2, 16064064, precision="bf16x6_w"),
    _sc("bf16x6-stem-auto", 2, 64, 96, 4, 64, 7, 2, 0, stem=True, precision="bf16x6", auto=(64, 64, 48)),
]
BF16_TOL = {"bf16x3": 2e-4, "bf16x3_w": 2e-4, "bf16x6": 2e-5, "bf16x6_w": 2e-5}     # test_conv2d_bf16x3_mode / test_conv2d_bf16x6_mode_is_fp32_accurate, outputs O(1)


def _plan(c, **over):
    kw = dict(stride=c["stride"], tile=c["tile"], norm=c["norm"], precision=c["precision"], splitk=c["splitk"])
    kw.update(over)
    return ic.plan(c["B"], c["H"], c["W"], c["cin"], c["cout"], c["kh"], c["kw"], **kw)


def _layer(c):
    """Inputs of a case on the CPU: x NCHW float32 (the stem's from preprocess_u8 arithmetic), w OIHW, shift, and for a fused
    norm the float32 statistics with channel means of either sign and distinct offsets per image."""
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in c["name"]))
    B, H, W, cin, cout, k = c["B"], c["H"], c["W"], c["cin"], c["cout"], c["kh"]
    if c["stem"]:
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        x = None
    else:
        img = None
        off = torch.where(torch.arange(cin) % 2 == 0, 1.5, -1.5).view(1, cin, 1, 1) + 0.25 * torch.arange(B).view(B, 1, 1, 1)
        x = torch.randn((B, cin, H, W), generator=g) * 2.0 + off
    real_cin = 3 if c["stem"] else cin
    w = torch.randn((cout, real_cin, k, k), generator=g) / np.sqrt(real_cin * k * k)
    shift = torch.randn((cout,), generator=g) * 0.5
    return img, x, w, shift


def _run_stats_case(c, extra_part=4096, **conv_kw):
    """Run the convolution with statistics twice.  Returns the plan, the kernel's output (NCHW, CPU), the float64 reference and
    magnitude, the partial buffer of the first run (CPU) and the reported rows."""
    ops = _ops()
    img, x, w, shift = _layer(c)
    B, cout, k, stride = c["B"], c["cout"], c["kh"], c["stride"]
    if c["stem"]:
        xin = ops.preprocess_u8(img.cuda())
        x = nchw(xin)                                        # 4 channels, the last one zero: the operand the kernel reads
        w = torch.cat([w, torch.zeros_like(w[:, :1])], 1)
        wp = ops.pack_conv_weight(w, 4).cuda()
    else:
        xin = nhwc(x)
        wp = ops.pack_conv_weight(w).cuda()
    if c["precision"] == "bf16x3_w":
        wp = ops.split_conv_weight(wp.cpu()).cuda()
    elif c["precision"] == "bf16x6_w":
        wp = ops.split_conv_weight3(wp.cpu()).cuda()
    kw = dict(stride=stride, shift=shift.cuda(), tile=c["tile"], precision=c["precision"])
    operand = x
    if c["norm"]:
        mean = x.double().mean(dim=(2, 3)).float()
        rstd = (1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)).float()
        kw.update(nmean=mean.cuda(), nrstd=rstd.cuda())
        # the staging code's own arithmetic: fmaxf((v - mu) * rs, 0) in fp32, zero padding applied after it
        operand = torch.clamp_min((x - mean.view(B, -1, 1, 1)) * rstd.view(B, -1, 1, 1), 0.0)
    ws = None
    if c["splitk"]:
        ws = torch.zeros((65536 + 64 * 4 * 64 * 64 * 4,), dtype=torch.uint8, device="cuda")
        kw.update(splitk_ws=ws)
    kw.update(conv_kw)
    ref = F.conv2d(operand.double(), w.double(), stride=stride, padding=k // 2) + shift.double().view(1, -1, 1, 1)
    mag = F.conv2d(operand.double().abs(), w.double().abs(), stride=stride, padding=k // 2) + shift.double().abs().view(1, -1, 1, 1)
    p = _plan(c)
    need = B * p["rows"] * cout * 2
    parts, outs = [], []
    for _ in range(2):
        part = torch.full((need + extra_part,), float("nan"), device="cuda")
        out, rows = ops.conv2d_nhwc(xin, wp, k, k, cout, stats_part=part, **kw)
        parts.append(part.cpu())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    same = torch.equal(parts[0][:need], parts[1][:need])
    info = dict(xin=xin, wp=wp, kw=kw, ws=ws)
    return p, nchw(outs[0]), ref, mag, parts[0], rows, same, info


def _check_partials(c, p, out, part, rows):
    B, cout = c["B"], c["cout"]
    assert rows == p["rows"] > 0, (rows, p)
    need = B * rows * cout * 2
    assert bool(torch.isfinite(part[:need]).all()), "a partial the host counted was never written"
    assert bool(torch.isnan(part[need:]).all()), "written past [B][rows][Cout][2]"
    pr = part[:need].view(B, rows, cout, 2)
    labels = ic.row_labels(p)
    ratios = ic.partial_ratios(pr, out, labels, rows)
    for k, r in ratios.items():
        _note(f"partials {k}", r)
    assert not ic.partial_violations(pr, out, labels, rows), (c["name"], ratios)
    mean, rstd = _ops().inorm_finalize(part[:need].cuda(), B, rows, p["Ho"] * p["Wo"], cout)
    fr = ic.finalized_ratios(mean.cpu(), rstd.cpu(), out, ic.K_STATS * ic.U)
    for k, r in fr.items():
        _note(f"finalised {k} (epilogue partials)", r)
    assert fr["mean"] <= 1.0 and fr["rstd"] <= 1.0, (c["name"], fr)


@gpu
@pytest.mark.parametrize("c", STATS_CASES, ids=[c["name"] for c in STATS_CASES])
def test_direct_kernel_epilogue_statistics(cuda, c):
    """ofx_conv2d_stats on the direct kernels: the row count the launcher's rule gives, exactly B * rows * Cout * 2 floats written,
    a repeat bit-identical, every row's (sum, sum of squares) and the per-image totals within K_STATS of the float64 sums of the
    kernel's own output over that row's pixels, the finalised mean / rstd within their bounds, and the output itself within
    K_DIRECT of the float64 convolution."""
    p, out, ref, mag, part, rows, same, info = _run_stats_case(c)
    _note("conv output (direct, K_DIRECT)", wc.check(out, ref, mag, wc.K_DIRECT, c["name"]))
    _check_partials(c, p, out, part, rows)
    assert same, "the partials of a second launch differ"
    if c["splitk"]:
        # the split ran, the way test_conv2d_split_k_small_grids checks it: counters back at zero, another summation order
        assert p["splits"] > 1
        assert int(info["ws"][:65536].view(torch.int32).abs().max()) == 0
        kw = {k: v for k, v in info["kw"].items() if k != "splitk_ws"}
        plain = _ops().conv2d_nhwc(info["xin"], info["wp"], c["kh"], c["kw"], c["cout"], **kw)
        assert not torch.equal(nchw(plain), out)
        assert not bool(wc.violations(nchw(plain), ref, mag, wc.K_DIRECT).any())


@gpu
@pytest.mark.parametrize("c", BF16_CASES, ids=[c["name"] for c in BF16_CASES])
def test_split_bf16_precisions_leave_statistics_of_their_own_output(cuda, c):
    """The split-bf16 modes produce the partials too (the engine's bf16 modes rely on it): rows by the remapped tile, the sums
    referred to the kernel's own fp32 output under the same bounds, the output under the bf16 tolerances."""
    p, out, ref, mag, part, rows, same, info = _run_stats_case(c)
    err = (out.double() - ref).abs().max().item()
    _note(f"conv output abs error ({c['precision']})", err)
    assert 0 < err < BF16_TOL[c["precision"]], err
    _check_partials(c, p, out, part, rows)
    assert same


NO_STATS = [
    ("relu", _sc("no-relu", 2, 16, 32, 64, 64, 3, 1, 16128064), dict(act="relu")),
    ("res", _sc("no-res", 2, 16, 32, 64, 64, 3, 1, 16128064), dict(res=True)),
    ("straddle", _sc("no-straddle", 2, 24, 24, 64, 128, 3, 2, 16128128), {}),          # 12 x 12 = 144 rows per image, BM = 128
    ("straddle-64", _sc("no-straddle-64", 3, 10, 10, 16, 64, 3, 1, 16064064), {}),     # 100 rows per image, BM = 64
    ("short", _sc("no-short", 2, 16, 32, 64, 64, 3, 1, 16128064), dict(short=True)),
    ("short-general", _sc("no-short-general", 2, 32, 32, 64, 128, 3, 2, 16128128), dict(short=True)),
]


@gpu
@pytest.mark.parametrize("why,c,how", NO_STATS, ids=[n[0] for n in NO_STATS])
def test_launches_that_must_not_produce_statistics(cuda, why, c, how):
    """An activation, a residual merge, a tile that would straddle two images, or a buffer one float too small: rows = 0, every
    float of `part` still NaN, and the output is what the plain call gives."""
    ops = _ops()
    _, x, w, shift = _layer(c)
    xin, wp = nhwc(x), ops.pack_conv_weight(w).cuda()
    kw = dict(stride=c["stride"], shift=shift.cuda(), tile=c["tile"])
    if how.get("act"):
        kw.update(act=how["act"])
    if how.get("res"):
        Ho, Wo = ic.out_size(c["H"], c["W"], c["kh"], c["kw"], c["stride"])
        kw.update(res=torch.randn((c["B"], Ho, Wo, c["cout"]), device="cuda"))
    would = _plan(c)["rows"]
    if why.startswith("straddle"):
        assert would == 0 and (_plan(c)["Ho"] * _plan(c)["Wo"]) % _plan(c)["bm"] != 0
        n = 1 << 16
    elif how.get("short"):
        assert would > 0
        n = c["B"] * would * c["cout"] * 2 - 1
    else:
        assert would > 0 and _plan(c, act=how.get("act"), res=bool(how.get("res")))["rows"] == 0
        n = c["B"] * would * c["cout"] * 2 + 64
    part = torch.full((n,), float("nan"), device="cuda")
    out, rows = ops.conv2d_nhwc(xin, wp, c["kh"], c["kw"], c["cout"], stats_part=part, **kw)
    plain = ops.conv2d_nhwc(xin, wp, c["kh"], c["kw"], c["cout"], **kw)
    assert rows == 0
    assert bool(torch.isnan(part).all())
    assert torch.equal(out, plain)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. ofx_inorm_stats

STATS_C = [4, 8, 16, 24, 32, 64, 96, 128, 256]
STATS_B = [1, 7, 8, 9]
STATS_HW = [(1, 1), (1, 3), (7, 9), (15, 17), (1, 257), (64, 96)]        # 1, 3, 63, 255, 257, 6144 pixels
LARGE_MAP = (384, 256)


def _stat_input(B, H, W, C, g):
    """Per channel (c % 4): plain; constant (var = 0); |mean| / std = 1e3; +-large values.  Distinct per image."""
    hw = H * W
    x = torch.randn((B, H, W, C), generator=g) * 2.0 + 0.5
    b = torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1)
    x[..., 1::4] = 0.75 + 0.125 * b
    x[..., 2::4] = 100.0 + b + 0.1 * torch.randn((B, H, W, len(range(2, C, 4))), generator=g)
    amp = 1e4 if hw >= 63 else 30.0          # (a map of 1 or 3 pixels can be constant: var + eps = eps takes no 1e8 next to it)
    sign = torch.where(torch.rand((B, H, W, len(range(3, C, 4))), generator=g) < 0.5, -1.0, 1.0)
    x[..., 3::4] = sign * amp * (1.0 + 0.01 * b)
    return x


def _check_f64_pass(x_nhwc, mean, rstd, what):
    v = x_nhwc.permute(0, 3, 1, 2)
    hw = v.shape[2] * v.shape[3]
    fr = ic.finalized_ratios(mean.cpu(), rstd.cpu(), v, 2.0 ** -52 * hw)
    _note("f64 pass mean", fr["mean"])
    _note("f64 pass rstd", fr["rstd"])
    assert fr["mean"] <= 1.0 and fr["rstd"] <= 1.0, (what, fr)
    const = ic.stats64(v)["var"] == 0
    if bool(const.any()):        # constant channels: rstd = 1 / sqrt(eps) up to the bound above
        assert float((rstd.cpu().double()[const] * np.sqrt(1e-5) - 1.0).abs().max()) < 1e-3


@gpu
@pytest.mark.parametrize("C", STATS_C)
def test_f64_statistics_pass(cuda, C):
    """Every thread layout of the partial kernel (C / 4 channel groups of 256 / (C / 4) rows), both slice counts (B < 8: 256, from
    8 on: 64), maps with fewer pixels than slices, constant / offset / large channels -- and the statistics of a channel slice."""
    ops = _ops()
    g = torch.Generator().manual_seed(100 + C)
    for B in STATS_B:
        for (H, W) in STATS_HW:
            if H * W == 6144 and B in (7, 9):
                continue                       # the cross product is thinned at the one sizeable map, not at the edges
            x = _stat_input(B, H, W, C, g)
            mean, rstd = ops.inorm_stats(x.cuda())
            _check_f64_pass(x, mean, rstd, (C, B, H, W))
    # ld > C: the slice [off, off + C) of rows 1.5x as wide (neighbouring channels hold large values a wrong stride would pick up)
    for B, (H, W) in ((1, (7, 9)), (8, (15, 17)), (3, (64, 96))):
        ld = C + C // 2 + (4 - (C + C // 2) % 4) % 4
        for off in (0, ld - C):
            wide = torch.full((B, H, W, ld), 3e4)
            x = _stat_input(B, H, W, C, g)
            wide[..., off:off + C] = x
            mean, rstd = ops.inorm_stats(wide.cuda(), c_off=off, c=C)
            assert tuple(mean.shape) == (B, C)
            _check_f64_pass(x, mean, rstd, ("slice", C, B, H, W, off))


@gpu
def test_f64_statistics_pass_on_one_large_map_and_its_refusals(cuda):
    ops = _ops()
    from sd_animation_optical_flow_amd import _lib
    g = torch.Generator().manual_seed(7)
    for B, C in ((1, 64), (8, 24)):
        x = _stat_input(B, LARGE_MAP[0], LARGE_MAP[1], C, g)
        mean, rstd = ops.inorm_stats(x.cuda())
        _check_f64_pass(x, mean, rstd, ("large", B, C))
    for C in (260, 6):             # C <= 256 and C % 4 == 0: refused with OFX_EALIGN (include/ofx.h)
        with pytest.raises(_lib.OfxError) as e:
            ops.inorm_stats(torch.zeros((1, 4, 4, C), device="cuda"))
        assert e.value.code == -2


# ---------------------------------------------------------------------------------------------------------------------------------
# d. ofx_inorm_finalize on synthetic partials

FIN_ROWS = [1, 63, 64, 65, 511, 512, 513, 1000]
FIN_C = [2, 4, 6, 96, 256]
FIN_B = [1, 3]


def _synthetic_partials(B, rows, C, g):
    """Sums of mixed sign and scale per row, with sums of squares that keep the variance positive: Q_r >= S_r^2 and HW = 16 rows
    give (sum S / HW)^2 <= sum Q / (16 HW)."""
    scale = 10.0 ** torch.randint(-2, 3, (B, rows, C), generator=g).float()
    S = torch.randn((B, rows, C), generator=g) * scale
    Q = S * S + torch.rand((B, rows, C), generator=g) * scale
    return torch.stack([S, Q], -1).contiguous(), 16 * rows


@gpu
@pytest.mark.parametrize("rows", FIN_ROWS)
def test_finalize_on_synthetic_partials(cuda, rows):
    """Both sides of the unrolled loop's boundary (r + 7 * 64 < rows), fewer rows than the 64 row groups, channel counts that are
    no multiple of the 4 channels of a workgroup.  The outputs are guard-padded (the entry point is called directly): a thread of
    a channel past C that wrote would land in the next image's slots, and for the last image past [B][C], where NaN must stay."""
    import ctypes as C_
    from sd_animation_optical_flow_amd import _lib
    g = torch.Generator().manual_seed(rows)
    GUARD = 64
    for C in FIN_C:
        for B in FIN_B:
            part, HW = _synthetic_partials(B, rows, C, g)
            pd = part.cuda()
            bufs = [torch.full((B * C + GUARD,), float("nan"), device="cuda") for _ in range(2)]
            _lib.check(_lib.lib().ofx_inorm_finalize(C_.c_void_p(pd.data_ptr()), C_.c_void_p(bufs[0].data_ptr()), C_.c_void_p(bufs[1].data_ptr()),
                                                     B, rows, HW, C, 1e-5, C_.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "ofx_inorm_finalize")
            assert all(bool(torch.isnan(b[B * C:]).all()) for b in bufs), (rows, C, B, "written past [B][C]")
            mean, rstd = (b[:B * C].view(B, C) for b in bufs)
            fr = ic.stat_ratios(mean.cpu(), rstd.cpu(), ic.partials_reference(part, HW), 2.0 ** -52 * rows, 2.0)
            _note("finalize mean", fr["mean"])
            _note("finalize rstd", fr["rstd"])
            assert fr["mean"] <= 1.0 and fr["rstd"] <= 1.0, (rows, C, B, fr)


# ---------------------------------------------------------------------------------------------------------------------------------
# e. ofx_inorm_apply

APPLY_MODES = {          # name: (relu, residual, normalised residual)
    "plain": (0, False, False), "relu": (1, False, False), "raw-residual": (1, True, False), "normalised-residual": (1, True, True),
    "normalised-relu-residual": (3, True, True),
}
APPLY_SHAPES = ([(B, HW, C) for C in (4, 8, 24, 96, 256, 1024) for B in (1, 3) for HW in (1, 7, 6144) if not (C == 1024 and HW == 6144 and B == 3)]
                + [(5000, 7, 4), (5000, 7, 24), (5000, 1, 96), (5000, 1, 256), (5000, 1, 1024)])


def _apply_stats(B, C, g):
    """Statistics with means of either sign and distinct values per image and channel (a wrong [b][c] index shows)."""
    mean = (torch.randn((B, C), generator=g) + torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)).contiguous()
    rstd = (0.5 + torch.rand((B, C), generator=g)).contiguous()
    return mean, rstd


@gpu
@pytest.mark.parametrize("mode", list(APPLY_MODES))
def test_inorm_apply_every_mode_as_floats_and_against_float64(cuda, mode):
    ops = _ops()
    relu, has_res, norm_res = APPLY_MODES[mode]
    g = torch.Generator().manual_seed(len(mode))
    for (B, HW, C) in APPLY_SHAPES:
        x = torch.randn((B, HW, 1, C), generator=g) * 2.0
        mean, rstd = _apply_stats(B, C, g)
        res = torch.randn((B, HW, 1, C), generator=g) * 2.0 if has_res else None
        rm, rs = _apply_stats(B, C, g) if norm_res else (None, None)
        dev = lambda t: None if t is None else t.cuda()
        xd, resd = dev(x), dev(res)
        out = ops.inorm_apply(xd, dev(mean), dev(rstd), res=resd, res_mean=dev(rm), res_rstd=dev(rs), relu=relu)
        assert out.data_ptr() not in (xd.data_ptr(), 0 if resd is None else resd.data_ptr())
        assert torch.equal(xd.cpu(), x) and (res is None or torch.equal(resd.cpu(), res))      # the inputs are only read
        cl = lambda t: None if t is None else t.permute(0, 3, 1, 2)                              # [B, C, HW, 1]
        want = ic.apply_f32(cl(x), mean, rstd, cl(res), rm, rs, relu)
        got = cl(out.cpu())
        bad = got != want
        assert not bool(bad.any()), (mode, B, HW, C, int(bad.sum()), float((got - want).abs().max()))
        ref, mag = ic.apply_f64(cl(x), mean, rstd, cl(res), rm, rs, relu)
        r = wc.worst_ratio(got, ref, mag)
        _note("apply vs float64 (K_APPLY)", r)
        assert r <= ic.K_APPLY, (mode, B, HW, C, r)
    if mode == "relu":       # True / False keep meaning 1 / 0
        a = ops.inorm_apply(xd, dev(mean), dev(rstd), relu=True)
        b = ops.inorm_apply(xd, dev(mean), dev(rstd), relu=False)
        assert torch.equal(a, out) and float(b.min()) < 0 and torch.equal(torch.relu(b), a)


@gpu
def test_inorm_apply_refuses_more_than_1024_channels(cuda):
    ops = _ops()
    from sd_animation_optical_flow_amd import _lib
    z = torch.zeros((1, 2, 2, 1028), device="cuda")
    s = torch.zeros((1, 1028), device="cuda")
    with pytest.raises(_lib.OfxError) as e:
        ops.inorm_apply(z, s, s)
    assert e.value.code == -1


# ---------------------------------------------------------------------------------------------------------------------------------
# f. norm + ReLU on load in the direct kernels

NORM_TILES = [16128096, 16128128, 16128064, 16128192, 32128032, 16064064, 32064064, 2032064064, 16256064, 0]
NORM_MAPS = [(16, 32), (13, 22)]        # whole 8x16 (and 16x16 / 8x8) patches; every patch tile hangs over


@gpu
@pytest.mark.parametrize("tile", NORM_TILES)
@pytest.mark.parametrize("H,W", NORM_MAPS)
def test_direct_kernels_pad_after_normalising_on_load(cuda, tile, H, W):
    """The direct-kernel twin of test_norm_and_relu_on_load_pads_after_normalising: the operand is relu((x - mean) * rstd) and the
    zero padding is that of the normalised map.  Channel means alternate in sign (normalising the padding would feed
    relu(-mean * rstd) into every border tap) and every image has its own offset.  The staging code computes
    fmaxf((v - mu) * rs, 0) in fp32 (conv.hip, a_commit / norm_a) -- the same form as here, so no extra rounding is allowed."""
    ops = _ops()
    B, c, co = 3, 64, 96
    g = torch.Generator().manual_seed(tile % 1000 + H)
    w = torch.randn((co, c, 3, 3), generator=g) / np.sqrt(c * 9)
    shift = torch.randn((co,), generator=g) * 0.1
    off = torch.where(torch.arange(c) % 2 == 0, 1.5, -1.5).view(1, c, 1, 1) * (1.0 + 0.5 * torch.arange(B).view(B, 1, 1, 1))
    x = torch.randn((B, c, H, W), generator=g) * 2.0 + off
    mean = x.double().mean(dim=(2, 3)).float()
    rstd = (1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)).float()
    xn = torch.clamp_min((x - mean.view(B, c, 1, 1)) * rstd.view(B, c, 1, 1), 0.0)
    ref, mag = wc.reference(xn, w, 3, 3, shift=shift)
    out = nchw(ops.conv2d_nhwc(nhwc(x), ops.pack_conv_weight(w).cuda(), 3, 3, co, shift=shift.cuda(), nmean=mean.cuda(),
                               nrstd=rstd.cuda(), tile=tile))
    for name, sl in (("all", np.s_[:]), ("top", np.s_[:, :, 0]), ("bottom", np.s_[:, :, -1]), ("left", np.s_[:, :, :, 0]),
                     ("right", np.s_[:, :, :, -1])):
        r = wc.check(out[sl], ref[sl], mag[sl], wc.K_DIRECT, f"tile {tile} {H}x{W} {name}")
        _note(f"norm on load, {name}", r)


# ---------------------------------------------------------------------------------------------------------------------------------
# g. CPU self-tests: what the tables cover, and what the checker catches

def test_stats_cases_cover_the_launcher_table_schedules_strides_and_patches():
    plans = [(_plan(c), c) for c in STATS_CASES]
    assert all(p["rows"] > 0 for p, _ in plans)
    assert {(p["bm"], p["bn"]) for p, _ in plans} == set(ic.WAVES_M)                      # every entry of setup_stats' table
    for kind in ("general", "scalar", "patch"):
        assert {(p["bm"], p["bn"]) for p, _ in plans if p["kind"] == kind}, kind
    # the patch kernel on whole and on overhanging maps, for every tile that has it; the 8x8-patch small tile on whole maps
    big = {(256, 64), (128, 128), (128, 64), (128, 192), (128, 96)}
    assert {(p["bm"], p["bn"]) for p, _ in plans if p["kind"] == "patch" and p["whole"]} == big | {(64, 64)}
    assert {(p["bm"], p["bn"]) for p, _ in plans if p["kind"] == "patch" and not p["whole"]} == big
    # both strides on the kernels that are not tied to stride 1, the stem, the downsample
    for stride in (1, 2):
        assert {p["kind"] for p, c in plans if c["stride"] == stride} >= {"general", "scalar"}
    assert {(c["kh"], c["stride"]) for _, c in plans} == {(3, 1), (3, 2), (7, 2), (1, 2)}
    assert all(c["stem"] == (c["kh"] == 7) for _, c in plans)
    # every tile code the issue names, and the automatic choice landing on each kind of tile
    assert {c["tile"] for _, c in plans} == {16256064, 16128128, 16128064, 16128192, 16128096, 32128032, 16064064, 32064064, 2032064064, 0}
    assert {(p["bm"], p["bn"]) for p, c in plans if c["tile"] == 0} >= {(256, 64), (128, 32), (64, 64)}
    assert any(p["paired"] for p, _ in plans) and {p["kind"] for p, _ in plans if p["splits"] > 1} == {"patch", "scalar"}
    assert {c["cout"] for _, c in plans} == {64, 70, 96, 128} and {c["B"] for _, c in plans} == {1, 2, 3}
    # with and without the fused norm on every schedule
    for kind in ("general", "scalar", "patch"):
        assert {c["norm"] for p, c in plans if p["kind"] == kind} == {False, True}, kind
    # the largest map is one 384x256 stage
    assert max(p["Ho"] * p["Wo"] for p, _ in plans) == 384 * 256
    # the split-bf16 table: the three tiles the modes map onto, a remap that changes the rows, patch whole / overhanging
    bplans = [(_plan(c), c) for c in BF16_CASES]
    assert {(p["bm"], p["bn"]) for p, _ in bplans} == {(128, 128), (128, 64), (64, 64)}
    assert any(p["rows"] != _plan(c, precision="fp32")["rows"] for p, c in bplans)
    assert {p["whole"] for p, _ in bplans if p["kind"] == "patch"} == {True, False}
    assert {c["precision"] for _, c in bplans} == {"bf16x3", "bf16x3_w", "bf16x6", "bf16x6_w"}


def test_automatic_choices_are_where_the_table_says():
    """The tile = 0 cases rest on the launcher's tuning heuristics as restated in inorm_check.plan() (the chip-fill count, the patch
    cover, the pairing limit, the split-K rule, the 256x64 promotion).  If this fails after a retune, the heuristic moved: update
    plan() and the literals, the statistics themselves are not in question."""
    autos = [c for c in STATS_CASES + BF16_CASES if c["tile"] == 0]
    assert autos and all(c["auto"] is not None for c in autos)
    assert all(c["auto"] is None for c in STATS_CASES + BF16_CASES if c["tile"] != 0)
    for c in autos:
        p = _plan(c)
        assert (p["bm"], p["bn"], p["rows"]) == c["auto"], (c["name"], p)


def test_row_labels_partition_every_map_into_rows_of_the_right_size():
    for c in STATS_CASES + BF16_CASES:
        p = _plan(c)
        labels = ic.row_labels(p)
        counts = torch.bincount(labels, minlength=p["rows"])
        assert counts.numel() == p["rows"], c["name"]
        if p["kind"] == "patch" and not p["whole"]:
            assert int(counts.max()) <= p["wm"] and int(counts.sum()) == p["Ho"] * p["Wo"]
        else:
            assert bool((counts == p["wm"]).all()), c["name"]


def test_other_case_tables_cover_their_edges():
    assert {1, 7} <= set(STATS_B) and {8, 9} <= set(STATS_B)                               # both sides of the slice-count switch
    assert {h * w for h, w in STATS_HW} == {1, 3, 63, 255, 257, 6144}
    assert any(256 % (C // 4) != 0 for C in STATS_C) and {4, 256} <= set(STATS_C)          # 240 / 252 active threads; the extremes
    assert any(h * w < 64 for h, w in STATS_HW)                                            # fewer pixels than slices
    # finalize: the unrolled loop runs for a row group g iff g + 448 < rows; both sides, and rows < 64
    assert any(r <= 448 for r in FIN_ROWS) and {511, 512, 513} <= set(FIN_ROWS) and min(FIN_ROWS) < 64
    assert any(C % 4 for C in FIN_C)
    # apply: 2, 6, 24 threads per row, a block of 240, the 1024-channel limit, one slice per image, one pixel
    assert {c for _, _, c in APPLY_SHAPES} == {4, 8, 24, 96, 256, 1024}
    assert {b for b, _, _ in APPLY_SHAPES} == {1, 3, 5000} and {hw for _, hw, _ in APPLY_SHAPES} == {1, 7, 6144}
    assert set(APPLY_MODES.values()) == {(0, False, False), (1, False, False), (1, True, False), (1, True, True), (3, True, True)}


def _exact_partials(p, B, C, g):
    v = (torch.randn((B, C, p["Ho"], p["Wo"]), generator=g, dtype=torch.float64) * 1.5
         + torch.tensor([0.7, -1.2, 0.3, 2.0], dtype=torch.float64)[:C].view(1, C, 1, 1))
    labels = ic.row_labels(p)
    S, Q, _ = ic.row_sums(v, labels, p["rows"])
    return v, labels, torch.stack([S, Q], -1)


def _bugged(name, part, v, p):
    """`part` [B, rows, C, 2] float64 with one simulated kernel bug."""
    out = part.clone()
    wpt = p["bm"] // p["wm"]                        # wave rows per tile
    r = int(ic.row_labels(p)[-1])                   # the row of the map's last pixel (a later row of an overhanging patch can be empty)
    if name == "wave_row_dropped":
        out[0, r] = 0.0
    elif name == "masked_pixel_included":           # one value of typical size (the channel's rms) that is not a pixel of the map
        rms = (v[0] ** 2).mean(dim=(1, 2)).sqrt()
        out[0, r, :, 0] += rms
        out[0, r, :, 1] += rms * rms
    elif name == "tile_credited_to_next_image":     # the last tile of image 0 lands in the first tile's rows of image 1
        out[1, :wpt] += out[0, -wpt:]
        out[0, -wpt:] = 0.0
    elif name == "sum_and_squares_swapped":
        out = out.flip(-1)
    return out


PARTIAL_BUGS = ["wave_row_dropped", "masked_pixel_included", "tile_credited_to_next_image", "sum_and_squares_swapped"]


def _map_sizes():
    seen, out = set(), []
    for c in STATS_CASES + BF16_CASES:
        p = _plan(c)
        key = (p["kind"], p["bm"], p["bn"], p["Ho"], p["Wo"])
        if key not in seen:
            seen.add(key)
            out.append((c["name"], p))
    return out


def test_the_checker_catches_each_simulated_statistics_bug_at_every_map_size():
    """Which check catches what: the PER-ROW check catches every bug at every map size of the table (a row holds at most 64
    values, so one value too many or too few is 1/64 of it against a bound of 64 u ~ 4e-6).  The PER-IMAGE TOTALS catch them too up
    to the largest map of the table (one rms-sized value against 64 u HW rms = 0.37 rms at 384x256), but not beyond: at 1024x1024
    the totals pass a single extra pixel and only the per-row check sees it.  The padded pixel count is caught by the finalised
    mean and rstd."""
    g = torch.Generator().manual_seed(11)
    over = 0
    for name, p in _map_sizes():
        v, labels, exact = _exact_partials(p, 2, 4, g)
        rows, hw = p["rows"], p["Ho"] * p["Wo"]
        # the float32 rounding of the right answer passes, and so does an error of half the bound
        assert not ic.partial_violations(exact.float(), v, labels, rows), name
        _, _, A = ic.row_sums(v, labels, rows)
        nudged = exact.clone()
        nudged[..., 0] += 0.5 * ic.K_STATS * ic.U * A
        nudged[..., 1] *= 1.0 + 0.5 * ic.K_STATS * ic.U
        assert not ic.partial_violations(nudged, v, labels, rows), name
        m, s = ic.finalize64(exact.float(), hw)
        fr = ic.finalized_ratios(m.float(), s.float(), v, ic.K_STATS * ic.U)
        assert fr["mean"] <= 1.0 and fr["rstd"] <= 1.0, (name, fr)
        for bug in PARTIAL_BUGS:
            bad = ic.partial_violations(_bugged(bug, exact, v, p).float(), v, labels, rows)
            assert {k for k in bad if k.startswith("row")}, (name, bug, "per-row check")
            assert {k for k in bad if k.startswith("total")}, (name, bug, "totals")
        # a mean over the padded rather than the real pixel count (overhanging patches only: elsewhere the two agree)
        if p["kind"] == "patch" and not p["whole"]:
            over += 1
            padded = -(-p["Ho"] // p["ph"]) * p["ph"] * -(-p["Wo"] // p["pw"]) * p["pw"]
            assert padded > hw
            m, s = ic.finalize64(exact.float(), padded)
            fr = ic.finalized_ratios(m.float(), s.float(), v, ic.K_STATS * ic.U)
            assert fr["mean"] > 1.0 and fr["rstd"] > 1.0, (name, fr)
    assert over >= 5
    # beyond the table: one extra pixel in a 1024x1024 map is below the bound of the totals; the per-row check still catches it
    p = ic.plan(2, 1024, 1024, 64, 64, 3, 3, tile=16128064)
    v, labels, exact = _exact_partials(p, 2, 2, g)
    bad = ic.partial_violations(_bugged("masked_pixel_included", exact, v, p).float(), v, labels, p["rows"])
    assert bad == {"row_S", "row_Q"}


def test_the_checker_counts_an_unwritten_partial_as_a_violation():
    p = _plan(STATS_CASES[0])
    v, labels, exact = _exact_partials(p, 2, 4, torch.Generator().manual_seed(1))
    part = exact.float()
    part[1, 3, 2, 1] = float("nan")
    assert ic.partial_violations(part, v, labels, p["rows"]) == {"row_Q", "total_Q"}


def test_the_apply_restatement_and_its_float64_twin_agree_and_catch_a_dropped_mode_bit():
    g = torch.Generator().manual_seed(2)
    x, res = torch.randn((2, 8, 5, 1), generator=g) * 2, torch.randn((2, 8, 5, 1), generator=g) * 2
    (m, s), (rm, rs) = _apply_stats(2, 8, g), _apply_stats(2, 8, g)
    for relu, r, a, b in [(0, None, None, None), (1, None, None, None), (1, res, None, None), (1, res, rm, rs), (3, res, rm, rs)]:
        ref, mag = ic.apply_f64(x, m, s, r, a, b, relu)
        assert wc.worst_ratio(ic.apply_f32(x, m, s, r, a, b, relu), ref, mag) <= ic.K_APPLY
    # bit 1 ignored (the residual not ReLU'd), or the statistics of the wrong image: far outside
    ref, mag = ic.apply_f64(x, m, s, res, rm, rs, 3)
    assert wc.worst_ratio(ic.apply_f32(x, m, s, res, rm, rs, 1), ref, mag) > 1e3
    assert wc.worst_ratio(ic.apply_f32(x, m.flip(0), s, res, rm, rs, 3), ref, mag) > 1e3
