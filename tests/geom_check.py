"""The direct convolutions off 'same' padding: the geometries, the case table and the simulated bugs.  Not a conftest: imported by
name, and importable without a device.  ofx_conv_desc carries padH, padW, Hout and Wout as four free integers (include/ofx.h: taps
outside the image contribute zero, Hout and Wout are the caller's); the tables of fp32_check.py, bf16_check.py and f16_check.py hold
the kernels to float64 with padH = KH // 2, padW = KW // 2 and the output size that follows, and to nothing else.  One production
layer is off that setting -- the VAE encoder's Downsample (vae.py: 3x3, stride 2, pad (0, 0), out_hw (H / 2, W / 2)).  This table
runs the general gather and the scalar-coordinate schedule of igemm_kernel (csrc/conv.hip) on such descriptors.

Nothing of the three modules is restated: a case here is a case of theirs with the two optional keys `pad` and `out_hw`
(wino_check.geometry_of), registered with the module whose inputs, oracle, bound, guard rows, buffers and descriptor it uses
(fp32_check.register / bf16_check.register; the fp16 cases take f16_check's inputs and derived bound and fp32_check's guarded
buffers and descriptor, with `precision` set).  The reference of a geometry is wino_check.conv64_geometry: zero-pad, F.conv2d with no
padding, crop.  No new tolerance: a geometry changes which terms enter a sum, not the arithmetic, and an output here has at most the
K terms of a 'same' output -- K_DIRECT, K_of(prec) and f16_check's derived bound apply as they stand.

Geometries (GEOMS), each on map T = 2x10x14 (two images: a wrap into the next image shows; every distinguishing tap exists):
    down        3x3 s2  pad (0,0)  out (H/2, W/2)      the VAE's Downsample: zeros below and right only
    valid       3x3 s1  pad (0,0)  out (H-2, W-2)      no padding at all, Hout Wout != Hin Win
    valid-s2    3x3 s2  pad (0,0)  natural             on T the last input row and column are unused, on R (9x17) they are used
    wide        3x3 s1  pad (2,2)  out (H+2, W+2)      a corner output touches one pixel
    ring        3x3 s1  pad (3,3)  out (H+4, W+4)      a ring of outputs with no tap inside the image
    ring-1x1    1x1 s1  pad (1,1)  out (H+2, W+2)      likewise
    asym-h / -w 3x3 s1  pad (1,0) / (0,1)  out (H, W-2) / (H-2, W)      padH != padW
    valid-1x5 / -5x1    s1  pad (0,0)  out (H, W-4) / (H-4, W)          the 1-D filters off the halo patch
    crop        3x3 s1  pad (1,1)  out (H-3, W-5)      an output smaller than the natural one
    over        3x3 s1  pad (1,1)  out (H+2, W+3)      rows and columns beyond the natural one
Schedules: Cin 4 / 12 / 44 reach the general gather, Cin 32 / 64 and two segments c0 = c1 = 32 the scalar-coordinate schedule; no
case may be on the halo patch (test_geom_check_host.py).  The `ring` cases carry a shift and ReLU and nothing else: where no tap is
inside the image the accumulator is an exact 0, 0 * scale + shift rounds nowhere, and the stored value must be relu(shift[n]) bit for
bit (`no_tap`).  Shift / addend / res / scale go only to cases where |shift| + |addend| + |res| <= the convolution's magnitude at
every element, which the oracles assert.

Simulated bugs, each the float64 convolution of the reference's operands gathered tap by tap (`gather_conv`, which without a bug is
a second statement of the reference) with one thing wrong, listed for a case only where it changes the result (`bugs_for`):
    same_padding_assumed        k // 2 used for the pads
    pads_swapped                padH and padW exchanged
    zero_tap_replicated         taps outside the image clamp to the edge pixel
    right_tap_wraps_a_row       a tap with ix >= Win reads pixel (iy + 1, ix - Win): the linear pixel index without the test
    bottom_tap_wraps_an_image   a tap with iy >= Hin reads row iy - Hin of image b + 1 (zero for the last image)
    rows_by_input_size          the output row index decomposed with Hin Win / Win instead of Hout Wout / Wout
    padding_normalised          the norm cases: the geometry's own zeros run through the norm on load
"""
import functools

import torch

import bf16_check as bc
import f16_check as FC
import fp32_check as fc
import wino_check as wc

GATHER, SCALAR, PATCH = fc.GATHER, fc.SCALAR, fc.PATCH
PREC_F16, PREC_F16_EPI = FC.PREC_F16, FC.PREC_F16 | 256
MAPS = dict(T=(2, 10, 14), R=fc.MAPS["R"], G=fc.MAPS["G"], D=fc.MAPS["D"], M=(2, 12, 20))   # M: the model's call, below

# name -> (KH, KW, stride, (padH, padW), (H, W) -> (Hout, Wout))
GEOMS = {
    "down": (3, 3, 2, (0, 0), lambda H, W: (H // 2, W // 2)),
    "valid": (3, 3, 1, (0, 0), lambda H, W: (H - 2, W - 2)),
    "valid-s2": (3, 3, 2, (0, 0), lambda H, W: ((H - 3) // 2 + 1, (W - 3) // 2 + 1)),
    "wide": (3, 3, 1, (2, 2), lambda H, W: (H + 2, W + 2)),
    "ring": (3, 3, 1, (3, 3), lambda H, W: (H + 4, W + 4)),
    "ring-1x1": (1, 1, 1, (1, 1), lambda H, W: (H + 2, W + 2)),
    "asym-h": (3, 3, 1, (1, 0), lambda H, W: (H, W - 2)),
    "asym-w": (3, 3, 1, (0, 1), lambda H, W: (H - 2, W)),
    "valid-1x5": (1, 5, 1, (0, 0), lambda H, W: (H, W - 4)),
    "valid-5x1": (5, 1, 1, (0, 0), lambda H, W: (H - 4, W)),
    "crop": (3, 3, 1, (1, 1), lambda H, W: (H - 3, W - 5)),
    "over": (3, 3, 1, (1, 1), lambda H, W: (H + 2, W + 3)),
}
RINGS = ("ring", "ring-1x1")
RING_EXTRA = dict(shift=True, shift_amp=0.001, act="relu", exact_zero=True)


def _base(name, geom, mp, c0, cout, c1, extra):
    B, H, W = MAPS[mp]
    kh, kw, stride, pad, ohw = GEOMS[geom]
    if geom == "down":
        assert H % 2 == 0 and W % 2 == 0
    return dict(name="g-" + name, geom=geom, map=mp, B=B, H=H, W=W, c0=c0, c1=c1, cout=cout, kh=kh, kw=kw, stride=stride, pad=pad,
                out_hw=ohw(H, W), extra=extra)


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32: fp32_check's cases (name, row of kTiles, plan = (bm, bn, bk, ks, ksplit, mode))

FP32 = []


def _f32(name, geom, mp, c0, cout, row, mode, *, c1=0, ksplit=1, auto=False, **extra):
    tile, bm, bn, bk, ks, sk = fc.ROWS[row]
    assert (ksplit > 1) == sk
    if sk:
        extra["ws"] = True
    c = _base(name, geom, mp, c0, cout, c1, extra)
    fam = "norm" if extra.get("norm") else "plaint" if extra.get("act") in ("tanh", "sigmoid") else "plain"
    c.update(row=row, fam=fam, tile=0 if auto else tile, plan=(bm, bn, bk, ks, ksplit, mode), precision=0)
    FP32.append(fc.register(c))


# ---- every geometry on both schedules, the rows in turn
_f32("valid-gather", "valid", "T", 4, 72, "128x128", GATHER)
_f32("valid-scalar", "valid", "T", 32, 72, "64x64", SCALAR)
_f32("valid-s2-gather", "valid-s2", "T", 12, 72, "256x64", GATHER)
_f32("valid-s2-scalar", "valid-s2", "T", 64, 72, "128x128", SCALAR)
_f32("valid-s2-R-gather", "valid-s2", "R", 4, 72, "64x64", GATHER)                    # 9x17: the last row and column are read
_f32("valid-s2-R-scalar", "valid-s2", "R", 32, 72, "128x64", SCALAR)
_f32("wide-gather", "wide", "T", 4, 200, "128x192", GATHER)                           # 384 rows, two N tiles
_f32("wide-scalar", "wide", "T", 32, 72, "256x64", SCALAR)                            # two 256-row tiles
_f32("ring-gather", "ring", "T", 12, 72, "128x96", GATHER, **RING_EXTRA)
_f32("ring-scalar", "ring", "T", 32, 72, "128x64k32", SCALAR, **RING_EXTRA)
_f32("ring-1x1-gather", "ring-1x1", "T", 4, 72, "64x64k16", GATHER, **RING_EXTRA)
_f32("ring-1x1-scalar", "ring-1x1", "T", 32, 24, "128x32", SCALAR, **RING_EXTRA)
_f32("asym-h-gather", "asym-h", "T", 12, 72, "128x64", GATHER)
_f32("asym-h-scalar", "asym-h", "T", 64, 72, "128x96", SCALAR)
_f32("asym-w-gather", "asym-w", "T", 4, 72, "128x128k32", GATHER)
_f32("asym-w-scalar", "asym-w", "T", 32, 72, "64x64k16", SCALAR)
_f32("valid-1x5-gather", "valid-1x5", "T", 12, 72, "128x64k32", GATHER)
_f32("valid-1x5-scalar", "valid-1x5", "T", 32, 72, "128x128k32", SCALAR)
_f32("valid-5x1-gather", "valid-5x1", "T", 4, 24, "128x32", GATHER)
_f32("valid-5x1-scalar", "valid-5x1", "T", 64, 72, "64x64x2", SCALAR)
_f32("crop-gather", "crop", "T", 12, 72, "64x64x2", GATHER)
_f32("crop-scalar", "crop", "T", 32, 72, "128x64", SCALAR)
_f32("over-gather", "over", "T", 4, 72, "64x64k16", GATHER)
_f32("over-scalar", "over", "T", 64, 72, "128x128", SCALAR)
# ---- two segments
_f32("down-x2", "down", "T", 32, 72, "128x128k32", SCALAR, c1=32)
_f32("valid-x2", "valid", "T", 32, 72, "128x64", SCALAR, c1=32)
_f32("wide-x2", "wide", "T", 32, 72, "64x64", SCALAR, c1=32)
# ---- `down` on every fp32 row of kTiles, on each of gather / scalar the row has (128x192 has no scalar schedule)
for _row in fc.ROWS:
    if _row == "64x64sk":
        continue
    _co = 24 if _row == "128x32" else 72
    _f32(f"down-{_row}-gather", "down", "T", 12 if _row in ("128x96", "64x64") else 4, _co, _row, GATHER)
    if _row != "128x192":
        _f32(f"down-{_row}-scalar", "down", "D" if _row == "256x64" else "T", 64 if _row in ("128x64", "64x64k16") else 32, _co, _row, SCALAR)
_f32("down-64x64sk-gather", "down", "T", 44, 120, "64x64sk", GATHER, ksplit=2)        # K = 396: 13 chunks; 70 rows, 120 channels: ragged
_f32("down-64x64sk-scalar", "down", "T", 64, 120, "64x64sk", SCALAR, ksplit=3)        # K = 576: 18 chunks
# ---- `down` by feature
_f32("down-norm-gather", "down", "T", 12, 72, "128x64", GATHER, norm=True)
_f32("down-norm-scalar", "down", "T", 32, 72, "64x64", SCALAR, norm=True, act="relu")
_f32("down-slice", "down", "T", 32, 72, "128x128", SCALAR, ldo=96, out_off=16)
_f32("down-tanh", "down", "T", 12, 72, "64x64k16", GATHER, act="tanh", shift=True)
_f32("down-ssrr", "down", "T", 64, 72, "128x64k32", SCALAR, scale=True, shift=True, res=True, act="relu")
_f32("valid-addend-shift", "valid", "T", 32, 96, "128x96", SCALAR, addend=True, shift=True, ldadd=128)
# ---- as the model calls it (vae.py: encoder.down.N.downsample.conv): tile = 0, a bias, no workspace
_f32("model-fp32", "down", "M", 128, 128, "64x64x2", SCALAR, auto=True, shift=True)
FP32_IDS = [c["name"] for c in FP32]

# ---------------------------------------------------------------------------------------------------------------------------------
# fp16: f16_check's inputs and derived bound, fp32_check's guarded buffers and descriptor; plan = (bm, bn, bk, mode)

F16 = []


def _f16(name, geom, mp, c0, cout, tile, plan, *, c1=0, precision=PREC_F16, **extra):
    c = _base("f16-" + name, geom, mp, c0, cout, c1, extra)
    c.update(tile=tile, plan=plan, precision=precision)
    F16.append(c)


for _geom in GEOMS:                                                                   # every geometry on both schedules of one tile
    if _geom != "down":
        _ex = RING_EXTRA if _geom in RINGS else {}
        _f16(f"{_geom}-gather", _geom, "T", 4, 72, 32064064, (64, 64, 32, GATHER), **_ex)
        _f16(f"{_geom}-scalar", _geom, "T", 64, 72, 32064064, (64, 64, 32, SCALAR), **_ex)
for _bm, _bn in ((128, 128), (128, 64), (64, 64)):                                    # `down` on f16_check's 12 forced instantiations
    for _bk in (16, 32):
        _t = _bk * 1000000 + _bm * 1000 + _bn
        _f16(f"down-{_bm}x{_bn}-bk{_bk}-gather", "down", "T", 4, 72, _t, (_bm, _bn, _bk, GATHER))
        _f16(f"down-{_bm}x{_bn}-bk{_bk}-scalar", "down", "T", 32, 72, _t, (_bm, _bn, _bk, SCALAR), c1=32 if _bm == 128 and _bn == 128 else 0)
_f16("down-norm-gather", "down", "T", 12, 72, 32128064, (128, 64, 32, GATHER), precision=PREC_F16_EPI, norm=True)
_f16("down-norm-scalar", "down", "T", 32, 72, 16064064, (64, 64, 16, SCALAR), precision=PREC_F16_EPI, norm=True)
_f16("down-small", "down", "T", 32, 72, 32064064, (64, 64, 32, SCALAR), mag=1e-3)     # subnormal halves next to zero taps
_f16("model-fp16", "down", "M", 128, 128, 0, (64, 64, 32, SCALAR), shift=True)
F16_IDS = [c["name"] for c in F16]

# ---------------------------------------------------------------------------------------------------------------------------------
# split bf16: bf16_check's cases, plan = {precision number: (bm, bn, bk, patch)}; every case runs under all four precisions

BF16 = []


def _b16(name, geom, c0, cout, tile, plan, **extra):
    c = _base("bf16-" + name, geom, "T", c0, cout, 0, extra)
    c.update(tile=tile, plan=plan if isinstance(plan, dict) else {p: plan for p in (1, 2, 3, 4)})
    BF16.append(bc.register(c))


for _geom in ("down", "valid", "wide"):
    for _bm, _bn in ((64, 64), (128, 64), (128, 128)):
        _b16(f"{_geom}-{_bm}x{_bn}", _geom, 4, 72, 16000000 + _bm * 1000 + _bn, (_bm, _bn, 16, 0))
    _b16(f"{_geom}-bk32", _geom, 12, 72, 32128128, bc.BK32)                           # only bf16x3 has the BK = 32 tile
_b16("down-norm", "down", 8, 72, 16064064, (64, 64, 16, 0), norm=True)
BF16_IDS = [c["name"] for c in BF16]


def geom_cases():
    """[(arithmetic, case)] of every case: 'fp32', 'fp16', 'bf16'."""
    return [("fp32", c) for c in FP32] + [("fp16", c) for c in F16] + [("bf16", c) for c in BF16]


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp16 cases in fp32_check's layout

@functools.lru_cache(maxsize=None)
def _f16_by_name(name):
    c = F16[F16_IDS.index(name)]
    t = FC.inputs(c)
    x = t["x"] if t["x2"] is None else torch.cat([t["x"], t["x2"]], 3)
    t = dict(x=x, w=t["w"], scale=t["scale"], shift=t["shift"], addend=t["addend"], res=t["res"], nmean=None, nrstd=None)
    operand = x
    if c["extra"].get("norm"):                                           # statistics as fp32_check.inputs forms them
        f = x.reshape(c["B"], c["H"] * c["W"], x.shape[3])
        t["nmean"] = f.mean(1).contiguous()
        t["nrstd"] = (1.0 / torch.sqrt(f.var(1, unbiased=False) + fc.NORM_EPS)).contiguous()
        # what the kernel rounds to half is the float32 fmaxf((x - mean) * rstd, 0), restated bit for bit (test_gpu_encoder_norm_f16.py:
        # the staging code leaves nothing to contract), so the bound stays the derived one
        operand = fc.norm_on_load(x, t["nmean"], t["nrstd"])
    ref, bound = FC.reference(c, dict(t, x=operand, x2=None))
    return t, operand, ref, bound


def f16_tensors(c):
    """fp32_check.inputs' layout of f16_check.inputs(c) (x: both segments; nmean / nrstd for the norm cases)."""
    return _f16_by_name(c["name"])[0]


def f16_reference(c):
    """-> (ref, bound) of f16_check.reference, of the normalised operand for the norm cases."""
    return _f16_by_name(c["name"])[2:]


# ---------------------------------------------------------------------------------------------------------------------------------
# the convolution gathered tap by tap, with or without a simulated bug

BUGS = ("same_padding_assumed", "pads_swapped", "zero_tap_replicated", "right_tap_wraps_a_row", "bottom_tap_wraps_an_image",
        "rows_by_input_size", "padding_normalised")


def gather_conv(c, x, w, bug=None):
    """x NHWC [B,H,W,cin], w OIHW -> float64 [B,Hout,Wout,cout]: every output row m decomposed into (b, oy, ox), every tap's pixel
    looked up by its index, as igemm_kernel does it (conv.hip: a_iy0 / a_ix0 / the (unsigned) tests).  bug: one of BUGS (header)."""
    B, H, W, s, (kh, kw) = c["B"], c["H"], c["W"], c["stride"], w.shape[2:]
    (ph, pw), (Ho, Wo) = wc.geometry_of(c)
    if bug == "same_padding_assumed":
        ph, pw = kh // 2, kw // 2
    if bug == "pads_swapped":
        ph, pw = pw, ph
    m = torch.arange(B * Ho * Wo)
    hw, wrow = (H * W, W) if bug == "rows_by_input_size" else (Ho * Wo, Wo)
    b, rem = m // hw, m % hw
    oy, ox = rem // wrow, rem % wrow
    N = B * H * W
    flat = torch.cat([x.double().reshape(N, -1), torch.zeros((1, x.shape[3]), dtype=torch.float64)])
    acc = torch.zeros((m.numel(), w.shape[0]), dtype=torch.float64)
    for ky in range(kh):
        for kx in range(kw):
            iy, ix = oy * s - ph + ky, ox * s - pw + kx
            lin = (b * H + iy) * W + ix
            inside = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W) & (b < B)
            idx = torch.where(inside, lin, N)
            if bug == "zero_tap_replicated":
                idx = (b * H + iy.clamp(0, H - 1)) * W + ix.clamp(0, W - 1)
            if bug == "right_tap_wraps_a_row":                           # pixel (iy + 1, ix - Win) has the linear index of (iy, ix)
                idx = torch.where((ix >= W) & (iy >= 0) & (iy < H) & (lin < N), lin, idx)
            if bug == "bottom_tap_wraps_an_image":                       # row iy - Hin of image b + 1: the same linear index
                idx = torch.where((iy >= H) & (iy < 2 * H) & (ix >= 0) & (ix < W) & (b + 1 < B), lin, idx)
            acc += flat[idx] @ w[:, :, ky, kx].double().t()
    return acc.reshape(B, Ho, Wo, -1)


def bugs_for(c):
    """The simulated bugs that change case c's result, from its geometry alone (header)."""
    B, H, W, s, kh, kw = c["B"], c["H"], c["W"], c["stride"], c["kh"], c["kw"]
    (ph, pw), (Ho, Wo) = wc.geometry_of(c)
    below, right = (Ho - 1) * s - ph + kh - 1 >= H, (Wo - 1) * s - pw + kw - 1 >= W
    names = set()
    if (ph, pw) != (kh // 2, kw // 2):
        names.add("same_padding_assumed")
    if ph != pw:
        names.add("pads_swapped")
    if ph > 0 or pw > 0 or below or right:
        names.add("zero_tap_replicated")
        if c["extra"].get("norm"):
            names.add("padding_normalised")
    if right:
        names.add("right_tap_wraps_a_row")
    if below and B > 1:
        names.add("bottom_tap_wraps_an_image")
    if Wo != W or (Ho != H and B > 1):
        names.add("rows_by_input_size")
    return names


class Oracle:
    """One run's float64 side in one shape, whatever module holds it: `pairs` [(x piece, w piece)] whose convolutions sum to the
    accumulator, epilogue(acc) -> out, out, ratio(got) -> |error| over the bound's unit, K (the bound in that unit), violates(got),
    no_tap (the outputs with no tap inside the image)."""

    def violates(self, got):
        return not self.ratio(got) <= self.K


def oracle(arith, c, prec=None):
    """arith 'fp32' / 'fp16' / 'bf16' (prec: the precision number of a bf16 run)."""
    o = Oracle()
    o.c = c
    if arith == "fp16":
        t, operand, ref, bound = _f16_by_name(c["name"])
        assert t["scale"] is None and t["addend"] is None and t["res"] is None
        o.pairs, o.out, o.K = [(operand.half(), t["w"].half())], ref, 1.0
        sh = 0.0 if t["shift"] is None else t["shift"].double()
        o.epilogue = lambda acc: torch.relu(acc + sh) if c["extra"].get("act") == "relu" else acc + sh
        o.ratio = lambda got: FC.worst_ratio(got, ref, bound)
        o.operand, o.w, o.nmean, o.nrstd = t["x"], t["w"], t["nmean"], t["nrstd"]
        o.no_tap = wc.conv64_geometry(torch.ones_like(operand[..., :1]), torch.ones((1, 1, c["kh"], c["kw"])), c["stride"], *wc.geometry_of(c))[..., 0] == 0
        return o
    if arith == "fp32":
        r = fc.reference(c["name"])
        o.pairs, o.K = [(r.x, r.t["w"])], fc.K_FP32
        o.ratio = lambda got: fc.ratio(r, got)
    else:
        fam = bc.FAMILY[prec]
        r = bc.reference(c["name"], fam)
        o.pairs = [(r.xp[i], r.wp[j]) for i, j in bc.PRODUCTS[fam]] if fam == "x3" else [(r.x, r.t["w"])]
        o.K = bc.K_of(prec)
        o.ratio = lambda got: bc.ratio(r, got)
        o.violates = lambda got: bc.violates(r, got, o.K)
    o.r, o.out = r, r.out
    o.epilogue = lambda acc: r.epilogue(acc)[1]
    o.operand, o.w, o.nmean, o.nrstd = r.t["x"], r.t["w"], r.t["nmean"], r.t["nrstd"]
    o.no_tap = fc.conv(c, torch.ones_like(r.x[..., :1]), torch.ones((1, 1, c["kh"], c["kw"])))[..., 0] == 0
    if arith == "fp32":
        o.violates = lambda got: fc.violates(r, got)
        assert torch.equal(o.no_tap[..., None].expand_as(r.no_tap), r.no_tap)
    return o


def simulated_bugs(arith, c, prec=None):
    """{bug name: the float64 output} for every simulated bug that concerns case c."""
    o = oracle(arith, c, prec)
    out = {}
    for bug in sorted(bugs_for(c)):
        if bug == "padding_normalised":                                  # the geometry's own zeros, run through the norm on load
            xpad = wc.pad_nhwc(o.operand, wc.pad_amounts(c["H"], c["W"], c["kh"], c["kw"], c["stride"], *wc.geometry_of(c)))
            xn = fc.norm_on_load(xpad, o.nmean, o.nrstd)
            pairs = [(xn.half(), o.w.half())] if arith == "fp16" else [(xn, o.w)] if len(o.pairs) == 1 else \
                [(bc.pieces(xn, "x3")[i], bc.pieces(o.w, "x3")[j]) for i, j in bc.PRODUCTS["x3"]]
            acc = sum(wc.conv64_geometry(x, w, c["stride"], *wc.geometry_of(c), padded=True) for x, w in pairs)
        else:
            acc = sum(gather_conv(c, x, w, bug) for x, w in o.pairs)
        out[bug] = o.epilogue(acc)
    return out
