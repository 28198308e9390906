"""The geometries, the case table and the simulated bugs of geom_check.py, as far as the host can tell: every case reaches exactly the
plan it names and never the halo patch; the halo-patch schedule and the three Winograd routes refuse a descriptor off 'same' padding
(planned on the direct kernels' general / scalar schedules; a forced Winograd tile is OFX_EINVAL); a negative pad is OFX_EINVAL with
nothing written; the geometry reference equals what it restates; the table covers what it is there for; every simulated bug stands
outside the bound at every case it lists and changes nothing at the cases it does not.  CPU only; needs the built library
(ofx_conv2d_plan is pure: no device)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import bf16_check as bc
import f16_check as FC
import fp32_check as fc
import geom_check as gc
import wino_check as wc

PTR = 0x10000                       # non-null, 256-byte aligned, never dereferenced
EINVAL = -1
G, S, P = gc.GATHER, gc.SCALAR, gc.PATCH
TILE_WINOGRAD, TILE_WINOGRAD4 = 1, 2        # include/ofx.h
RUNS = [(a, c, p) for a, c in gc.geom_cases() for p in ((1, 2, 3, 4) if a == "bf16" else (None,))]
RUN_IDS = [c["name"] + ("" if p is None else f"-prec{p}") for a, c, p in RUNS]


def _plan(d):
    from sd_animation_optical_flow_amd import _lib
    p = _lib.ConvPlan()
    return _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 0, C.byref(p)), p


def _desc(arith, c, prec=None):
    return bc.descriptor(c, prec, lambda name: PTR) if arith == "bf16" else fc.descriptor(c, lambda name: PTR, PTR)


def _with(d, **kw):
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# plans

@pytest.mark.parametrize("arith,c,prec", RUNS, ids=RUN_IDS)
def test_every_case_reaches_the_plan_it_names_and_never_the_halo_patch(arith, c, prec):
    d = _desc(arith, c, prec)
    (ph, pw), (Ho, Wo) = wc.geometry_of(c)
    assert (d.padH, d.padW, d.Hout, d.Wout, d.stride, d.KH, d.KW) == (ph, pw, Ho, Wo, c["stride"], c["kh"], c["kw"])
    assert (ph, pw, Ho, Wo) != (c["kh"] // 2, c["kw"] // 2, c["H"], c["W"])                  # off 'same' geometry
    st, p = _plan(d)
    assert st == 0 and p.path == 0, (st, p.path)
    print(f"{c['name']}: {p.bm}x{p.bn} BK {p.bk} KS {p.ks} ksplit {p.ksplit} {fc.MODE_NAME[p.mode]}, {p.mtiles} x {p.ntiles} tiles")
    assert p.mode in (G, S)
    if arith == "fp32":
        assert p.prec == 0 and (p.bm, p.bn, p.bk, p.ks, p.ksplit, p.mode) == c["plan"]
        assert (p.bm, p.bn, p.bk, p.ks, p.ksplit > 1) == fc.row_key(c["row"])
    elif arith == "fp16":
        assert p.prec == FC.PREC_F16 and (p.bm, p.bn, p.bk, p.mode) == c["plan"] and p.ks == 1 and p.ksplit == 1
    else:
        assert p.prec == prec and (p.bm, p.bn, p.bk, p.mode) == c["plan"][prec] and p.ks == 1 and p.ksplit == 1
    assert p.mtiles == -(-c["B"] * Ho * Wo // p.bm) and p.ntiles == -(-c["cout"] // p.bn)
    if p.mode == S:
        assert (c["c0"] + c["c1"]) % p.bk == 0 and c["c0"] % p.bk == 0
    if c["extra"].get("ws"):
        assert p.ksplit > 1 and c["tile"] == 0 and 65536 + p.mtiles * p.ntiles * p.ksplit * 64 * 64 * 4 <= fc.WS_BYTES


def test_the_model_call_is_pinned():
    """The Downsample of the first-stage encoder at Cin = Cout = 128 on a 2x12x20 map, tile 0, a bias, no workspace: 120 rows in
    64x64 tiles, in fp32 with paired pipelines (a small grid, Kpad 1152), both on the scalar-coordinate schedule."""
    c32, c16 = gc.FP32[gc.FP32_IDS.index("g-model-fp32")], gc.F16[gc.F16_IDS.index("g-f16-model-fp16")]
    for c in (c32, c16):
        assert (c["tile"], c["c0"], c["c1"], c["cout"], (c["B"], c["H"], c["W"])) == (0, 128, 0, 128, (2, 12, 20))
        assert (c["kh"], c["kw"], c["stride"], c["pad"], c["out_hw"]) == (3, 3, 2, (0, 0), (6, 10))
        assert c["extra"] == dict(shift=True)
    st, p = _plan(_desc("fp32", c32))
    assert st == 0 and (p.path, p.prec, p.bm, p.bn, p.bk, p.ks, p.ksplit, p.mode, p.mtiles, p.ntiles) == (0, 0, 64, 64, 32, 2, 1, S, 2, 2)
    st, p = _plan(_desc("fp16", c16))
    assert st == 0 and (p.path, p.prec, p.bm, p.bn, p.bk, p.ks, p.ksplit, p.mode, p.mtiles, p.ntiles) == (0, 5, 64, 64, 32, 1, 1, S, 2, 2)


def _probe(geom, mp, c0, cout, tile, precision=0, **kw):
    """A descriptor outside the table: geometry `geom` (None: 'same' with the geometry's filter at stride 1) on map mp."""
    B, H, W = mp
    kh, kw_, stride, pad, ohw = gc.GEOMS[geom] if isinstance(geom, str) else geom
    c = dict(name="probe", B=B, H=H, W=W, c0=c0, c1=0, cout=cout, kh=kh, kw=kw_, stride=stride, pad=pad, out_hw=ohw(H, W), tile=tile,
             precision=precision, extra={})
    return _with(fc.descriptor(c, lambda name: PTR), **kw)


def _same(geom):
    kh, kw, *_ = gc.GEOMS[geom]
    return (kh, kw, 1, (kh // 2, kw // 2), lambda H, W: (H, W))


@pytest.mark.parametrize("geom", [g for g in gc.GEOMS if g != "ring-1x1"])
def test_no_geometry_is_ever_planned_on_the_halo_patch(geom):
    """On a map of whole patches with whole channel slabs, where the same filter with 'same' padding IS on the halo patch -- on the
    automatic plan and on a forced patch-capable tile, in fp32, fp16 and split bf16 -- the geometry is not: `asym-*` (one pad off),
    `crop` / `over` (only the size off) and the strided ones included."""
    for mp in ((2, 16, 16), (2, 8, 16), (64, 64, 96)):                    # (the automatic plan: a grid large enough for the patch tiles)
        for tile, precision in ((0, 0), (0, 5), (0, 1)) if mp[0] == 64 else ((16128064, 0), (16128128, 0), (16256064, 0), (32064064, 0), (128064, 5), (64064, 5), (16128064, 1), (16128128, 3)):
            st, p = _plan(_probe(_same(geom), mp, 64, 64, tile, precision))
            assert st == 0 and p.path == 0 and p.mode == P, (mp, tile, precision, p.mode)   # the control
            st, p = _plan(_probe(geom, mp, 64, 64, tile, precision))
            assert st == 0 and p.path == 0 and p.mode in (G, S), (geom, mp, tile, precision, p.mode)
            assert p.mode == (G if precision in (1, 3) else S)                               # (split bf16 has no scalar schedule)


@pytest.mark.parametrize("geom", [g for g in gc.GEOMS if gc.GEOMS[g][2] == 1 and g != "ring-1x1"])
def test_the_winograd_routes_refuse_a_geometry(geom):
    """With wino_w and wino4_w set, at a size where the 'same' layer takes a Winograd route (64 frames of 64x96, 128 -> 64 channels:
    on the F(4x4,3x3) grid gate; F(2x2,3x3) without its operand; F(4,5) for the 1-D filters), a geometry is planned on the direct
    kernels, and a tile that forces a route is OFX_EINVAL."""
    mp, one_d = (64, 64, 96), gc.GEOMS[geom][0] != gc.GEOMS[geom][1]
    ops = dict(wino_w=PTR, wino4_w=PTR)
    assert _plan(_probe(_same(geom), mp, 128, 64, 0, **ops))[1].path == (2 if one_d else 3)  # the controls
    assert _plan(_probe(_same(geom), mp, 128, 64, 0, wino_w=PTR))[1].path == (2 if one_d else 1)
    assert _plan(_probe(_same(geom), mp, 128, 64, TILE_WINOGRAD, **ops))[0] == 0
    for kw in (ops, dict(wino_w=PTR), dict(wino4_w=PTR)):
        st, p = _plan(_probe(geom, mp, 128, 64, 0, **kw))
        assert st == 0 and p.path == 0 and p.mode == S, (geom, kw, st, p.path, p.mode)
    for tile in (TILE_WINOGRAD, TILE_WINOGRAD4):
        assert _plan(_probe(geom, mp, 128, 64, tile, **ops))[0] == EINVAL, (geom, tile)


def test_a_negative_pad_is_rejected_with_nothing_written():
    """conv_validate: padH < 0 or padW < 0 is OFX_EINVAL from the plan query and from ofx_conv2d, before any launch (host buffers,
    a poisoned output); ops.conv2d_nhwc raises before the call."""
    from sd_animation_optical_flow_amd import _lib, ops
    POISON = 7.25
    x, w = torch.zeros((1, 8, 16, 32)), torch.zeros((64, 288))
    out = torch.full((1, 8, 16, 64), POISON)

    def desc(**kw):
        d = _lib.ConvDesc()
        d.in0, d.ld0, d.c0, d.w, d.out, d.ldo = x.data_ptr(), 32, 32, w.data_ptr(), out.data_ptr(), 64
        d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = 1, 8, 16, 8, 16, 64
        d.KH, d.KW, d.stride, d.padH, d.padW = 3, 3, 1, 1, 1
        return _with(d, **kw)

    assert _plan(desc())[0] == 0 and _plan(desc(padH=0, padW=0))[0] == 0
    for bad in (dict(padH=-1), dict(padW=-1), dict(padH=-1, padW=-1), dict(padH=-1, Hout=6), dict(padW=-2, precision=5), dict(padH=-1, precision=1)):
        assert _plan(desc(**bad))[0] == EINVAL, bad
        assert _lib.lib().ofx_conv2d(C.byref(desc(**bad)), None) == EINVAL, bad
    assert bool((out == POISON).all())
    for pad in ((-1, 0), (0, -1), (-1, -1)):
        with pytest.raises(RuntimeError, match="pad must be >= 0"):
            ops.conv2d_nhwc(x, w, 3, 3, 64, pad=pad, out=out)             # (before the tensors are looked at: no device needed)
    assert bool((out == POISON).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference

def test_the_geometry_reference_equals_what_it_restates():
    nchw = lambda a: a.double().permute(0, 3, 1, 2)
    # `down`: the reference's own F.pad(x, (0, 1, 0, 1)) + stride-2 convolution without padding, exactly
    for name in ("g-down-128x128-gather", "g-down-256x64-scalar", "g-model-fp32"):
        c, r = fc.case(name), fc.reference(name)
        want = F.conv2d(F.pad(nchw(r.x), (0, 1, 0, 1)), r.t["w"].double(), stride=2).permute(0, 2, 3, 1)
        assert torch.equal(r.acc, want) and tuple(r.acc.shape[1:3]) == (c["H"] // 2, c["W"] // 2)
    c = gc.F16[gc.F16_IDS.index("g-f16-down-64x64-bk32-scalar")]
    t = FC.inputs(c)
    want = F.conv2d(F.pad(nchw(t["x"].half()), (0, 1, 0, 1)), t["w"].half().double(), stride=2).permute(0, 2, 3, 1)
    assert torch.equal(gc.f16_reference(c)[0], want)
    r = bc.reference("g-bf16-down-64x64", "x6")
    assert torch.equal(r.acc, F.conv2d(F.pad(nchw(r.x), (0, 1, 0, 1)), r.t["w"].double(), stride=2).permute(0, 2, 3, 1))
    # default keys: the geometry path gives what the old `conv` of the three modules gives, strides and 1-D / 7x7 filters included
    for name in ("p-128x128-gather", "p-128x128-scalar-s2", "p-256x64-scalar-s2", "p-128x64-patch-5x1", "p-128x128-patch-seam-x2", "auto-1x1-s2",
                 "auto-stem-7x7-s2", "n-64x64k16-scalar"):
        c, r = fc.case(name), fc.reference(name)
        assert "pad" not in c and "out_hw" not in c
        assert wc.geometry_of(c) == ((c["kh"] // 2, c["kw"] // 2), tuple(r.acc.shape[1:3]))
        assert torch.equal(wc.conv64_geometry(r.x, r.t["w"], c["stride"], *wc.geometry_of(c)), r.acc), name
        explicit = dict(c, pad=fc.pad_of(c), out_hw=fc.out_hw(c))
        assert torch.equal(fc.conv(explicit, r.x, r.t["w"]), r.acc)
    for c in (bc.case("stride2-3x3-96"), bc.case("patch-1x5-128x128-x2")):
        r = bc.reference(c["name"], "x6")
        assert torch.equal(bc.conv(dict(c, pad=bc.pad_of(c), out_hw=bc.out_hw(c)), r.x, r.t["w"]), r.acc)
    for c in FC.CASES[:6]:
        t = FC.inputs(c)
        ref, bound = FC.reference(c, t)
        ref2, bound2 = FC.reference(dict(c, pad=FC.pad_of(c), out_hw=FC.out_hw(c)), t)
        assert torch.equal(ref, ref2) and torch.equal(bound, bound2), c["name"]


@pytest.mark.parametrize("arith,c", gc.geom_cases(), ids=[c["name"] for a, c in gc.geom_cases()])
def test_the_conditions_of_the_bound_hold_and_the_gathered_convolution_agrees(arith, c):
    """The oracles assert their conditions themselves (|shift| + |addend| + |res| <= the convolution's magnitude, unsaturated
    activations); here the reference is also held to the convolution gathered tap by tap, index by index, and the ring to its mask."""
    o = gc.oracle(arith, c, 3 if arith == "bf16" else None)
    (ph, pw), (Ho, Wo) = wc.geometry_of(c)
    assert tuple(o.out.shape) == (c["B"], Ho, Wo, c["cout"]) and o.out.dtype == torch.float64 and bool(torch.isfinite(o.out).all())
    again = o.epilogue(sum(gc.gather_conv(c, x, w) for x, w in o.pairs))
    scale = float(o.out.abs().max())
    assert float((again - o.out).abs().max()) <= 1e-13 * max(scale, 1.0)
    assert not o.violates(o.out.float())
    # the outputs with no tap inside the image: the ring geometries' frame, and nowhere else
    yy, xx = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    s, kh, kw = c["stride"], c["kh"], c["kw"]
    none = (yy * s - ph + kh - 1 < 0) | (yy * s - ph >= c["H"]) | (xx * s - pw + kw - 1 < 0) | (xx * s - pw >= c["W"])
    assert torch.equal(o.no_tap, none[None].expand(c["B"], Ho, Wo))
    assert bool(none.any()) == (c["geom"] in gc.RINGS + ("over",))       # (`over`: the rows and columns beyond the natural output, too)
    assert (c["geom"] in gc.RINGS) == bool(c["extra"].get("exact_zero"))
    assert float(o.out[o.no_tap].abs().max() if c["geom"] == "over" else 0.0) == 0.0         # no epilogue operand there: exact zeros
    if c["geom"] in gc.RINGS:
        assert c["extra"] == gc.RING_EXTRA                               # a shift and ReLU and nothing else
        shift = (gc.f16_tensors(c) if arith == "fp16" else o.r.t)["shift"]
        assert torch.equal(o.out[o.no_tap], torch.relu(shift.double())[None, None, None].expand_as(o.out)[o.no_tap])
        assert int(none.sum()) == 2 * (Ho + Wo) - 4 and bool((shift > 0).any()) and bool((shift < 0).any())   # a frame one output wide


# ---------------------------------------------------------------------------------------------------------------------------------
# coverage

def _has_scalar(row):
    return fc.row_key(row)[1] != 192                                     # tile_has_scalar of conv.hip at PREC 0 (test_fp32_check_host.py)


def coverage_gaps(fp32, f16, bf16):
    """What the tables miss of the minimum the header of geom_check.py promises: a list of sentences, empty when nothing is missing."""
    gaps = []
    mode = lambda c: c["plan"][5] if len(c["plan"]) == 6 else c["plan"][3]
    plain = lambda c: not any(c["extra"].get(k) for k in ("norm", "ldo", "res", "scale", "addend", "mag", "act")) and c["c1"] in (0, 32 if len(c["plan"]) == 4 else 0)
    # fp32: every geometry on both schedules; two segments for down / valid / wide
    for geom in gc.GEOMS:
        for m in (G, S):
            if not any(c["geom"] == geom and mode(c) == m and c["c1"] == 0 and not any(c["extra"].get(k) for k in ("norm", "ldo", "res", "scale", "addend")) for c in fp32):
                gaps.append(f"fp32: no {geom} case on {fc.MODE_NAME[m]}")
            if not any(c["geom"] == geom and mode(c) == m and c["plan"][:3] == (64, 64, 32) for c in f16):
                gaps.append(f"fp16: no {geom} case on {fc.MODE_NAME[m]} of the 64x64 BK 32 tile")
    for geom in ("down", "valid", "wide"):
        if not any(c["geom"] == geom and c["c0"] == c["c1"] == 32 and mode(c) == S for c in fp32):
            gaps.append(f"fp32: no two-segment {geom} case")
    for mp in ("T", "R"):                                                # valid-s2: with the last input row and column unused, and read
        for m in (G, S):
            if not any(c["geom"] == "valid-s2" and c["map"] == mp and mode(c) == m for c in fp32):
                gaps.append(f"fp32: no valid-s2 case on map {mp} on {fc.MODE_NAME[m]}")
    # fp32: `down` on every row, on each of gather / scalar the row has, with no feature but the geometry
    for row in fc.ROWS:
        for m in (G, S) if _has_scalar(row) else (G,):
            if not any(c["geom"] == "down" and c["row"] == row and mode(c) == m and plain(c) and c["map"] != "M" for c in fp32):
                gaps.append(f"fp32: no down case on {row} {fc.MODE_NAME[m]}")
    down = [c for c in fp32 if c["geom"] == "down"]
    for m in (G, S):
        if not any(c["extra"].get("norm") and mode(c) == m for c in down):
            gaps.append(f"fp32: no down case with the norm on load on {fc.MODE_NAME[m]}")
    for what, ok in (("split-K on the 64x64 split row at Cout 120", lambda c: c["plan"][4] > 1 and c["cout"] == 120 and c["extra"].get("ws")),
                     ("paired pipelines", lambda c: c["plan"][3] == 2),
                     ("an out-slice", lambda c: fc.ldo_of(c) > c["cout"] and fc.out_off_of(c) > 0),
                     ("tanh", lambda c: c["extra"].get("act") == "tanh"),
                     ("the model's call", lambda c: c["map"] == "M" and c["tile"] == 0 and (c["c0"], c["cout"]) == (128, 128))):
        if not any(ok(c) for c in down):
            gaps.append(f"fp32: no down case with {what}")
    # fp16: `down` on the 12 forced instantiations, the norm on load through fp16_epi, subnormal halves, the model's call
    d16 = [c for c in f16 if c["geom"] == "down"]
    for bm, bn in ((128, 128), (128, 64), (64, 64)):
        for bk in (16, 32):
            for m in (G, S):
                if not any(c["plan"] == (bm, bn, bk, m) and c["tile"] == bk * 1000000 + bm * 1000 + bn and plain(c) for c in d16):
                    gaps.append(f"fp16: no down case on {bm}x{bn} BK {bk} {fc.MODE_NAME[m]}")
    for what, ok in (("the norm on load through fp16_epi", lambda c: c["extra"].get("norm") and c["precision"] == gc.PREC_F16_EPI),
                     ("mag = 1e-3", lambda c: c["extra"].get("mag") == 1e-3),
                     ("the model's call", lambda c: c["map"] == "M" and c["tile"] == 0 and (c["c0"], c["cout"]) == (128, 128) and c["precision"] == 5)):
        if not any(ok(c) for c in d16):
            gaps.append(f"fp16: no down case with {what}")
    # split bf16: down / valid / wide on the three tiles and on the forced bf16x3 BK 32 tile, gather, under all four precisions; a norm
    for geom in ("down", "valid", "wide"):
        for key in ((64, 64, 16, 0), (128, 64, 16, 0), (128, 128, 16, 0)):
            if not any(c["geom"] == geom and all(c["plan"][p] == key for p in (1, 2, 3, 4)) and not c["extra"] for c in bf16):
                gaps.append(f"bf16: no {geom} case on {key[0]}x{key[1]}")
        if not any(c["geom"] == geom and c["plan"] == bc.BK32 and c["tile"] == 32128128 for c in bf16):
            gaps.append(f"bf16: no {geom} case on the bf16x3 BK 32 tile")
    if not any(c["extra"].get("norm") for c in bf16):
        gaps.append("bf16: no norm-on-load case")
    return gaps


def test_the_tables_cover_what_they_are_there_for():
    assert coverage_gaps(gc.FP32, gc.F16, gc.BF16) == []
    assert len(fc.ROWS) == 12 and sum(_has_scalar(r) for r in fc.ROWS) == 11
    # maps: the issue's T, two images; each geometry on a map where every distinguishing tap exists (T, but for the R twin of valid-s2)
    assert gc.MAPS["T"] == (2, 10, 14) and {c["map"] for a, c in gc.geom_cases()} == {"T", "R", "D", "M"}
    for a, c in gc.geom_cases():
        (ph, pw), (Ho, Wo) = wc.geometry_of(c)
        assert min(Ho, Wo) >= 1 and c["B"] * Ho * Wo <= 512 and c["c0"] + c["c1"] <= 128   # a few hundred rows at the most
    c = fc.case("g-valid-s2-gather")                                     # on T the last input row and column are unused, on R they are read
    assert (fc.out_hw(c)[0] - 1) * 2 + 2 == c["H"] - 2 and (fc.out_hw(c)[1] - 1) * 2 + 2 == c["W"] - 2
    c = fc.case("g-valid-s2-R-gather")
    assert (fc.out_hw(c)[0] - 1) * 2 + 2 == c["H"] - 1 and (fc.out_hw(c)[1] - 1) * 2 + 2 == c["W"] - 1
    assert fc.ldadd_of(fc.case("g-valid-addend-shift")) > fc.case("g-valid-addend-shift")["cout"]
    # the registry left the three modules' own tables alone
    assert len(fc.CASES) == 94 and len(bc.CASES) == 32 and len(FC.CASES) == 24 and not set(fc.OTHER) & set(fc.IDS)


def _without(cases, name):
    rest = [c for c in cases if c["name"] != name]
    assert len(rest) == len(cases) - 1, name
    return rest


def test_removing_a_single_cover_is_noticed():
    """The coverage is a property of the tables, not of their length: without any single `down` row-by-schedule case, or any
    geometry's only gather or scalar case, coverage_gaps says what is missing."""
    only = []
    for row in fc.ROWS:
        for m in ("gather", "scalar") if _has_scalar(row) else ("gather",):
            only.append((f"g-down-{row}-{m}", f"fp32: no down case on {row} {m}"))
    for geom in gc.GEOMS:
        if geom != "down":
            only += [(f"g-{geom}-gather", f"fp32: no {geom} case on gather"), (f"g-{geom}-scalar", f"fp32: no {geom} case on scalar")]
    assert len(only) == 23 + 22
    for name, gap in only:
        gaps = coverage_gaps(_without(gc.FP32, name), gc.F16, gc.BF16)
        assert gaps == [gap.replace("valid-s2 case", "valid-s2 case on map T")], name   # (valid-s2's twin on R keeps the schedule: the map goes)
    for name in ("g-valid-s2-R-gather", "g-valid-s2-R-scalar", "g-down-x2", "g-valid-x2", "g-wide-x2", "g-down-norm-gather", "g-down-norm-scalar",
                 "g-down-slice", "g-down-tanh", "g-model-fp32"):
        assert len(coverage_gaps(_without(gc.FP32, name), gc.F16, gc.BF16)) == 1, name
    for c in gc.F16:                                                     # (the norm on load has a case per schedule where one is asked for)
        if not c["extra"].get("norm"):
            assert len(coverage_gaps(gc.FP32, _without(gc.F16, c["name"]), gc.BF16)) >= 1, c["name"]
    for c in gc.BF16:
        assert len(coverage_gaps(gc.FP32, gc.F16, _without(gc.BF16, c["name"]))) == 1, c["name"]


# ---------------------------------------------------------------------------------------------------------------------------------
# simulated bugs

_margins = {}


@pytest.mark.parametrize("arith,c,prec", RUNS, ids=RUN_IDS)
def test_every_simulated_bug_is_outside_the_bound_where_it_is_listed_and_changes_nothing_elsewhere(arith, c, prec):
    o = gc.oracle(arith, c, prec)
    bugs = gc.simulated_bugs(arith, c, prec)
    assert set(bugs) == gc.bugs_for(c) and bugs
    ratios = {k: o.ratio(v) for k, v in bugs.items()}
    _margins[(c["name"], prec)] = ratios
    print(f"{c['name']}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f" against {o.K}")
    missed = [k for k, v in bugs.items() if not o.violates(v)]
    assert not missed, missed
    if prec in (None, 3):                                                # a bug that is not listed is the convolution itself, bit for bit
        right = [gc.gather_conv(c, x, w) for x, w in o.pairs]
        for bug in set(gc.BUGS) - gc.bugs_for(c) - {"padding_normalised"}:
            assert all(torch.equal(gc.gather_conv(c, x, w, bug), y) for (x, w), y in zip(o.pairs, right)), bug


def test_where_every_simulated_bug_is_listed_and_the_narrowest_margin():
    runs = gc.geom_cases()
    count = {b: sum(b in gc.bugs_for(c) for a, c in runs) for b in gc.BUGS}
    print(count)
    assert all(v >= 2 for v in count.values()), count
    by_geom = {g: set().union(*(gc.bugs_for(c) for a, c in runs if c["geom"] == g and c["B"] > 1)) - {"padding_normalised"} for g in gc.GEOMS}
    every = {"same_padding_assumed", "zero_tap_replicated", "right_tap_wraps_a_row", "bottom_tap_wraps_an_image", "rows_by_input_size"}
    assert by_geom["down"] == every and by_geom["wide"] == every and by_geom["ring"] == every and by_geom["ring-1x1"] == every
    assert by_geom["valid"] == by_geom["valid-s2"] == by_geom["valid-1x5"] == by_geom["valid-5x1"] == {"same_padding_assumed", "rows_by_input_size"}
    side = {"same_padding_assumed", "pads_swapped", "zero_tap_replicated", "rows_by_input_size"}
    assert by_geom["asym-h"] == side | {"bottom_tap_wraps_an_image"}     # pad (1, 0), out (H, W-2): zeros above and below, none beside
    assert by_geom["asym-w"] == side | {"right_tap_wraps_a_row"}
    assert by_geom["crop"] == {"zero_tap_replicated", "rows_by_input_size"}
    assert by_geom["over"] == {"zero_tap_replicated", "right_tap_wraps_a_row", "bottom_tap_wraps_an_image", "rows_by_input_size"}
    assert "padding_normalised" in gc.bugs_for(fc.case("g-down-norm-gather")) and "padding_normalised" in gc.bugs_for(bc.case("g-bf16-down-norm"))
    assert "bottom_tap_wraps_an_image" not in gc.bugs_for(fc.case("g-valid-s2-R-gather"))    # one image: nothing to wrap into
    worst = None
    for arith, c in runs:
        for prec in ((1, 3) if arith == "bf16" else (None,)):
            o = gc.oracle(arith, c, prec)
            for k, v in gc.simulated_bugs(arith, c, prec).items():
                m = o.ratio(v) / o.K
                if worst is None or m < worst[0]:
                    worst = (m, k, c["name"], prec)
    print(f"narrowest margin: {worst[1]} at {worst[2]} (precision {worst[3]}) stands at {worst[0]:.4g} times its bound")
    assert worst[0] > 100
