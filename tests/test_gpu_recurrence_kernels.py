"""The hand-written kernels of the RAFT iteration other than the convolutions, against float64: the flow head (flow_head.hip through
ofx_flow_head, and the generic OFX_EPI_FLOW epilogue of ofx_conv2d), the 4-level radius-4 correlation lookup (the blocked kernel of
corr.hip) and the convex upsample (upsample_inl.h, through ofx_upsample_flow and ofx_upsample_flow_warp).

Every reference is float64 from the exact fp32 inputs the kernel was given, checked elementwise with the operand-scaled bound of
recurrence_check.py; what the kernels must write bit for bit, and what they must leave alone (sentinels in every unwritten slot and
in guard floats behind every buffer), is checked exactly.  The case lists are fixed, and CPU tests assert what they cover with the
kernels' own formulas (launch branch, strip and block residues, window overlaps).  The CPU tests of the checker show that it
catches the kernel bugs it is meant to catch.
"""
import ctypes as C

import pytest
import torch

import recurrence_check as rc
import wino_check as wc

SENT = 0x7FC0FFEE                    # a quiet NaN with a payload: kept bit for bit wherever nothing may be written
GUARD = 64                           # floats behind every output buffer

# worst ratios seen by this module's GPU tests, per kernel (read by hand when the K in recurrence_check.py are re-measured)
MEASURED = {}


def _note(kernel, ratio):
    MEASURED[kernel] = max(MEASURED.get(kernel, 0.0), ratio)
    print(f"MEASURED {kernel} {MEASURED[kernel]:.4g}")


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def _sentinel(n):
    return torch.full((n,), SENT, dtype=torch.int32).view(torch.float32)


def _guarded(t):
    """A device copy of t followed by GUARD sentinel floats: (flat buffer, the view shaped like t)."""
    buf = _sentinel(t.numel() + GUARD)
    buf[:t.numel()] = t.reshape(-1)
    buf = buf.cuda()
    return buf, buf[:t.numel()].view(t.shape)


def _guard_intact(buf, what):
    assert rc.same_bits(buf[-GUARD:].cpu(), _sentinel(GUARD)), f"{what}: write past the end of the buffer"


# ---------------------------------------------------------------------------------------------------------------------------------
# flow head cases: (B, h, w, ldx, layout, coordinate offset).  layout 'engine' = hx rows of 384 with the flow at 254 (raft_engine.cpp),
# 'flow' = a bare [M, 2] flow array.  Channels of x past 256 hold NaN.
FH_CASES = [
    (1, 1, 1, 256, "engine", 0.0),
    (3, 1, 5, 384, "flow", 0.0),
    (2, 3, 1, 256, "engine", 0.0),
    (1, 2, 2, 256, "flow", 0.0),
    (4, 6, 3, 384, "engine", 1000.0),
    (2, 7, 13, 256, "engine", 0.0),
    (3, 9, 12, 384, "flow", -700.0),
    (2, 16, 20, 256, "engine", 0.0),
    (1, 13, 30, 256, "engine", 0.0),
    (5, 5, 14, 384, "engine", 0.0),
    (1024, 1, 1, 256, "flow", 0.0),             # 1024 strips: the last one-wave launch
    (1025, 1, 1, 256, "flow", 0.0),             # 1025: the first four-wave launch
    (7, 61, 75, 384, "engine", 0.0),
    (6, 64, 96, 256, "engine", 300.0),
    (16384, 1, 1, 256, "engine", 0.0),          # the last launch without grid stride
    (16385, 1, 1, 384, "flow", 0.0),            # the first with it
    (40000, 1, 1, 256, "flow", 0.0),            # two or three strips per wave
    (17000, 2, 3, 384, "engine", 0.0),          # grid stride over 2 x 3 maps: strip rows end inside the next image
    (30, 31, 71, 256, "engine", 0.0),
]
# ofx_conv2d's OFX_EPI_FLOW on the same inputs: one grid of a handful of tiles, one that fills the chip
FLOW_CONV_CASES = [(2, 7, 13, 256, "engine", 0.0), (6, 64, 96, 384, "engine", 300.0)]


def _flow_head_inputs(case, seed):
    B, h, w, ldx, layout, off = case
    g = torch.Generator().manual_seed(seed)
    x = _sentinel(B * h * w * ldx).view(B, h, w, ldx)
    x[..., :256] = torch.relu(torch.randn((B, h, w, 256), generator=g))             # fh1's output is ReLU'd
    wt = torch.randn((2, 256, 3, 3), generator=g) * 0.03
    bias = torch.randn(2, generator=g)
    coords = rc.grid32(B, h, w) + torch.randn((B, h, w, 2), generator=g) * 4.0 + off
    ldh, flow_off = (384, 254) if layout == "engine" else (2, 0)
    hx = _sentinel(B * h * w * ldh).view(B, h, w, ldh)
    frows = _sentinel(B * h * w * 16).view(B, h, w, 16)
    return x, wt, bias, coords, hx, flow_off, frows


def _run_flow_head(case, seed):
    ops = _ops()
    x, wt, bias, coords, hx, flow_off, frows = _flow_head_inputs(case, seed)
    xd = x.cuda()
    cb, cd = _guarded(coords)
    hb, hd = _guarded(hx)
    fb, fd = _guarded(frows)
    ops.flow_head(xd, ops.pack_conv_weight(wt).cuda(), bias.cuda(), cd, hd, fd, flow_off)
    torch.cuda.synchronize()
    for buf, what in ((cb, "coords1"), (hb, "hx"), (fb, "frows")):
        _guard_intact(buf, f"{case} {what}")
    assert rc.same_bits(xd.cpu(), x)
    return (x, wt, bias, coords, hx, flow_off, frows), (cd.cpu(), hd.cpu(), fd.cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("case", FH_CASES, ids=lambda c: "x".join(map(str, c[:3])) + f"-ld{c[3]}-{c[4]}")
def test_flow_head_against_float64(cuda, case):
    (x, wt, bias, coords, hx, flow_off, frows), (c1, hx_out, fr_out) = _run_flow_head(case, 11)
    ref, mag = rc.flow_head_reference(x, wt, bias, coords)
    _note("flow_head", rc.check_coords(c1, ref, mag, rc.K_FLOW_HEAD, f"flow head {case}"))
    rc.check_flow_contract(c1, hx_out, flow_off, fr_out, hx, frows, f"flow head {case}")


def _conv_flow(x, wt, bias, coords, hx, flow_off):
    """The same update through ofx_conv2d(OFX_EPI_FLOW): (coords1, hx, flow4) on the host, guards checked."""
    from sd_animation_optical_flow_amd import _lib
    ops = _ops()
    B, h, w, ldx = x.shape
    xd = x.cuda()
    wp = ops.pack_conv_weight(wt).cuda()
    bd = bias.cuda()
    cb, cd = _guarded(coords)
    hb, hd = _guarded(hx)
    f4b, f4d = _guarded(_sentinel(B * h * w * 4).view(B, h, w, 4))
    d = _lib.ConvDesc()
    d.in0, d.ld0, d.c0 = xd.data_ptr(), ldx, 256
    d.w, d.shift = wp.data_ptr(), bd.data_ptr()
    d.aux_coords, d.aux_h, d.ldh, d.aux_flow4 = cd.data_ptr(), hd.data_ptr() + 4 * flow_off, hd.shape[-1], f4d.data_ptr()
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, h, w, h, w, 2
    d.KH, d.KW, d.stride, d.padH, d.padW = 3, 3, 1, 1, 1
    d.act, d.epi = 0, ops.EPI_FLOW
    ops.conv2d_desc(d)
    torch.cuda.synchronize()
    for buf, what in ((cb, "coords1"), (hb, "hx"), (f4b, "flow4")):
        _guard_intact(buf, f"EPI_FLOW {what}")
    return cd.cpu(), hd.cpu(), f4d.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", FLOW_CONV_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_conv2d_flow_epilogue_against_float64_and_the_flow_head(cuda, case):
    (x, wt, bias, coords, hx, flow_off, frows), (c1_fh, _, _) = _run_flow_head(case, 12)
    c1, hx_out, f4 = _conv_flow(x, wt, bias, coords, hx, flow_off)
    ref, mag = rc.flow_head_reference(x, wt, bias, coords)
    _note("epi_flow", rc.check_coords(c1, ref, mag, rc.K_FLOW_CONV, f"EPI_FLOW {case}"))
    flow = c1 - rc.grid32(*c1.shape[:3])
    assert rc.same_bits(hx_out[..., flow_off:flow_off + 2], flow)
    other = torch.ones(hx.shape[-1], dtype=torch.bool)
    other[flow_off:flow_off + 2] = False
    assert rc.same_bits(hx_out[..., other], hx[..., other])
    assert rc.same_bits(f4[..., :2], flow), "flow4 slots 0, 1 = the flow"
    assert rc.same_bits(f4[..., 2:], _sentinel(f4[..., 2:].numel()).view(f4[..., 2:].shape)), "flow4 slots 2, 3 written"
    # the two kernels agree within the sum of their bounds (two roundings of the coordinate)
    wc.check(c1, c1_fh.double(), mag, rc.K_FLOW_HEAD + rc.K_FLOW_CONV, f"EPI_FLOW vs flow head {case}", extra=2 * rc.half_ulp32(ref))


# ---------------------------------------------------------------------------------------------------------------------------------
# lookup: maps (B, h, w) whose levels end in partial blocks, with a level 3 of 1x1 / 1xn / 2x8, and M % 4 != 0
LOOKUP_MAPS = [(1, 13, 11), (2, 9, 29), (1, 23, 70)]
LOOKUP_LDO = 331                     # > 324: columns 324..330 are guards
SPECIAL = [1e7 - 1, -(1e7 - 1), 1e7, -1e7, 1e8, -1e8, -0.0]


def lookup_coords(h, w):
    """Coordinates (x, y) placed on the lookup's edges, level by level (fp32-exact values)."""
    out = []
    fracs = (0.0, 0.25, 0.5, 0.8125)
    for l in range(rc.LEVELS):
        s = float(2 ** l)
        hl, wl = h >> l, w >> l
        # windows starting at every residue of x mod 8 and y mod 4 (the 4 x 8 blocks), over the map and straddling its edges
        for rx in range(8):
            for ry in range(4):
                kx = (rx + ry + l) % (-(-wl // 8) + 1) - 1
                ky = (rx + 2 * ry + l) % (-(-hl // 4) + 1) - 1
                fx, fy = fracs[(rx + ry) % 4], fracs[(rx * 3 + ry + l) % 4]
                out.append(((8 * kx + rx + rc.RADIUS + fx) * s, (4 * ky + ry + rc.RADIUS + fy) * s))
        # windows that overlap the map by exactly one tap or by none, on each side and at the corners
        lo = (-4.0, -4.5, -5.0, -5.5)                        # one, one, none, none
        hx_, hy_ = (wl + 3.0, wl + 3.5, wl + 4.0, wl + 4.5), (hl + 3.0, hl + 3.5, hl + 4.0, hl + 4.5)
        cx, cy = wl / 2.0, hl / 2.0
        for v in lo:
            out += [(v * s, cy * s), (cx * s, v * s), (v * s, v * s)]
        for vx, vy in zip(hx_, hy_):
            out += [(vx * s, cy * s), (cx * s, vy * s), (vx * s, vy * s)]
        out += [(lo[1] * s, hy_[1] * s), (hx_[0] * s, lo[0] * s)]
    # odd integers (integers at level 0 only), multiples of 8 (integers at every level), half-integers
    for k in range(-3, max(h, w) + 3, 2):
        out += [(float(k), float(k % (h + 2))), (float(k % (w + 2)), float(k))]
    for k in range(-8, max(h, w) + 9, 8):
        out += [(float(k), float(abs(k) % (h + 1))), (float(k) + 0.5, float(k) - 0.5)]
    # the sanity cut-off |c / 2^l| < 1e7 and the signed zero
    for v in SPECIAL:
        out += [(v, h / 3.0), (w / 3.0, v), (v, v)]
    out.append((-0.0, -0.0))
    return torch.tensor(out, dtype=torch.float32)


def _lookup(pyr, coords, B, h, w, ldo):
    from sd_animation_optical_flow_amd import _lib
    M = B * h * w
    ob, od = _guarded(_sentinel(M * ldo).view(M, ldo))
    cd = coords.cuda()
    arr = (C.c_void_p * 4)(*[p.data_ptr() for p in pyr])
    _lib.check(_lib.lib().ofx_corr_lookup(arr, C.c_void_p(cd.data_ptr()), C.c_void_p(od.data_ptr()), ldo, B, h, w, 4, 4,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ofx_corr_lookup")
    torch.cuda.synchronize()
    _guard_intact(ob, "lookup out")
    out = od.cpu()
    assert rc.same_bits(out[:, 324:], _sentinel(M * (ldo - 324)).view(M, ldo - 324)), "lookup wrote past column 324"
    return out[:, :324]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LOOKUP_MAPS, ids=lambda s: "x".join(map(str, s)))
def test_corr_lookup_edges_against_float64(cuda, shape):
    ops = _ops()
    B, h, w = shape
    M = B * h * w
    g = torch.Generator().manual_seed(21)
    f1 = torch.randn((B, h, w, 256), generator=g)
    f2 = torch.randn((B, h, w, 256), generator=g)
    pyr = ops.corr_volume(f1.cuda(), f2.cuda())
    flat = [ops.corr_unblock(p, h >> l, w >> l).cpu() for l, p in enumerate(pyr)]
    pts = lookup_coords(h, w)
    nchunk = -(-len(pts) // M)
    fill = rc.grid32(B, h, w).reshape(-1, 2) + (torch.rand((M, 2), generator=g) - 0.5) * 9.0
    for i in range(nchunk):
        coords = fill.clone()
        part = pts[i * M:(i + 1) * M]
        coords[:len(part)] = part
        out = _lookup(pyr, coords.contiguous(), B, h, w, LOOKUP_LDO)
        ref, mag, extra = rc.lookup_reference(flat, coords, B, h, w)
        _note("lookup", wc.check(out, ref, mag, rc.K_LOOKUP, f"lookup {shape} chunk {i}", extra=extra))
    # and the ops wrapper (ldo = 324) on the random fill
    out = ops.corr_lookup(pyr, fill.reshape(B, h, w, 2).cuda(), B, h, w).cpu().reshape(M, 324)
    ref, mag, extra = rc.lookup_reference(flat, fill, B, h, w)
    _note("lookup", wc.check(out, ref, mag, rc.K_LOOKUP, f"lookup {shape} via ops", extra=extra))


# ---------------------------------------------------------------------------------------------------------------------------------
# convex upsample
UP_SHAPES = [(1, 1, 1), (2, 1, 2), (1, 3, 3), (3, 2, 5), (2, 5, 6), (1, 4, 7), (2, 7, 9), (3, 6, 8)]
UP_LOGITS = ["random", "dominant", "equal"]
UP_COORDS = ["near", "far"]


def upsample_inputs(shape, logits, coords, seed):
    B, h, w = shape
    g = torch.Generator().manual_seed(seed)
    if logits == "random":
        mask = torch.randn((B, h, w, 576), generator=g) * 3.0
    elif logits == "dominant":                           # per sub-pixel one tap at +80, the others at -80 (exp underflows)
        mask = torch.full((B, h, w, 9, 64), -80.0)
        k = torch.randint(0, 9, (B, h, w, 1, 64), generator=g)
        mask.scatter_(3, k, 80.0)
        mask = mask.reshape(B, h, w, 576)
    else:
        mask = torch.full((B, h, w, 576), 1.75)
    c = rc.grid32(B, h, w) + (torch.rand((B, h, w, 2), generator=g) - 0.5) * 12.0
    if coords == "far":                                  # |c| ~ 1e3: c - x rounds, and 8 (c - x) carries it
        c = c + torch.where(torch.rand((B, h, w, 2), generator=g) < 0.5, -1000.0, 1000.0)
    return c.contiguous(), mask.contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_against_float64_and_the_fused_warp(cuda, shape):
    ops = _ops()
    B, h, w = shape
    for li, logits in enumerate(UP_LOGITS):
        for ci, cs in enumerate(UP_COORDS):
            c, m = upsample_inputs(shape, logits, cs, 100 + 10 * li + ci)
            cd, md = c.cuda(), m.cuda()
            ob, od = _guarded(_sentinel(B * 64 * h * w * 2).view(B, 8 * h, 8 * w, 2))
            from sd_animation_optical_flow_amd import _lib
            _lib.check(_lib.lib().ofx_upsample_flow(C.c_void_p(cd.data_ptr()), C.c_void_p(md.data_ptr()), C.c_void_p(od.data_ptr()),
                                                    B, h, w, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ofx_upsample_flow")
            torch.cuda.synchronize()
            _guard_intact(ob, "flow_up")
            out = od.cpu()
            ref, mag = rc.upsample_reference(c, m)
            _note("upsample", wc.check(out, ref, mag, rc.K_UPSAMPLE, f"upsample {shape} {logits} {cs}"))
            frame = torch.randint(0, 256, (8 * h, 8 * w, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
            fl, _ = ops.upsample_flow_warp(cd, md, frame)
            assert rc.same_bits(fl.cpu(), out), f"{shape} {logits} {cs}: fused upsample + warp flow differs"


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the checker catches each simulated kernel bug; the case lists cover what they claim

def _fh_small(seed=3, off=1000.0):
    case = (2, 5, 11, 256, "engine", off)
    x, wt, bias, coords, hx, flow_off, frows = _flow_head_inputs(case, seed)
    return x, wt, bias, coords


def _flagged(out, ref, mag, K, extra=0.0):
    return bool(wc.violations(out, ref, mag, K, extra=extra).any())


def test_flow_head_checker_catches_simulated_bugs():
    x, wt, bias, coords = _fh_small()
    ref, mag = rc.flow_head_reference(x, wt, bias, coords)
    extra = rc.half_ulp32(ref)
    K = rc.K_FLOW_HEAD
    # a correct fp32 kernel: delta rounded once, then the coordinate add rounded once -- passes
    xn = x[..., :256].permute(0, 3, 1, 2)
    conv = wc.conv64(xn, wt, 3, 3).permute(0, 2, 3, 1)
    delta32 = (conv + bias.double()).float()
    good = coords + delta32
    assert not _flagged(good, ref, mag, K, extra)
    # the bias added after the coordinate: (coords1 + conv) + bias rounds twice at the coordinate's magnitude
    assert _flagged((coords + conv.float()) + bias, ref, mag, K, extra)
    # a dropped tap
    w_drop = wt.clone()
    w_drop[:, :, 0, 2] = 0
    ref_drop, _ = rc.flow_head_reference(x, w_drop, bias, coords)
    assert _flagged(ref_drop, ref, mag, K, extra)
    # the last, partial strip row (h = 5: row 4) skipped
    skip = ref.clone()
    skip[:, 4:] = coords[:, 4:].double()
    assert _flagged(skip, ref, mag, K, extra)
    # frows with the slots mirrored (3 + d instead of 3 - d)
    B, h, w, _ = x.shape
    hx = _sentinel(B * h * w * 384).view(B, h, w, 384)
    fr0 = _sentinel(B * h * w * 16).view(B, h, w, 16)
    hx_out = hx.clone()
    flow = good - rc.grid32(B, h, w)
    hx_out[..., 254:256] = flow
    fr_ok = rc.frows_expected(flow, fr0)
    rc.check_flow_contract(good, hx_out, 254, fr_ok, hx, fr0, "correct")
    fr_bad = fr0.clone()
    for s in range(7):
        d = s - 3
        lo, hi = max(0, -d), min(w, w - d)
        fr_bad[:, :, lo:hi, 2 * (6 - s):2 * (6 - s) + 2] = flow[:, :, lo + d:hi + d]
    with pytest.raises(AssertionError, match="frows"):
        rc.check_flow_contract(good, hx_out, 254, fr_bad, hx, fr0, "mirrored")


def _synthetic_pyramid(B, h, w, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B * h * w, h >> l, w >> l), generator=g) for l in range(4)]


def test_lookup_checker_catches_simulated_bugs():
    B, h, w = 1, 13, 11
    M = B * h * w
    pyr = _synthetic_pyramid(B, h, w)
    pts = lookup_coords(h, w)[:M]
    ref, mag, extra = rc.lookup_reference(pyr, pts, B, h, w)
    K = rc.K_LOOKUP
    assert not _flagged(ref.float(), ref, mag, K, extra)
    # x and y offsets swapped (channel i * 9 + j read as j * 9 + i)
    swapped = ref.reshape(M, 4, 9, 9).transpose(2, 3).reshape(M, 324)
    assert _flagged(swapped, ref, mag, K, extra)
    # one level sampled at c / 2^(l - 1) or c / 2^(l + 1)
    for l in range(4):
        for dl in (-1, 1):
            if l + dl < 0:
                continue
            scaled, _, _ = rc.lookup_reference(pyr, pts * 2.0 ** (l - (l + dl)), B, h, w)
            bad = ref.clone()
            bad[:, l * 81:(l + 1) * 81] = scaled[:, l * 81:(l + 1) * 81]
            assert _flagged(bad, ref, mag, K, extra), (l, dl)


def test_upsample_checker_catches_simulated_bugs():
    for shape in ((2, 5, 6), (1, 1, 3)):
        c, m = upsample_inputs(shape, "random", "near", 9)
        ref, mag = rc.upsample_reference(c, m)
        assert not _flagged(ref.float(), ref, mag, rc.K_UPSAMPLE)
        bad, _ = rc.upsample_reference(c, m, transposed=True)
        assert _flagged(bad, ref, mag, rc.K_UPSAMPLE), shape


def test_flow_head_cases_cover_every_branch_and_residue():
    branches = {rc.flow_head_branch(*c[:3]) for c in FH_CASES}
    assert branches == {"wave", "quad", "stride"}
    assert {c[1] % 4 for c in FH_CASES} >= {0, 1, 2, 3}
    assert {c[2] % 8 for c in FH_CASES} >= set(range(8))
    assert {1, 2, 3} <= {c[2] for c in FH_CASES} and any(c[1] == 1 for c in FH_CASES) and any(c[1:3] == (1, 1) for c in FH_CASES)
    assert any(c[0] > 1 and c[1] % 4 for c in FH_CASES)                  # strip rows that end inside an image
    assert any(c[0] > 1 and c[1] % 4 and rc.flow_head_branch(*c[:3]) == "stride" for c in FH_CASES)
    assert {c[3] for c in FH_CASES} == {256, 384} and {c[4] for c in FH_CASES} == {"engine", "flow"}
    # the branch boundaries themselves
    strips = {c[0] * -(-c[1] // 4) * -(-c[2] // 8) for c in FH_CASES}
    assert {1024, 1025, 16384, 16385} <= strips
    assert {rc.flow_head_branch(*c[:3]) for c in FLOW_CONV_CASES} == {"wave", "quad"}


def test_lookup_cases_cover_every_block_residue_and_edge():
    for B, h, w in LOOKUP_MAPS:
        pts = lookup_coords(h, w).tolist()
        for l in range(4):
            hl, wl = h >> l, w >> l
            res = {(rc.window_start(x, l) % 8, rc.window_start(y, l) % 4) for x, y in pts
                   if abs(x) < 1e6 and abs(y) < 1e6}
            assert len(res) == 32, (h, w, l)
            ovx = {rc.overlap(x, l, wl) for x, y in pts}
            ovy = {rc.overlap(y, l, hl) for x, y in pts}
            for ov in (ovx, ovy):
                assert {(1, "lo"), (1, "hi"), (0, "lo"), (0, "hi")} <= ov, (h, w, l, ov)
            # integer and non-integer coordinates at this level (9- and 10-column windows)
            frac = {float(torch.tensor(x, dtype=torch.float32)) / 2 ** l % 1.0 == 0.0 for x, _ in pts}
            assert frac == {True, False}
        # odd integers: integers at level 0, not at level 1
        assert any(x == int(x) and int(x) % 2 == 1 for x, _ in pts)
        assert set(SPECIAL) <= {x for x, _ in pts} and any(str(x) == "-0.0" for x, _ in pts)
    # partial blocks at some level, a level 3 of 1x1 and one of 1xn, M % 4 != 0
    lv = [[(h >> l, w >> l) for l in range(4)] for _, h, w in LOOKUP_MAPS]
    assert any(hl % 4 and wl % 8 for m in lv for hl, wl in m)
    assert any(m[3] == (1, 1) for m in lv) and any(m[3][0] == 1 and m[3][1] > 1 for m in lv)
    assert all((B * h * w) % 4 for B, h, w in LOOKUP_MAPS)


def test_upsample_cases_cover_partial_groups_and_thin_maps():
    assert {s[2] % 4 for s in UP_SHAPES} == {0, 1, 2, 3}
    assert {1, 2, 3} <= {s[2] for s in UP_SHAPES} and any(s[1] == 1 for s in UP_SHAPES) and any(s[0] > 1 for s in UP_SHAPES)


def test_flow_head_preconditions():
    """ofx_flow_head checks what the kernel assumes before any HIP call (testable without a device)."""
    from sd_animation_optical_flow_amd import _lib
    lib = _lib.lib()
    buf = torch.zeros(4096)                      # 64-byte aligned host memory: only the pointer values matter here
    p = buf.data_ptr()
    ok = dict(x=p, ldx=256, w=p, kpad=2304, bias=p, coords1=p, hx_flow=p, ldh=384, frows=p, B=1, h=4, w_=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ofx_flow_head(a["x"], a["ldx"], a["w"], a["kpad"], a["bias"], a["coords1"], a["hx_flow"], a["ldh"], a["frows"],
                                 a["B"], a["h"], a["w_"], None)
    for name in ("x", "w", "bias", "coords1", "hx_flow", "frows"):
        assert call(**{name: None}) == -1, name
    for kw in (dict(B=0), dict(h=0), dict(w_=-1), dict(ldx=252), dict(kpad=2300), dict(ldh=1), dict(B=1 << 14, h=256, w_=256)):
        assert call(**kw) == -1, kw
    for kw in (dict(ldx=258), dict(kpad=2306), dict(x=p + 8), dict(w=p + 4), dict(coords1=p + 4)):
        assert call(**kw) == -2, kw
    # the ops wrapper refuses host tensors before it reaches the library
    z = torch.zeros((1, 4, 8, 256))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        _ops().flow_head(z, torch.zeros((2, 2304)), torch.zeros(2), torch.zeros((1, 4, 8, 2)), torch.zeros((1, 4, 8, 384)),
                         torch.zeros((1, 4, 8, 16)), 254)
