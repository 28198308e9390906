"""The fused Winograd convolutions (conv_wino.hip) against float64 across shapes, layouts and grid sizes the benchmark never reaches.

Every GPU case is checked elementwise with the operand-scaled bound of wino_check.py.  The case lists are drawn on the CPU from
fixed seeds, and CPU tests assert what they cover: every workgroup-count class of the XCD remap (wino_patch), the Cout tails and
the segment splits.  The CPU test of the checker shows that it catches the kernel bugs it is meant to catch.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wino_check as wc
from gru_check import GUARD, _at, _conv_rows, _guarded, _rows_of

ALGS = {"3x3": (3, 3), "1x5": (1, 5), "5x1": (5, 1)}
CBLK = {"3x3": 64, "1x5": 128, "5x1": 128}       # output channels per workgroup
EPI_PLAIN, EPI_ZR, EPI_Q = 0, 1, 2
HD, HX_LD, GADD_LD = 128, 384, 768               # raft_engine.cpp: hx rows [h | motion | inp], gadd rows [zr1 | q1 | zr2 | q2]
GOFF = {"zr1": 0, "q1": 256, "zr2": 384, "q2": 640}

# worst ratios seen by this module's GPU tests, per kernel (read by hand when K in wino_check.py is re-measured)
MEASURED = {}


def _note(kernel, ratio):
    MEASURED[kernel] = max(MEASURED.get(kernel, 0.0), ratio)


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def workgroups(alg, B, H, W, cout):
    return B * (H // 8) * (W // 16) * -(-cout // CBLK[alg])


def wg_class(n):
    """The three branches of wino_patch: fewer than 8 workgroups (q8 = 0), a multiple of 8 (r8 = 0), or both q8 > 0 and r8 != 0."""
    return "lt8" if n < 8 else "mul8" if n % 8 == 0 else "rem8"


# ---------------------------------------------------------------------------------------------------------------------------------
# the checker itself (CPU): each simulated kernel bug, applied to a float64 result, must be caught

def _halo_shift(x, alg):
    """The input one pixel off along the kernel's long axis (the halo staged from the wrong origin)."""
    return torch.roll(x, 1, dims=2 if alg == "5x1" else 3)


def _simulated_bugs(alg, x, w, sh):
    kh, kw = ALGS[alg]
    ref = wc.conv64(x, w, kh, kw) + sh.double().view(1, -1, 1, 1)
    bugs = {}
    w_drop = w.clone()
    w_drop[:, :, kh // 2, kw // 2 + (1 if kw > 1 else 0)] = 0             # one tap of every filter dropped
    bugs["tap_dropped"] = wc.conv64(x, w_drop, kh, kw) + sh.double().view(1, -1, 1, 1)
    out = ref.clone()
    shifted = wc.conv64(_halo_shift(x, alg), w, kh, kw) + sh.double().view(1, -1, 1, 1)
    if alg == "5x1":
        out[:, :, 7::8] = shifted[:, :, 7::8]                             # the bottom row of every patch from a shifted halo
    else:
        out[..., 15::16] = shifted[..., 15::16]                           # the right column of every patch
    bugs["halo_shifted_at_patch_edge"] = out
    if kh > 1:                                                            # (1x5: no vertical halo to leak into)
        ph = kh // 2
        xp = F.pad(x.double(), (0, 0, ph, ph))
        xp[:-1, :, -ph] = x[1:, :, 0].double()                            # image b's bottom halo row = image b + 1's first row
        leak = F.conv2d(xp, w.double(), padding=(0, kw // 2)) + sh.double().view(1, -1, 1, 1)
        bugs["next_image_row_in_bottom_halo"] = leak
    out = ref.clone()
    out[:, 32:64] = ref[:, 64:96]                                         # block 64..95 stored in the 32..63 slot
    bugs["channel_block_in_wrong_slot"] = out
    out = ref.clone()
    out[:, -1] = float("nan")                                             # the last output channel never written (NaN prefill)
    bugs["cout_tail_unwritten"] = out
    return ref, bugs


EXPECTED_CAUGHT = {
    "3x3": {"tap_dropped", "halo_shifted_at_patch_edge", "next_image_row_in_bottom_halo", "channel_block_in_wrong_slot",
            "cout_tail_unwritten"},
    "5x1": {"tap_dropped", "halo_shifted_at_patch_edge", "next_image_row_in_bottom_halo", "channel_block_in_wrong_slot",
            "cout_tail_unwritten"},
    "1x5": {"tap_dropped", "halo_shifted_at_patch_edge", "channel_block_in_wrong_slot", "cout_tail_unwritten"},
}


@pytest.mark.parametrize("alg", list(ALGS))
@pytest.mark.parametrize("dist", ["normal", "relu", "tanh"])
def test_the_checker_catches_each_simulated_kernel_bug(alg, dist):
    kh, kw = ALGS[alg]
    K = wc.K_F23 if alg == "3x3" else wc.K_F45
    g = torch.Generator().manual_seed(kh * 10 + kw)
    x = _draw_input((2, 32, 16, 32), dist, g)
    w = torch.randn((97, 32, kh, kw), generator=g) / np.sqrt(32 * kh * kw)
    sh = torch.randn((97,), generator=g) * 0.1
    ref, bugs = _simulated_bugs(alg, x, w, sh)
    _, mag = wc.reference(x, w, kh, kw, shift=sh)
    assert set(bugs) == EXPECTED_CAUGHT[alg]
    caught = {name for name, out in bugs.items() if bool(wc.violations(out, ref, mag, K).any())}
    assert caught == EXPECTED_CAUGHT[alg]
    # ... while the float32 rounding of the right answer, and a perturbation of a few ulp of the magnitude, pass
    assert not bool(wc.violations(ref.float(), ref, mag, K).any())
    assert not bool(wc.violations(ref + 0.5 * K * wc.EPS * mag, ref, mag, K).any())


def test_the_checker_counts_nan_as_a_violation():
    ref = torch.zeros(4, dtype=torch.float64)
    assert bool(wc.violations(torch.tensor([0.0, float("nan"), 0.0, 0.0]), ref, torch.ones(4), 1e6).any())


# ---------------------------------------------------------------------------------------------------------------------------------
# the seeded sweep of the plain epilogue (cases drawn on the CPU)

def _draw_input(shape, dist, g):
    x = torch.randn(shape, generator=g)
    if dist == "relu":     # a ReLU'd activation: non-negative, non-zero mean
        return torch.relu(x) * 2.0 + 1.0 + 2.0 * torch.rand((1, shape[1], 1, 1), generator=g)
    if dist == "tanh":
        return torch.tanh(2.0 * x)
    return x


def _case(alg, B, H, W, c0, c1, cout, **kw):
    c = dict(alg=alg, B=B, H=H, W=W, c0=c0, c1=c1, cout=cout, xoff0=0, ld0=c0, xoff1=0, ld1=c1, ooff=0, ldo=cout, scale=False,
             shift=True, relu=True, addend=False, aoff=0, ldad=cout, dist="normal", wmul=1.0, seed=0)
    c.update(kw)
    return c


def _fixed_cases(alg):
    """Hand-picked: the map extremes, the workgroup counts 9 / 13 / 255 / 510, every Cout tail, splits off 64-channel boundaries."""
    one_d = alg != "3x3"
    cs = [
        _case(alg, 1, 8, 16, 32, 0, 64),                                   # one patch: the halo clipped on all four sides
        _case(alg, 1, 8, 256, 32, 0, 48, dist="relu"),                     # one patch row, wide
        _case(alg, 1, 128, 16, 32, 0, 48, dist="tanh"),                    # one patch column, tall
        _case(alg, 5, 16, 32, 32, 0, 40),                                  # several images of two patch rows each
        _case(alg, 1, 24, 48, 32, 0, 64 if not one_d else 128),            # 9 workgroups
        _case(alg, 1, 8, 208, 16, 0, 64 if not one_d else 100),            # 13 workgroups
        _case(alg, 1, 136, 240, 16, 0, 64 if not one_d else 128, dist="relu"),   # 255 patches: a 1088x1920 frame's 1/8 map
        _case(alg, 2, 136, 240, 16, 0, 33 if not one_d else 127, dist="tanh"),   # 2 x 255
        _case(alg, 1, 16, 32, 96, 160, 96, xoff0=16, ld0=128, xoff1=32, ld1=196),   # segment split at 96
        _case(alg, 2, 8, 32, 224, 32, 40, xoff0=4, ld0=256, ld1=36),                # segment split at 224
        _case(alg, 1, 16, 48, 128, 0, 64, xoff0=0, ld0=384, ooff=128, ldo=384, dist="tanh"),   # h inside an hx row
    ]
    couts = (1, 33, 63, 64, 65, 126, 192) if not one_d else (1, 32, 96, 127, 129, 200)
    for i, co in enumerate(couts):
        cs.append(_case(alg, 1 + i % 3, 16, 32, 64, 0, co, ooff=3 * i, ldo=co + 3 * i + 5, scale=i % 2 == 1, relu=i % 3 != 2,
                        addend=one_d and i % 2 == 0, aoff=2 * i, ldad=co + 2 * i + 1, seed=i))
    return cs


N_CASES = 40


def _drawn_cases(alg):
    rng = np.random.default_rng({"3x3": 101, "1x5": 102, "5x1": 103}[alg])
    kh, kw = ALGS[alg]
    cs = _fixed_cases(alg)
    while len(cs) < N_CASES:
        B = int(rng.integers(1, 6))
        H = 8 * int(rng.choice([1, 2, 3, 4, 5, 8, 16]))
        W = 16 * int(rng.choice([1, 2, 3, 5, 7, 8, 16]))
        cin = 16 * int(rng.integers(1, 21))
        c0 = cin
        if cin >= 64 and rng.random() < 0.5:   # two segments of whole 32-channel chunks (ofx_conv2d refuses others: OFX_EALIGN)
            cin = 32 * (cin // 32)
            c0 = 32 * int(rng.integers(1, cin // 32))
        cout = int(rng.integers(1, 257))
        if B * H * W * cin * cout * kh * kw > 3e8:                      # keeps the float64 reference cheap
            continue
        xoff0 = 4 * int(rng.integers(0, 9)) if rng.random() < 0.5 else 0
        ld0 = c0 + xoff0 + (4 * int(rng.integers(0, 9)) if rng.random() < 0.5 else 0)
        ld1 = cin - c0 + 4 * int(rng.integers(0, 5))
        ooff = int(rng.integers(0, 40)) if rng.random() < 0.5 else 0
        ldo = cout + ooff + (int(rng.integers(0, 40)) if rng.random() < 0.5 else 0)
        add = alg != "3x3" and rng.random() < 0.5
        aoff = int(rng.integers(0, 8)) if add else 0
        cs.append(_case(alg, B, H, W, c0, cin - c0, cout, xoff0=xoff0, ld0=ld0, ld1=ld1, ooff=ooff, ldo=ldo,
                        scale=bool(rng.random() < 0.5), shift=bool(rng.random() < 0.7), relu=bool(rng.random() < 0.5),
                        addend=add, aoff=aoff, ldad=cout + aoff + int(rng.integers(0, 5)),
                        dist=str(rng.choice(["normal", "relu", "tanh"])), wmul=float(rng.choice([0.1, 1.0, 4.0])),
                        seed=int(rng.integers(0, 1 << 30))))
    return cs


CASES = {alg: _drawn_cases(alg) for alg in ALGS}


@pytest.mark.parametrize("alg", list(ALGS))
def test_the_sweep_draws_every_class(alg):
    cs = CASES[alg]
    assert len(cs) == N_CASES
    classes = {wg_class(workgroups(alg, c["B"], c["H"], c["W"], c["cout"])) for c in cs}
    assert classes == {"lt8", "mul8", "rem8"}
    wgs = {workgroups(alg, c["B"], c["H"], c["W"], c["cout"]) for c in cs}
    assert {9, 13, 255, 510} <= wgs
    couts = {c["cout"] for c in cs}
    assert set((1, 33, 63, 64, 65, 126, 192) if alg == "3x3" else (1, 32, 96, 127, 129, 200)) <= couts
    assert {(96, 160), (224, 32)} <= {(c["c0"], c["c1"]) for c in cs}    # slab boundaries that are not 64- or 128-channel ones
    assert sum(1 for c in cs if c["c1"] and c["c0"] % 64) >= 3
    assert {(1, 8, 16), (1, 8, 256), (1, 128, 16)} <= {(c["B"], c["H"], c["W"]) for c in cs}
    assert any(c["B"] > 1 and c["H"] > 8 for c in cs)                   # several images of several patch rows
    assert any(c["ld0"] > c["c0"] + c["xoff0"] and c["xoff0"] for c in cs)
    assert any(c["ldo"] > c["cout"] + c["ooff"] and c["ooff"] for c in cs)
    assert {c["dist"] for c in cs} == {"normal", "relu", "tanh"}
    assert {c["relu"] for c in cs} == {True, False} and {c["scale"] for c in cs} == {True, False}
    if alg != "3x3":
        assert any(c["addend"] for c in cs)
    for c in cs:
        assert c["xoff0"] + c["c0"] <= c["ld0"] and c["xoff1"] + c["c1"] <= max(c["ld1"], 1)
        assert c["ooff"] + c["cout"] <= c["ldo"] and c["aoff"] + c["cout"] <= c["ldad"]
        assert c["H"] % 8 == 0 and c["W"] % 16 == 0 and (c["c0"] + c["c1"]) % 16 == 0 and c["c0"] % (32 if c["c1"] else 16) == 0


def _desc(B, H, W, kh, kw, cout):
    from sd_animation_optical_flow_amd import _lib
    d = _lib.ConvDesc()
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, H, W, H, W, cout
    d.KH, d.KW, d.stride, d.padH, d.padW = kh, kw, 1, kh // 2, kw // 2
    return d


def _run(d):
    from sd_animation_optical_flow_amd import _lib
    st = _lib.lib().ofx_conv2d(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, st


def _rows_buffer(B, H, W, ld, off, x_nchw, fill, g):
    """[B, H, W, ld] on the device with x's channels at [off, off + C) and `fill` + noise in the rest of every row."""
    buf = fill + torch.rand((B, H, W, ld), generator=g)
    buf[..., off:off + x_nchw.shape[1]] = x_nchw.permute(0, 2, 3, 1)
    return buf.cuda()


def run_plain_case(c):
    """Launch the fused kernel (forced) and the direct kernel on case c; check both against float64, the layout and the repeat."""
    ops = _ops()
    alg = c["alg"]
    kh, kw = ALGS[alg]
    B, H, W, c0, c1, co = c["B"], c["H"], c["W"], c["c0"], c["c1"], c["cout"]
    cin = c0 + c1
    g = torch.Generator().manual_seed(c["seed"])
    x = _draw_input((B, cin, H, W), c["dist"], g)
    w = torch.randn((co, cin, kh, kw), generator=g) * (c["wmul"] / np.sqrt(cin * kh * kw))
    sc = torch.rand((co,), generator=g) + 0.5 if c["scale"] else None
    sh = torch.randn((co,), generator=g) * 0.3 if c["shift"] else None
    add = torch.randn((B, co, H, W), generator=g) if c["addend"] else None
    ref, mag = wc.reference(x, w, kh, kw, sc, sh, add, c["relu"])

    x0 = _rows_buffer(B, H, W, c["ld0"], c["xoff0"], x[:, :c0], 100.0, g)   # neighbours of the segment: large, never read
    x1 = _rows_buffer(B, H, W, c["ld1"], c["xoff1"], x[:, c0:], -100.0, g) if c1 else None
    ad = _rows_buffer(B, H, W, c["ldad"], c["aoff"], add, 1000.0, g) if add is not None else None
    wp = ops.pack_conv_weight(w).cuda()
    u = (ops.wino_conv_weight(w) if alg == "3x3" else ops.wino15_conv_weight(w)).cuda()
    dsc, dsh = (None if sc is None else sc.cuda()), (None if sh is None else sh.cuda())

    def launch(wino):
        out = torch.full((B, H, W, c["ldo"]), float("nan"), device="cuda")
        d = _desc(B, H, W, kh, kw, co)
        d.in0, d.ld0, d.c0 = x0.data_ptr() + 4 * c["xoff0"], c["ld0"], c0
        if c1:
            d.in1, d.ld1, d.c1 = x1.data_ptr() + 4 * c["xoff1"], c["ld1"], c1
        d.w = wp.data_ptr()
        d.scale = 0 if dsc is None else dsc.data_ptr()
        d.shift = 0 if dsh is None else dsh.data_ptr()
        d.out, d.ldo = out.data_ptr() + 4 * c["ooff"], c["ldo"]
        if ad is not None:
            d.addend, d.ldadd = ad.data_ptr() + 4 * c["aoff"], c["ldad"]
        d.act, d.epi = (1 if c["relu"] else 0), EPI_PLAIN
        if wino:
            d.wino_w, d.tile = u.data_ptr(), ops.TILE_WINOGRAD
        _run(d)
        return out

    win = launch(True)
    direct = launch(False)
    kern = "F23" if alg == "3x3" else "F45"
    sel = slice(c["ooff"], c["ooff"] + co)
    for out in (win, direct):   # channels outside [ooff, ooff + cout) of every row stay untouched
        assert bool(torch.isnan(out[..., :c["ooff"]]).all()) and bool(torch.isnan(out[..., c["ooff"] + co:]).all()), c
    got = win[..., sel].permute(0, 3, 1, 2).cpu()
    gotd = direct[..., sel].permute(0, 3, 1, 2).cpu()
    r = wc.check(got, ref, mag, wc.K_F23 if alg == "3x3" else wc.K_F45, f"{kern} {c}")
    rd = wc.check(gotd, ref, mag, wc.K_DIRECT, f"direct {c}")
    _note(kern, r)
    _note("direct", rd)
    assert not torch.equal(got, gotd), c                                 # the fused kernel really ran
    again = launch(True)
    assert torch.equal(win.view(torch.int32), again.view(torch.int32)), c   # repeats bit for bit
    return r, rd


@pytest.mark.gpu
@pytest.mark.parametrize("alg", list(ALGS))
@pytest.mark.parametrize("c0,c1", [(48, 208), (64, 80), (32, 16)])
def test_two_segments_off_32_channel_chunks_are_refused(cuda, alg, c0, c1):
    """Two input segments must both be whole 32-channel chunks, on either route (ofx_conv2d validates for the direct kernel first).
    c0 = 64 + c1 = 80 and 32 + 16 are cases the sweep caught: with cin % 32 == 16, a 32-channel K chunk of the general direct
    schedule wraps from one tap's last in1 channels to the next tap's first in0 channels, and the chunk's single segment choice
    read half of it from the wrong tensor -- a silently wrong result, now OFX_EALIGN."""
    ops = _ops()
    kh, kw = ALGS[alg]
    xa, xb = torch.zeros((1, 8, 16, c0), device="cuda"), torch.zeros((1, 8, 16, c1), device="cuda")
    w = torch.zeros((64, c0 + c1, kh, kw))
    u = (ops.wino_conv_weight(w) if alg == "3x3" else ops.wino15_conv_weight(w)).cuda()
    for tile in (ops.TILE_WINOGRAD, 0):
        with pytest.raises(RuntimeError) as e:
            ops.conv2d_nhwc(xa, ops.pack_conv_weight(w).cuda(), kh, kw, 64, x2=xb, wino_w=u, tile=tile)
        assert e.value.code == -2, e.value                                # OFX_EALIGN


@pytest.mark.gpu
@pytest.mark.parametrize("alg", list(ALGS))
def test_plain_epilogue_sweep_against_float64(cuda, alg):
    worst = [run_plain_case(c) for c in CASES[alg]]
    r_win, r_dir = max(w[0] for w in worst), max(w[1] for w in worst)
    # the same scale as the direct kernel over the sweep (the per-case form: test_gpu_conv_winograd*.py, unit-normal inputs)
    _note(f"same_scale_{alg}", r_win / r_dir)
    assert r_win <= wc.K_SAME_SCALE * r_dir, (r_win, r_dir)


# ---------------------------------------------------------------------------------------------------------------------------------
# the update block's 3x3 layers with the engine's exact descriptors (raft_engine.cpp, run_recurrence), 27 patches

ENGINE_3X3 = {   # name: (cin, ld0, in offset, Cout, ldo, out offset)
    "convc2": (256, 256, 0, 192, 256, 0),         # c1 -> corflo[:, :192]
    "conv": (256, 256, 0, 126, HX_LD, 128),       # corflo -> hx[:, 128:254]
    "fh1": (128, HX_LD, 0, 256, 256, 0),          # h = hx[:, :128] -> c1
    "convf2": (128, 128, 0, 64, 256, 192),        # f1 -> corflo[:, 192:256]
}


@pytest.mark.gpu
@pytest.mark.parametrize("layer", list(ENGINE_3X3))
def test_engine_3x3_layer_descriptors_against_float64(cuda, layer):
    cin, ld0, xoff, co, ldo, ooff = ENGINE_3X3[layer]
    c = _case("3x3", 3, 24, 48, cin, 0, co, xoff0=xoff, ld0=ld0, ooff=ooff, ldo=ldo, dist="relu" if layer != "fh1" else "tanh",
              seed=len(layer))
    assert workgroups("3x3", 3, 24, 48, co) % 8 and 3 * 3 * 3 == 27
    run_plain_case(c)


# ---------------------------------------------------------------------------------------------------------------------------------
# the GRU gate epilogues in the engine's layout, with guard rows around every destination

GRU_MAPS = [(1, 8, 16), (1, 8, 128), (1, 64, 16), (3, 24, 48), (1, 136, 240), (2, 136, 240)]


def _check_rows(B, H, W):
    """Rows of the map checked against float64: all of a small map; on a large one, the first and last patch rows of every image
    and the seam between patch rows 1 and 2 (the float64 reference of a 256-channel 1x5 / 5x1 layer at 136x240 is the cost)."""
    if B * H * W <= 4096:
        return list(range(H))
    return sorted({0, 1, 2, 6, 7, 8, 9, 14, 15, 16, 17, H - 9, H - 8, H - 3, H - 2, H - 1})


def _gru_state(B, H, W, seed):
    M = B * H * W
    g = torch.Generator().manual_seed(seed)
    hx = torch.cat([torch.tanh(torch.randn((M, HD), generator=g)), torch.relu(torch.randn((M, HD), generator=g)) * 2.0,
                    torch.randn((M, HD), generator=g)], 1)
    gadd = torch.randn((M, GADD_LD), generator=g) * 0.3
    return g, _guarded(M, HX_LD, g, hx), _guarded(M, GADD_LD, g, gadd)


def run_gru_case(epi, alg, B, H, W, seed, cout=None, goff=None):
    ops = _ops()
    kh, kw = ALGS[alg]
    M = B * H * W
    g, hx, gadd = _gru_state(B, H, W, seed)
    rows = _check_rows(B, H, W)
    hxb = hx[GUARD:GUARD + M]
    if epi == EPI_ZR:
        cout = cout or 2 * HD
        hd = cout // 2
        goff = GOFF["zr1"] if goff is None else goff
        w = torch.randn((cout, 2 * HD, kh, kw), generator=g) * (1.5 / np.sqrt(2 * HD * 5))
        xin = hxb[:, :2 * HD]
        zbuf0, rhbuf0 = _guarded(M, hd, g, float("nan")), _guarded(M, hd, g, float("nan"))
    else:
        cout, hd = HD, HD
        goff = GOFF["q1"] if goff is None else goff
        w = torch.randn((HD, 2 * HD, kh, kw), generator=g) * (1.5 / np.sqrt(2 * HD * 5))
        rh_in = torch.tanh(torch.randn((M, HD), generator=g)) * 0.5
        zbuf0, rhbuf0 = _guarded(M, HD, g), _guarded(M, HD, g, rh_in)
        xin = torch.cat([rh_in, hxb[:, HD:2 * HD]], 1)
    xin = xin.reshape(B, H, W, -1).permute(0, 3, 1, 2)
    addv = _rows_of(gadd[GUARD:GUARD + M, goff:goff + cout], B, H, W, rows).double()
    v = _conv_rows(xin, w, kh, kw, rows) + addv
    mag = _conv_rows(xin.abs(), w.abs(), kh, kw, rows) + addv.abs()
    wp, u = ops.pack_conv_weight(w).cuda(), ops.wino15_conv_weight(w).cuda()

    def launch(wino):
        dhx, dg, dz, drh = hx.cuda(), gadd.cuda(), zbuf0.cuda(), rhbuf0.cuda()
        d = _desc(B, H, W, kh, kw, cout)
        d.w = wp.data_ptr()
        d.act, d.epi = 0, epi
        d.addend, d.ldadd = _at(dg, GADD_LD) + 4 * goff, GADD_LD
        d.aux_h, d.ldh = _at(dhx, HX_LD), HX_LD
        d.aux_z = _at(dz, hd)
        if epi == EPI_ZR:
            d.in0, d.ld0, d.c0 = _at(dhx, HX_LD), HX_LD, 2 * HD
            d.aux_rh = _at(drh, hd)
        else:
            d.in0, d.ld0, d.c0 = _at(drh, HD), HD, HD
            d.in1, d.ld1, d.c1 = _at(dhx, HX_LD) + 4 * HD, HX_LD, HD
        if wino:
            d.wino_w, d.tile = u.data_ptr(), ops.TILE_WINOGRAD
        _run(d)
        bits = lambda t: t.cpu().view(torch.int32)
        assert torch.equal(bits(dg), bits(gadd))                         # the addend is only read
        if epi == EPI_ZR:
            assert torch.equal(bits(dhx), bits(hx))                      # hx (guard rows included) is only read
            for got in (dz.cpu(), drh.cpu()):                            # z and r * h: every row written, the guard rows untouched
                assert bool(torch.isnan(got[:GUARD]).all() and torch.isnan(got[GUARD + M:]).all())
            return dz.cpu()[GUARD:GUARD + M], drh.cpu()[GUARD:GUARD + M]
        out = dhx.cpu()
        assert torch.equal(bits(out[:, HD:]), bits(hx[:, HD:]))          # only the h channels ...
        # ... of the rows below M
        assert torch.equal(bits(out[:GUARD]), bits(hx[:GUARD])) and torch.equal(bits(out[GUARD + M:]), bits(hx[GUARD + M:]))
        assert torch.equal(bits(dz.cpu()), bits(zbuf0)) and torch.equal(bits(drh.cpu()), bits(rhbuf0))
        return (out[GUARD:GUARD + M, :HD],)

    def check(res, K, kern):
        if epi == EPI_ZR:
            z, rh = (_rows_of(t, B, H, W, rows) for t in res)
            h = _rows_of(hxb[:, :hd], B, H, W, rows).double()
            zr = torch.sigmoid(v)
            # sigmoid' <= 1/4 carries the pre-activation bound to z and, times |h|, to r * h
            r1 = wc.check(z, zr[:, :hd], mag[:, :hd], K, f"{kern} z {alg} {B}x{H}x{W}", 0.25, wc.ACT_ULP)
            r2 = wc.check(rh, zr[:, hd:] * h, mag[:, hd:], K, f"{kern} r*h {alg} {B}x{H}x{W}", 0.25 * h.abs(),
                          wc.ACT_ULP * h.abs().clamp_min(1.0))
            return max(r1, r2)
        hn = _rows_of(res[0], B, H, W, rows)
        z = _rows_of(zbuf0[GUARD:GUARD + M], B, H, W, rows).double()
        h = _rows_of(hxb[:, :HD], B, H, W, rows).double()
        ref = (1 - z) * h + z * torch.tanh(v)
        return wc.check(hn, ref, mag, K, f"{kern} h {alg} {B}x{H}x{W}", z, wc.ACT_ULP)   # tanh' <= 1, weighted by z

    kern = "F45_ZR" if epi == EPI_ZR else "F45_Q"
    win = launch(True)
    direct = launch(False)
    r = check(win, wc.K_F45_GRU, kern)
    rd = check(direct, wc.K_DIRECT, "direct")
    _note(kern, r)
    _note("direct", rd)
    assert not torch.equal(win[0], direct[0])                            # the fused kernel really ran
    again = launch(True)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(win, again))   # bit for bit
    return r, rd


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ["1x5", "5x1"])
@pytest.mark.parametrize("epi", [EPI_ZR, EPI_Q], ids=["zr", "q"])
@pytest.mark.parametrize("B,H,W", GRU_MAPS)
def test_gru_epilogues_over_maps_against_float64(cuda, B, H, W, epi, alg):
    n = workgroups(alg, B, H, W, 2 * HD if epi == EPI_ZR else HD)
    if (B, H, W) == (3, 24, 48):
        assert wg_class(n) == "rem8"
    pass_ = "1" if alg == "1x5" else "2"
    goff = GOFF[("zr" if epi == EPI_ZR else "q") + pass_]
    for seed in (B * H + W, 7 * W + H):
        run_gru_case(epi, alg, B, H, W, seed, goff=goff)


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ["1x5", "5x1"])
@pytest.mark.parametrize("B,H,W", [(1, 8, 16), (3, 24, 48)])
def test_gru_zr_with_two_blocks_on_each_side_of_the_split(cuda, B, H, W, alg):
    """Cout 512: z from blocks 0-1, r * h from blocks 2-3 (hd = 256 reads h and the motion features as the r * h operand)."""
    run_gru_case(EPI_ZR, alg, B, H, W, 5 + W, cout=512)


# ---------------------------------------------------------------------------------------------------------------------------------
# automatic routing at the thresholds

LAYERS = {   # name: (kh, kw, cin, cout)
    "convc2": (3, 3, 256, 192), "conv": (3, 3, 256, 126), "fh1": (3, 3, 128, 256), "convf2": (3, 3, 128, 64),
    "gru.zr1": (1, 5, 256, 256), "gru.q1": (1, 5, 256, 128), "gru.zr2": (5, 1, 256, 256), "gru.q2": (5, 1, 256, 128),
}


def route_fused(kh, kw, B, H, W, cout):
    """ofx_conv_wino_choose (its shape test and grid gates) as documented, for a plain fp32 stride-1 'same' layer with the operand given and the
    automatic tile: whole 8x16 patches, then 3x3 at >= 1024 workgroups of 64 output channels, 1x5 / 5x1 at >= 256 patches."""
    if H % 8 or W % 16:
        return False
    patches = B * (H // 8) * (W // 16)
    return patches * -(-cout // 64) >= 1024 if (kh, kw) == (3, 3) else patches >= 256


FUSED_1D = {"gru.zr1", "gru.q1", "gru.zr2", "gru.q2"}
ROUTES = [   # (B, H, W, the layers that take the fused kernel)
    (1, 136, 240, set()),                                            # 255 patches; fh1 1020 workgroups < 1024
    (2, 136, 240, {"convc2", "fh1"} | FUSED_1D),                     # 510; conv (2 blocks) 1020, convf2 (1 block) 510
    (5, 64, 96, set()),                                              # 240 patches; fh1 960
    (6, 64, 96, {"fh1"} | FUSED_1D),                                 # 288; fh1 1152, convc2 864
    (2, 136, 248, set()),                                            # not whole patches
]


def test_the_routing_table_restates_the_documented_predicate():
    for B, H, W, fused in ROUTES:
        assert {n for n, (kh, kw, _, co) in LAYERS.items() if route_fused(kh, kw, B, H, W, co)} == fused, (B, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,fused", ROUTES, ids=[f"B{r[0]}x{r[1]}x{r[2]}" for r in ROUTES])
def test_automatic_route_at_the_thresholds(cuda, B, H, W, fused):
    """Fused when the result differs from the direct kernel's, direct when it is equal bit for bit."""
    ops = _ops()
    g = torch.Generator().manual_seed(B + H + W)
    for name, (kh, kw, cin, co) in LAYERS.items():
        x = torch.randn((B, H, W, cin), generator=g).cuda()
        w = torch.randn((co, cin, kh, kw), generator=g) / np.sqrt(cin * kh * kw)
        wp = ops.pack_conv_weight(w).cuda()
        u = (ops.wino_conv_weight(w) if kh == 3 else ops.wino15_conv_weight(w)).cuda()
        auto = ops.conv2d_nhwc(x, wp, kh, kw, co, act="relu", wino_w=u)
        direct = ops.conv2d_nhwc(x, wp, kh, kw, co, act="relu")
        assert (not torch.equal(auto, direct)) == (name in fused), (name, B, H, W)
        assert (auto - direct).abs().max().item() < 1e-3, name


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end where the route changes inside one frame size

@pytest.mark.gpu
def test_two_1088x1920_pairs_match_their_single_pair_runs(cuda):
    """B = 2 at 1088x1920 (a 1080p frame padded): 255 patches per image, so the batch runs the F(4,5) GRU and F(2x2,3x3) for convc2
    and fh1 (conv and convf2 stay direct), while each single pair runs only direct kernels.  Every pair must match its own run."""
    from sd_animation_optical_flow_amd.raft import RaftEngine
    from sd_animation_optical_flow_amd.weights import random_state_dict
    eng = RaftEngine(random_state_dict(0), "cuda")
    B, H, W = 2, 1088, 1920
    g = torch.Generator().manual_seed(17)
    base = torch.rand((1, 3, H + 32, W + 32), generator=g)
    base = F.conv2d(base, torch.ones((3, 1, 5, 5)) / 25.0, padding=2, groups=3)
    base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)[0].permute(1, 2, 0)
    key = base[16:16 + H, 16:16 + W].contiguous().cuda()
    frames = torch.stack([base[16 + 2 * b - 1:16 + 2 * b - 1 + H, 16 + 3 * b - 2:16 + 3 * b - 2 + W] for b in range(B)])
    frames = frames.contiguous().cuda()
    up = eng.forward(frames, key, iters=6)
    assert tuple(up.shape) == (B, H, W, 2) and torch.isfinite(up).all()
    for b in range(B):
        single = eng.forward(frames[b:b + 1], key, iters=6)
        assert torch.isfinite(single).all()
        assert (up[b:b + 1] - single).abs().max().item() < 1e-4, b
