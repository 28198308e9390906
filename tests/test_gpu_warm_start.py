"""-m gpu: warm start (RAFT.forward(flow_init=...)) on the native engine and forward_interpolate on the device.

forward_interpolate against the reference's own outputs (tests/golden/raft_warm_ref_128x160.npz) and the numpy brute force of
tests/warm_start_check.py; the warm-started flows of both networks against the fixture and the float64 restatement (the project's bar:
mean flow EPE < 1e-3 px); an all-zero init against no init, bit for bit, on every entry point and schedule; slicing, padding, the
split-bf16 modes, argument checks, and the RAFT_2(warm_start=True) chain.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import warm_start_check as WS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_warm_ref_128x160.npz")
FLOAT_FIELDS = ("smooth", "random", "leaving")


def _frames(seed, B, H, W):
    """A blurred-noise key frame and B shifted copies (uint8 HWC)."""
    g = torch.Generator().manual_seed(seed)
    base = F.avg_pool2d(torch.rand((1, 3, H + 32, W + 32), generator=g), 5, 1, 2)
    base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)
    key = base[0, :, 16:16 + H, 16:16 + W].permute(1, 2, 0).contiguous()
    frames = []
    for b in range(B):
        dx, dy = (3 * b + 2) % 7 - 3, (5 * b + 1) % 5 - 2
        frames.append(base[0, :, 16 + dy:16 + dy + H, 16 + dx:16 + dx + W].permute(1, 2, 0).contiguous())
    return key, torch.stack(frames)


def _init(B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn((B, 2, 3, 4), generator=g) * 2.0
    return F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).contiguous().cuda()


def _epe(a, b):
    return (a.double() - b.double()).pow(2).sum(-1).sqrt().mean().item()


def _nhwc(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 2, 3, 1).contiguous()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def basic(cuda, raft_sd):
    from sd_animation_optical_flow_amd.raft import RaftEngine
    return RaftEngine(raft_sd)


@pytest.fixture(scope="module")
def small_sd():
    from sd_animation_optical_flow_amd.weights import random_state_dict
    return random_state_dict(0, small=True)


@pytest.fixture(scope="module")
def small(cuda, small_sd):
    from sd_animation_optical_flow_amd.raft import RaftEngine
    return RaftEngine(small_sd)


# ---------------------------------------------------------------------------------------------------------- forward_interpolate
def _fi(field_2hw):
    from sd_animation_optical_flow_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(field_2hw)).permute(1, 2, 0).contiguous().cuda()
    return ops.forward_interpolate(t).permute(2, 0, 1).cpu().numpy()


@pytest.mark.parametrize("name", FLOAT_FIELDS)
def test_forward_interpolate_is_the_reference_bit_for_bit(cuda, gold, name):
    assert np.array_equal(_fi(gold["fi_in_" + name]), gold["fi_out_" + name])


def test_forward_interpolate_breaks_ties_to_the_lowest_index(cuda, gold):
    f = gold["fi_in_ties"]
    out = _fi(f)
    brute, pick = WS.forward_interpolate_brute(f, return_index=True)
    assert np.array_equal(out, brute)
    d2, dmin = WS.nearest_d2(f, pick)
    assert np.array_equal(d2, dmin)


def test_forward_interpolate_gives_nan_without_a_valid_source(cuda, gold):
    from sd_animation_optical_flow_amd import ops
    assert np.isnan(_fi(gold["fi_in_invalid"])).all()
    # in a batch: only the field without sources is NaN
    a = torch.from_numpy(gold["fi_in_invalid"]).permute(1, 2, 0)
    b = torch.zeros_like(a) + 0.25
    out = ops.forward_interpolate(torch.stack([b, a, b]).contiguous().cuda()).cpu()
    assert torch.isnan(out[1]).all() and torch.isfinite(out[0]).all() and torch.equal(out[0], out[2])


def test_forward_interpolate_batch_equals_single_fields(cuda):
    from sd_animation_optical_flow_amd import ops
    g = torch.Generator().manual_seed(3)
    h, w = 34, 50
    fields = [torch.rand((h, w, 2), generator=g) * 8 - 4, torch.randn((h, w, 2), generator=g) * 10,
              torch.zeros((h, w, 2)), torch.full((h, w, 2), 60.0), torch.randn((h, w, 2), generator=g).round()]
    batch = torch.stack(fields).cuda()
    out = ops.forward_interpolate(batch)
    assert torch.isnan(out[3]).all()                                  # (every source of field 3 leaves the frame)
    for i, f in enumerate(fields):
        one = ops.forward_interpolate(f.cuda())
        assert torch.equal(out[i].isnan(), one.isnan()) and torch.equal(out[i].nan_to_num(), one.nan_to_num()), i


@pytest.mark.parametrize("hw", [(1, 37), (29, 1), (17, 23), (68, 120)])
def test_forward_interpolate_odd_sizes_against_the_brute_force(cuda, hw):
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w)
    f = (rng.standard_normal((2, h, w)) * 3).astype(np.float32)
    f[:, rng.random((h, w)) < 0.1] = 0.0                     # some zero flow: row 0 / column 0 sources are never valid
    assert np.array_equal(_fi(f), WS.forward_interpolate_brute(f), equal_nan=True)


def test_forward_interpolate_with_a_large_hole(cuda):
    """Sources pushed out of most of the frame: the ring search walks far, the result is still the brute force's."""
    h, w = 40, 56
    rng = np.random.default_rng(9)
    f = (rng.standard_normal((2, h, w)) * 0.3).astype(np.float32)
    f[0, :, : w - 6] += 200.0
    assert np.array_equal(_fi(f), WS.forward_interpolate_brute(f))


def test_ofgen_forward_interpolate_is_the_reference_drop_in(cuda, gold):
    from sd_animation_optical_flow_amd import ofgen
    for name in FLOAT_FIELDS:
        out = ofgen.forward_interpolate(torch.from_numpy(gold["fi_in_" + name]))
        assert out.device.type == "cpu" and out.dtype == torch.float32 and tuple(out.shape) == gold["fi_in_" + name].shape
        assert np.array_equal(out.numpy(), gold["fi_out_" + name])


def test_forward_interpolate_argument_checks(cuda):
    from sd_animation_optical_flow_amd import _lib, ops
    with pytest.raises(RuntimeError):
        ops.forward_interpolate(torch.zeros((4, 5, 2)))                                  # CPU tensor
    with pytest.raises(RuntimeError):
        ops.forward_interpolate(torch.zeros((4, 5, 3), device="cuda"))
    x = torch.zeros((1, 4, 5, 2), device="cuda")
    need = _lib.lib().ofx_forward_interpolate_scratch_bytes(1, 4, 5)
    s = torch.empty((need,), dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    assert L.ofx_forward_interpolate(C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), C.c_void_p(s.data_ptr()), need, 1, 4, 5, None) != 0
    y = torch.empty_like(x)
    assert L.ofx_forward_interpolate(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(s.data_ptr()), need - 4, 1, 4, 5, None) != 0


# ---------------------------------------------------------------------------------------------------------- engine
def _gold_pair(gold):
    i1 = torch.from_numpy(gold["image1"][0]).permute(1, 2, 0).contiguous().cuda()[None]
    i2 = torch.from_numpy(gold["image2"][0]).permute(1, 2, 0).contiguous().cuda()[None]
    return i1, i2


@pytest.mark.parametrize("case", ["basic", "basic_3", "basic_outside"])
def test_basic_warm_start_against_the_reference(basic, gold, case):
    i1, i2 = _gold_pair(gold)
    sfx = {"basic": "", "basic_3": "_3", "basic_outside": "_outside"}[case]
    init = _nhwc(gold["flow_init_outside" if case == "basic_outside" else "flow_init"]).cuda()
    keep = init.clone()
    up, low = basic.forward(i1, i2, iters=3 if case == "basic_3" else 20, want_low=True, flow_init=init)
    assert torch.equal(init, keep)                                  # the caller's init is not modified
    ref_up = _nhwc(gold["flow_up" + sfx])
    if ref_up.shape[1] != up.shape[1]:
        up = up[:, ::2, ::2]
    e_up, e_lo = _epe(up.cpu(), ref_up), _epe(low.cpu(), _nhwc(gold["flow_low" + sfx]))
    assert e_up < 1e-3 and e_lo < 1e-3, (e_up, e_lo)
    cold = basic.forward(i1, i2, iters=3 if case == "basic_3" else 20)
    if case == "basic_3":
        assert _epe(cold[:, ::2, ::2].cpu(), ref_up) > 0.1            # the init did enter


def test_small_warm_start_against_the_reference(small, gold):
    i1, i2 = _gold_pair(gold)
    up, low = small.forward(i1, i2, iters=20, want_low=True, flow_init=_nhwc(gold["flow_init"]).cuda()[0])   # [h,w,2] for B == 1
    e_up, e_lo = _epe(up.cpu(), _nhwc(gold["small_flow_up"])), _epe(low.cpu(), _nhwc(gold["small_flow_low"]))
    assert e_up < 1e-3 and e_lo < 1e-3, (e_up, e_lo)


@pytest.mark.parametrize("net", ["basic", "small"])
def test_warm_start_against_the_float64_restatement_264x392(request, raft_sd, small_sd, net):
    eng = request.getfixturevalue(net)
    H, W, iters = 264, 392, 8
    key, frames = _frames(31, 1, H, W)
    init = _init(1, H // 8, W // 8, 5)
    up = eng.forward(frames.cuda(), key.cuda(), iters=iters, flow_init=init)
    a, b = frames.permute(0, 3, 1, 2).float(), key[None].permute(0, 3, 1, 2).float()
    i = init.permute(0, 3, 1, 2).cpu()
    _, ref = WS.raft_forward_warm(raft_sd, a, b, i, iters) if net == "basic" else WS.raft_small_forward_warm(small_sd, a, b, i, iters)
    e = _epe(up.cpu(), ref.permute(0, 2, 3, 1))
    assert e < 1e-3, e


def _entry_points(eng, fr, k, iters, init, **kw):
    """The four entry points on the same pairs (fr[b] -> k): forward, forward(warp_frame=), forward_pairs, forward_pairs(warp_frame=)."""
    B = fr.shape[0]
    ai = (255 - k).contiguous()
    out = {"forward": eng.forward(fr, k, iters=iters, flow_init=init, **kw)}
    out["forward_warp"] = eng.forward(fr, k, iters=iters, flow_init=init, warp_frame=ai, **kw)
    images = torch.cat([fr, k[None]]).contiguous()
    if not kw:
        out["pairs"] = eng.forward_pairs(images, list(range(B)), [B] * B, iters=iters, flow_init=init)
        out["pairs_warp"] = eng.forward_pairs(images, list(range(B)), [B] * B, iters=iters, flow_init=init, warp_frame=ai, n_warp=B)
    return out


@pytest.mark.parametrize("net", ["basic", "small"])
def test_zero_init_is_no_init_bit_for_bit(request, net):
    """An all-zero flow_init takes the warm-start kernel and must give exactly the cold flows: every entry point, the serial and
    side-stream schedules, shared image1 / image2, alternate correlation."""
    eng = request.getfixturevalue(net)
    H, W, B, iters = 128, 160, 2, 5
    key, frames = _frames(12, B, H, W)
    fr, k = frames.cuda(), key.cuda()
    zero = torch.zeros((B, H // 8, W // 8, 2), device="cuda")
    for kw in ({}, {"serial": True}):
        cold, warm = _entry_points(eng, fr, k, iters, None, **kw), _entry_points(eng, fr, k, iters, zero, **kw)
        for name in cold:
            c, w = cold[name], warm[name]
            assert all(torch.equal(x, y) for x, y in zip(c if isinstance(c, tuple) else (c,), w if isinstance(w, tuple) else (w,))), (name, kw)
    # shared image1 (one key frame -> B frames) and shared image2 with flow_low out
    assert torch.equal(eng.forward(k, fr, iters=iters, flow_init=zero), eng.forward(k, fr, iters=iters))
    cu, cl = eng.forward(fr, k, iters=iters, want_low=True)
    wu, wl = eng.forward(fr, k, iters=iters, want_low=True, flow_init=zero)
    assert torch.equal(cu, wu) and torch.equal(cl, wl)
    # alternate correlation (per-pair frames)
    k2 = k[None].repeat(B, 1, 1, 1).contiguous()
    assert torch.equal(eng.forward(fr, k2, iters=iters, alternate_corr=True, flow_init=zero), eng.forward(fr, k2, iters=iters, alternate_corr=True))


@pytest.mark.parametrize("net", ["basic", "small"])
def test_per_pair_inits_land_on_their_pairs(request, net):
    """Pair b of a batch takes field b of flow_init: a batch of mixed inits equals, pair by pair and bit for bit, the same batch run with
    every pair on that pair's init (same batch size: same schedule)."""
    eng = request.getfixturevalue(net)
    H, W, B, iters = 128, 160, 3, 6
    key, frames = _frames(13, B, H, W)
    fr, k = frames.cuda(), key.cuda()
    init = _init(B, H // 8, W // 8, 7)
    mixed, low = eng.forward(fr, k, iters=iters, want_low=True, flow_init=init)
    for b in range(B):
        same, same_low = eng.forward(fr, k, iters=iters, want_low=True, flow_init=init[b:b + 1].repeat(B, 1, 1, 1).contiguous())
        assert torch.equal(mixed[b], same[b]) and torch.equal(low[b], same_low[b]), b
        if net == "small":                                           # (the small network's schedule is batch-size independent)
            assert torch.equal(mixed[b:b + 1], eng.forward(fr[b:b + 1], k, iters=iters, flow_init=init[b]))
    pairs = eng.forward_pairs(torch.cat([fr, k[None]]).contiguous(), list(range(B)), [B] * B, iters=iters, flow_init=init)
    if net == "small":
        assert torch.equal(pairs, mixed)
    else:                                # (the basic network's pair-list executor rounds its shared key frame differently)
        assert (pairs - mixed).abs().max().item() < 1e-3


def test_sliced_batch_takes_its_slice_of_the_init(cuda, raft_sd):
    from sd_animation_optical_flow_amd import _lib
    from sd_animation_optical_flow_amd.raft import RaftEngine
    B, H, W, iters = 5, 256, 192, 6
    key, frames = _frames(14, B, H, W)
    fr, k = frames.cuda(), key.cuda()
    init = _init(B, H // 8, W // 8, 8)
    whole = RaftEngine(raft_sd)
    ref_up, ref_low = whole.forward(fr, k, iters=iters, want_low=True, flow_init=init)
    eng = RaftEngine(raft_sd)
    eng.ws_budget_bytes = int(_lib.lib().ofx_raft_workspace_bytes(eng._h, 2, H, W))
    assert eng.pairs_that_fit(B, H, W) == 2
    up, low = eng.forward(fr, k, iters=iters, want_low=True, flow_init=init)
    assert (up - ref_up).abs().max().item() < 1e-3 and (low - ref_low).abs().max().item() < 1e-3
    cold = eng.forward(fr, k, iters=iters)
    assert (cold - ref_up).abs().max().item() > 1e-2                 # the slices really were warm


def test_split_modes_with_an_init_stay_inside_their_tolerances(cuda, raft_sd, basic):
    """The split-bf16 modes with a warm start, against the float64 restatement: bf16x3 inside the 1e-3 px bar, bf16x6 as close as the
    fp32 path (the tolerances of tests/test_gpu_raft.py's split-mode tests)."""
    from sd_animation_optical_flow_amd.raft import RaftEngine
    H, W, B, iters = 256, 384, 1, 12
    key, frames = _frames(15, B, H, W)
    fr, k = frames.cuda(), key.cuda()
    init = _init(B, H // 8, W // 8, 9)
    _, ref = WS.raft_forward_warm(raft_sd, frames.permute(0, 3, 1, 2).float(), key[None].permute(0, 3, 1, 2).float(),
                                  init.permute(0, 3, 1, 2).cpu(), iters)
    ref = ref.permute(0, 2, 3, 1)
    e32 = _epe(basic.forward(fr, k, iters=iters, flow_init=init).cpu(), ref)
    e3 = _epe(RaftEngine(raft_sd, precision="bf16x3").forward(fr, k, iters=iters, flow_init=init).cpu(), ref)
    e6 = _epe(RaftEngine(raft_sd, precision="bf16x6").forward(fr, k, iters=iters, flow_init=init).cpu(), ref)
    assert e32 < 1e-3 and 1e-6 < e3 < 1e-3 and e6 < 1e-3 and e6 < 4 * e32 + 2e-5, (e32, e3, e6)


@pytest.mark.parametrize("net", ["basic", "small"])
def test_padded_frames_take_the_init_on_the_padded_grid(request, raft_sd, small_sd, net):
    """132x156 frames pad to 136x160 (InputPadder): flow_init is [17, 20, 2], and the result is the warm forward of the padded pair."""
    from sd_animation_optical_flow_amd.raft import RaftEngine
    eng = request.getfixturevalue(net)
    key, frames = _frames(16, 1, 132, 156)
    init = _init(1, 17, 20, 10)
    up = eng.forward(frames.cuda(), key.cuda(), iters=6, flow_init=init)
    assert tuple(up.shape) == (1, 136, 160, 2)
    a, b = RaftEngine.pad_to_8(frames), RaftEngine.pad_to_8(key[None])
    assert torch.equal(up, eng.forward(a.cuda(), b.cuda(), iters=6, flow_init=init))
    with pytest.raises(RuntimeError):
        eng.forward(frames.cuda(), key.cuda(), iters=6, flow_init=_init(1, 16, 19, 10))   # the unpadded grid is refused
    a64, b64 = a.permute(0, 3, 1, 2).float(), b.permute(0, 3, 1, 2).float()
    i = init.permute(0, 3, 1, 2).cpu()
    _, ref = WS.raft_forward_warm(raft_sd, a64, b64, i, 6) if net == "basic" else WS.raft_small_forward_warm(small_sd, a64, b64, i, 6)
    assert _epe(up.cpu(), ref.permute(0, 2, 3, 1)) < 1e-3


def test_bad_flow_init_arguments(basic):
    from sd_animation_optical_flow_amd import _lib
    H, W, B = 128, 160, 2
    key, frames = _frames(17, B, H, W)
    fr, k = frames.cuda(), key.cuda()
    good = torch.zeros((B, H // 8, W // 8, 2), device="cuda")
    for bad in (good.cpu(), good.double(), good[:1], good[:, :-1], torch.zeros((B, H // 8, W // 8, 3), device="cuda"), good[0]):
        with pytest.raises(RuntimeError):
            basic.forward(fr, k, iters=2, flow_init=bad)
    images = torch.cat([fr, k[None]]).contiguous()
    with pytest.raises(RuntimeError):
        basic.forward_pairs(images, [0, 1], [2, 2], iters=2, flow_init=good[:1])             # one init for two pairs
    # the C ABI: the flag without flow_low
    ws = basic._workspace(B, H, W)
    up = torch.empty((B, H, W, 2), device="cuda")
    from sd_animation_optical_flow_amd.raft import FLAG_FLOW_INIT
    st = _lib.lib().ofx_raft_forward(basic._h, C.c_void_p(fr.data_ptr()), C.c_void_p(k.data_ptr()), B, H, W, 2, FLAG_FLOW_INIT | 2,
                                     C.c_void_p(up.data_ptr()), None, C.c_void_p(ws.data_ptr()), ws.numel(), None)
    assert st == -1, st                                                                   # OFX_EINVAL
    a1, a2 = (C.c_int * B)(0, 1), (C.c_int * B)(2, 2)
    need = _lib.lib().ofx_raft_workspace_bytes_pairs(basic._h, 3, B, H, W)
    wsp = torch.empty((need,), dtype=torch.uint8, device="cuda")
    st = _lib.lib().ofx_raft_forward_pairs(basic._h, C.c_void_p(images.data_ptr()), 3, a1, a2, B, H, W, 2, FLAG_FLOW_INIT,
                                           C.c_void_p(up.data_ptr()), None, C.c_void_p(wsp.data_ptr()), need, None)
    assert st == -1, st


# ---------------------------------------------------------------------------------------------------------- surface
def test_raft2_warm_start_chain(cuda, raft_sd, tmp_path):
    from sd_animation_optical_flow_amd import ofgen, ops
    from sd_animation_optical_flow_amd.raft import RaftEngine
    path = os.path.join(tmp_path, "raft.pth")
    torch.save(raft_sd, path)
    H, W = 128, 160
    key, frames = _frames(18, 3, H, W)
    seq = [key.numpy()] + [frames[b].numpy() for b in range(3)]            # "BGR" frames as cv2 hands them over
    warm = ofgen.RAFT_2(path, iters=6, warm_start=True)
    cold = ofgen.RAFT_2(path, iters=6)
    eng = RaftEngine(raft_sd, cnet_norm="batch")
    dev = lambda a: torch.from_numpy(a).cuda()[None]
    low = None
    for t in range(3):
        got = warm.calc(seq[t], seq[t + 1])
        init = None if low is None else ops.forward_interpolate(low)
        up, low = eng.forward(dev(seq[t]), dev(seq[t + 1]), iters=6, bgr=True, want_low=True, flow_init=init)
        assert np.array_equal(got, up[0].cpu().numpy()), t
        if t == 0:
            assert np.array_equal(got, cold.calc(seq[0], seq[1]))         # the first call is cold
    warm.reset()
    assert np.array_equal(warm.calc(seq[1], seq[2]), cold.calc(seq[1], seq[2]))
    small_a, small_b = seq[2][:, :128].copy(), seq[3][:, :128].copy()      # a size change starts cold
    assert np.array_equal(warm.calc(small_a, small_b), cold.calc(small_a, small_b))
