"""-m gpu: the small RAFT network (raft-small.pth) on the native engine.

Against the reference's own outputs (tests/golden/raft_small_ref_128x160.npz, tests/golden/make_golden_small.py) at 128x160, and
against the float64 restatement tests/small_raft_check.py at sizes the fixture does not cover (the project's bar: mean flow EPE
< 1e-3 px).  Plus the upflow8 kernels, bit-for-bit agreement of the engine's four entry points, the surface (RAFT_2, create_of_algo,
FrameSynthesizer) and the workspace / slicing logic.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import small_raft_check as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_small_ref_128x160.npz")


def _frames(seed, B, H, W):
    """Trackable synthetic frames: a blurred-noise key frame and B shifted copies (uint8 HWC)."""
    g = torch.Generator().manual_seed(seed)
    base = F.avg_pool2d(torch.rand((1, 3, H + 32, W + 32), generator=g), 5, 1, 2)
    base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)
    key = base[0, :, 16:16 + H, 16:16 + W].permute(1, 2, 0).contiguous()
    frames = []
    for b in range(B):
        dx, dy = (3 * b + 2) % 7 - 3, (5 * b + 1) % 5 - 2
        frames.append(base[0, :, 16 + dy:16 + dy + H, 16 + dx:16 + dx + W].permute(1, 2, 0).contiguous())
    return key, torch.stack(frames)


def _epe(a, b):
    return (a.double() - b.double()).pow(2).sum(-1).sqrt().mean().item()


@pytest.fixture(scope="module")
def small_sd():
    from sd_animation_optical_flow_amd.weights import random_state_dict
    return random_state_dict(0, small=True)


@pytest.fixture(scope="module")
def small(cuda, small_sd):
    from sd_animation_optical_flow_amd.raft import RaftEngine
    return RaftEngine(small_sd)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def test_engine_reports_the_small_variant(small, cuda):
    from sd_animation_optical_flow_amd import _lib
    from sd_animation_optical_flow_amd.raft import RaftEngine
    from sd_animation_optical_flow_amd.weights import random_state_dict
    assert small.variant == "small" and _lib.lib().ofx_raft_variant(small._h) == 1
    basic = RaftEngine(random_state_dict(0))
    assert basic.variant == "basic" and _lib.lib().ofx_raft_variant(basic._h) == 0


def test_stages_and_final_flow_against_the_reference_fixture(small, gold):
    """Feature maps, context, the radius-3 lookups (integer coordinates inside the forward; fractional and far ones through the
    engine's own pyramid), one update step (h and delta), and the 20-iteration flow of the reference small network."""
    from sd_animation_optical_flow_amd import ops
    i1 = torch.from_numpy(gold["image1"][0]).permute(1, 2, 0).contiguous().cuda()[None]
    i2 = torch.from_numpy(gold["image2"][0]).permute(1, 2, 0).contiguous().cuda()[None]
    H, W = i1.shape[1:3]
    h, w = H // 8, W // 8
    up, lo = small.forward(i1, i2, iters=1, want_low=True)
    nhwc = lambda a: torch.from_numpy(a.astype(np.float32)).permute(0, 2, 3, 1).reshape(-1)
    for nm in ("fmap1", "fmap2"):
        ref = nhwc(gold[nm + "_f16"])
        assert (small.buffer(nm).cpu() - ref).abs().max().item() < 2e-3 * max(1.0, ref.abs().max().item()), nm   # (f16 fixture)
    hx = small.buffer("hx").cpu().reshape(h * w, 256)
    assert (hx[:, 96:160] - nhwc(gold["inp_f16"]).reshape(-1, 64)).abs().max().item() < 2e-3
    assert (hx[:, :96] - nhwc(gold["update_net1_f16"]).reshape(-1, 96)).abs().max().item() < 2e-3   # h after one update
    assert hx[:, 242:].abs().max().item() == 0.0                                                  # the pad columns stay zero
    corr = small.buffer("corr").cpu().reshape(h, w, 224)
    ref = torch.from_numpy(gold["lookup_int"][0]).permute(1, 2, 0)
    assert (corr[::3, ::3, :196] - ref).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item())
    assert corr[:, :, 196:].abs().max().item() == 0.0
    d1 = torch.from_numpy(gold["update_delta1"][0]).permute(1, 2, 0)
    assert (lo[0].cpu() - d1).abs().max().item() < 1e-4                                         # flow after one step = delta
    # the lookup at fractional / far coordinates on the engine's pyramid (the forward above left it in the workspace)
    pyr = [small.buffer(f"pyr{l}").cuda() for l in range(4)]
    c0 = torch.stack(torch.meshgrid(torch.arange(w).float(), torch.arange(h).float(), indexing="xy"), -1)[None]
    jit = torch.from_numpy(gold["lookup_jitter"]).permute(0, 2, 3, 1)
    for nm, s in (("frac", 5.0), ("far", 60.0)):
        out = ops.corr_lookup(pyr, (c0 + jit * s).contiguous().cuda(), 1, h, w, radius=3)[0].cpu()
        ref = torch.from_numpy(gold["lookup_" + nm][0]).permute(1, 2, 0)
        assert (out[::3, ::3] - ref).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item()), nm
    up, lo = small.forward(i1, i2, iters=20, want_low=True)
    ref_up = torch.from_numpy(gold["flow_up"]).permute(0, 2, 3, 1)
    ref_lo = torch.from_numpy(gold["flow_low"]).permute(0, 2, 3, 1)
    e_up, e_lo = _epe(up.cpu(), ref_up), _epe(lo.cpu(), ref_lo)
    print(f"small net vs reference at 128x160: flow_up EPE {e_up:.3e}, flow_low {e_lo:.3e} px")
    assert e_up <= 1e-4 and e_lo <= 1e-4 / 8 * 2


def test_upflow8_of_a_known_flow_against_the_reference(cuda, gold):
    from sd_animation_optical_flow_amd import ops
    flow = torch.from_numpy(gold["upflow8_in"])
    B, _, h, w = flow.shape
    coords = (flow + SR.coords_grid(B, h, w, torch.float32)).permute(0, 2, 3, 1).contiguous().cuda()
    out = ops.upflow8(coords).cpu()
    ref = torch.from_numpy(gold["upflow8_out"]).permute(0, 2, 3, 1)
    assert (out - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("H,W,B", [(264, 392, 3), (512, 768, 2)])
def test_against_the_float64_restatement_off_the_fixture(small, small_sd, H, W, B):
    key, frames = _frames(3 + B, B, H, W)
    up, lo = small.forward(frames.cuda(), key.cuda(), iters=20, want_low=True)
    img2 = key.permute(2, 0, 1)[None].repeat(B, 1, 1, 1)
    lo_r, up_r = SR.raft_small_forward(small_sd, frames.permute(0, 3, 1, 2), img2, 20)
    e_up, e_lo = _epe(up.cpu(), SR.nhwc(up_r)), _epe(lo.cpu(), SR.nhwc(lo_r))
    print(f"small net vs float64 at {H}x{W} B={B}: flow_up EPE {e_up:.3e} px, flow_low {e_lo:.3e}")
    assert e_up < 1e-3 and e_lo < 1e-3 / 8 * 2


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 5), (3, 7, 1), (2, 5, 9), (4, 16, 24), (5, 12, 9)])
def test_upflow8_kernel_against_interpolate(cuda, shape):
    from sd_animation_optical_flow_amd import ops
    B, h, w = shape
    g = torch.Generator().manual_seed(B * 100 + h * 10 + w)
    flow = (torch.rand((B, 2, h, w), generator=g) - 0.5) * 20.0
    coords = (flow + SR.coords_grid(B, h, w, torch.float32)).permute(0, 2, 3, 1).contiguous().cuda()
    out = ops.upflow8(coords).cpu()
    ref = SR.nhwc(SR.upflow8(flow.double()))
    assert tuple(out.shape) == (B, 8 * h, 8 * w, 2)
    assert (out.double() - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("shape", [(4, 16, 24), (5, 12, 9), (6, 17, 10), (2, 17, 10), (1, 8, 8)])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_upflow8_with_the_warp_inside_is_the_two_kernels_bit_for_bit(cuda, shape, sign):
    """`ofx_upflow8_warp` = `ofx_upflow8` then the bilinear `ofx_warp_u8` of one shared frame, flows that leave the frame included."""
    from sd_animation_optical_flow_amd import ops
    B, h, w = shape
    g = torch.Generator().manual_seed(41)
    coords = SR.coords_grid(B, h, w, torch.float32) + (torch.rand((B, 2, h, w), generator=g) - 0.5) * 9.0
    coords[0, :, 0, 0] += 500.0                                            # far outside: zeros padding
    c = coords.permute(0, 2, 3, 1).contiguous().cuda()
    frame = torch.randint(0, 256, (8 * h, 8 * w, 3), generator=g, dtype=torch.uint8).cuda()
    flow_ref = ops.upflow8(c)
    warped_ref = ops.warp(frame, flow_ref, mode="bilinear", sign=sign)
    flow, warped = ops.upflow8_warp(c, frame, sign=sign)
    assert torch.equal(flow, flow_ref)
    if B >= 4:      # `ofx_warp_u8` hands batches of >= 4 frames to the shared-key-frame kernel whose sampling function the fused kernel calls
        assert torch.equal(warped, warped_ref)
    else:           # smaller batches take the generic bilinear kernel (weights form, contraction off): 1 LSB apart on rounding ties only
        d = (warped.int() - warped_ref.int()).abs()
        assert d.max().item() <= 1 and (d > 0).float().mean().item() < 1e-3
    none, warped2 = ops.upflow8_warp(c, frame, sign=sign, want_flow=False)
    assert none is None and torch.equal(warped2, warped)


def test_the_four_entry_points_agree_bit_for_bit(small):
    """forward (shared key frame / repeated key frame / one pair at a time), forward(warp_frame=), forward_pairs and
    forward_pairs(warp_frame=) on the same pairs: one arithmetic."""
    from sd_animation_optical_flow_amd import ops
    H, W, B = 128, 160, 3
    key, frames = _frames(11, B, H, W)
    fr, k = frames.cuda(), key.cuda()
    key_ai = (255 - k).contiguous()
    shared = small.forward(fr, k, iters=12)
    repeated = small.forward(fr, k[None].repeat(B, 1, 1, 1).contiguous(), iters=12)
    single = torch.cat([small.forward(fr[b:b + 1], k[None], iters=12) for b in range(B)])
    assert torch.equal(shared, repeated) and torch.equal(shared, single)
    wflow, warped = small.forward(fr, k, iters=12, warp_frame=key_ai)
    assert torch.equal(wflow, shared)
    assert torch.equal(warped, ops.warp(key_ai, shared, mode="bilinear", sign=1.0))
    none, warped_nf = small.forward(fr, k, iters=12, warp_frame=key_ai, want_flow=False)
    assert none is None and torch.equal(warped_nf, warped)
    images = torch.cat([fr, k[None]]).contiguous()
    pairs = small.forward_pairs(images, [0, 1, 2], [3, 3, 3], iters=12)
    assert torch.equal(pairs, shared)
    pflow, pwarped = small.forward_pairs(images, [0, 1, 2, 3], [3, 3, 3, 0], iters=12, warp_frame=key_ai, n_warp=3)
    assert torch.equal(pflow[:3], shared) and torch.equal(pwarped, warped)
    back = small.forward(k[None], fr[:1], iters=12)
    assert torch.equal(pflow[3:], back)
    # shared image1 against repeated image1
    s1 = small.forward(k, fr, iters=12)
    r1 = small.forward(k[None].repeat(B, 1, 1, 1).contiguous(), fr, iters=12)
    assert torch.equal(s1, r1)


def test_bgr_flag(small):
    H, W = 128, 160
    key, frames = _frames(12, 2, H, W)
    rgb = small.forward(frames.cuda(), key.cuda(), iters=6)
    bgr = small.forward(frames.flip(-1).contiguous().cuda(), key.flip(-1).contiguous().cuda(), iters=6, bgr=True)
    assert torch.equal(rgb, bgr)


def test_alternate_corr_against_the_volume_and_the_fixture(small, gold):
    i1 = torch.from_numpy(gold["image1"][0]).permute(1, 2, 0).contiguous().cuda()[None]
    i2 = torch.from_numpy(gold["image2"][0]).permute(1, 2, 0).contiguous().cuda()[None]
    vol = small.forward(i1, i2, iters=20)
    alt = small.forward(i1, i2, iters=20, alternate_corr=True)
    ref = torch.from_numpy(gold["flow_up_alt"]).permute(0, 2, 3, 1)
    e_vol, e_ref = _epe(alt.cpu(), vol.cpu()), _epe(alt.cpu()[:, ::2, ::2], ref)
    print(f"small net alternate corr: {e_vol:.3e} px from the volume path, {e_ref:.3e} px from the reference's alt-corr flow")
    assert e_vol <= 1e-4 and e_ref <= 1e-4


def test_raft2_and_create_of_algo_load_a_small_checkpoint(cuda, small_sd, gold, tmp_path):
    """A raft-small-shaped .pth (DataParallel `module.` keys) through the reference's two entry points, with no other argument."""
    from sd_animation_optical_flow_amd import ofgen, pdcnet_of
    path = str(tmp_path / "raft-small.pth")
    torch.save({"module." + k: v for k, v in small_sd.items()}, path)
    r2 = ofgen.RAFT_2(model=path)
    assert r2.model.variant == "small"
    flow = r2.calc(gold["raft2_frame1"], gold["raft2_frame2"])       # BGR frames, padded to 136x160, not un-padded (as RAFT_2)
    assert flow.shape == gold["raft2_flow"].shape and flow.dtype == np.float32
    e = float(np.sqrt(((flow - gold["raft2_flow"]) ** 2).sum(-1)).mean())
    print(f"RAFT_2(raft-small) vs the reference driven the same way: EPE {e:.3e} px")
    assert e <= 1e-4

    algo = pdcnet_of.create_of_algo(path)
    assert algo.network.variant == "small"
    key, frames = _frames(5, 3, 96, 128)
    f1, f2 = key.numpy(), frames[0].numpy()
    flow, conf, logc = algo.calc(f1, f2)
    assert flow.shape == (96, 128, 2) and flow.dtype == np.float32
    assert conf.shape == (96, 128) and conf.dtype == np.float32 and logc.shape == (96, 128)
    assert conf.min() >= 0 and conf.max() <= 1
    src = torch.from_numpy(np.stack([f1[:, :, ::-1], f2[:, :, ::-1]]).copy()).cuda()
    tgt = torch.from_numpy(np.stack([f2[:, :, ::-1], f1[:, :, ::-1]]).copy()).cuda()
    fe, ce = algo.calc_batch(src, tgt)
    assert np.abs(fe[0] - flow).max() < 1e-4 and np.abs(ce[0] - conf).max() < 1e-4
    kd, fd = key.cuda(), frames.cuda()
    kai = (255 - kd).contiguous()
    fl, cf, _, wp = algo.calc_batch_device(kd, fd, warp_frame=kai)
    fl2, cf2, _ = algo.calc_batch_device(kd, fd)
    assert torch.equal(fl, fl2) and torch.equal(cf, cf2)
    from sd_animation_optical_flow_amd import ops
    assert torch.equal(wp, ops.warp(kai, fl.contiguous(), mode="bilinear", sign=1.0))
    pf, pc = algo.calc_pairs(torch.cat([fd, kd[None]]).contiguous(), [(3, 0), (3, 1)])[:2]
    assert (pf - fl[:2]).abs().max().item() < 1e-3
    assert algo.to(torch.device("cuda:0")) is algo


def test_frame_synthesizer_on_a_small_engine_and_algo(small, small_sd):
    from sd_animation_optical_flow_amd import clip, ops, pdcnet_of
    H, W, T = 96, 128, 3
    key, frames = _frames(9, T, H, W)
    kd, fd = key.cuda(), frames.cuda()
    kai = (255 - kd).contiguous()
    conf = torch.rand((T, H, W), generator=torch.Generator().manual_seed(4)).cuda()
    eng = clip.FrameSynthesizer(engine=small, warp_mode="bilinear", thres=0.9, ksize=7)
    f3, w3, m3 = eng(fd, kd, kai, confidence=conf)
    assert torch.equal(f3, small.forward(fd, kd, iters=20))
    assert torch.equal(w3, ops.warp(kai, f3.contiguous(), mode="bilinear", sign=1.0))
    algo = pdcnet_of.create_of_algo(small_sd)
    fused = clip.FrameSynthesizer(algo, warp_mode="bilinear", thres=0.9, ksize=7)
    plain = clip.FrameSynthesizer(algo, warp_mode="bilinear", thres=0.9, ksize=7, fuse_warp=False)
    a = fused.synthesize(fd, kd, kai)
    b = plain.synthesize(fd, kd, kai)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_split_precisions_are_refused_for_the_small_network(cuda, small_sd):
    from sd_animation_optical_flow_amd.raft import RaftEngine
    for kw in ({"volume_precision": "bf16x6"}, {"volume_precision": "bf16x3"}, {"precision": "bf16x3"}, {"precision": "bf16x6"}):
        with pytest.raises(ValueError):
            RaftEngine(small_sd, **kw)
    e = RaftEngine(small_sd, cnet_norm="batch")        # no BatchNorm: the switch changes nothing
    key, frames = _frames(2, 1, 128, 160)
    e2 = RaftEngine(small_sd)
    assert torch.equal(e.forward(frames.cuda(), key.cuda(), iters=4), e2.forward(frames.cuda(), key.cuda(), iters=4))


def test_workspace_and_slicing(small, cuda):
    from sd_animation_optical_flow_amd import _lib
    from sd_animation_optical_flow_amd.raft import RaftEngine
    from sd_animation_optical_flow_amd.weights import random_state_dict
    L = _lib.lib()
    basic = RaftEngine(random_state_dict(0))
    for B in (1, 16, 64):
        s, b = L.ofx_raft_workspace_bytes(small._h, B, 512, 768), L.ofx_raft_workspace_bytes(basic._h, B, 512, 768)
        assert 0 < s < b
        sp, bp = L.ofx_raft_workspace_bytes_pairs(small._h, B + 1, B, 512, 768), L.ofx_raft_workspace_bytes_pairs(basic._h, B + 1, B, 512, 768)
        assert 0 < sp < bp
    assert (small.pairs_per_call(512, 768), basic.pairs_per_call(512, 768), RaftEngine.max_pairs(512, 768)) == (341, 113, 113)
    H, W, B = 128, 160, 3
    key, frames = _frames(13, B, H, W)
    whole = small.forward(frames.cuda(), key.cuda(), iters=8)
    eng = RaftEngine(random_state_dict(0, small=True))
    eng.ws_budget_bytes = int(L.ofx_raft_workspace_bytes(eng._h, 1, H, W))
    assert eng.pairs_that_fit(B, H, W) == 1
    sliced = eng.forward(frames.cuda(), key.cuda(), iters=8)
    assert torch.equal(sliced, whole)
    assert eng._ws.numel() < L.ofx_raft_workspace_bytes(eng._h, 2, H, W)


def test_the_c_side_refuses_mixed_and_partial_dicts(cuda, small_sd):
    """`ofx_raft_create` checks the key set again, whatever the Python side did: OFX_EKEY for keys of both networks or a missing key."""
    import ctypes as C
    from sd_animation_optical_flow_amd import _lib
    from sd_animation_optical_flow_amd.weights import random_state_dict
    L = _lib.lib()

    def create(sd):
        keep, arr = [], (_lib.Tensor * len(sd))()
        for n, (k, v) in enumerate(sd.items()):
            t = v.detach().float().contiguous()
            keep.append(t)
            arr[n].name, arr[n].data, arr[n].ndim = k.encode(), t.data_ptr(), t.dim()
            for j in range(4):
                arr[n].shape[j] = t.shape[j] if j < t.dim() else 1
        h = C.c_void_p()
        rc = L.ofx_raft_create(arr, len(sd), C.byref(h))
        if rc == 0:
            L.ofx_raft_destroy(h)
        return rc

    basic = {k: v for k, v in random_state_dict(0).items() if v.dtype.is_floating_point}
    ekey = create({"no.such.weight": torch.zeros(4)})          # what the engine has always answered for a dict it cannot use
    assert ekey < 0
    assert create(dict(small_sd)) == 0 and create(basic) == 0
    mixed = dict(small_sd)
    mixed["update_block.mask.0.weight"] = basic["update_block.mask.0.weight"]
    assert create(mixed) == ekey
    mixed2 = dict(basic)
    mixed2["fnet.layer1.0.conv3.weight"] = small_sd["fnet.layer1.0.conv3.weight"]
    assert create(mixed2) == ekey
    assert create({k: v for k, v in small_sd.items() if k != "update_block.gru.convq.bias"}) == ekey
