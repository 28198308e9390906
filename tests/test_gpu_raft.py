"""-m gpu: end-to-end parity of the native RAFT engine against the CPU oracle (same seeded weights).

Bar (BASELINE.json north_star): flow EPE <= 1e-3 px vs the reference on identical inputs.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import raft_oracle as RO


def _frames(seed, B, H, W, smooth=True):
    """Synthetic trackable frames: blurred noise key frame, frames = key frame shifted by a smooth field."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((1, 3, H + 32, W + 32), generator=g)
    if smooth:
        k = torch.ones((3, 1, 5, 5)) / 25.0
        base = torch.nn.functional.conv2d(base, k, padding=2, groups=3)
        base = (base - base.min()) / (base.max() - base.min())
    key = (base[0, :, 16:16 + H, 16:16 + W] * 255).round().to(torch.uint8)
    frames = []
    for b in range(B):
        dx, dy = (3 * b + 2) % 7 - 3, (5 * b + 1) % 5 - 2
        f = (base[0, :, 16 + dy:16 + dy + H, 16 + dx:16 + dx + W] * 255).round().to(torch.uint8)
        frames.append(f)
    to_hwc = lambda t: t.permute(1, 2, 0).contiguous()
    return to_hwc(key), torch.stack([to_hwc(f) for f in frames])


def _oracle_flow(sd, img1_hwc, img2_hwc, iters, trace=None, alt=False):
    a = img1_hwc.permute(0, 3, 1, 2).float()
    b = img2_hwc.permute(0, 3, 1, 2).float()
    lo, up = RO.raft_forward(sd, a, b, iters=iters, trace=trace, alternate_corr=alt)
    return lo.permute(0, 2, 3, 1).contiguous(), up.permute(0, 2, 3, 1).contiguous()


def _epe(a, b):
    return (a - b).pow(2).sum(-1).sqrt().mean().item()


@pytest.fixture(scope="module")
def engine(cuda, raft_sd):
    from sd_animation_optical_flow_amd.raft import RaftEngine
    return RaftEngine(raft_sd)


def test_stage_parity_one_iteration(engine, raft_sd):
    """Every stage buffer after a 1-iteration forward: feature maps, context, pyramid, lookup, GRU state."""
    H, W, B = 128, 160, 2
    key, frames = _frames(1, B, H, W)
    img2 = key[None].repeat(B, 1, 1, 1)
    tr = {}
    lo_ref, up_ref = _oracle_flow(raft_sd, frames, img2, 1, trace=tr)
    up, lo = engine.forward(frames.cuda(), img2.cuda(), iters=1, want_low=True)
    h, w = H // 8, W // 8
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1)
    fm1 = engine.buffer("fmap1").cpu()
    assert (fm1 - nhwc(tr["fmap1"])).abs().max().item() < 2e-4
    fm2 = engine.buffer("fmap2").cpu()
    assert (fm2 - nhwc(tr["fmap2"])).abs().max().item() < 2e-4
    for l in range(4):
        from sd_animation_optical_flow_amd import ops
        p = ops.corr_unblock(engine.buffer(f"pyr{l}"), h >> l, w >> l).cpu()      # 4x8-blocked slices -> [M, h_l, w_l]
        assert (p.reshape(-1) - tr["pyramid"][l].reshape(-1)).abs().max().item() < 5e-4, l
    hx = engine.buffer("hx").cpu().reshape(B * h * w, 384)
    # hx row layout: [h(128) | motion(126) flow(2) | inp(128)]
    assert (hx[:, 256:384] - tr["inp"].permute(0, 2, 3, 1).reshape(-1, 128)).abs().max().item() < 2e-4
    assert (hx[:, 254:256] - lo_ref.reshape(-1, 2)).abs().max().item() < 2e-4     # flow slot = coords1 - coords0
    assert (hx[:, :128] - tr["net_it0"].permute(0, 2, 3, 1).reshape(-1, 128)).abs().max().item() < 5e-4
    mask = engine.buffer("mask").cpu()
    assert (mask - nhwc(tr["mask"])).abs().max().item() < 1e-3
    assert (lo.cpu() - lo_ref).abs().max().item() < 2e-4
    assert _epe(up.cpu(), up_ref) < 1e-3
    corr = engine.buffer("corr").cpu().reshape(-1, 336)              # rows of 336: 324 features + 12 zeros (convc1's whole chunks)
    assert (corr[:, :324].reshape(-1) - nhwc(tr["corr_it0"]).reshape(-1)).abs().max().item() < 5e-4
    assert not corr[:, 324:].any()


@pytest.mark.parametrize("H, W, B", [(128, 160, 2), (512, 768, 8)])
def test_stage_parity_two_iterations(engine, raft_sd, H, W, B):
    """The second iteration is the first to read what the flow head leaves behind: convf1's 16-float flow rows (frows) and the flow
    slot of hx.  The flow after iteration 2, from the engine's coords1, elementwise and on the border ring of the 1/8 map on its own
    (where a wrong or missing frows slot would sit).  B = 8 at 512x768: the flow head's four-wave launch (1536 strips) and the
    Winograd routes of the update block.  Measured on MI355X: 3.8e-6 (ring 1.9e-6) at 2 x 128x160, 1.5e-5 (ring 7.6e-6) at
    8 x 512x768, against the 2e-4 bar of the one-iteration test."""
    key, frames = _frames(5, B, H, W)
    img2 = key[None].repeat(B, 1, 1, 1)
    tr = {"keep_iters": (2,)}
    _oracle_flow(raft_sd, frames, img2, 2, trace=tr)
    engine.forward(frames.cuda(), img2.cuda(), iters=2)
    h, w = H // 8, W // 8
    ref = tr["flow_low_at"][2].permute(0, 2, 3, 1)
    grid = RO.coords_grid(B, h, w).permute(0, 2, 3, 1)
    flow = engine.buffer("coords1").cpu().reshape(B, h, w, 2) - grid
    hx = engine.buffer("hx").cpu().reshape(B, h, w, 384)
    assert torch.equal(hx[..., 254:256], flow)                           # the flow slot is coords1 - grid, bit for bit
    err = (flow - ref).abs()
    ring = torch.zeros((h, w), dtype=torch.bool)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
    worst, worst_ring = err.max().item(), err[:, ring].max().item()
    print(f"two iterations {B}x{H}x{W}: max |flow - oracle| {worst:.3g}, border ring {worst_ring:.3g}")
    assert worst < 2e-4 and worst_ring < 2e-4, (worst, worst_ring)


@pytest.mark.parametrize("H,W,B", [(128, 160, 3), (200, 136, 1)])
def test_full_flow_epe_small(engine, raft_sd, H, W, B):
    key, frames = _frames(2, B, H, W)
    img2 = key[None].repeat(B, 1, 1, 1)
    _, up_ref = _oracle_flow(raft_sd, frames, img2, 20)
    up = engine.forward(frames.cuda(), img2.cuda(), iters=20)
    epe = _epe(up.cpu(), up_ref)
    assert epe < 1e-3, epe
    assert (up.cpu() - up_ref).abs().max().item() < 2e-2
    # shared key frame (zero batch stride in the correlation GEMM) == the replicated batch.  Not bit for bit: the key
    # frame is encoded alone instead of in a batch of B, and the launcher picks tiles / K splits by problem size, so
    # the fp32 summation order inside its convolutions differs; identical calls do repeat exactly
    up_sh = engine.forward(frames.cuda(), key.cuda(), iters=20)
    assert (up_sh - up).abs().max().item() < 1e-4
    assert torch.equal(up_sh, engine.forward(frames.cuda(), key.cuda(), iters=20))


def test_config_c1_256x384_pair(engine, raft_sd):
    """BASELINE config #1 shape (W=256, H=384), one pair, 20 iterations, BGR entry like RAFT_2.calc."""
    H, W = 384, 256
    key, frames = _frames(3, 1, H, W)
    _, up_ref = _oracle_flow(raft_sd, frames, key[None], 20)
    up = engine.forward(frames.flip(-1).contiguous().cuda(), key.flip(-1).contiguous().cuda()[None], iters=20, bgr=True)
    assert _epe(up.cpu(), up_ref) < 1e-3


def test_headline_size_512x768_pair_against_the_oracle(engine, raft_sd):
    """The bench workload's frame size, 20 iterations, one pair: EPE against the CPU oracle (about a second of CPU)."""
    H, W = 768, 512
    key, frames = _frames(8, 1, H, W)
    _, up_ref = _oracle_flow(raft_sd, frames, key[None], 20)
    up = engine.forward(frames.cuda(), key.cuda(), iters=20)
    assert _epe(up.cpu(), up_ref) < 1e-3


def test_alternate_corr_engine_path(engine, raft_sd):
    H, W, B = 128, 128, 2
    key, frames = _frames(4, B, H, W)
    img2 = key[None].repeat(B, 1, 1, 1)
    _, up_ref = _oracle_flow(raft_sd, frames, img2, 6)
    up = engine.forward(frames.cuda(), img2.cuda(), iters=6, alternate_corr=True)
    assert _epe(up.cpu(), up_ref) < 1e-3


def test_alternate_corr_path_keeps_the_pad_columns_of_the_feature_rows_zero(engine):
    """On the volume-free path the 12 pad columns of the lookup's 336-float rows are zeroed ONCE in front of the loop (the local
    correlation writes 324 of them) and `convc1` multiplies them by zero weights every iteration -- 0 * NaN would be NaN, so nothing
    may ever write there.  After 7 iterations on a workspace that was poisoned beforehand: columns 324.. are exactly zero, the
    features in front of them are finite and not all zero (round-5 ADVICE)."""
    H, W, B = 128, 128, 2
    key, frames = _frames(9, B, H, W)
    img2 = key[None].repeat(B, 1, 1, 1)
    engine.forward(frames.cuda(), img2.cuda(), iters=2, alternate_corr=True)          # sizes the workspace
    engine._ws.view(torch.float32)[: engine._ws.numel() // 4].fill_(float("nan"))     # stale contents of the worst kind
    up = engine.forward(frames.cuda(), img2.cuda(), iters=7, alternate_corr=True)
    assert torch.isfinite(up).all()
    corr = engine.buffer("corr").view(-1, 336)
    assert corr.shape[0] == B * (H // 8) * (W // 8)
    assert torch.equal(corr[:, 324:], torch.zeros_like(corr[:, 324:]))
    assert torch.isfinite(corr[:, :324]).all() and corr[:, :324].abs().sum() > 0


def test_forward_pairs_encodes_each_image_once(engine, raft_sd):
    """Indexed pairs (KeyframeConv's N x N sweep): same flows as the pair-by-pair forward and the oracle."""
    H, W = 128, 160
    key, frames = _frames(7, 3, H, W)
    imgs = torch.cat([key[None], frames])                    # 4 distinct images
    idx1, idx2 = [1, 2, 3, 0, 2, 3], [0, 0, 1, 3, 2, 2]      # includes an identity pair and both directions
    out = engine.forward_pairs(imgs.cuda(), idx1, idx2, iters=8)
    ref = engine.forward(imgs[idx1].contiguous().cuda(), imgs[idx2].contiguous().cuda(), iters=8)
    assert (out - ref).abs().max().item() < 1e-4
    _, up_ref = _oracle_flow(raft_sd, imgs[idx1], imgs[idx2], 8)
    assert _epe(out.cpu(), up_ref) < 1e-3
    with pytest.raises(RuntimeError):
        engine.forward_pairs(imgs.cuda(), [0, 9], [1, 1])    # index out of range -> OFX_EINVAL


def test_bf16x3_fast_mode_stays_inside_the_epe_bar(cuda, raft_sd):
    """The opt-in split-bf16 mode: flow EPE vs the fp32 oracle must stay below the 1e-3 px parity bar."""
    from sd_animation_optical_flow_amd.raft import RaftEngine
    fast = RaftEngine(raft_sd, precision="bf16x3")
    for (H, W, B, seed) in ((128, 160, 2, 11), (256, 384, 1, 12)):
        key, frames = _frames(seed, B, H, W)
        _, up_ref = _oracle_flow(raft_sd, frames, key[None].repeat(B, 1, 1, 1), 20)
        up = fast.forward(frames.cuda(), key.cuda(), iters=20)
        epe = _epe(up.cpu(), up_ref)
        assert epe < 1e-3, epe
        assert epe > 1e-6            # not the fp32 path by accident


def test_bf16x6_mode_matches_fp32_to_rounding_level(cuda, raft_sd, engine):
    """Three-piece split-bf16 arithmetic: the flow must sit as close to the oracle as the native fp32 path does."""
    from sd_animation_optical_flow_amd.raft import RaftEngine
    six = RaftEngine(raft_sd, precision="bf16x6")
    for (H, W, B, seed) in ((128, 160, 2, 11), (256, 384, 1, 12)):
        key, frames = _frames(seed, B, H, W)
        _, up_ref = _oracle_flow(raft_sd, frames, key[None].repeat(B, 1, 1, 1), 20)
        up6 = six.forward(frames.cuda(), key.cuda(), iters=20)
        up32 = engine.forward(frames.cuda(), key.cuda(), iters=20)
        e6, e32 = _epe(up6.cpu(), up_ref), _epe(up32.cpu(), up_ref)
        assert e6 < 1e-3 and e6 < 4 * e32 + 2e-5, (e6, e32)
        assert not torch.equal(up6, up32)


def test_non_multiple_of_8_is_padded_like_input_padder(engine, raft_sd):
    H, W = 100, 90
    key, frames = _frames(5, 1, H, W)
    ref = RO.raft2_calc(raft_sd, frames[0].flip(-1).numpy(), key.flip(-1).numpy(), iters=4, cnet_norm="eval")
    up = engine.forward(frames.flip(-1).contiguous().cuda(), key.flip(-1).contiguous().cuda()[None], iters=4, bgr=True)
    assert tuple(up.shape[1:3]) == ref.shape[:2] == (104, 96)      # the reference does not un-pad
    assert _epe(up[0].cpu(), torch.from_numpy(ref)) < 1e-3


@pytest.mark.parametrize("B", [3, 24])
def test_batch_consistency_512x768(engine, B):
    """Full BASELINE size: a pair's flow must not depend on its batch neighbours or position
    (each pair is an independent unit -- the property frame-parallel sharding relies on).  B = 24 also crosses
    the launcher's tile thresholds: the batch runs the 128x128 / 128x192 / 128x96 tiles and their GRU epilogues,
    the single pair the 64x64 paired-pipeline tiles that the oracle tests validate -- the two must agree."""
    H, W = 768, 512
    key, frames = _frames(6, B, H, W)
    up = engine.forward(frames.cuda(), key.cuda(), iters=3)
    assert torch.isfinite(up).all()
    for b in sorted({1, B - 1}):
        single = engine.forward(frames[b:b + 1].cuda(), key.cuda(), iters=3)
        assert (up[b:b + 1] - single).abs().max().item() < 1e-4, b


def test_small_batch_stream_overlap_is_bit_identical_to_serial(engine):
    """B <= 5 at 512x768 runs the three encoders and the two motion-encoder branches on side streams; the
    kernels and their arithmetic are the same, so the flow must be bit-identical to the one-stream schedule,
    also when calls alternate back to back (the side streams are joined before the call returns)."""
    for (H, W, B, seed) in ((384, 512, 1, 21), (768, 512, 2, 22)):
        key, frames = _frames(seed, B, H, W)
        a, k = frames.cuda(), key.cuda()
        ser = engine.forward(a, k, iters=12, serial=True)
        for _ in range(3):
            ovl = engine.forward(a, k, iters=12)
            assert torch.equal(ovl, ser)
        both = engine.forward(a, a.flip(0).contiguous(), iters=5)            # per-pair image2: third encoder chain
        assert torch.equal(both, engine.forward(a, a.flip(0).contiguous(), iters=5, serial=True))
    out = engine.forward_pairs(torch.cat([key[None], frames]).cuda(), [1, 0], [0, 2], iters=6)
    assert torch.isfinite(out).all()


def test_small_grids_repeat_bit_for_bit(engine):
    """Split-K exchanges partial tiles between workgroups: a missing visibility wait shows up as run-to-run noise
    (it did, once: a workgroup-scope release fence does not wait for the stores on this target).  Identical calls
    must repeat exactly, in both schedules, at shapes where every layer of the update block is split."""
    g = torch.Generator(device="cuda").manual_seed(0)
    for (B, H, W, it) in ((2, 336, 280, 12), (3, 128, 160, 8), (1, 384, 256, 6)):
        a = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        k = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        for serial in (False, True):
            ref = engine.forward(a, k, iters=it, serial=serial).clone()
            for _ in range(12):
                assert torch.equal(engine.forward(a, k, iters=it, serial=serial), ref), (B, H, W, serial)


def test_a_batch_larger_than_the_memory_budget_runs_in_slices(cuda, raft_sd):
    """The executor's workspace grows with (H/8 x W/8)^2 per pair (the correlation pyramid).  RaftEngine.pairs_that_fit slices a
    batch that would not fit the free device memory; here the budget is forced down to three pairs' worth: same flows (pairs are
    independent; small and large grids differ by rounding only), and the slices really were taken."""
    from sd_animation_optical_flow_amd.raft import RaftEngine
    import bench
    B, H, W = 8, 256, 192
    frames, key, _, _ = bench.make_clip(B, H, W, torch.device("cuda"))
    whole = RaftEngine(raft_sd)
    ref = whole.forward(frames, key, iters=6)
    eng = RaftEngine(raft_sd)
    from sd_animation_optical_flow_amd import _lib
    need3 = _lib.lib().ofx_raft_workspace_bytes(eng._h, 3, H, W)
    eng.ws_budget_bytes = int(need3)
    assert eng.pairs_that_fit(B, H, W) == 3 and eng.pairs_that_fit(2, H, W) == 2
    out = eng.forward(frames, key, iters=6)
    assert eng._ws.numel() <= need3                                   # never allocated more than the budget
    assert tuple(out.shape) == tuple(ref.shape) and (out - ref).abs().max().item() < 1e-3
    eng.ws_budget_bytes = 1                                           # nothing fits: one pair at a time, the allocator decides
    assert eng.pairs_that_fit(B, H, W) == 1
    up, low, warped = eng.forward(frames, key, iters=6, want_low=True, warp_frame=key)
    assert (up - ref).abs().max().item() < 1e-3 and tuple(low.shape) == (B, H // 8, W // 8, 2) and tuple(warped.shape) == (B, H, W, 3)


_EDGE_SCRIPT = r"""
import hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd.raft import RaftEngine
from sd_animation_optical_flow_amd.weights import random_state_dict
eng = RaftEngine(random_state_dict(0), "cuda")
g = torch.Generator(device="cuda").manual_seed(5)
h = hashlib.sha256()
for (B, H, W, it) in ((1, 384, 256, 7), (2, 336, 280, 5), (4, 256, 192, 4), (1, 768, 512, 3)):
    a = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    k = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    h.update(eng.forward(a, k, iters=it).cpu().numpy().tobytes())
print("FLOWS", h.hexdigest())
"""


def test_event_edges_on_kernels_match_marker_edges(cuda):
    """Small grids run the flow branch of the motion encoder on a side stream; since round 6 its fork and join events ride on the
    flow head's / convf2's own dispatch packets (hipExtLaunchKernelGGL stop events, OFX_LAUNCH) instead of hipEventRecord markers.
    The switch is read once per process, so two child processes: the same flows, bit for bit, either way -- a dependency lost in
    the plumbing would show as a different (or run-to-run unstable) result on these under-filled grids."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra):
        env = dict(os.environ, **extra)
        out = subprocess.run([sys.executable, "-c", _EDGE_SCRIPT, root], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return [l for l in out.stdout.splitlines() if l.startswith("FLOWS")][-1]

    on_kernels = run({})
    assert on_kernels == run({}), "the kernel-carried edges do not repeat"
    assert on_kernels == run({"OFX_NO_STOP_EVENT": "1"})


# ------------------------------------------------------------------------------------------------
# round 2: the benchmarked configuration itself, the reference's own vectors, and saturated gates
# ------------------------------------------------------------------------------------------------
def test_engine_against_the_reference_raft_vectors_directly(engine, raft_sd):
    """One hop, no oracle in between: the HIP engine on the inputs of tests/golden/raft_ref_128x160.npz against the
    outputs the REAL reference RAFT (RAFT/core/raft.py:86-144, imported by make_golden.py) produced for them."""
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "raft_ref_128x160.npz"))
    i1 = torch.from_numpy(g["image1"]).permute(0, 2, 3, 1).contiguous().cuda()
    i2 = torch.from_numpy(g["image2"]).permute(0, 2, 3, 1).contiguous().cuda()
    up, lo = engine.forward(i1, i2, iters=20, want_low=True)
    ref_up = torch.from_numpy(g["flow_up"]).permute(0, 2, 3, 1)
    ref_lo = torch.from_numpy(g["flow_low"]).permute(0, 2, 3, 1)
    assert _epe(up.cpu(), ref_up) < 1e-3
    assert _epe(lo.cpu(), ref_lo) < 1e-3
    assert (up.cpu() - ref_up).abs().max().item() < 1e-2
    # stage vectors of the same file (stored in half precision: compare with a matching tolerance)
    fm1 = engine.buffer("fmap1").cpu().reshape(1, 16, 20, 256).permute(0, 3, 1, 2)
    ref_fm1 = torch.from_numpy(g["fmap1_f16"].astype(np.float32))
    assert (fm1 - ref_fm1).abs().max().item() < 2e-3 * max(1.0, ref_fm1.abs().max().item())
    from sd_animation_optical_flow_amd import ops
    p3 = ops.corr_unblock(engine.buffer("pyr3"), 2, 2).cpu().reshape(-1)
    assert (p3 - torch.from_numpy(g["pyr3"]).reshape(-1)).abs().max().item() < 5e-4


def test_bench_workload_c3_b64_20iters_512x768(engine, raft_sd):
    """BASELINE configs[2] exactly as bench.py times it: 64 frames of the synthetic clip against one shared key
    frame, 20 iterations.  Frames {0, 31, 63} against the CPU oracle; every frame against its own single-pair
    run (a pair's flow must not depend on the batch it rides in); warp + mask of the batch against their oracles
    on those frames."""
    import bench
    from oracle import mask_oracle, warp_oracle
    from sd_animation_optical_flow_amd import ops
    B, H, W = 64, bench.H, bench.W
    frames, key, key_ai, conf = bench.make_clip(B, H, W, torch.device("cuda"))
    # THE step bench.py times (bench.make_step: clip.FrameSynthesizer over the engine, the AI key frame warped inside the convex
    # upsample, then the mask) -- flow, warped and mask below all come out of it
    flow, warped, mask = bench.make_step(engine, frames, key, key_ai, conf)()
    assert tuple(flow.shape) == (B, H, W, 2) and torch.isfinite(flow).all()
    assert tuple(warped.shape) == (B, H, W, 3) and tuple(mask.shape) == (B, H, W)
    kf = key.cpu().permute(2, 0, 1)[None].float()
    for b in (0, 31, 63):
        _, up = RO.raft_forward(raft_sd, frames[b].cpu().permute(2, 0, 1)[None].float(), kf, iters=bench.ITERS)
        e = _epe(flow[b].cpu(), up[0].permute(1, 2, 0))
        assert e < 1e-3, (b, e)
    worst = 0.0
    for b in range(B):
        single = engine.forward(frames[b:b + 1], key, iters=bench.ITERS)
        worst = max(worst, (flow[b:b + 1] - single).abs().max().item())
    assert worst < 2e-3, worst                         # 20 recurrent fp32 iterations, different tile schedules
    # the two-kernel tail (upsample, then ofx_warp_and_mask) must give the same bytes as the fused one
    warped2, mask2 = ops.warp_and_mask(key_ai, flow, conf, warp_mode="bilinear", thres=0.95, ksize=7)
    assert torch.equal(warped2, warped) and torch.equal(mask2, mask)
    for b in (0, 31, 63):
        ref_w = warp_oracle.warp_frame(key_ai.cpu().numpy(), flow[b].cpu().numpy(), mode="bilinear")
        d = np.abs(warped[b].cpu().numpy().astype(np.int32) - ref_w.astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3          # u8 rounding of an fp32 blend
        c = conf[b].cpu().numpy()
        ref_m, _ = mask_oracle.generate_mask(c, c.copy(), 0.95, 7)
        assert np.array_equal(mask[b].cpu().numpy(), ref_m)


def test_raft2_as_written_at_the_bench_size(raft_sd):
    """`ofgen.RAFT_2`'s network (context-encoder BatchNorm on each image's own statistics, cnet_norm='batch') on the bench clip
    through the bench's own step: 8 frames of 512x768 against the shared key frame, frames {0, 7} against the CPU oracle in the same
    mode -- and at least 0.1 px away from the eval-mode network, so the two cannot be mixed up."""
    import bench
    from sd_animation_optical_flow_amd.raft import RaftEngine
    B, H, W = 8, bench.H, bench.W
    frames, key, key_ai, conf = bench.make_clip(B, H, W, torch.device("cuda"))
    engb = RaftEngine(raft_sd, cnet_norm="batch")
    flow, warped, mask = bench.make_step(engb, frames, key, key_ai, conf)()
    kf = key.cpu().permute(2, 0, 1)[None].float()
    for b in (0, 7):
        a = frames[b].cpu().permute(2, 0, 1)[None].float()
        _, up = RO.raft_forward(raft_sd, a, kf, iters=bench.ITERS, cnet_norm="batch")
        e = _epe(flow[b].cpu(), up[0].permute(1, 2, 0))
        assert e < 1e-3, (b, e)
    _, up_eval = RO.raft_forward(raft_sd, frames[0].cpu().permute(2, 0, 1)[None].float(), kf, iters=bench.ITERS)
    assert _epe(flow[0].cpu(), up_eval[0].permute(1, 2, 0)) > 0.1


def test_large_batch_on_a_map_that_is_not_whole_patches(engine, raft_sd):
    """64 frames of 264x392: every resolution of the network (132x196, 66x98, 33x49) leaves the last 8x16 patch of each row and
    column hanging over the map, and the batch is large enough for the 128-row halo-patch tiles.  Two frames against the CPU
    oracle, every frame against its own single-pair run (which takes the small-grid kernels)."""
    import bench
    B, H, W, iters = 64, 264, 392, 6
    frames, key, _, _ = bench.make_clip(B, H, W, torch.device("cuda"))
    flow = engine.forward(frames, key, iters=iters)
    assert tuple(flow.shape) == (B, H, W, 2) and torch.isfinite(flow).all()
    kf = key.cpu().permute(2, 0, 1)[None].float()
    for b in (0, 63):
        _, up = RO.raft_forward(raft_sd, frames[b].cpu().permute(2, 0, 1)[None].float(), kf, iters=iters)
        e = _epe(flow[b].cpu(), up[0].permute(1, 2, 0))
        assert e < 1e-3, (b, e)
    worst = 0.0
    for b in range(0, B, 7):
        single = engine.forward(frames[b:b + 1], key, iters=iters)
        worst = max(worst, (flow[b:b + 1] - single).abs().max().item())
    assert worst < 1e-3, worst


def test_saturated_gates_stay_inside_the_bar(cuda, raft_sd):
    """The GRU epilogues evaluate sigmoid / tanh with v_exp_f32 / v_rcp_f32 (ofx_internal.h) instead of libm.  A trained
    checkpoint drives the gates into saturation far more than seeded weights do: scale the update block's gate and
    motion-encoder weights x4 (and the context features with them) and hold the result to the same bar."""
    from sd_animation_optical_flow_amd.raft import RaftEngine
    sd = {k: v.clone() for k, v in raft_sd.items()}
    for k in sd:
        if k.startswith("update_block.gru.conv") or k.startswith("update_block.encoder.convc"):
            sd[k] = sd[k] * 4.0
    eng = RaftEngine(sd)
    H, W, B = 128, 160, 2
    key, frames = _frames(31, B, H, W)
    img2 = key[None].repeat(B, 1, 1, 1)
    tr = {}
    lo_ref, up_ref = _oracle_flow(sd, frames, img2, 6, trace=tr)
    up, lo = eng.forward(frames.cuda(), img2.cuda(), iters=6, want_low=True)
    h, w = H // 8, W // 8
    net_ref = tr["net_it0"]
    sat = (net_ref.abs() > 0.999).float().mean().item()
    hx = eng.buffer("hx").cpu().reshape(B * h * w, 384)
    assert torch.isfinite(up).all()
    assert _epe(up.cpu(), up_ref) < 1e-3, _epe(up.cpu(), up_ref)
    assert (lo.cpu() - lo_ref).abs().max().item() < 5e-3
    assert hx[:, :128].abs().max().item() <= 1.0 + 1e-6          # h is a convex mix of tanh values
    print(f"saturated fraction of the hidden state after iteration 0: {sat:.3f}")


# ------------------------------------------------------------------------------------------------
# round 3: a float64 yardstick under the headline-size parity, degenerate inputs for the epilogue statistics
# ------------------------------------------------------------------------------------------------
def test_headline_size_parity_against_a_float64_yardstick(engine, raft_sd):
    """At the benchmarked size the HIP flow sits 2-3e-4 px from the fp32 CPU oracle, the small tests 3e-6: which of the two
    drifts?  The same network evaluated in float64 (oracle.raft_oracle.to_float64) is the yardstick: over 20 recurrent
    iterations on the bench clip's frames the HIP path must be no further from it than 1.5x what the fp32 CPU oracle is,
    and inside the 1e-3 px bar by itself.  tools/epe_curve.py prints the per-iteration curve (profiles/r03_epe_curve.txt)."""
    import bench
    H, W = bench.H, bench.W
    frames, key, _, _ = bench.make_clip(64, H, W, torch.device("cuda"))
    sd64 = RO.to_float64(raft_sd)
    kf = key.cpu().permute(2, 0, 1)[None].float()
    flow = engine.forward(frames, key, iters=bench.ITERS)
    for b in (31,):        # one pair here (the float64 oracle costs ~20 s of CPU per pair); bench.py's `verified` block reports three
        a = frames[b].cpu().permute(2, 0, 1)[None].float()
        _, up32 = RO.raft_forward(raft_sd, a, kf, iters=bench.ITERS)
        _, up64 = RO.raft_forward(sd64, a.double(), kf.double(), iters=bench.ITERS)
        r64 = up64[0].permute(1, 2, 0)
        e_gpu = _epe(flow[b].cpu().double(), r64)
        e_cpu = _epe(up32[0].permute(1, 2, 0).double(), r64)
        print(f"pair {b}: HIP vs f64 {e_gpu:.3e} px, fp32 CPU oracle vs f64 {e_cpu:.3e} px")
        assert e_gpu < 1e-3, (b, e_gpu)
        assert e_gpu <= 1.5 * e_cpu + 2e-5, (b, e_gpu, e_cpu)


def test_split_modes_at_the_bench_size_against_the_oracles(raft_sd):
    """The opt-in split-bf16 arithmetics on BASELINE configs[2] itself -- 64 frames of 512x768 against the shared key frame, 20
    iterations, through `bench.make_step` (the step bench.py times, with the engine built in that mode) -- held to the oracles on
    frames {0, 63}: bf16x6 ("fp32-level accuracy") must sit no further from the float64 evaluation of the network than 1.5x what
    the fp32 CPU oracle does (+ 2e-5 px), bf16x3 inside the 1e-3 px parity bar against the fp32 oracle.  Before round 5 the
    modes met the oracle at 128x160 / 256x384 only; at this size their only check was bench.py's own `flow_epe_vs_fp32_px`."""
    import bench
    from sd_animation_optical_flow_amd.raft import RaftEngine
    B, H, W = 64, bench.H, bench.W
    frames, key, key_ai, conf = bench.make_clip(B, H, W, torch.device("cuda"))
    flows = {}
    for mode in ("bf16x6", "bf16x3"):
        eng = RaftEngine(raft_sd, precision=mode)
        flow, warped, mask = bench.make_step(eng, frames, key, key_ai, conf)()
        assert tuple(flow.shape) == (B, H, W, 2) and torch.isfinite(flow).all()
        assert tuple(warped.shape) == (B, H, W, 3) and tuple(mask.shape) == (B, H, W)
        flows[mode] = flow[[0, 63]].cpu()
        del eng, flow, warped, mask
    assert not torch.equal(flows["bf16x6"], flows["bf16x3"])                  # two arithmetics, not one engine twice
    sd64 = RO.to_float64(raft_sd)
    kf = key.cpu().permute(2, 0, 1)[None].float()
    for k, b in enumerate((0, 63)):
        a = frames[b].cpu().permute(2, 0, 1)[None].float()
        _, up32 = RO.raft_forward(raft_sd, a, kf, iters=bench.ITERS)
        _, up64 = RO.raft_forward(sd64, a.double(), kf.double(), iters=bench.ITERS)
        r32, r64 = up32[0].permute(1, 2, 0), up64[0].permute(1, 2, 0)
        e_cpu = _epe(r32.double(), r64)
        e6 = _epe(flows["bf16x6"][k].double(), r64)
        e3 = _epe(flows["bf16x3"][k], r32)
        print(f"pair {b}: bf16x6 vs f64 {e6:.3e} px (fp32 CPU oracle vs f64 {e_cpu:.3e}), bf16x3 vs fp32 oracle {e3:.3e} px")
        assert e6 <= 1.5 * e_cpu + 2e-5, (b, e6, e_cpu)
        assert e3 < 1e-3, (b, e3)
        assert e3 > 1e-6                                                      # not the fp32 path by accident


def test_volume_precision_at_the_bench_size_against_the_oracles(raft_sd):
    """`RaftEngine(volume_precision=...)`: ONLY the correlation volume on the bf16 matrix cores (csrc/corr_split.hip), every convolution
    exact fp32 -- on BASELINE configs[2] through `bench.make_step`, frames {0, 63} against the oracles: the three-plane form no further
    from the float64 network than 1.5x what the fp32 CPU oracle is (+ 2e-5 px), the two-plane form inside the 1e-3 px bar; both
    different from the fp32 engine's flow (the option took effect), warp and mask shapes intact."""
    import bench
    from sd_animation_optical_flow_amd.raft import RaftEngine
    B, H, W = 64, bench.H, bench.W
    frames, key, key_ai, conf = bench.make_clip(B, H, W, torch.device("cuda"))
    flows = {}
    for mode in (None, "bf16x6", "bf16x3"):
        eng = RaftEngine(raft_sd, volume_precision=mode)
        flow, warped, mask = bench.make_step(eng, frames, key, key_ai, conf)()
        assert tuple(flow.shape) == (B, H, W, 2) and torch.isfinite(flow).all()
        assert tuple(warped.shape) == (B, H, W, 3) and tuple(mask.shape) == (B, H, W)
        flows[mode] = flow[[0, 63]].cpu()
        del eng, flow, warped, mask
    assert not torch.equal(flows["bf16x6"], flows[None]) and not torch.equal(flows["bf16x3"], flows[None])
    assert not torch.equal(flows["bf16x6"], flows["bf16x3"])
    sd64 = RO.to_float64(raft_sd)
    kf = key.cpu().permute(2, 0, 1)[None].float()
    for k, b in enumerate((0, 63)):
        a = frames[b].cpu().permute(2, 0, 1)[None].float()
        _, up32 = RO.raft_forward(raft_sd, a, kf, iters=bench.ITERS)
        _, up64 = RO.raft_forward(sd64, a.double(), kf.double(), iters=bench.ITERS)
        r32, r64 = up32[0].permute(1, 2, 0), up64[0].permute(1, 2, 0)
        e_cpu = _epe(r32.double(), r64)
        e6 = _epe(flows["bf16x6"][k].double(), r64)
        e0 = _epe(flows[None][k].double(), r64)
        e3 = _epe(flows["bf16x3"][k], r32)
        print(f"pair {b}: volume bf16x6 vs f64 {e6:.3e} px (fp32 engine {e0:.3e}, fp32 CPU oracle {e_cpu:.3e}), volume bf16x3 vs fp32 oracle {e3:.3e} px")
        assert e6 <= 1.5 * e_cpu + 2e-5, (b, e6, e_cpu)
        assert e3 < 1e-3, (b, e3)


def test_volume_precision_in_the_pair_list_executor(cuda, raft_sd):
    """The indexed-pairs executor (`forward_pairs`: KeyframeConv's ordered pairs, ofgen_keyframe_inpaint.py:627-668) with the split
    volume: one launch over the device-side pair list, every image split once per role.  Against the fp32 executor on the same pairs."""
    from sd_animation_optical_flow_amd.raft import RaftEngine
    g = torch.Generator().manual_seed(8)
    imgs = torch.randint(0, 256, (4, 128, 256, 3), generator=g, dtype=torch.uint8).cuda()
    # 96 ordered pairs of 4 images: (pairs x 2 row groups of the 16x32 map) fill the 256 CUs' first round to 0.75 -- below that the
    # executor keeps the generic GEMM (`ofx_corr_volsplit_pays`) and the option has no effect
    i1 = [0, 1, 2, 3, 0, 2] * 16
    i2 = [1, 0, 3, 1, 3, 0] * 16
    ref = RaftEngine(raft_sd).forward_pairs(imgs, i1, i2, iters=8)
    for mode, tol in (("bf16x6", 2e-4), ("bf16x3", 2e-3)):
        got = RaftEngine(raft_sd, volume_precision=mode).forward_pairs(imgs, i1, i2, iters=8)
        e = _epe(got.cpu(), ref.cpu())
        print(mode, "pair-list flow EPE vs fp32 executor", e)
        assert e < tol and not torch.equal(got, ref), (mode, e)


def _degenerate_frames(kind, B, H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    if kind == "constant":                       # zero variance everywhere but at the zero-padded borders
        a = torch.full((B, H, W, 3), 200, dtype=torch.uint8)
        k = torch.full((H, W, 3), 200, dtype=torch.uint8)
    elif kind == "one_lsb":                      # sigma <= 1 LSB around a large mean: sum x^2 / n - mu^2 cancels
        a = (200 + torch.randint(0, 2, (B, H, W, 3), generator=g)).to(torch.uint8)
        k = (200 + torch.randint(0, 2, (H, W, 3), generator=g)).to(torch.uint8)
    elif kind == "saturated":                    # 0 / 255 only
        a = (torch.randint(0, 2, (B, H, W, 3), generator=g) * 255).to(torch.uint8)
        k = (torch.randint(0, 2, (H, W, 3), generator=g) * 255).to(torch.uint8)
    elif kind == "bright":
        a = (250 + torch.randint(0, 6, (B, H, W, 3), generator=g)).to(torch.uint8)
        k = (250 + torch.randint(0, 6, (H, W, 3), generator=g)).to(torch.uint8)
    else:                                        # half flat, half texture
        a = torch.randint(0, 256, (B, H, W, 3), generator=g).to(torch.uint8)
        k = torch.randint(0, 256, (H, W, 3), generator=g).to(torch.uint8)
        a[:, :, : W // 2] = 17
        k[:, : W // 2] = 17
    return a.contiguous(), k.contiguous()


@pytest.mark.parametrize("kind", ["constant", "one_lsb", "saturated", "bright", "half_flat"])
@pytest.mark.parametrize("cnet_norm", ["eval", "batch"])
def test_epilogue_statistics_on_degenerate_frames(cuda, raft_sd, kind, cnet_norm):
    """The feature encoder's instance-norm statistics (and the context encoder's in 'batch' mode) come out of the convolution
    epilogues as per-wave fp32 (sum, sum of squares), var = q/HW - mu^2 (conv.hip, net_misc.hip): the inputs that can break
    that are maps with (almost) no variance.  Feature maps after the encoders against the oracle, the 12-iteration flow against
    the oracle, and both against the schedule that takes the statistics with their own f64 pass."""
    from sd_animation_optical_flow_amd.raft import RaftEngine
    eng = RaftEngine(raft_sd, cnet_norm=cnet_norm)
    B, H, W, iters = 2, 256, 384, 12
    a, k = _degenerate_frames(kind, B, H, W)
    tr = {}
    lo_ref, up_ref = RO.raft_forward(raft_sd, a.permute(0, 3, 1, 2).float(), k.permute(2, 0, 1)[None].repeat(B, 1, 1, 1).float(),
                                     iters=iters, trace=tr, cnet_norm=cnet_norm)
    up_ref = up_ref.permute(0, 2, 3, 1)
    res = {}
    for sep in (False, True):
        up = eng.forward(a.cuda(), k.cuda(), iters=iters, separate_stats=sep)
        assert torch.isfinite(up).all()
        fm1 = eng.buffer("fmap1").cpu().reshape(B, H // 8, W // 8, 256)
        hx = eng.buffer("hx").cpu().reshape(B, H // 8, W // 8, 384)
        res[sep] = (up.cpu(), fm1, hx[..., 256:])
    fm_ref = tr["fmap1"].permute(0, 2, 3, 1)
    inp_ref = tr["inp"].permute(0, 2, 3, 1)
    scale = max(1.0, fm_ref.abs().max().item())
    for sep in (False, True):
        up, fm1, inp = res[sep]
        # on (almost) flat maps the normalisation divides rounding noise by sqrt(var + 1e-5): the oracle's own fp32 statistics are
        # no better placed than ours, so the feature maps are held to the oracle loosely and to each other tightly (below)
        assert (fm1 - fm_ref).abs().max().item() < 5e-3 * scale, (sep, (fm1 - fm_ref).abs().max().item())
        assert (inp - inp_ref).abs().max().item() < 5e-3 * max(1.0, inp_ref.abs().max().item())
        assert _epe(up, up_ref) < 1e-3, (sep, _epe(up, up_ref))
    assert (res[False][1] - res[True][1]).abs().max().item() < 2e-3 * scale
    assert _epe(res[False][0], res[True][0]) < 5e-4


def test_forward_with_the_warp_inside_the_upsample(engine, raft_sd):
    """`RaftEngine.forward(warp_frame=...)` (ofx_raft_forward_warp): the AI key frame is warped inside the convex upsample.  Same flow,
    and the warped frames are byte for byte `ops.warp(key_ai, flow, 'bilinear')` of the plain forward -- for a frame size that needs
    InputPadder as well, for both warp conventions, and with the full-resolution flow left unwritten."""
    from sd_animation_optical_flow_amd import ops
    for (H, W, B, seed) in ((128, 160, 5, 51), (256, 384, 4, 52)):       # >= 4 frames: ops.warp then takes the same sampling kernel
        key, frames = _frames(seed, B, H, W)
        g = torch.Generator().manual_seed(seed)
        key_ai = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).cuda()
        flow = engine.forward(frames.cuda(), key.cuda(), iters=8)
        for sign in (1.0, -1.0):
            ref = ops.warp(key_ai, flow, mode="bilinear", sign=sign)
            f2, warped = engine.forward(frames.cuda(), key.cuda(), iters=8, warp_frame=key_ai, warp_sign=sign)
            assert torch.equal(f2, flow) and torch.equal(warped, ref)
        none, warped = engine.forward(frames.cuda(), key.cuda(), iters=8, warp_frame=key_ai, want_flow=False)
        assert none is None and torch.equal(warped, ops.warp(key_ai, flow, mode="bilinear"))
        f3, lo3, w3 = engine.forward(frames.cuda(), key.cuda(), iters=8, warp_frame=key_ai, want_low=True)
        assert torch.equal(f3, flow) and tuple(lo3.shape) == (B, H // 8, W // 8, 2) and torch.equal(w3, warped)
    with pytest.raises(RuntimeError):
        engine.forward(frames.cuda(), key.cuda(), iters=1, warp_frame=key_ai[:100])          # not the frame size
    with pytest.raises(ValueError):
        engine.forward(frames.cuda(), key.cuda(), iters=1, want_flow=False)                  # nothing to return
