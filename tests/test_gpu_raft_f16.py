"""-m gpu: `RaftEngine(precision="fp16")` end to end -- RAFT's mixed precision (`args.mixed_precision`, RAFT/core/raft.py:99,110,127).

THE NORTH-STAR BAR OF THE DEFAULT PATH (flow EPE <= 1e-3 px against the reference, tests/test_gpu_raft.py) DOES NOT APPLY TO THIS
MODE: half-precision operands put the flow ~1.7e-2 px from the float64 truth after 20 iterations, on the reference itself as on
the device.  The bar here is the project's own for this arithmetic (tests/test_gpu_unet_precision.py), measured on the reference:

    yardstick   tests/golden/raft_ref_autocast_128x160.npz (make_golden_raft_autocast.py): the REAL reference RAFT with
                mixed_precision=True under torch.autocast("cpu", float16) on the seeded weights and `_frames(11, 2, 128, 160)` at
                20 iterations -- its EPE against the float64 oracle, `autocast_vs_f64` (1.66e-2 px), and the EPE of the same module in
                fp32 with F.conv2d's two operands rounded to half, `emulated_vs_f64` (1.77e-2 px): the engine's arithmetic on the CPU
    bar         device EPE against float64 <= 2 x autocast_vs_f64
    not fp32    device EPE >= 0.25 x emulated_vs_f64 (the fp32 path sits three orders of magnitude below), and the flows are not
                torch.equal to the fp32 engine's

The float64 flows are computed once per module and shared.  Case b (136x168) has a 1/8 map of 17 x 21: no whole halo patch."""
import os
from unittest import mock

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import raft_oracle as RO

GOLD = os.path.join(os.path.dirname(__file__), "golden", "raft_ref_autocast_128x160.npz")
ITERS = 20


def _epe(a, b):
    return (a.double() - b.double()).pow(2).sum(-1).sqrt().mean().item()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def ref64(gold, raft_sd):
    """{tag: float64 flow [B,H,W,2]} of the stored cases, by the float64 oracle the yardstick was measured against."""
    sd64 = RO.to_float64(raft_sd)
    out = {}
    for tag in (str(t) for t in gold["cases"]):
        i1 = torch.from_numpy(gold[f"image1_{tag}"]).permute(0, 3, 1, 2).double()
        i2 = torch.from_numpy(gold[f"image2_{tag}"]).permute(2, 0, 1).double()[None].expand(i1.shape[0], -1, -1, -1)
        out[tag] = RO.raft_forward(sd64, i1, i2, iters=ITERS)[1].permute(0, 2, 3, 1).contiguous()
    return out


@pytest.fixture(scope="module")
def f16(cuda, raft_sd):
    from sd_animation_optical_flow_amd.raft import RaftEngine
    return RaftEngine(raft_sd, precision="fp16")


@pytest.fixture(scope="module")
def f32(cuda, raft_sd):
    from sd_animation_optical_flow_amd.raft import RaftEngine
    return RaftEngine(raft_sd)


def _inputs(gold, tag):
    return torch.from_numpy(gold[f"image1_{tag}"]).cuda(), torch.from_numpy(gold[f"image2_{tag}"]).cuda()


def _bar(gold, tag, epe, what, ref="float64"):
    auto, emu = float(gold[f"autocast_vs_f64_{tag}"]), float(gold[f"emulated_vs_f64_{tag}"])
    print(f"{what} [{tag}]: EPE vs {ref} {epe:.3e} px; autocast {auto:.3e}, emulation {emu:.3e}; bar {2 * auto:.3e}, floor {0.25 * emu:.3e}")
    assert epe <= 2.0 * auto, (what, tag, epe, auto)
    assert epe >= 0.25 * emu, (what, tag, epe, emu)


def test_the_yardstick_is_what_the_header_says(gold, ref64):
    assert [str(t) for t in gold["cases"]] == ["a", "b"]
    for tag, shape in (("a", (2, 128, 160, 2)), ("b", (2, 136, 168, 2))):
        auto, emu, f32d = (float(gold[f"{k}_vs_f64_{tag}"]) for k in ("autocast", "emulated", "fp32"))
        assert tuple(gold[f"flow_{tag}"].shape) == shape and gold[f"flow_{tag}"].dtype == np.float32
        assert 5e-3 < auto < 5e-2 and emu <= 1.5 * auto and f32d < 1e-4 < 0.01 * auto
        # the stored flow is that run, and the float64 flows here are the ones it was measured against
        assert abs(_epe(torch.from_numpy(gold[f"flow_{tag}"]), ref64[tag]) - auto) < 1e-6
    assert abs(float(gold["autocast_vs_f64_a"]) - 1.66e-2) < 1e-4 and abs(float(gold["emulated_vs_f64_a"]) - 1.77e-2) < 1e-4


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fp16_flow_against_float64_under_the_autocast_bar(gold, ref64, f16, f32, tag):
    i1, i2 = _inputs(gold, tag)
    up, lo = f16.forward(i1, i2, iters=ITERS, want_low=True)
    assert torch.isfinite(up).all() and tuple(lo.shape) == (i1.shape[0], i1.shape[1] // 8, i1.shape[2] // 8, 2)
    _bar(gold, tag, _epe(up.cpu(), ref64[tag]), "forward")
    assert torch.equal(up, f16.forward(i1, i2, iters=ITERS))                 # repeats bit for bit (no split-K, no atomics)
    up32 = f32.forward(i1, i2, iters=ITERS)
    assert not torch.equal(up, up32)
    assert _epe(up32.cpu(), ref64[tag]) < 1e-4                               # the default path is where it was
    # the volume stayed exact fp32: its pyramid is the fp32 engine's on the fp16 feature maps, i.e. finite and not the fp32 run's
    assert torch.isfinite(f16.buffer("pyr0")).all()


def test_every_entry_point_goes_through_the_same_arithmetic(gold, ref64, f16, f32):
    """alternate_corr, forward_pairs, the warm start and the fused warp in fp16: the same bar.  The float64 oracle has no warm start;
    the fp32 engine from the same initial flow stands in for it (it sits ~5e-6 px from float64, tests/test_gpu_warm_start.py)."""
    from sd_animation_optical_flow_amd import ops
    i1, i2 = _inputs(gold, "a")
    B = i1.shape[0]
    up, lo = f16.forward(i1, i2, iters=ITERS, want_low=True)
    alt = f16.forward(i1, i2, iters=ITERS, alternate_corr=True)
    _bar(gold, "a", _epe(alt.cpu(), ref64["a"]), "alternate_corr")
    imgs = torch.cat([i1, i2[None]])
    pr = f16.forward_pairs(imgs, list(range(B)), [B] * B, iters=ITERS)
    _bar(gold, "a", _epe(pr.cpu(), ref64["a"]), "forward_pairs")
    warm, warm32 = f16.forward(i1, i2, iters=ITERS, flow_init=lo), f32.forward(i1, i2, iters=ITERS, flow_init=lo)
    assert _epe(warm.cpu(), up.cpu()) > 1.0                                  # (the init was used: another 20 iterations from it)
    _bar(gold, "a", _epe(warm.cpu(), warm32.cpu()), "warm start", ref="the fp32 engine from the same initial flow")
    key_ai = (255 - i2).contiguous()
    up_w, warped = f16.forward(i1, i2, iters=ITERS, warp_frame=key_ai)
    assert torch.equal(up_w, up)
    d = (warped.int() - ops.warp(key_ai, up, mode="bilinear").int()).abs()   # (two frames: ops.warp may take another sampling kernel)
    assert int(d.max()) <= 1 and float((d > 0).float().mean()) < 1e-3


def test_bench_step_in_fp16(gold, ref64, f16):
    """The benchmark's step (`clip.FrameSynthesizer`, as bench.make_step builds it) over the fp16 engine on one 128x160 batch."""
    from sd_animation_optical_flow_amd import clip
    i1, i2 = _inputs(gold, "a")
    B, H, W = i1.shape[:3]
    g = torch.Generator().manual_seed(5)
    conf = torch.rand((B, H, W), generator=g).cuda()
    key_ai = (255 - i2).contiguous()
    synth = clip.FrameSynthesizer(engine=f16, warp_mode="bilinear", thres=0.95, ksize=7, iters=ITERS, fuse_warp=True)
    flow, warped, mask = synth(i1, i2, key_ai, confidence=conf)
    assert tuple(flow.shape) == (B, H, W, 2) and torch.isfinite(flow).all()
    assert tuple(warped.shape) == (B, H, W, 3) and warped.dtype == torch.uint8
    assert tuple(mask.shape) == (B, H, W) and mask.dtype == torch.uint8
    _bar(gold, "a", _epe(flow.cpu(), ref64["a"]), "FrameSynthesizer")


def test_raft2_mixed_precision_is_the_fp16_engine(gold, raft_sd):
    from sd_animation_optical_flow_amd.ofgen import RAFT_2
    from sd_animation_optical_flow_amd.raft import RaftEngine
    a, b = gold["image1_a"][0], gold["image2_a"]
    r2 = RAFT_2(model=raft_sd, mixed_precision=True)
    assert r2.model.precision == "fp16" and RAFT_2(model=raft_sd).model.precision == "fp32"
    flo = r2.calc(a, b)
    eng = RaftEngine(raft_sd, cnet_norm="batch", precision="fp16")
    want = eng.forward(torch.from_numpy(a).cuda()[None], torch.from_numpy(b).cuda()[None], iters=20, bgr=True)[0].cpu().numpy()
    assert flo.shape == want.shape == (128, 160, 2) and np.array_equal(flo, want)
    assert not np.array_equal(flo, RAFT_2(model=raft_sd).calc(a, b))


def test_volume_precision_combines_and_batches_agree(gold, ref64, raft_sd, f16):
    from sd_animation_optical_flow_amd.raft import RaftEngine
    i1, i2 = _inputs(gold, "a")
    both = RaftEngine(raft_sd, precision="fp16", volume_precision="bf16x3")
    _bar(gold, "a", _epe(both.forward(i1, i2, iters=ITERS).cpu(), ref64["a"]), "fp16 + volume bf16x3")
    # B = 1 and B = 2: the shared pair, within the bar of each other and of float64
    two = f16.forward(i1, i2, iters=ITERS)
    one = f16.forward(i1[:1], i2, iters=ITERS)
    d = _epe(one[0].cpu(), two[0].cpu())
    print(f"B = 1 against B = 2, the shared pair: EPE {d:.3e} px")
    assert d <= 2.0 * float(gold["autocast_vs_f64_a"])
    e1 = _epe(one[0].cpu(), ref64["a"][0])
    assert e1 <= 2.0 * _epe(torch.from_numpy(gold["flow_a"][0]), ref64["a"][0]), e1       # the single pair under the bar of ITS pair


def test_flag_combinations_on_the_device(raft_sd, f16, gold):
    """OFX_RAFT_F16 with OFX_RAFT_BF16X3 / _BF16X6 is OFX_EINVAL from the C entry point; the small network rejects the flag."""
    from sd_animation_optical_flow_amd import raft
    from sd_animation_optical_flow_amd.weights import load_checkpoint
    i1, i2 = _inputs(gold, "a")
    for extra in (raft.FLAG_BF16X3, raft.FLAG_BF16X6):
        with mock.patch.dict(raft.PRECISIONS, {"fp16": raft.FLAG_F16 | extra}):
            with pytest.raises(RuntimeError, match="-1|EINVAL|invalid"):
                f16.forward(i1, i2, iters=2)
    assert torch.isfinite(f16.forward(i1, i2, iters=2)).all()               # the engine is fine afterwards
    small = raft.RaftEngine(load_checkpoint("random-small:0"))
    with mock.patch.dict(raft.PRECISIONS, {"fp32": raft.FLAG_F16}):
        with pytest.raises(RuntimeError, match="-1|EINVAL|invalid"):
            small.forward(i1, i2, iters=2)
