"""The fused Winograd F(4x4,3x3) convolution (conv_wino.hip): the second route of the update block's plain 3x3 layers.

Every case is forced with TILE_WINOGRAD4 and checked elementwise against float64 with the operand-scaled bound of wino_check
(K_F43, wino44_check.py); it must differ from the F(2x2,3x3) result (the new kernel ran) and repeat bit for bit.  GPU tests are
marked -m gpu.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino44_check as w4  # noqa: E402
import wino_check as wc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def _check(case, seed):
    ops = _ops()
    c = w4.make(case, seed)
    opw = w4.operands(ops, c["w"])
    got, dst = w4.run(ops, c, ops.TILE_WINOGRAD4, opw)
    ratio = wc.worst_ratio(got, c["ref"], c["mag"])
    print(f"{case[0]}: worst ratio {ratio:.3g} (K_F43 = {w4.K_F43})")
    wc.check(got, c["ref"], c["mag"], w4.K_F43, case[0])
    off_chunk = c["x1"] is not None and (c["x0"].shape[1] % 32 or c["x1"].shape[1] % 32)
    f22, _ = w4.run(ops, c, ops.TILE_WINOGRAD, opw, joined=bool(off_chunk))
    wc.check(f22, c["ref"], c["mag"], wc.K_F23, case[0] + " F(2x2)")
    if off_chunk:   # only the forced F(4x4) route takes such a split
        with pytest.raises(RuntimeError):
            w4.run(ops, c, ops.TILE_WINOGRAD, opw)
    assert not torch.equal(got, f22), "the F(4x4) kernel did not run"
    again, _ = w4.run(ops, c, ops.TILE_WINOGRAD4, opw)
    assert torch.equal(got, again), "not bit-identical on a second call"
    if dst is not None:
        ld, off = c["dst"]
        assert bool(torch.isnan(dst[..., :off]).all()) and bool(torch.isnan(dst[..., off + c["co"]:]).all()), "neighbours written"
        assert not bool(torch.isnan(dst[..., off:off + c["co"]]).any())
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("case", w4.CASES, ids=[c[0] for c in w4.CASES])
def test_forced_route_against_float64(cuda, case):
    _check(case, 100 + w4.CASES.index(case))


@pytest.mark.gpu
@pytest.mark.parametrize("layer", w4.ENGINE_LAYERS, ids=[l[0] for l in w4.ENGINE_LAYERS])
def test_engine_layer_descriptors_against_float64(cuda, layer):
    name, seg, co, relu = layer
    _check((name, 2, 32, 64, seg, co, "relu", relu, True, None), 200 + w4.ENGINE_LAYERS.index(layer))


@pytest.mark.gpu
def test_automatic_route_on_both_sides_of_the_gate(cuda):
    """tile = 0 with both operands: the F(4x4) result above the gate (768 workgroups of one 16x32 patch x 64 channels), the
    F(2x2) result below it -- each bit for bit the forced launch."""
    ops = _ops()
    for B, above in ((24, True), (23, False)):
        c = w4.make(("gate", B, 64, 256, (16, 0), 64, "normal", True, False, None), 300 + B)   # 32 patches per image
        opw = w4.operands(ops, c["w"])
        auto, _ = w4.run(ops, c, 0, opw)
        f44, _ = w4.run(ops, c, ops.TILE_WINOGRAD4, opw)
        f22, _ = w4.run(ops, c, ops.TILE_WINOGRAD, opw)
        assert not torch.equal(f44, f22)
        assert torch.equal(auto, f44 if above else f22), (B, above)
        # without the F(4x4) operand: as before
        wp, u2, _ = opw
        only2 = ops.conv2d_nhwc(w4.nhwc(c["x0"]), wp, 3, 3, 64, act="relu", wino_w=u2)
        assert torch.equal(w4.nchw(only2), f22)


@pytest.mark.gpu
def test_forced_route_is_rejected_where_it_does_not_fit(cuda):
    ops = _ops()
    for (H, W) in ((16, 16), (8, 32)):
        c = w4.make(("nofit", 1, H, W, (16, 0), 64, "normal", False, False, None), 400 + H)
        with pytest.raises(RuntimeError):
            w4.run(ops, c, ops.TILE_WINOGRAD4, w4.operands(ops, c["w"]))
    c = w4.make(("no_operand", 1, 16, 32, (16, 0), 64, "normal", False, False, None), 401)
    wp, u2, _ = w4.operands(ops, c["w"])
    with pytest.raises(RuntimeError):
        w4.run(ops, c, ops.TILE_WINOGRAD4, (wp, u2, None))


_ENGINE_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd.raft import RaftEngine
from sd_animation_optical_flow_amd.weights import random_state_dict
eng = RaftEngine(random_state_dict(0), "cuda")
B, H, W = 2, 128, 160
g = torch.Generator().manual_seed(5)
base = torch.rand((1, 3, H + 32, W + 32), generator=g)
base = torch.nn.functional.conv2d(base, torch.ones((3, 1, 5, 5)) / 25.0, padding=2, groups=3)
base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)[0].permute(1, 2, 0)
key = base[16:16 + H, 16:16 + W].contiguous()
frames = torch.stack([base[16 + b - 1:16 + b - 1 + H, 16 + 2 * b - 1:16 + 2 * b - 1 + W] for b in range(B)])
up = eng.forward(frames.contiguous().cuda(), key.cuda(), iters=6)
np.save(sys.argv[2], up.cpu().numpy())
"""


@pytest.mark.gpu
def test_engine_flow_without_a_whole_patch_is_bit_identical_with_the_switch(cuda, tmp_path):
    """B = 2 at 128x160 is 16x20 at 1/8 resolution: no whole 16x32 patch, so the flow must be the same bits with and without
    OFX_CONV_NO_WINOGRAD4 (read once per process, hence child processes)."""
    def run(tag, extra):
        env = {k: v for k, v in os.environ.items() if k not in ("OFX_CONV_NO_WINOGRAD", "OFX_CONV_NO_WINOGRAD4")}
        env.update(extra)
        path = str(tmp_path / f"{tag}.npy")
        out = subprocess.run([sys.executable, "-c", _ENGINE_SCRIPT, ROOT, path], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return np.load(path)

    a = run("with", {})
    b = run("without", {"OFX_CONV_NO_WINOGRAD4": "1"})
    assert np.isfinite(a).all() and np.array_equal(a, b)


_ROUTE_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd.raft import RaftEngine
from sd_animation_optical_flow_amd.weights import random_state_dict
eng = RaftEngine(random_state_dict(0), "cuda")
B, H, W = 32, 512, 768
g = torch.Generator().manual_seed(11)
base = torch.rand((1, 3, H + 32, W + 32), generator=g)
base = torch.nn.functional.conv2d(base, torch.ones((3, 1, 5, 5)) / 25.0, padding=2, groups=3)
base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)[0].permute(1, 2, 0)
key = base[16:16 + H, 16:16 + W].contiguous()
frames = torch.stack([base[16 + (b % 5) - 2:16 + (b % 5) - 2 + H, 16 + (3 * b % 7) - 3:16 + (3 * b % 7) - 3 + W] for b in range(B)])
up = eng.forward(frames.contiguous().cuda(), key.cuda(), iters=4)
np.save(sys.argv[2], up.cpu().numpy())
"""


@pytest.mark.gpu
def test_engine_flow_with_and_without_the_route(cuda, tmp_path):
    """32 pairs of 512x768 (64x96 at 1/8: 12 patches per image) put conv (768 workgroups), convc2 (1152), fh1 and mask.0 (1536)
    on the F(4x4,3x3) kernel; OFX_CONV_NO_WINOGRAD4 (read once per process, hence child processes) keeps F(2x2,3x3).  The flows
    must differ (the route was taken) by less than 1e-4 px, the bar of the F(2x2,3x3) route's own test."""
    def run(tag, extra):
        env = {k: v for k, v in os.environ.items() if k not in ("OFX_CONV_NO_WINOGRAD", "OFX_CONV_NO_WINOGRAD4")}
        env.update(extra)
        path = str(tmp_path / f"{tag}.npy")
        out = subprocess.run([sys.executable, "-c", _ROUTE_SCRIPT, ROOT, path], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return np.load(path)

    f44 = run("f44", {})
    f22 = run("f22", {"OFX_CONV_NO_WINOGRAD4": "1"})
    epe = float(np.sqrt(((f44.astype(np.float64) - f22) ** 2).sum(-1)).mean())
    print(f"EPE between the routes {epe:.3g} px, max abs {np.abs(f44 - f22).max():.3g}")
    assert np.isfinite(f44).all() and 0 < epe < 1e-4, epe
