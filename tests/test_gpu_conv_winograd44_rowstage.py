"""The F(4x4,3x3) kernel's slab pipeline (conv_wino.hip, wino44_conv_kernel) at the smallest shapes at which it can go wrong.

The kernel walks the input channels in 8-channel slabs, two per trip, through double-buffered LDS images one barrier per slab
apart.  What that can get wrong shows at particular depths -- one trip, where the prologue alone feeds both slabs; two, the first
reuse of both buffers; three and four, the first overwrite of a buffer while other waves still read its neighbour -- on borders
(out-of-map halo rows and columns must transform to zero), in the epilogue (a Cout tail into a strided destination), and as a race
on a grid that keeps every CU busy for several rounds.  Cases: wino44_rowstage_cases.py.

Every case is forced with TILE_WINOGRAD4, checked elementwise against float64 with wino_check's operand-scaled bound and K_F43,
and compared bit for bit with the output recorded by tools/wino44_bits.py (tests/golden/wino44_rowstage/: the array, or its
SHA-256 where the array is too large to commit) from the kernel as it stood before its operands' row transform was staged.  A
change of the kernel's schedule keeps these bits; a change of its arithmetic records new ones.  GPU tests are marked -m gpu.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino44_rowstage_cases as rc  # noqa: E402
from wino44_check import K_F43, make, operands, run  # noqa: E402
from wino_check import check, worst_ratio  # noqa: E402


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def _golden_equal(name, got):
    path = os.path.join(rc.GOLDEN, name + ".npy")
    if got.numel() * 4 <= rc.MAX_ARRAY_BYTES:
        return torch.equal(got, torch.from_numpy(np.load(path)))
    with open(os.path.join(rc.GOLDEN, "sha256.json")) as f:
        return rc.sha256(got) == json.load(f)[name]


@pytest.mark.gpu
@pytest.mark.parametrize("case", rc.CASES, ids=[c[0] for c in rc.CASES])
def test_against_float64_and_the_recorded_bits(cuda, case):
    ops = _ops()
    name = case[0]
    c = make(case, rc.seed(case))
    opw = operands(ops, c["w"])
    got, dst = run(ops, c, ops.TILE_WINOGRAD4, opw)
    print(f"{name}: worst ratio {worst_ratio(got, c['ref'], c['mag']):.3g} (K_F43 = {K_F43})")
    check(got, c["ref"], c["mag"], K_F43, name)
    if dst is not None:
        ld, off = c["dst"]
        assert bool(torch.isnan(dst[..., :off]).all()) and bool(torch.isnan(dst[..., off + c["co"]:]).all()), "neighbours written"
        assert not bool(torch.isnan(dst[..., off:off + c["co"]]).any())
    assert _golden_equal(name, got), "not the recorded bits"
    # a missing barrier or a wrong wait is a race: five more launches, five times the same bits
    for k in range(5):
        again, _ = run(ops, c, ops.TILE_WINOGRAD4, opw)
        assert torch.equal(got, again), f"launch {k + 2} differs from the first"
