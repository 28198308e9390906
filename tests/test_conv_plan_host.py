"""The convolution launcher's plan, asked of the library on the host (ofx_conv2d_plan: the launcher's own validation and rule, no
operand read, no device), against the independent Python restatement the encoder-norm tests steer by (inorm_check.plan), and the
Winograd gate against its documented conditions.  No GPU: the descriptors carry dummy, aligned, never-dereferenced pointers."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import inorm_check as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000                       # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40                       # "room for anything": statistics floats / split-K scratch bytes
PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16x3_w": 2, "bf16x6": 3, "bf16x6_w": 4}
KINDS = {0: "general", 1: "scalar", 2: "patch"}
TILE_WINOGRAD = 1
EINVAL = -1


def _lib():
    from sd_animation_optical_flow_amd import _lib
    return _lib


def _desc(B, H, W, cin, cout, kh, kw, stride=1, tile=0, precision="fp32", norm=False, splitk=False, wino=False, act=0):
    d = _lib().ConvDesc()
    d.in0, d.ld0, d.c0, d.w = PTR, cin, cin, PTR
    d.out, d.ldo = PTR, cout
    if norm:
        d.nmean, d.nrstd = PTR, PTR
    d.B, d.Hin, d.Win = B, H, W
    d.Hout, d.Wout = ic.out_size(H, W, kh, kw, stride)
    d.Cout, d.KH, d.KW, d.stride, d.padH, d.padW = cout, kh, kw, stride, kh // 2, kw // 2
    d.act, d.tile, d.precision = act, tile, PRECISIONS[precision]
    if splitk:
        d.splitk_ws, d.splitk_ws_bytes = PTR, BIG
    if wino:
        d.wino_w = PTR
    return d


def _query(d, stats_cap=BIG):
    p = _lib().ConvPlan()
    st = _lib().lib().ofx_conv2d_plan(C.byref(d), stats_cap, 0, C.byref(p))
    return st, p


GRID = dict(
    B=(1, 2, 4, 16),
    HW=((8, 16), (16, 16), (46, 62), (64, 96), (68, 120), (96, 128)),
    cin=(16, 32, 64, 96),
    cout=(2, 32, 64, 96, 128, 192, 256, 576),
    k=((1, 1), (3, 3), (1, 5), (5, 1), (7, 7)),
    stride=(1, 2),
    precision=tuple(PRECISIONS),
    norm=(False, True),
    splitk=(False, True),
    tile=(0, 16128064, 32064064, 2032064064),
)


def test_plan_agrees_with_the_python_restatement():
    """Single-segment plain-epilogue layers without a Winograd operand, over the product of GRID: tile, chunk length, A-side
    schedule, K splits, paired pipelines and statistics rows, field by field."""
    total = skipped = 0
    seen = set()
    bad = []
    for B, (H, W), cin, cout, (kh, kw), stride, prec, norm, splitk, tile in itertools.product(*GRID.values()):
        total += 1
        st, p = _query(_desc(B, H, W, cin, cout, kh, kw, stride, tile, prec, norm, splitk))
        if st != 0:
            skipped += 1
            continue
        want = ic.plan(B, H, W, cin, cout, kh, kw, stride=stride, tile=tile, norm=norm, precision=prec, splitk=splitk)
        got = dict(bm=p.bm, bn=p.bn, bk=p.bk, kind=KINDS[p.mode], splits=p.ksplit, paired=p.ks == 2, rows=p.stats_rows)
        assert p.path == 0
        if any(want[k] != v for k, v in got.items()):
            if len(bad) < 10:
                bad.append(((B, H, W, cin, cout, kh, kw, stride, prec, norm, splitk, tile), got, {k: want[k] for k in got}))
            continue
        seen.add(got["kind"])
        if got["splits"] > 1:
            seen.add("split")
        if got["paired"]:
            seen.add("paired")
        if tile == 0 and (p.bm, p.bn) == (256, 64):
            seen.add("promoted")
    assert not bad, bad
    assert skipped * 2 < total, (skipped, total)
    assert seen == {"general", "scalar", "patch", "split", "paired", "promoted"}, seen


def _wino_expected(B, H, W, cin, cout, kh, kw, stride):
    """Whether ofx_conv_wino_choose takes an fp32 plain ReLU / identity layer with 'same' padding and an aligned
    operand, from their documented conditions: stride 1, a map of whole 8x16 patches, whole 16-channel slabs; then 3x3: at least
    1024 (patch, 64-channel block) workgroups; 1x5 / 5x1: at least 256 patches."""
    fits = (kh, kw) in ((3, 3), (1, 5), (5, 1)) and stride == 1 and H % 8 == 0 and W % 16 == 0 and cin % 16 == 0
    patches = B * (H // 8) * (W // 16)
    pays = patches * -(-cout // 64) >= 1024 if (kh, kw) == (3, 3) else patches >= 256
    return fits and pays


def test_winograd_gate():
    """tile = 0 with a Winograd operand: the fused path exactly where the layer fits and the grid pays, on both sides of the
    1024-patch-column (3x3) and 256-patch (1x5 / 5x1) thresholds."""
    cases = [
        (2, 64, 128, 64, 128, 3, 3, 1),      # 128 patches x 2 blocks = 256 columns: direct
        (8, 64, 128, 64, 128, 3, 3, 1),      # 512 x 2 = 1024: fused
        (8, 64, 128, 64, 64, 3, 3, 1),       # 512 x 1: direct
        (16, 64, 120, 64, 64, 3, 3, 1),      # 120 % 16 != 0: does not fit
        (16, 64, 128, 64, 64, 3, 3, 2),      # strided: does not fit
        (16, 64, 128, 24, 64, 3, 3, 1),      # 24 channels: no whole slab
        (16, 64, 128, 64, 65, 3, 3, 1),      # 1024 x 2: fused
        (3, 64, 128, 128, 128, 1, 5, 1),     # 192 patches: direct
        (4, 64, 128, 128, 128, 1, 5, 1),     # 256: fused
        (4, 64, 128, 128, 128, 5, 1, 1),
        (4, 64, 128, 128, 128, 7, 7, 1),     # no Winograd form
    ]
    paths = set()
    for B, H, W, cin, cout, kh, kw, stride in cases:
        st, p = _query(_desc(B, H, W, cin, cout, kh, kw, stride, wino=True, act=1), stats_cap=0)
        assert st == 0
        want = _wino_expected(B, H, W, cin, cout, kh, kw, stride)
        assert (p.path != 0) == want, (B, H, W, cin, cout, kh, kw, stride, p.path)
        if want:
            assert p.path == (1 if kh == 3 else 2)
        paths.add(p.path)
    assert paths == {0, 1, 2}
    # statistics are of raw outputs: one row per 8x16 patch from the fused 3x3 kernel, and only with room for them
    st, p = _query(_desc(8, 64, 128, 64, 128, 3, 3, wino=True), stats_cap=BIG)
    assert st == 0 and p.path == 1 and p.stats_rows == 8 * 8
    st, p = _query(_desc(8, 64, 128, 64, 128, 3, 3, wino=True), stats_cap=8 * 64 * 128 * 2 - 1)
    assert st == 0 and p.path == 0


def test_forced_winograd_on_a_shape_that_does_not_fit_is_rejected():
    assert _query(_desc(2, 64, 128, 64, 128, 3, 3, tile=TILE_WINOGRAD, wino=True))[0] == 0       # fits: forced below the threshold
    assert _query(_desc(2, 64, 120, 64, 128, 3, 3, tile=TILE_WINOGRAD, wino=True))[0] == EINVAL
    assert _query(_desc(2, 64, 128, 64, 128, 3, 3, stride=2, tile=TILE_WINOGRAD, wino=True))[0] == EINVAL
    assert _query(_desc(2, 64, 128, 64, 128, 3, 3, tile=TILE_WINOGRAD))[0] == EINVAL             # no operand


_CHILD = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
from sd_animation_optical_flow_amd import _lib
d, p = _lib.ConvDesc(), _lib.ConvPlan()          # 16 frames of 68 x 120, 64 -> 128 channels, 3x3
d.in0 = d.w = d.out = 0x10000
d.ld0 = d.c0 = 64
d.ldo = d.Cout = 128
d.B, d.Hin, d.Win, d.Hout, d.Wout = 16, 68, 120, 68, 120
d.KH = d.KW = 3
d.stride = d.padH = d.padW = 1
st = _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 0, C.byref(p))
print(st, p.bm, p.bn, p.bk, p.mode, p.mtiles)
"""


def _child_plan(env_value):
    env = dict(os.environ)
    env.pop("OFX_PATCH_MAX_WASTE", None)
    if env_value is not None:
        env["OFX_PATCH_MAX_WASTE"] = env_value
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, check=True, capture_output=True, text=True)
    return out.stdout.split()


def test_malformed_knob_falls_back_to_the_default():
    """The knobs are read once per process: each setting in a fresh child.  A 68 x 120 map is covered 1.13x by 8x16 patches: past the
    default bound of 1.09, so the default plan is not the halo patch (mode 2), and a well-formed larger bound makes it one."""
    default = _child_plan(None)
    assert default[:3] == ["0", "128", "128"] and default[4] != "2", default
    for bad in ("abc", "1.2x", "0.5", ""):
        assert _child_plan(bad) == default, bad
    assert _child_plan("1.2")[4] == "2"
