"""Host side of the fused variants of the Winograd F(4x4,3x3) route (plan path 4): a descriptor with a residual merge, a fused
norm or requested statistics plans to path 4 where the plain kernel's shape rules, the F(2x2,3x3) route's rules for the fused norm
and the grid gate hold, never to path 3, and falls back to F(2x2,3x3) or the direct kernels otherwise.  No GPU.
"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 4096


def _lib():
    from sd_animation_optical_flow_amd import _lib
    return _lib


def _desc(B=64, H=64, W=96, c0=128, c1=0, co=64, stride=1, w2=True, w4=True, act=1, **kw):
    L = _lib()
    d = L.ConvDesc()
    d.in0, d.ld0, d.c0 = PTR, c0, c0
    if c1:
        d.in1, d.ld1, d.c1 = 2 * PTR, c1, c1
    d.w, d.out, d.ldo = PTR, PTR, co
    d.B, d.Hin, d.Win, d.Cout = B, H, W, co
    d.Hout, d.Wout = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    d.KH = d.KW = 3
    d.stride, d.padH, d.padW = stride, 1, 1
    d.act = act
    if w2:
        d.wino_w = PTR
    if w4:
        d.wino4_w = PTR
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _plan(d, stats=0):
    L = _lib()
    p = L.ConvPlan()
    st = L.lib().ofx_conv2d_plan(C.byref(d), stats, 0, C.byref(p))
    return st, p.path, p.stats_rows


NORM = dict(nmean=PTR, nrstd=PTR)
RES = dict(res=PTR, ldres=64)
BIG = 1 << 30          # statistics room, floats


def test_fused_descriptors_take_path_4_on_and_above_the_gate():
    # 64x96: 12 patches of 16x32 per image; the gate is 768 workgroups (patches x 64-channel blocks)
    for B in (64, 65, 128):
        assert _plan(_desc(B=B, **NORM)) == (0, 4, 0)
        assert _plan(_desc(B=B, **RES)) == (0, 4, 0)
        assert _plan(_desc(B=B, act=0), stats=BIG) == (0, 4, 12)
        assert _plan(_desc(B=B, act=0, **NORM), stats=BIG) == (0, 4, 12)
        assert _plan(_desc(B=B, **NORM, **RES)) == (0, 4, 0)
    assert _plan(_desc(B=16, co=256, **NORM)) == (0, 4, 0)                     # 16 * 12 * 4 = 768
    assert _plan(_desc(B=22, co=192, res=PTR, ldres=192)) == (0, 4, 0)         # 792
    assert _plan(_desc(B=32, co=96, c0=96, act=0, **NORM), stats=BIG) == (0, 4, 12)   # 96 channels: two blocks, 768
    # the three encoder stages of 64 pairs of 512x768 (fnet: norm on load + statistics)
    for c, H, W in ((64, 384, 256), (96, 192, 128), (128, 96, 64)):
        assert _plan(_desc(B=64, H=H, W=W, c0=c, co=c, act=0, **NORM), stats=BIG) == (0, 4, (H // 16) * (W // 32))
        assert _plan(_desc(B=64, H=H, W=W, c0=c, co=c, res=PTR, ldres=c)) == (0, 4, 0)


def test_path_1_just_below_the_gate():
    assert _plan(_desc(B=63, **NORM)) == (0, 1, 0)                             # 756 workgroups: F(2x2) as before
    assert _plan(_desc(B=63, **RES)) == (0, 1, 0)
    assert _plan(_desc(B=63, act=0), stats=BIG) == (0, 1, 48)                  # one row per 8x16 patch there
    assert _plan(_desc(B=63, act=0, **NORM), stats=BIG) == (0, 1, 48)
    assert _plan(_desc(B=15, co=256, **NORM)) == (0, 1, 0)
    assert _plan(_desc(B=21, co=192, res=PTR, ldres=192)) == (0, 1, 0)         # 756
    # small batches never take it, and plan as a descriptor without the operand does
    for kw in (NORM, RES):
        assert _plan(_desc(B=5, co=256, **kw))[1] in (0, 1)
        assert _plan(_desc(B=5, co=256, **kw))[:2] == _plan(_desc(B=5, co=256, w4=False, **kw))[:2]


def test_statistics_rows_and_room():
    B, H, W, co = 64, 64, 96, 64
    rows = (H // 16) * (W // 32)
    need = B * rows * co * 2
    assert _plan(_desc(act=0), stats=need) == (0, 4, rows)
    assert _plan(_desc(act=0), stats=need - 1)[1] != 4                         # one float too small
    assert _plan(_desc(act=0), stats=4 * need) == (0, 4, rows)
    # statistics are of raw outputs: not of a ReLU, not with a residual merge
    assert _plan(_desc(act=1), stats=BIG)[1] != 4
    assert _plan(_desc(act=0, **RES), stats=BIG)[1] != 4
    assert _plan(_desc(B=192, H=32, W=64, act=0), stats=BIG) == (0, 4, 4)           # 192 * 4 patches


def test_never_path_4():
    big = dict(B=256, co=64)                                                   # 3072 workgroups at 64x96

    def path(d, valid=True):
        st, pth, _ = _plan(d)
        assert (st == 0) == valid, st
        return pth

    assert path(_desc(**big, **NORM)) == 4
    assert path(_desc(B=2048, H=16, W=32, co=64, **NORM)) == 4
    assert path(_desc(c0=192, c1=64, **big, **NORM), valid=False) not in (3, 4)   # two input segments with a fused norm
    assert path(_desc(c0=192, c1=64, **big, **RES)) == 4                       # (a residual merge takes two)
    assert path(_desc(addend=PTR, ldadd=64, **big, **RES)) not in (3, 4)
    assert path(_desc(stride=2, **big, **RES)) not in (3, 4)
    assert path(_desc(B=2048, H=8, W=32, co=64, **NORM)) not in (3, 4)
    assert path(_desc(B=2048, H=16, W=16, co=64, **RES)) not in (3, 4)
    assert path(_desc(wino4_w=PTR + 4, **big, **NORM)) not in (3, 4)           # 16-byte aligned operand
    assert path(_desc(nmean=PTR + 4, nrstd=PTR, **big), valid=False) not in (3, 4)   # ... and mean / rstd
    assert path(_desc(nmean=PTR, **big), valid=False) not in (3, 4)            # a mean without its rstd
    assert path(_desc(c0=24, **big, **RES)) not in (3, 4)                      # whole 16-channel slabs
    # the fused norm stages 2 x Cin floats in the LDS the slabs leave free: at most 1744 input channels (16 images x 12 x 4 = 768)
    wide = dict(B=16, co=256)
    assert path(_desc(c0=1744, **wide, **NORM)) == 4
    assert path(_desc(c0=1760, **wide, **NORM)) == 1
    assert path(_desc(c0=1760, **wide)) == 3                                   # (the plain kernel has no such limit)
    assert path(_desc(c0=1760, **wide, res=PTR, ldres=256)) == 4               # (nor has the residual merge)
    assert path(_desc(res=PTR, ldres=32, **big), valid=False) not in (3, 4)    # a residual row shorter than Cout
    assert path(_desc(w4=False, **big, **NORM)) == 1                           # without the operand: as before
    assert path(_desc(w4=False, **big, **RES)) == 1
    # a fused descriptor never plans to the plain kernel, a plain one never to the fused variants
    assert path(_desc(**big)) == 3
    assert path(_desc(B=64)) == 3


def test_forced_tile():
    L = _lib()
    small = dict(B=1, H=16, W=32, tile=2)
    assert _plan(_desc(**small, **NORM)) == (0, 4, 0)                          # forced below the gate
    assert _plan(_desc(**small, **RES)) == (0, 4, 0)
    assert _plan(_desc(**small, act=0), stats=BIG) == (0, 4, 1)
    assert _plan(_desc(**small, act=0, **NORM), stats=BIG) == (0, 4, 1)
    assert _plan(_desc(**small, **NORM, **RES)) == (0, 4, 0)
    assert _plan(_desc(**small)) == (0, 3, 0)
    assert _plan(_desc(**small, c0=1744, **NORM)) == (0, 4, 0)
    bad = [
        (dict(act=0, **RES), BIG),                                             # statistics with a residual merge
        (dict(act=1), BIG),                                                    # statistics of a ReLU
        (dict(act=0), 1 * 1 * 64 * 2 - 1),                                     # statistics room one float too small
        (dict(c0=96, c1=32, **NORM), 0),                                       # fused norm over two segments
        (dict(H=8, W=32, **RES), 0),
        (dict(H=16, W=16, **NORM), 0),
        (dict(stride=2, **RES), 0),
        (dict(addend=PTR, ldadd=64, **RES), 0),
        (dict(w4=False, **NORM), 0),
        (dict(c0=1760, **NORM), 0),                                            # more channels than the staged means have room for
    ]
    for kw, stats in bad:
        st = _plan(_desc(**{**small, **kw}), stats=stats)[0]
        assert st != 0 and "invalid" in L.error_string(st).lower(), kw


_SWITCH_SCRIPT = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd import _lib
paths = []
for kind in ("norm", "res", "stats", "plain"):
    d = _lib.ConvDesc()
    d.in0, d.ld0, d.c0 = 4096, 128, 128
    d.w, d.out, d.ldo = 4096, 4096, 64
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = 64, 64, 96, 64, 96, 64
    d.KH = d.KW = 3
    d.stride = d.padH = d.padW = 1
    d.act = 0 if kind == "stats" else 1
    d.wino_w = d.wino4_w = 4096
    if kind == "norm":
        d.nmean = d.nrstd = 4096
    if kind == "res":
        d.res, d.ldres = 4096, 64
    p = _lib.ConvPlan()
    assert _lib.lib().ofx_conv2d_plan(C.byref(d), (1 << 30) if kind == "stats" else 0, 0, C.byref(p)) == 0
    paths.append(p.path)
print(*paths)
"""


def test_the_switches_are_read_by_the_plan():
    """OFX_CONV_NO_WINOGRAD4 keeps F(2x2,3x3) where the fused F(4x4,3x3) variants would run; OFX_CONV_NO_WINOGRAD turns every
    route off (each read once per process, hence child processes; the plan needs no GPU)."""
    def run(extra):
        env = {k: v for k, v in os.environ.items() if k not in ("OFX_CONV_NO_WINOGRAD", "OFX_CONV_NO_WINOGRAD4")}
        env.update(extra)
        out = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout.split()[-4:]

    assert run({}) == ["4", "4", "4", "3"]
    assert run({"OFX_CONV_NO_WINOGRAD4": "1"}) == ["1", "1", "1", "1"]
    assert run({"OFX_CONV_NO_WINOGRAD": "1"}) == ["0", "0", "0", "0"]
