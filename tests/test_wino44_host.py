"""Host side of the Winograd F(4x4,3x3) route: the weight transform ofx_wino44_conv_weight and the launcher's plan.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

OFX_EINVAL = -1   # include/ofx.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def _lib():
    from sd_animation_optical_flow_amd import _lib
    return _lib


G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
             dtype=np.float64)


def index(q, o, c, NB, cin):
    """The documented operand order (conv_wino.hip, ofx_wino44_conv_weight): point q, output channel o = 32 nb + n, input channel
    c = 8 c8 + 4 h + 2 s + e at float ((((q NB + nb) cin / 8 + c8) 2 + s) 2 + h) 64 + 2 n + e."""
    nb, n = o // 32, o % 32
    c8, h, s, e = c // 8, (c % 8) // 4, (c % 4) // 2, c % 2
    return ((((q * NB + nb) * (cin // 8) + c8) * 2 + s) * 2 + h) * 64 + 2 * n + e


@pytest.mark.parametrize("cin", [16, 48, 256])
@pytest.mark.parametrize("co", [1, 33, 64, 65, 126, 192])
def test_weight_transform_against_numpy_float64(co, cin):
    ops = _ops()
    rng = np.random.default_rng(1000 * co + cin)
    w = (rng.standard_normal((co, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    got = ops.wino44_conv_weight(torch.from_numpy(w)).numpy()
    NB = 2 * ((co + 63) // 64)
    assert got.shape == (36 * NB * 32 * cin,)
    # U = G g G^T in float64, point 6 i + j; the sums left to right (1/6 and 1/24 are not exact: the order is part of the result)
    g = w.astype(np.float64)
    gg = [[G[i, 0] * g[:, :, 0, x] + G[i, 1] * g[:, :, 1, x] + G[i, 2] * g[:, :, 2, x] for x in range(3)] for i in range(6)]
    u = np.stack([gg[i][0] * G[j, 0] + gg[i][1] * G[j, 1] + gg[i][2] * G[j, 2] for i in range(6) for j in range(6)])
    ref = np.zeros_like(got)
    q, o, c = np.meshgrid(np.arange(36), np.arange(co), np.arange(cin), indexing="ij")
    ref[index(q, o, c, NB, cin)] = u.astype(np.float32)                                   # rounded once; the padding stays zero
    assert np.array_equal(got, ref)


def test_size_query_and_slab_rule():
    lib = _lib().lib()
    assert lib.ofx_wino44_conv_weight(None, 126, 256, None) == 36 * 128 * 256
    assert lib.ofx_wino44_conv_weight(None, 1, 16, None) == 36 * 64 * 16
    assert lib.ofx_wino44_conv_weight(None, 64, 24, None) == OFX_EINVAL                   # Cin must be whole 16-channel slabs
    w = torch.zeros((64, 24, 3, 3))
    out = torch.zeros((36 * 64 * 32,))
    assert lib.ofx_wino44_conv_weight(C.c_void_p(w.data_ptr()), 64, 24, C.c_void_p(out.data_ptr())) == OFX_EINVAL
    with pytest.raises(Exception):
        _ops().wino44_conv_weight(torch.zeros((8, 24, 3, 3)))


def _desc(B=64, H=64, W=96, c0=128, c1=0, co=64, stride=1, w2=True, w4=True, **kw):
    L = _lib()
    d = L.ConvDesc()
    d.in0, d.ld0, d.c0 = 4096, c0, c0
    if c1:
        d.in1, d.ld1, d.c1 = 8192, c1, c1
    d.w, d.out, d.ldo = 4096, 4096, co
    d.B, d.Hin, d.Win, d.Cout = B, H, W, co
    d.Hout, d.Wout = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    d.KH = d.KW = 3
    d.stride, d.padH, d.padW = stride, 1, 1
    d.act = 1
    if w2:
        d.wino_w = 4096
    if w4:
        d.wino4_w = 4096
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _plan(d, stats=0):
    L = _lib()
    p = L.ConvPlan()
    st = L.lib().ofx_conv2d_plan(C.byref(d), stats, 0, C.byref(p))
    return st, p.path


GATE = 768   # workgroups: 16x32 patches x 64-channel blocks (the F(4x4,3x3) row's grid gate in conv_wino.hip)


def test_plan_takes_path_3_where_it_fits_and_pays():
    # 64x96: 12 patches per image
    assert _plan(_desc(B=64, co=64)) == (0, 3)                     # 768 workgroups: on the gate
    assert _plan(_desc(B=63, co=64)) == (0, 1)                     # 756: below it, F(2x2) as before
    assert _plan(_desc(B=16, co=256)) == (0, 3)                    # 16 * 12 * 4 = 768
    assert _plan(_desc(B=15, co=256)) == (0, 1)
    assert _plan(_desc(B=22, co=192)) == (0, 3)                    # 792
    assert _plan(_desc(B=21, co=192)) == (0, 1)                    # 756
    assert _plan(_desc(B=32, co=126, c0=192, c1=64)) == (0, 3)     # two segments, 126 -> two blocks
    assert _plan(_desc(B=5, co=256)) == (0, 0) or _plan(_desc(B=5, co=256)) == (0, 1)   # small batches: never path 3
    assert _plan(_desc(B=5, co=256))[1] == _plan(_desc(B=5, co=256, w4=False))[1]


def test_plan_shape_rules():
    big = dict(B=2048, co=64)
    assert _plan(_desc(H=16, W=32, **big)) == (0, 3)
    assert _plan(_desc(H=16, W=16, **big))[1] != 3
    assert _plan(_desc(H=8, W=32, **big))[1] != 3
    assert _plan(_desc(stride=2, **big))[1] != 3
    assert _plan(_desc(addend=4096, ldadd=64, **big))[1] != 3
    assert _plan(_desc(nmean=4096, nrstd=4096, **big))[1] != 3
    assert _plan(_desc(res=4096, ldres=64, **big))[1] != 3
    assert _plan(_desc(c0=24, **big))[1] != 3                      # whole 16-channel slabs
    assert _plan(_desc(wino4_w=4100, **big))[1] != 3               # 16-byte aligned operand
    assert _plan(_desc(**big), stats=1 << 30)[1] != 3              # requested statistics


def test_forced_tile():
    L = _lib()
    assert _plan(_desc(B=1, H=16, W=32, tile=2)) == (0, 3)         # forced below the gate
    for bad in (dict(H=16, W=16), dict(H=8, W=32), dict(w4=False), dict(stride=2), dict(addend=4096, ldadd=64)):
        st, _ = _plan(_desc(B=1, tile=2, **{"H": 16, "W": 32, **bad}))
        assert st != 0 and "invalid" in L.error_string(st).lower(), bad


def test_descriptors_without_the_new_operand_plan_as_before():
    assert _plan(_desc(B=64, co=64, w4=False)) == (0, 1)
    assert _plan(_desc(B=2, co=64, w4=False)) == (0, 0)
    assert _plan(_desc(B=64, co=64, w2=False, w4=False)) == (0, 0)
    assert _plan(_desc(B=64, co=64, w2=False)) == (0, 3)           # the F(4x4) operand alone


_SWITCH_SCRIPT = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd import _lib
paths = []
for B, co in ((64, 64), (16, 256), (2, 64)):        # 768 and 768 workgroups (on the gate), and a small batch
    d = _lib.ConvDesc()
    d.in0, d.ld0, d.c0 = 4096, 128, 128
    d.w, d.out, d.ldo = 4096, 4096, co
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, 64, 96, 64, 96, co
    d.KH = d.KW = 3
    d.stride = d.padH = d.padW = d.act = 1
    d.wino_w = d.wino4_w = 4096
    p = _lib.ConvPlan()
    assert _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 0, C.byref(p)) == 0
    paths.append(p.path)
print(*paths)
"""


def test_the_switches_are_read_by_the_plan():
    """OFX_CONV_NO_WINOGRAD4 keeps F(2x2,3x3) where F(4x4,3x3) would run; OFX_CONV_NO_WINOGRAD turns every route off (each read
    once per process, hence child processes; the plan needs no GPU)."""
    def run(extra):
        env = {k: v for k, v in os.environ.items() if k not in ("OFX_CONV_NO_WINOGRAD", "OFX_CONV_NO_WINOGRAD4")}
        env.update(extra)
        out = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout.split()[-3:]

    assert run({}) == ["3", "3", "0"]
    assert run({"OFX_CONV_NO_WINOGRAD4": "1"}) == ["1", "1", "0"]
    assert run({"OFX_CONV_NO_WINOGRAD": "1"}) == ["0", "0", "0"]
