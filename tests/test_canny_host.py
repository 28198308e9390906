"""No device: the restatement of cv2.Canny in tests/canny_check.py against oracle/keyframe_oracle.py and a frozen fixture, the
properties of the inputs the GPU test relies on (asserted on what the restatement returns), `ops.canny`'s refusals and the C ABI of
`ofx_canny_u8`."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import canny_check as CK   # noqa: E402
from oracle import keyframe_oracle as KO   # noqa: E402

EINVAL, EALIGN, ENOMEM = -1, -2, -3


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("noisy", [False, True], ids=["smooth", "noisy"])
def test_one_channel_equals_the_keyframe_oracle(seed, noisy):
    img = CK.seeded_images(70, 101, 1, seed)[0]
    if noisy:
        img = np.random.default_rng(seed).integers(0, 256, size=img.shape).astype(np.uint8)
    for low, high in ((100, 200), (20, 60), (0, 0), (255, 255)):
        assert np.array_equal(CK.canny_map(img, low, high), KO.canny_map(img, low, high))
        assert np.array_equal(CK.canny_u8(img, low, high), KO.canny(img, low, high))


def test_frozen_fixture():
    gold = np.load(os.path.join(HERE, "golden", "canny_semantics.npz"))
    names = sorted({k.split(".")[0] for k in gold.files})
    assert names == ["colour", "grey", "swapped"]
    for n in names:
        low, high = gold[f"{n}.thr"]
        assert np.array_equal(CK.canny_u8(gold[f"{n}.in"], low, high), gold[f"{n}.out"]), n


def test_serpentine_properties():
    s = CK.serpentine(30, 60)
    assert s.shape == (160, 160)
    mp = CK.canny_map(s, 100, 200)
    ys, xs = np.nonzero(mp == 2)
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (15, 21, 7, 20)            # strong pixels in the first tile only
    e = CK.canny_u8(s, 100, 200)
    assert np.array_equal(e, KO.canny(s, 100, 200))
    assert int((e > 0).sum()) == 1644 and int((e[-32:] > 0).sum()) == 322           # the far end is on
    assert not CK.canny_u8(CK.serpentine(30, 30), 100, 200).any()
    iso = CK.with_isolated_band(s)
    assert int((CK.canny_map(iso, 100, 200) == 0).sum()) > int((mp == 0).sum())     # more candidates ...
    assert np.array_equal(CK.canny_u8(iso, 100, 200), e)                            # ... and nothing more in the map
    sweeps = CK.sweep_count(mp)
    assert sweeps == 26 and sweeps > 3 * CK.SWEEP_BATCH


def test_colour_serpentine_properties():
    img = CK.colour_serpentine()
    assert not img[..., 1].any() and np.array_equal(img[..., 2], CK.serpentine(30, 30))
    mp = CK.canny_map(img, 100, 200)
    ys, xs = np.nonzero(mp == 2)
    assert ys.max() < 32 and xs.max() < 32
    e = CK.canny_u8(img, 100, 200)
    assert int((e[-32:] > 0).sum()) == 322                                          # the far end is on
    assert CK.sweep_count(mp) > 3 * CK.SWEEP_BATCH
    assert not CK.canny_u8(CK.colour_serpentine(blue=False), 100, 200).any()        # zeroing B empties the map
    assert not CK.canny_u8(np.ascontiguousarray(img[..., 2]), 100, 200).any()       # R alone has no strong pixel


def test_channel_tie_keeps_the_lowest_channel():
    img = CK.tie_case()
    per = [KO._sobel16(img[..., c]) for c in range(3)]
    norms = [int(abs(dx[1, 1]) + abs(dy[1, 1])) for dx, dy in per]
    assert norms[0] == norms[1] > norms[2] and (per[0][0][1, 1], per[0][1][1, 1]) != (per[1][0][1, 1], per[1][1][1, 1])
    dx, dy = CK.gradient(img)
    assert (dx[1, 1], dy[1, 1]) == (per[0][0][1, 1], per[0][1][1, 1])
    dx, dy = CK.gradient(np.ascontiguousarray(img[..., ::-1]))                      # channel 2 first: it loses to a larger later norm
    assert (dx[1, 1], dy[1, 1]) == (per[1][0][1, 1], per[1][1][1, 1])


def test_thresholds_are_swapped_and_floored():
    assert CK.thresholds(200, 100) == (100, 200) and CK.thresholds(50.9, 150.2) == (50, 150) and CK.thresholds(-0.5, 3) == (-1, 3)
    img = CK.seeded_images(33, 41, 3, 5)[0]
    assert np.array_equal(CK.canny_u8(img, 200, 100), CK.canny_u8(img, 100, 200))
    assert np.array_equal(CK.canny_u8(img, 50.9, 150.2), CK.canny_u8(img, 50, 150))
    # |dx| + |dy| of a 3x3 Sobel is even, so a threshold's floor shows only across an even number: 51.9 -> 51, not 52
    assert np.array_equal(CK.canny_u8(img, 51.9, 150.2), CK.canny_u8(img, 51, 150))
    assert not np.array_equal(CK.canny_u8(img, 51.9, 150.2), CK.canny_u8(img, 52, 150))


def test_ops_canny_refuses_before_any_launch():
    from sd_animation_optical_flow_amd import ops
    for bad in (torch.zeros((1, 8, 8), dtype=torch.uint8),                          # a CPU tensor
                torch.zeros((1, 8, 8), dtype=torch.float32), torch.zeros((8, 8), dtype=torch.uint8),
                torch.zeros((1, 8, 8, 4), dtype=torch.uint8), np.zeros((1, 8, 8), dtype=np.uint8)):
        with pytest.raises(RuntimeError):
            ops.canny(bad, 100, 200)


def test_c_abi_declares_and_checks_the_new_entry():
    from sd_animation_optical_flow_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofx.h")).read(), flags=re.S)
    for name in ("ofx_canny_u8", "ofx_canny_u8_scratch_bytes"):
        assert re.search(rf"\b{name}\s*\(", txt) and name in _lib.SIGNATURES
    lib = _lib.lib()
    need = lib.ofx_canny_u8_scratch_bytes(2, 70, 101)
    assert need >= 2 * 70 * 101 + 32 and need % 256 == 0
    assert lib.ofx_canny_u8_scratch_bytes(0, 70, 101) == 0 and lib.ofx_canny_u8_scratch_bytes(1, 0, 5) == 0
    # argument validation happens before any HIP call: fake, never dereferenced pointers
    p, al = 0x10000, 0x20000
    call = lambda *a: lib.ofx_canny_u8(*a, None)
    assert call(None, 1, p, al, need, 2, 70, 101, 100, 200) == EINVAL
    assert call(p, 1, None, al, need, 2, 70, 101, 100, 200) == EINVAL
    assert call(p, 1, p, None, need, 2, 70, 101, 100, 200) == EINVAL
    for ch in (0, 2, 4):
        assert call(p, ch, p, al, need, 2, 70, 101, 100, 200) == EINVAL
    for B in (0, -1, 65536):
        assert call(p, 3, p, al, 1 << 40, B, 70, 101, 100, 200) == EINVAL
    assert call(p, 3, p, al, need, 2, 0, 101, 100, 200) == EINVAL
    assert call(p, 3, p, al + 16, need, 2, 70, 101, 100, 200) == EALIGN
    assert call(p, 3, p, al, need - 1, 2, 70, 101, 100, 200) == ENOMEM
