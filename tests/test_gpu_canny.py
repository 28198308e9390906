"""-m gpu: `ops.canny` (ofx_canny_u8) bit for bit against the restatement of cv2.Canny in tests/canny_check.py, on 1 and 3 channels:
sizes below, at and across the kernels' tiles, a batch, inputs whose hysteresis needs several batches of sweeps, every threshold
form; `ofx_detect_edges`, which shares the kernels, unchanged; `canny_condition` into `make_hint`.  Seconds."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import canny_check as CK   # noqa: E402
from oracle import keyframe_oracle as KO   # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 37), (33, 1), (9, 33), (32, 32), (64, 96), (70, 101)]
THRESHOLDS = [(100, 200), (200, 100), (0, 0), (255, 255), (50.9, 150.2), (51.9, 151.9)]


@pytest.fixture(scope="module")
def ops(cuda):
    from sd_animation_optical_flow_amd import ops as O
    return O


def _run(ops, imgs, low, high):
    return ops.canny(torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), low, high).cpu().numpy()


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("H,W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_sizes(ops, H, W, channels):
    img = CK.seeded_images(H, W, channels, 100 * H + W)
    for low, high in ((100, 200), (20, 60)):
        got = _run(ops, img, low, high)
        assert got.shape == (1, H, W) and got.dtype == np.uint8
        assert np.array_equal(got[0], CK.canny_u8(img[0], low, high)), (low, high, int((got[0] != CK.canny_u8(img[0], low, high)).sum()))


@pytest.mark.parametrize("channels", [1, 3])
def test_batch_of_different_images_and_every_threshold_form(ops, channels):
    imgs = CK.seeded_images(70, 101, channels, 7, n=3)
    imgs[1] //= 3                                                # weak edges only
    assert not np.array_equal(imgs[0], imgs[2])
    on = []
    for low, high in THRESHOLDS:
        got = _run(ops, imgs, low, high)
        for b in range(3):
            ref = CK.canny_u8(imgs[b], low, high)
            assert np.array_equal(got[b], ref), (low, high, b, int((got[b] != ref).sum()))
        on.append(int((got > 0).sum()))
    assert on[0] == on[1] and 0 < on[3] < on[0] < on[2]           # swapped thresholds; (255,255) keeps less, (0,0) more
    lo, hi = CK.thresholds(0, 0)
    mp = CK.canny_map(imgs[0], lo, hi)
    assert (mp == 2).any() and not (mp == 0).any()                # (0, 0): every candidate is strong


@pytest.mark.parametrize("name", ["grey", "grey-isolated", "grey-off", "colour", "colour-off"])
def test_serpentines(ops, name):
    """Strong pixels in the first 32x32 tile only; the path crosses all 25 tiles: 26 sweeps in the tile model, more than three
    batches of eight.  The -off inputs have candidates and no strong pixel: every output pixel is off."""
    img = {"grey": CK.serpentine(30, 60), "grey-isolated": CK.with_isolated_band(CK.serpentine(30, 60)), "grey-off": CK.serpentine(30, 30),
           "colour": CK.colour_serpentine(), "colour-off": CK.colour_serpentine(blue=False)}[name]
    ref = CK.canny_u8(img, 100, 200)
    if name.endswith("-off"):
        assert not ref.any() and (CK.canny_map(img, 100, 200) == 0).any()
    else:
        assert int((ref[-32:] > 0).sum()) == 322 and CK.sweep_count(CK.canny_map(img, 100, 200)) > 3 * CK.SWEEP_BATCH
    got = _run(ops, img[None], 100, 200)[0]
    assert np.array_equal(got, ref), int((got != ref).sum())
    assert set(np.unique(got)) <= {0, 255}


def test_colour_is_not_a_grey_conversion(ops):
    """The channel choice, not a luminance: one image whose map differs from Canny of max(B,G,R) and of every single channel."""
    img = CK.seeded_images(64, 96, 3, 11)[0]
    got = _run(ops, img[None], 100, 200)[0]
    assert np.array_equal(got, CK.canny_u8(img, 100, 200))
    for grey in [img.max(axis=2)] + [np.ascontiguousarray(img[..., c]) for c in range(3)]:
        assert not np.array_equal(got, CK.canny_u8(grey, 100, 200))
    tie = CK.tie_case()
    for t in (tie, np.ascontiguousarray(tie[..., ::-1])):
        big = np.zeros((9, 9, 3), dtype=np.uint8)
        big[3:6, 3:6] = t
        assert np.array_equal(_run(ops, big[None], 100, 200)[0], CK.canny_u8(big, 100, 200))


def test_refusals(ops):
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device="cuda")
    for bad in (z(1, 8, 8, dt=torch.float32), z(8, 8), z(1, 8, 8, 4), z(1, 8, 8, 1), z(1, 8, 16, 3)[:, :, ::2], z(1, 8, 8).cpu()):
        with pytest.raises(RuntimeError):
            ops.canny(bad, 100, 200)


def test_detect_edges_is_unchanged(cuda):
    from sd_animation_optical_flow_amd import ops as O
    frame = CK.seeded_images(70, 101, 3, 21)
    k = KO.estimated_kernel_size(101, 70)
    got = O.detect_edges(torch.from_numpy(frame).cuda(), k).cpu().numpy()[0]
    assert np.array_equal(got, KO.detect_edges(frame[0], k))


def test_canny_condition_feeds_make_hint_on_the_device(ops):
    from sd_animation_optical_flow_amd.controlnet import canny_condition, make_hint
    frame = CK.seeded_images(64, 96, 3, 3)[0]
    ref = CK.canny_u8(frame, 100, 200)
    cond = canny_condition(frame, 100, 200)                       # a numpy frame
    assert cond.is_cuda and cond.dtype == torch.uint8 and tuple(cond.shape) == (64, 96)
    assert np.array_equal(cond.cpu().numpy(), ref)
    dev_frame = torch.from_numpy(frame).cuda()
    cond2 = canny_condition(dev_frame, 100.0, 200.0)              # a device frame: nothing goes through the host
    assert torch.equal(cond, cond2)
    grey = canny_condition(np.ascontiguousarray(frame[..., 1]), 100, 200)
    assert np.array_equal(grey.cpu().numpy(), CK.canny_u8(np.ascontiguousarray(frame[..., 1]), 100, 200))
    hint = make_hint("canny", cond)
    assert hint.is_cuda and tuple(hint.shape) == (1, 3, 64, 96)
    want = torch.from_numpy(ref).float() / 255.0
    assert all(torch.equal(hint[0, c].cpu(), want) for c in range(3))
    with pytest.raises(ValueError):
        canny_condition(frame.astype(np.float32), 100, 200)
    with pytest.raises(ValueError):
        canny_condition(np.zeros((8, 8, 4), dtype=np.uint8), 100, 200)
