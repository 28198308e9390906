"""CPU: the numpy restatement of `fill_mask_input` (tests/fill_check.py) against the Pillow vectors of
tests/golden/fill_mask_pil.npz and, where Pillow is importable, against live Pillow; and the refusals of the new path that come
before a device is touched."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_check as FC   # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(FC.GOLDEN)


def test_restatement_reproduces_the_pillow_vectors(gold):
    names = [str(n) for n in gold["names"]]
    assert sorted(names) == ["a", "b", "c", "d", "e", "full", "none"]
    shapes = {n: gold[f"{n}_mask"].shape for n in names}
    assert {shapes[n] for n in "abcde"} == {(40, 24), (17, 300), (64, 96), (8, 8), (1, 1)}
    for n in names:
        assert np.array_equal(FC.fill_mask_input(gold[f"{n}_image"], gold[f"{n}_mask"]), gold[f"{n}_pil_fill"]), n
    assert not gold["full_pil_fill"].any()                                   # everything masked: nothing to bleed in
    assert np.array_equal(gold["none_pil_fill"], gold["none_image"])         # nothing masked: the frame itself
    pasted = FC.paste(gold["a_image"], gold["a_mask"])
    assert np.array_equal(FC.blur_rgba(pasted, 256), gold["a_pil_blur256"])


@pytest.mark.parametrize("seed,H,W,kind", [(1, 1, 1, "noise"), (2, 3, 700, "noise"), (3, 130, 70, "blobs"), (4, 33, 47, "noise"),
                                           (5, 5, 9, "full"), (6, 20, 31, "blobs"), (7, 2, 2, "noise"), (8, 9, 1, "blobs")])
def test_restatement_reproduces_live_pillow(seed, H, W, kind):
    pytest.importorskip("PIL")
    image, mask = FC.random_case(1000 + seed, H, W, kind)
    assert np.array_equal(FC.fill_mask_input(image, mask), FC.pil_fill_mask_input(image, mask))
    pasted = FC.paste(image, mask)
    for radius in (2, 7.5, 64):
        assert np.array_equal(FC.blur_rgba(pasted, radius), FC.pil_blur_rgba(pasted, radius)), radius


def test_unmasked_pixels_come_back_unchanged(gold):
    """Where the blurred mask is 0 the pasted pixel is opaque, so the radius-0 stage (alpha 255, coef1 = 255 * 128) replaces
    whatever the blurred stages left there."""
    cases = [(gold[f"{n}_image"], gold[f"{n}_mask"]) for n in ("a", "b", "c")]
    rng = np.random.default_rng(5)
    hole = np.zeros((48, 64), np.uint8)
    hole[10:30, 20:44] = 255                                                 # one blob: the blur leaves most of the frame at 0
    cases.append((rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), FC.HO.gaussian_blur_u8(hole, 4.0)))
    seen = 0
    for image, mask in cases:
        keep = mask == 0
        seen += int(keep.sum())
        out = FC.fill_mask_input(image, mask)
        assert np.array_equal(out[keep], image[keep])
    assert seen > 1000 and not np.array_equal(out, image)


def test_refusals_without_a_device():
    from sd_animation_optical_flow_amd.handoff import prepare_inpaint_inputs
    from sd_animation_optical_flow_amd.sampler import img2img_inpaint
    stub = types.SimpleNamespace(in_channels=9, out_channels=4, in_pad=12, cfg=dict(context_dim=64), device=torch.device("cpu"))
    img = np.zeros((64, 96, 3), np.uint8)
    with pytest.raises(NotImplementedError):                                 # no reference and fill_masked not asked for
        img2img_inpaint(stub, None, None, img, None, img[..., 0], None, None, fill_masked=False)
    with pytest.raises(ValueError, match="fill"):                            # noise["fill"] belongs to the fill_masked path
        img2img_inpaint(stub, None, None, img, img, img[..., 0], None, None, denoising_strength=0.5, ddim_steps=10,
                        noise=dict(fill=torch.zeros((1, 4, 8, 12))))
    with pytest.raises(ValueError, match="reference"):
        img2img_inpaint(stub, None, None, img, img, img[..., 0], None, None, denoising_strength=0.5, ddim_steps=10, fill_masked=True)
    with pytest.raises(ValueError, match="reference"):
        prepare_inpaint_inputs(img, img, img[..., 0], fill_masked=True, device="cpu")
