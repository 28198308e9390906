#!/usr/bin/env python3
"""Golden vectors of the `fill_mask_input` chain (guided_ldm_inpainting.py:161-176), produced by the REAL Pillow.

    python tests/golden/make_golden_fill.py        # writes tests/golden/fill_mask_pil.npz

For every case: a seeded frame and an already blurred 'L' mask go through Pillow's paste onto a premultiplied canvas, the six
GaussianBlur stages with their alpha_composite repeats and the final convert('RGB') (tests/fill_check.py:pil_fill_mask_input).
One case also keeps the radius-256 GaussianBlur of its pasted RGBa image, the input of the device's 4-channel blur.  The numpy
restatement (tests/fill_check.py) must reproduce every array bit for bit, checked here at generation time and again by
tests/test_fill_host.py.
"""
import os
import sys

import numpy as np
import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fill_check as FC  # noqa: E402

# name: (seed, H, W, kind)
CASES = {"a": (11, 40, 24, "blobs"),          # the radius-256 box radius (255) exceeds both sides
         "b": (12, 17, 300, "blobs"),
         "c": (13, 64, 96, "blobs"),
         "d": (14, 8, 8, "noise"),
         "e": (15, 1, 1, "noise"),
         "full": (16, 12, 20, "full"),        # everything masked: the canvas stays empty, the output is 0
         "none": (17, 12, 20, "none")}        # nothing masked: the output is the input


def main():
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array(sorted(CASES))}
    for name, (seed, H, W, kind) in CASES.items():
        image, mask = FC.random_case(seed, H, W, kind)
        want = FC.pil_fill_mask_input(image, mask)
        assert np.array_equal(FC.fill_mask_input(image, mask), want), name
        out[f"{name}_image"], out[f"{name}_mask"], out[f"{name}_pil_fill"] = image, mask, want
    assert not out["full_pil_fill"].any() and np.array_equal(out["none_pil_fill"], out["none_image"])
    pasted = FC.paste(out["a_image"], out["a_mask"])
    out["a_pil_blur256"] = FC.pil_blur_rgba(pasted, 256)
    assert np.array_equal(FC.blur_rgba(pasted, 256), out["a_pil_blur256"])
    path = FC.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; restatement == Pillow", PIL.__version__, "on all cases")


if __name__ == "__main__":
    main()
