"""Writes tests/golden/canny_semantics.npz: three small inputs and what tests/canny_check.py's restatement of cv2.Canny returns for
them, frozen so that the restatement cannot drift unnoticed (tests/test_canny_host.py compares).  No device, no reference tree:

    python tests/golden/make_golden_canny.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import canny_check as CK   # noqa: E402

CASES = (("grey", (1, 100.0, 200.0)), ("colour", (3, 50.9, 150.2)), ("swapped", (3, 200.0, 100.0)))


def main():
    out = {}
    for seed, (name, (ch, low, high)) in enumerate(CASES):
        img = CK.seeded_images(23, 37, ch, 900 + seed)[0]
        out[f"{name}.in"] = img
        out[f"{name}.thr"] = np.asarray([low, high], dtype=np.float64)
        out[f"{name}.out"] = CK.canny_u8(img, low, high)
        assert 0 < int((out[f"{name}.out"] > 0).sum()) < img.shape[0] * img.shape[1]
    np.savez_compressed(os.path.join(HERE, "canny_semantics.npz"), **out)


if __name__ == "__main__":
    main()
