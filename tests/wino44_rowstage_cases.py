"""Cases of the F(4x4,3x3) slab pipeline's tests (not a conftest: imported by name by tests/test_gpu_conv_winograd44_rowstage.py and
tools/wino44_bits.py): the smallest shapes at which a pipeline over 8-channel slabs, two per trip, double-buffered, can go wrong.

Tuples as wino44_check.CASES: (name, B, H, W, (c0, c1), Cout, distribution, relu, scale/shift, (ldo, offset) or None).
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino44_rowstage")
MAX_ARRAY_BYTES = 300 * 1024      # larger outputs are recorded as their SHA-256 (sha256.json)

CASES = [
    # channel depth on one 16x32 patch: one trip (the prologue alone feeds both slabs), the first reuse of both parities, the first
    # overwrite of a buffer while neighbouring waves still read the other -- in one segment and with a slab pair across the switch
    ("cin16", 1, 16, 32, (16, 0), 64, "normal", False, False, None),
    ("cin32", 1, 16, 32, (32, 0), 64, "normal", False, False, None),
    ("cin48", 1, 16, 32, (48, 0), 64, "normal", False, False, None),
    ("cin48_seg_32_16", 1, 16, 32, (32, 16), 64, "normal", False, False, None),
    ("cin64", 1, 16, 32, (64, 0), 64, "normal", False, False, None),
    # borders: 2x2 patches per image, out-of-map halo rows and columns on every border and shared halos between patches
    ("borders_2x2x2", 2, 32, 64, (32, 0), 64, "relu", True, True, None),
    # epilogue: a Cout tail into a strided destination with NaN-filled neighbours
    ("strided_co126_cin48", 1, 16, 32, (48, 0), 126, "tanh", True, True, (192, 33)),
    # a resident grid: 768 workgroups, three rounds over 256 CUs
    ("resident_768", 24, 64, 256, (48, 0), 64, "normal", True, False, None),
]
SEED0 = 500


def seed(case):
    return SEED0 + CASES.index(case)


def sha256(t):
    """SHA-256 of an NCHW float32 cpu tensor's bytes (C order)."""
    a = np.ascontiguousarray(t.numpy())
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()
