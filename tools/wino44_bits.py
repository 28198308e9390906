#!/usr/bin/env python3
"""The F(4x4,3x3) kernel's output bits on the cases of tests/wino44_rowstage_cases.py, forced with TILE_WINOGRAD4:

    python tools/wino44_bits.py write [DIR]    -> DIR/<case>.npy, or its SHA-256 in DIR/sha256.json where the array would be too
                                                  large to commit; DIR defaults to tests/golden/wino44_rowstage
    python tools/wino44_bits.py compare [DIR]  -> every case torch.equal / the same digest as recorded (exit status 1 otherwise)

Run `write` on the build whose bits are the reference (the parent of a schedule change), `compare` on the new one; OFX_LIB_PATH
selects a build.  tests/test_gpu_conv_winograd44_rowstage.py holds the kernel to the recorded bits."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wino44_check as w4  # noqa: E402
import wino44_rowstage_cases as rc  # noqa: E402
from sd_animation_optical_flow_amd import ops  # noqa: E402


def main():
    mode = sys.argv[1]
    assert mode in ("write", "compare")
    golden = sys.argv[2] if len(sys.argv) > 2 else rc.GOLDEN
    os.makedirs(golden, exist_ok=True)
    sha_path = os.path.join(golden, "sha256.json")
    shas = json.load(open(sha_path)) if mode == "compare" and os.path.exists(sha_path) else {}
    bad = []
    for case in rc.CASES:
        c = w4.make(case, rc.seed(case))
        got, _ = w4.run(ops, c, ops.TILE_WINOGRAD4, w4.operands(ops, c["w"]))
        name = case[0]
        path = os.path.join(golden, name + ".npy")
        small = got.numel() * 4 <= rc.MAX_ARRAY_BYTES
        if mode == "write":
            if small:
                np.save(path, got.numpy())
            else:
                shas[name] = rc.sha256(got)
            print(f"{name}: {tuple(got.shape)} {'array' if small else 'sha256 ' + shas[name][:16]}")
        else:
            same = torch.equal(got, torch.from_numpy(np.load(path))) if small else rc.sha256(got) == shas[name]
            print(f"{name}: {'identical' if same else 'DIFFERENT'}")
            if not same:
                bad.append(name)
    if mode == "write":
        with open(sha_path, "w") as f:
            json.dump(shas, f, indent=1, sort_keys=True)
            f.write("\n")
    if bad:
        print("different:", bad)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
