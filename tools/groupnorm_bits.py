#!/usr/bin/env python3
"""The output bits of `ops.groupnorm` and `ops.groupnorm_cat` on the runs of tests/groupnorm_bits_cases.py (every GN_CASES entry,
GN_LARGE without and with SiLU, every GNC_CASES entry), as SHA-256 digests:

    python tools/groupnorm_bits.py write [DIR]    -> DIR/sha256.json; DIR defaults to tests/golden/groupnorm_bits
    python tools/groupnorm_bits.py compare [DIR]  -> every run gives the recorded digest (exit status 1 otherwise)

Run `write` on the build whose bits are the reference (the parent of a change to the GroupNorm kernels), `compare` on the new one;
OFX_LIB_PATH selects a build.  tests/test_gpu_groupnorm_bits.py holds both entry points to the recorded digests."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import groupnorm_bits_cases as gb  # noqa: E402
from sd_animation_optical_flow_amd import ops  # noqa: E402


def main():
    mode = sys.argv[1]
    assert mode in ("write", "compare")
    path = os.path.join(sys.argv[2], "sha256.json") if len(sys.argv) > 2 else gb.GOLDEN
    shas = json.load(open(path)) if mode == "compare" else {}
    bad = []
    for name, make in gb.runs():
        sha = gb.sha256(make()(ops).cpu())
        if mode == "write":
            shas[name] = sha
            print(f"{name}: {sha[:16]}")
        else:
            same = sha == shas[name]
            print(f"{name}: {'identical' if same else 'DIFFERENT'}")
            if not same:
                bad.append(name)
    if mode == "write":
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(shas, f, indent=1, sort_keys=True)
            f.write("\n")
    if bad:
        print("different:", bad)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
