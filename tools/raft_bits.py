#!/usr/bin/env python3
"""The output bits of the RAFT engine on the runs of tests/raft_bits_cases.py (both networks, every schedule of the executor), as
SHA-256 digests:

    python tools/raft_bits.py write [DIR]    -> DIR/sha256.json; DIR defaults to tests/golden/raft_bits
    python tools/raft_bits.py compare [DIR]  -> every run gives the recorded digest (exit status 1 otherwise)

Run `write` on the build whose bits are the reference (the parent of a change to csrc/raft_engine.cpp), `compare` on the new one;
OFX_LIB_PATH selects a build.  Every run is launched twice: a run whose second launch differs from its first is reported and not
recorded.  tests/test_gpu_raft_bits.py holds every run to the recorded digests."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raft_bits_cases as rb  # noqa: E402


def main():
    mode = sys.argv[1]
    assert mode in ("write", "compare")
    path = os.path.join(sys.argv[2], os.path.basename(rb.GOLDEN)) if len(sys.argv) > 2 else rb.GOLDEN
    shas = json.load(open(path)) if mode == "compare" else {}
    bad = []
    for name, digests in rb.runs():
        sha, again = digests()
        if again != sha:
            print(f"{name}: NOT REPRODUCIBLE launch to launch", flush=True)
            bad.append(name)
        elif mode == "write":
            shas[name] = sha
            print(f"{name}: {sha[:16]}", flush=True)
        else:
            same = sha == shas.get(name)
            print(f"{name}: {'identical' if same else 'DIFFERENT'}", flush=True)
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
