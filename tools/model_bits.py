#!/usr/bin/env python3
"""The output bits of the five SD-stage models on the runs of tests/model_bits_cases.py (UNetModel, ControlNet, SpatialTransformer,
ClipTextEncoder, VaeEncoder / VaeDecoder on their goldens' inputs), as SHA-256 digests:

    python tools/model_bits.py write [DIR]          -> DIR/sha256.json; DIR defaults to tests/golden/model_bits
    python tools/model_bits.py compare [DIR]        -> every run gives the recorded digest (exit status 1 otherwise)
    python tools/model_bits.py write-weights [DIR]  -> DIR/weights_sha256.json: the seeded state dicts (host only, no GPU)

Run `write` on the tree whose bits are the reference (the parent of a change to the models' Python), `compare` on the new one.
tests/test_gpu_model_bits.py holds every run to the recorded digests, tests/test_model_weights_host.py the state dicts."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import model_bits_cases as mb  # noqa: E402


def main():
    mode = sys.argv[1]
    assert mode in ("write", "compare", "write-weights")
    default = mb.WEIGHTS_GOLDEN if mode == "write-weights" else mb.GOLDEN
    path = os.path.join(sys.argv[2], os.path.basename(default)) if len(sys.argv) > 2 else default
    shas = json.load(open(path)) if mode == "compare" else {}
    bad = []
    if mode == "write-weights":
        for name, make in mb.weight_cases():
            shas[name] = mb.state_dict_sha256(make())
            print(f"{name}: {shas[name][:16]}")
    for name, make in mb.runs() if mode != "write-weights" else ():
        launch = make()
        sha, again = mb.sha256(launch()), mb.sha256(launch())
        if again != sha:
            print(f"{name}: NOT REPRODUCIBLE launch to launch")
            bad.append(name)
        elif mode == "write":
            shas[name] = sha
            print(f"{name}: {sha[:16]}")
        else:
            same = sha == shas[name]
            print(f"{name}: {'identical' if same else 'DIFFERENT'}")
            if not same:
                bad.append(name)
    if mode != "compare":
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
