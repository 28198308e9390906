"""The five SD-stage models held to recorded output bits.

The digests in tests/golden/model_bits/sha256.json were written by tools/model_bits.py on the MI355X from the models as they stood
when each module still carried its own loading, packing and layer-call code; the runs (model_bits_cases.py) are the inputs of the
models' own goldens, whose outputs the float64 tests check.  A change of the models' Python keeps these bits; a change of a kernel's
arithmetic, a tile choice or a launch sequence records new ones.  A second launch must give the bits of the first.  GPU tests are
marked -m gpu.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_bits_cases as mb  # noqa: E402

RUNS = mb.runs()


@pytest.fixture(scope="module")
def recorded():
    with open(mb.GOLDEN) as f:
        return json.load(f)


def test_every_run_has_a_recorded_digest_and_no_other(recorded):
    assert sorted(recorded) == sorted(name for name, _ in RUNS)


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", RUNS, ids=[name for name, _ in RUNS])
def test_the_recorded_bits_twice(cuda, recorded, name, make):
    launch = make()
    first, again = mb.sha256(launch()), mb.sha256(launch())
    assert first == again, "the second launch differs from the first"
    assert first == recorded[name], "not the recorded bits"
