"""The six seeded stand-in state dicts (`random_*_state_dict`) held to recorded bits, without a GPU.

The golden generators (tests/golden/make_golden_*.py) load these weights into the reference's own modules, so the stored outputs
describe exactly these tensors.  tests/golden/model_bits/weights_sha256.json holds the SHA-256 over keys, shapes and bytes, in order,
of every case of model_bits_cases.weight_cases(), written (tools/model_bits.py write-weights) while each module still drew its
weights with a loop of its own."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_bits_cases as mb  # noqa: E402

CASES = mb.weight_cases()


@pytest.fixture(scope="module")
def recorded():
    with open(mb.WEIGHTS_GOLDEN) as f:
        return json.load(f)


def test_every_case_has_a_recorded_digest_and_no_other(recorded):
    assert sorted(recorded) == sorted(name for name, _ in CASES)
    assert len(CASES) == 2 * 7 + 2                                 # seven dicts at seeds 0 and 3, the two full VAE dicts at seed 0


@pytest.mark.parametrize("name,make", CASES, ids=[name for name, _ in CASES])
def test_the_recorded_weights(recorded, name, make):
    assert mb.state_dict_sha256(make()) == recorded[name]
