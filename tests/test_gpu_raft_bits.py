"""The RAFT engine held to recorded output bits.

The digests in tests/golden/raft_bits/sha256.json were written by tools/raft_bits.py on the MI355X from the library as it stood when
the executor's convolution launcher still took 27 positional arguments and carried one-shot members -- and, for the 12 runs added
with it (shared-frame index set-up, the small network's warped pairs, the per-pixel lookup, the split-plane volume), from the
library before the four forwards shared their argument check, correlation stage and tail; the runs (raft_bits_cases.py)
cover both networks and every schedule the executor takes, flows and registered intermediates alike.  A change of how the executor
describes or orders its launches keeps these bits; a change of a kernel's arithmetic, a tile choice or a route records new ones.  A
second launch must give the bits of the first.  GPU tests are marked -m gpu.
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raft_bits_cases as rb  # noqa: E402

RUNS = rb.runs()


@pytest.fixture(scope="module")
def recorded():
    with open(rb.GOLDEN) as f:
        return json.load(f)


def test_every_run_has_a_recorded_digest_and_no_other(recorded):
    assert sorted(recorded) == sorted(name for name, _ in RUNS)


@pytest.mark.gpu
@pytest.mark.parametrize("name,digests", RUNS, ids=[name for name, _ in RUNS])
def test_the_recorded_bits_twice(cuda, recorded, name, digests):
    first, again = digests()
    assert first == again, "the second launch differs from the first"
    assert first == recorded[name], "not the recorded bits"
