"""`ofx_groupnorm` and `ofx_groupnorm_cat` held to recorded output bits.

The two entry points run one set of kernels (sd_ops.hip: gn_partial_kernel, gn_finalize_kernel, gn_apply_kernel), so comparing one
with the other says nothing about the summation order.  The digests in tests/golden/groupnorm_bits/sha256.json were written by
tools/groupnorm_bits.py from the library as it stood when each entry point still had kernels of its own; the runs
(groupnorm_bits_cases.py) are the case tables of test_gpu_sd_ops.py and test_gpu_unet.py, which check the same outputs against
float64.  A change of the kernels' schedule or addressing keeps these bits; a change of their arithmetic records new ones.  A second
launch must give the bits of the first: a race in a reduction would not.  GPU tests are marked -m gpu.
"""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import groupnorm_bits_cases as gb  # noqa: E402

RUNS = gb.runs()


@pytest.fixture(scope="module")
def recorded():
    with open(gb.GOLDEN) as f:
        return json.load(f)


def test_every_run_has_a_recorded_digest_and_no_other(recorded):
    assert sorted(recorded) == sorted(name for name, _ in RUNS)


@pytest.mark.gpu
@pytest.mark.parametrize("name,make", RUNS, ids=[name for name, _ in RUNS])
def test_the_recorded_bits_twice(cuda, recorded, name, make):
    from sd_animation_optical_flow_amd import ops
    launch = make()
    first = launch(ops)
    again = launch(ops)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32)), "the second launch differs from the first"
    assert gb.sha256(first.cpu()) == recorded[name], "not the recorded bits"
