"""The compiled slab loop of the F(2x2,3x3) kernel keeps the schedule its source spells (conv_wino.hip, wino3x3_slabs).

The source reloads each weight fragment straight after the four MFMAs that consume it, one 8-channel step (28 MFMAs) ahead of
its next use.  Left to itself the compiler once sank every reload to its use to save registers and drained the weights with
the halo's wait after the barrier (profiles/r15_wino_prefetch_isa.txt); the matrix pipe then waited on L2 some five times per
slab.  tools/isa_loop_report.py reads the loop back from the gfx950 assembly; this test holds all six <NORM, RES, STATS>
instantiations to the schedule.  Needs hipcc only, no GPU; skipped where there is no hipcc.
"""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))
pytestmark = pytest.mark.skipif(not HIPCC, reason="no hipcc")

KERNELS = [f"wino_conv_kernel<{n}, {r}, {s}>" for n, r, s in
           [("false", "false", "false"), ("false", "false", "true"), ("false", "true", "false"), ("true", "false", "false"),
            ("true", "false", "true"), ("true", "true", "false")]]
# One step ahead is 28 MFMAs in the source; 16 (1024 matrix-pipe cycles, above the ~900 cycles of a miss to HBM) leaves the
# scheduler slack.
MIN_DISTANCE = 16


@pytest.fixture(scope="module")
def loops():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_loop_report
    finally:
        sys.path.pop(0)
    os.environ.setdefault("HIPCC", HIPCC)
    reps = isa_loop_report.report(os.path.join(isa_loop_report.CSRC, "conv_wino.hip"), name_filter="wino_conv_kernel")
    return {r["kernel"]: r for r in reps}


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_weight_prefetch_stays_a_step_ahead(loops, kernel):
    r = loops[kernel]
    print(kernel, {k: v for k, v in r.items() if k != "waits"})
    for w in r["waits"]:
        print("   ", w)
    assert (r["mfma"], r["weight_loads"], r["halo_loads"]) == (64, 16, 3)
    assert r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 256
    assert r["lds"] == 34816
    assert r["min_weight_distance"] is not None and r["min_weight_distance"] >= MIN_DISTANCE
    assert r["halo_store_wait"] != 0      # the halo's wait leaves the younger weight loads in flight
