"""The compiled slab loop of the F(4,5) kernels keeps the schedule its source spells (conv_wino.hip, wino_slabs_staged).

The source reloads each weight fragment for the next slab straight after the four MFMAs that consume it, 60 MFMAs ahead of its
next use.  Left to itself the compiler sank all sixteen reloads below the slab's last MFMAs and waited for them at the next
slab's first (profiles/r19_wino15_prefetch_isa.txt).  tools/isa_loop_report.py reads the loop back from the gfx950 assembly;
this test holds all six <VERT, EPI> instantiations to the schedule, as tests/test_wino_isa_schedule.py holds the F(2x2,3x3)
kernels.  Needs hipcc only, no GPU; skipped where there is no hipcc.
"""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))
pytestmark = pytest.mark.skipif(not HIPCC, reason="no hipcc")

KERNELS = [f"wino15_conv_kernel<{v}, {e}>" for v in ("false", "true") for e in (0, 1, 2)]
# One slab ahead is 60 MFMAs in the source; the floor is the 3x3 kernel's: 16 MFMAs are 1024 matrix-pipe cycles, above the ~900
# cycles of a miss to HBM.
MIN_DISTANCE = 16
MAX_LDS = 81920      # two workgroups per CU


@pytest.fixture(scope="module")
def loops():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_loop_report
    finally:
        sys.path.pop(0)
    os.environ.setdefault("HIPCC", HIPCC)
    reps = isa_loop_report.report(os.path.join(isa_loop_report.CSRC, "conv_wino.hip"), name_filter="wino15_conv_kernel")
    return {r["kernel"]: r for r in reps}


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_weight_prefetch_stays_a_slab_ahead(loops, kernel):
    r = loops[kernel]
    print(kernel, {k: v for k, v in r.items() if k != "waits"})
    for w in r["waits"]:
        print("   ", w)
    assert (r["mfma"], r["weight_loads"], r["halo_loads"]) == (64, 16, 3)
    assert r["scratch"] == 0
    assert r["vgpr"] + r["agpr"] <= 256
    assert r["lds"] <= MAX_LDS
    assert r["min_weight_distance"] is not None and r["min_weight_distance"] >= MIN_DISTANCE
    assert r["halo_store_wait"] is not None and r["halo_store_wait"] != 0      # the halo's wait leaves the weights in flight
