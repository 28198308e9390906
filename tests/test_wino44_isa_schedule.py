"""The compiled slab loop of the F(4x4,3x3) kernel keeps the schedule its source spells (conv_wino.hip, wino44_conv_kernel).

tools/isa_loop_report.py reads the loop back from the gfx950 assembly, as tests/test_wino15_isa_schedule.py does for the F(4,5)
kernels: two 8-channel slabs per trip (48 MFMAs, one barrier per slab), each weight fragment reloaded behind the MFMAs that
consumed it and waited for at least seven MFMAs later, and the register and LDS budget of one twelve-wave workgroup per CU at
three waves per SIMD.  The operand reads: how many MFMAs after their issue the LDS reads of a half-step are waited for
(profiles/r22_wino44_rowstage_isa.txt).  Needs hipcc only, no GPU; skipped where there is no hipcc.
"""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))
pytestmark = pytest.mark.skipif(not HIPCC, reason="no hipcc")

MIN_WEIGHT_DISTANCE = 7     # MFMAs between a weight fragment's load and its wait: the figure of the loop since it was written
MAX_VGPR = 168              # three waves per SIMD
MAX_LDS = 122880            # bytes, dynamic: the launch asks for kSmem44
# MFMAs between the issue of a half-step's operand reads and the wait that retires them.  The second half-step's six reads are
# issued in front of the first half-step's twelve MFMAs and waited for behind them: 12, the figure the compiled loop shows
# (profiles/r22_wino44_rowstage_isa.txt; 0 while every wave formed its operands from the halo).  The first half-step's reads
# follow the slab's barrier and cannot be early.
MIN_READ_DISTANCE = 12


@pytest.fixture(scope="module")
def loop():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_loop_report
    finally:
        sys.path.pop(0)
    os.environ.setdefault("HIPCC", HIPCC)
    reps = isa_loop_report.report(os.path.join(isa_loop_report.CSRC, "conv_wino.hip"), name_filter="wino44_conv_kernel")
    assert len(reps) == 1, [r["kernel"] for r in reps]
    r = reps[0]
    print({k: v for k, v in r.items() if k not in ("waits", "lds_waits")})
    for w in r["waits"] + r["lds_waits"]:
        print("   ", w)
    return r


def _smem_bytes():
    """The dynamic LDS the launch asks for (kSmem44), from the constants conv_wino.hip names: the larger of the staged slabs (raw
    halo and T, both double-buffered) and the output exchange."""
    import re
    src = open(os.path.join(ROOT, "sd_animation_optical_flow_amd", "csrc", "conv_wino.hip")).read()
    body = src[src.index("struct Halo44 {"):src.index("wino44_conv_kernel(const WinoK p)")]

    def const(name):
        return int(re.search(r"\b" + name + r" = (\d+)[,;]", body).group(1))
    assert re.search(r"tfloats = 6 \* 4 \* ltrow;", body) and re.search(r"kStage44 = 2 \* \(Halo44::floats \+ Halo44::tfloats\);", body)
    assert re.search(r"kXF4 = 12 \* 4 \* 16 \* kLDX4;", body)
    stage = 2 * (const("H") * const("lrow") + 6 * 4 * const("ltrow"))
    return 4 * max(stage, 12 * 4 * 16 * const("kLDX4"))


def test_two_slabs_per_trip_one_barrier_each(loop):
    assert (loop["mfma"], loop["barriers"]) == (48, 2)


def test_the_weight_prefetch_keeps_its_distance(loop):
    assert loop["min_weight_distance"] is not None and loop["min_weight_distance"] >= MIN_WEIGHT_DISTANCE


def test_resources(loop):
    assert loop["scratch"] == 0
    assert loop["vgpr"] + loop["agpr"] <= MAX_VGPR
    assert loop["lds"] == 0, "static LDS next to the dynamic allocation"
    assert _smem_bytes() <= MAX_LDS


def test_operand_reads_are_waited_for_behind_the_mfmas(loop):
    """Per slab, one wait at least retires operand reads issued MIN_READ_DISTANCE MFMAs earlier: two per trip."""
    far = [w for w in loop["lds_waits"] if w["reads"] and w["oldest_read_distance"] >= MIN_READ_DISTANCE]
    assert len(far) >= 2, loop["lds_waits"]
    assert loop["max_read_distance"] >= MIN_READ_DISTANCE
