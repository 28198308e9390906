"""The F(4x4,3x3) kernel's register budget (conv_wino.hip, wino44_conv_kernel): three waves per SIMD leave 168 VGPRs, of which 96
are accumulators, and the kernel is written around that (half-step weight fragments, staging addresses worked out again at
every slab).  A compiler that spills it instead would still compute the right values, slowly.  tools/kres.py reads the
compiler's resource remarks; needs hipcc only, no GPU; skipped where there is no hipcc.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="no hipcc")


def test_no_scratch_at_three_waves_per_simd():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kres
    finally:
        sys.path.pop(0)
    src = os.path.join(ROOT, "sd_animation_optical_flow_amd", "csrc", "conv_wino.hip")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c", src, "-o", os.devnull, kres.REMARKS]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [r for r in kres.parse_remarks(out.stderr) if "wino44_conv_kernel" in r["name"]]
    assert len(rows) == 1, [r["name"] for r in kres.parse_remarks(out.stderr)]
    r = rows[0]
    assert r["ScratchSize"] == 0 and r["VGPRs"] + r["AGPRs"] <= 168 and r["Occupancy"] >= 3, r
