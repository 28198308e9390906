#!/usr/bin/env python3
"""The reference's own mixed precision for the flow network, measured: the REAL reference RAFT (`/root/reference/RAFT/core`,
imported, not copied) with `args.mixed_precision = True`, run on the CPU in the build container:

    python tests/golden/make_golden_raft_autocast.py

With the switch on, `RAFT.forward` runs its two encoders and the update block under `autocast` (raft.py:99,110,127) and casts the
feature maps back with `.float()`; the correlation volume, the lookup, `coords1 + delta` and the convex upsample stay fp32.  The
module binds `autocast` to `torch.cuda.amp.autocast` at import; this script points that name at
`torch.autocast("cpu", dtype=torch.float16)` -- the same casting policy on the device this container has -- and changes nothing
else.  Weights: `oracle.raft_oracle.init_state_dict(0)`; inputs: the seeded frames of tests/test_gpu_raft.py (`_frames`), 20
iterations, the model in `.eval()`.

Stored in tests/golden/raft_ref_autocast_128x160.npz, per case `<tag>` (a: 128x160, 2 pairs, `_frames(11, ...)`; b: 136x168, whose
1/8 map of 17 x 21 is not whole 8x16 patches, `_frames(12, ...)`):
    image1_<tag> / image2_<tag>   uint8 [B,H,W,3] frames / [H,W,3] key frame
    flow_<tag>                    the autocast flow, float32 [B,H,W,2]
    autocast_vs_f64_<tag>         its mean end-point error against the float64 restatement `raft_oracle.raft_forward(to_float64(sd))`
    emulated_vs_f64_<tag>         the EPE of the SAME reference module in fp32 with the two operands of every `F.conv2d` rounded to half
                                  (`x.half().float()`, `w.half().float()`): the arithmetic of `RaftEngine(precision="fp16")` restated on
                                  the CPU -- a subset of autocast's roundings
    fp32_vs_f64_<tag>             the EPE of the untouched fp32 module, for scale
`autocast_vs_f64` is the yardstick of the engine's fp16 mode (tests/test_gpu_raft_f16.py holds the device to twice that); the script
asserts emulated / autocast <= 1.5 for every case it stores, so that the device has margin under that bar from the reference alone.
A case that misses the assertion is not stored.  Nothing of the reference's source text is stored -- only inputs and outputs.
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
REF = "/root/reference/RAFT/core"

from oracle import raft_oracle as RO   # noqa: E402

CASES = (("a", 11, 2, 128, 160), ("b", 12, 2, 136, 168))
ITERS = 20
MAX_RATIO = 1.5


def _epe(a, b):
    return float((a.double() - b.double()).pow(2).sum(1).sqrt().mean())


def _model(mixed):
    from raft import RAFT

    class NS:
        def __contains__(self, m):
            return hasattr(self, m)
    a = NS()
    a.small, a.mixed_precision, a.alternate_corr = False, mixed, False
    model = RAFT(a).eval()
    model.load_state_dict(RO.init_state_dict(0), strict=True)
    return model


class _half_operands:
    """F.conv2d with both operands rounded to half and everything else (the bias, the accumulation, the result) fp32."""

    def __enter__(self):
        self.orig = F.conv2d
        orig = self.orig
        F.conv2d = lambda x, w, *a, **k: orig(x.half().float(), w.half().float(), *a, **k)

    def __exit__(self, *exc):
        F.conv2d = self.orig


def main():
    warnings.filterwarnings("ignore")
    sys.path.insert(0, REF)
    import raft as raft_module
    from test_gpu_raft import _frames
    raft_module.autocast = lambda enabled=True: torch.autocast("cpu", dtype=torch.float16, enabled=enabled)
    sd64 = RO.to_float64(RO.init_state_dict(0))
    mixed, plain = _model(True), _model(False)
    out = {}
    for tag, seed, B, H, W in CASES:
        key, frames = _frames(seed, B, H, W)
        i1 = frames.permute(0, 3, 1, 2).float()
        i2 = key.permute(2, 0, 1).float()[None].expand(B, -1, -1, -1).contiguous()
        with torch.no_grad():
            _, up_auto = mixed(i1, i2, iters=ITERS, test_mode=True)
            _, up_32 = plain(i1, i2, iters=ITERS, test_mode=True)
            with _half_operands():
                _, up_emu = plain(i1, i2, iters=ITERS, test_mode=True)
            _, up_64 = RO.raft_forward(sd64, i1.double(), i2.double(), iters=ITERS)
        assert up_auto.dtype == torch.float32 and up_64.dtype == torch.float64
        d_auto, d_emu, d_32 = _epe(up_auto, up_64), _epe(up_emu, up_64), _epe(up_32, up_64)
        print(f"[{tag}] {B} x {H}x{W}: autocast vs float64 {d_auto:.3e} px, emulation vs float64 {d_emu:.3e} px (ratio {d_emu / d_auto:.2f}), "
              f"fp32 vs float64 {d_32:.3e} px; |flow| mean {float(up_64.abs().mean()):.2f}")
        assert d_32 < 1e-4 < d_auto, "the switch did nothing"
        if not d_emu <= MAX_RATIO * d_auto:
            print(f"[{tag}] NOT STORED: emulated / autocast = {d_emu / d_auto:.2f} > {MAX_RATIO}")
            continue
        out.update({f"image1_{tag}": frames.numpy(), f"image2_{tag}": key.numpy(),
                    f"flow_{tag}": up_auto.permute(0, 2, 3, 1).contiguous().numpy(),
                    f"autocast_vs_f64_{tag}": np.float64(d_auto), f"emulated_vs_f64_{tag}": np.float64(d_emu),
                    f"fp32_vs_f64_{tag}": np.float64(d_32)})
    assert "flow_a" in out, "the 128x160 case must be stored"
    out["cases"] = np.array(sorted(k[5:] for k in out if k.startswith("flow_")))
    path = os.path.join(HERE, "raft_ref_autocast_128x160.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("the reference is not mounted here; golden vectors can only be regenerated in the build container")
    main()
