#!/usr/bin/env python3
"""`RaftEngine(precision="fp16")` against the fp32 and bf16x3 engines on the bench step.

Times `bench.make_step` -- the product's `clip.FrameSynthesizer` fed by the flow network alone: flow, the warp inside the upsample,
the mask -- on `bench.make_clip(64, ...)` (64 frames of 512x768 against one key frame, 20 iterations) with one engine per
arithmetic, all three in ONE process, in alternating rounds (fp32, bf16x3, fp16, fp32, ...), every step timed with device events.
The same for a single pair (B = 1), where the fp16 convolutions run unsplit (that arithmetic has no split-K kernels).  Per mode:
the median step time and [fastest .. slowest]; the comparison that matters is between the modes of the same run.  Also printed: each
mode's flow EPE against the fp32 engine on the timed batch (what the faster arithmetic costs), and with --layers the per-layer times
of one fp16 forward next to one fp32 forward (HIP-event profiler).

    python tools/raft_f16_rate.py [--rounds 7] [--warmup 2] [--batches 64 1] [--layers]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                                 # noqa: E402
from sd_animation_optical_flow_amd import ops                                # noqa: E402
from sd_animation_optical_flow_amd.raft import RaftEngine                    # noqa: E402
from sd_animation_optical_flow_amd.weights import random_state_dict          # noqa: E402

H, W = bench.H, bench.W      # 768 x 512 rows x columns: "512x768"
MODES = ("fp32", "bf16x3", "fp16")


def timed(step):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def rates(B, rounds, warmup, dev, engines):
    frames, key, key_ai, conf = bench.make_clip(B, H, W, dev)
    steps = {m: bench.make_step(engines[m], frames, key, key_ai, conf) for m in MODES}
    flows = {}
    for m in MODES:                                      # every shape of the timed window, every mode
        for _ in range(warmup):
            flows[m] = steps[m]()[0]
    torch.cuda.synchronize()
    epe = {m: float((flows[m] - flows["fp32"]).pow(2).sum(-1).sqrt().mean()) for m in MODES}
    ms = {m: [] for m in MODES}
    for _ in range(rounds):
        for m in MODES:
            ms[m].append(timed(steps[m])[0])
    res = {}
    for m in MODES:
        med = statistics.median(ms[m])
        res[m] = {"mode": m, "B": B, "H": H, "W": W, "iters": bench.ITERS, "rounds": rounds, "ms_median": round(med, 3),
                  "ms_fastest": round(min(ms[m]), 3), "ms_slowest": round(max(ms[m]), 3), "pairs_per_s": round(B / med * 1e3, 2),
                  "epe_vs_fp32_engine_px": float(f"{epe[m]:.3e}")}
        print(json.dumps(res[m]), flush=True)
    print(json.dumps({"B": B, "fp16_over_fp32": round(res["fp32"]["ms_median"] / res["fp16"]["ms_median"], 3),
                      "fp16_over_bf16x3": round(res["bf16x3"]["ms_median"] / res["fp16"]["ms_median"], 3),
                      "bf16x3_over_fp32": round(res["fp32"]["ms_median"] / res["bf16x3"]["ms_median"], 3),
                      "what": "speed ratios of the medians (> 1: the first mode is faster)"}), flush=True)
    return res


def layers(B, dev, engines):
    frames, key, _, _ = bench.make_clip(B, H, W, dev)
    for m in ("fp32", "fp16"):
        engines[m].forward(frames, key, iters=bench.ITERS)
        torch.cuda.synchronize()
        ops.prof_enable(2)
        engines[m].forward(frames, key, iters=bench.ITERS)
        torch.cuda.synchronize()
        rec = ops.prof_collect()
        ops.prof_enable(0)
        total = sum(v["ms"] for v in rec.values())
        print(f"# {m}, one forward: B={B} {W}x{H} iters={bench.ITERS}, {total:.2f} ms in kernels (HIP-event profiler, per layer)")
        print(f"{'kernel:layer':<44}{'calls':>6}{'ms':>10}{'share':>8}{'avg us':>10}{'TFLOP/s':>9}")
        for k, v in sorted(rec.items(), key=lambda kv: -kv[1]["ms"])[:24]:
            tf = v["flops"] / v["ms"] / 1e9 if v["flops"] else float("nan")
            print(f"{k:<44}{v['calls']:>6}{v['ms']:>10.3f}{v['ms'] / total:>8.1%}{1e3 * v['ms'] / v['calls']:>10.1f}{tf:>9.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("raft_f16_rate.py measures on the GPU: no device, no number")
    dev = torch.device("cuda")
    sd = random_state_dict(0)
    engines = {m: RaftEngine(sd, dev, precision=m) for m in MODES}
    for B in a.batches:
        rates(B, a.rounds, a.warmup, dev, engines)
        torch.cuda.empty_cache()
    if a.layers:
        layers(a.batches[0], dev, engines)


if __name__ == "__main__":
    main()
