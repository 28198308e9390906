#!/usr/bin/env python3
"""The small RAFT network (raft-small.pth) against the basic one (raft-things.pth) on the bench step.

Times `bench.make_step` -- the product's `clip.FrameSynthesizer` fed by the flow network alone: flow, the warp inside the upsample,
the mask -- with a small engine and with the basic engine on the same synthetic 512x768 clip (`bench.make_clip`), at B = 1, 16 and
64 frames against one key frame, and prints one JSON line per (network, B) and a last line with the small / basic ratio per B.

    python tools/small_model_rate.py [--batches 1 16 64] [--steps 5] [--warmup 2]
    python tools/small_model_rate.py --layers 64        # per-layer times of one small-network forward (HIP-event profiler)
    python tools/small_model_rate.py --one-step 64      # ONE small-network step: the target of a rocprofv3 trace
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                                 # noqa: E402
from sd_animation_optical_flow_amd import ops                                # noqa: E402
from sd_animation_optical_flow_amd.raft import RaftEngine                    # noqa: E402
from sd_animation_optical_flow_amd.weights import random_state_dict          # noqa: E402

H, W = bench.H, bench.W      # 768 x 512 rows x columns: "512x768"


def step_for(variant, B, dev):
    eng = RaftEngine(random_state_dict(0, small=variant == "small"), dev)
    frames, key, key_ai, conf = bench.make_clip(B, H, W, dev)
    return eng, bench.make_step(eng, frames, key, key_ai, conf), (frames, key)


def rate(variant, B, steps, warmup, dev):
    _, step, _ = step_for(variant, B, dev)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"network": variant, "B": B, "H": H, "W": W, "iters": bench.ITERS, "pairs_per_s": round(B / dt, 2),
            "ms_per_step": round(dt * 1e3, 3), "steps": steps}


def layers(B, dev):
    eng, step, (frames, key) = step_for("small", B, dev)
    step()
    torch.cuda.synchronize()
    ops.prof_enable(2)
    eng.forward(frames, key, iters=bench.ITERS)
    torch.cuda.synchronize()
    rec = ops.prof_collect()
    ops.prof_enable(0)
    total = sum(v["ms"] for v in rec.values())
    print(f"# small network, one forward: B={B} {W}x{H} iters={bench.ITERS}, {total:.2f} ms in kernels (HIP-event profiler, per layer)")
    print(f"{'kernel:layer':<44}{'calls':>6}{'ms':>10}{'share':>8}{'avg us':>10}{'TFLOP/s':>9}")
    for k, v in sorted(rec.items(), key=lambda kv: -kv[1]["ms"]):
        tf = v["flops"] / v["ms"] / 1e9 if v["flops"] else float("nan")
        print(f"{k:<44}{v['calls']:>6}{v['ms']:>10.3f}{v['ms'] / total:>8.1%}{1e3 * v['ms'] / v['calls']:>10.1f}{tf:>9.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=0, metavar="B")
    ap.add_argument("--one-step", type=int, default=0, metavar="B")
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.layers:
        return layers(a.layers, dev)
    if a.one_step:
        _, step, _ = step_for("small", a.one_step, dev)
        step()
        torch.cuda.synchronize()
        return
    res = {}
    for B in a.batches:
        for variant in ("basic", "small"):
            r = rate(variant, B, a.steps, a.warmup, dev)
            res[(variant, B)] = r
            print(json.dumps(r), flush=True)
            torch.cuda.empty_cache()
    print(json.dumps({"small_over_basic": {str(B): round(res[("small", B)]["pairs_per_s"] / res[("basic", B)]["pairs_per_s"], 2)
                                           for B in a.batches}}))


if __name__ == "__main__":
    main()
