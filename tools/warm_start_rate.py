#!/usr/bin/env python3
"""Cost of the warm start (RAFT.forward(flow_init=...) with forward_interpolate on the device).

1. `ops.forward_interpolate` per field at 96x64 and 135x240 (the 1/8 grids of 768x512 and 1080x1920), B = 1 and 64: a smooth field
   (the usual case: every output pixel finds its source in the first rings) and one with a large hole (most sources pushed out of the
   frame: the ring search walks far).  Device time per call from HIP events, divided by B.
2. The per-pair time of a `RAFT_2` chain over consecutive 512x768 frames, warm (`warm_start=True`) against cold: wall time of
   `calc` (numpy in, numpy out, as the reference's drivers call it), and the device time of the engine call with and without
   `flow_init` plus the forward_interpolate.  Random weights: no statement about accuracy or iterations is made.

    python tools/warm_start_rate.py [--reps 50] [--frames 8]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                                 # noqa: E402
from sd_animation_optical_flow_amd import ofgen, ops                         # noqa: E402
from sd_animation_optical_flow_amd.raft import RaftEngine                    # noqa: E402
from sd_animation_optical_flow_amd.weights import random_state_dict          # noqa: E402


def field(kind, B, h, w, dev):
    g = torch.Generator().manual_seed(0)
    coarse = torch.randn((B, 2, 4, 6), generator=g) * 3.0
    f = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True)
    if kind == "hole":                       # three quarters of the columns point far outside the frame
        f[:, 0, :, : (3 * w) // 4] += 4.0 * w
    return f.permute(0, 2, 3, 1).contiguous().to(dev)


def time_device(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda")
    for (h, w) in ((96, 64), (135, 240)):
        for B in (1, 64):
            for kind in ("smooth", "hole"):
                f = field(kind, B, h, w, dev)
                us = time_device(lambda: ops.forward_interpolate(f), args.reps if kind == "smooth" else max(3, args.reps // 10))
                print(json.dumps({"what": "forward_interpolate", "grid": f"{h}x{w}", "B": B, "field": kind,
                                  "us_per_call": round(us, 1), "us_per_field": round(us / B, 2)}), flush=True)

    H, W = bench.H, bench.W
    sd = random_state_dict(0)
    frames, _, _, _ = bench.make_clip(args.frames + 1, H, W, dev)
    seq = [frames[t].cpu().numpy() for t in range(args.frames + 1)]
    for warm in (False, True):
        algo = ofgen.RAFT_2(sd, warm_start=warm)
        algo.calc(seq[0], seq[1])                                            # warm-up: a cold call, then (warm_start) a warm one --
        algo.calc(seq[1], seq[2])                                            # first uses load their kernels
        algo.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(args.frames):
            algo.calc(seq[t], seq[t + 1])
        ms = (time.perf_counter() - t0) / args.frames * 1e3
        rec = {"what": "RAFT_2.calc chain", "size": f"{W}x{H}", "warm_start": warm, "pairs": args.frames, "ms_per_pair": round(ms, 3)}
        if warm:     # the field the chain carries at its end: how many of its sources stay inside the frame, and what it costs
            low = algo._low
            h, w = low.shape[1:3]
            ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
            x1, y1 = xs + low[0, ..., 0].double(), ys + low[0, ..., 1].double()
            rec["valid_source_fraction"] = round(float(((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)).double().mean()), 4)
            rec["mean_abs_flow_low"] = round(float(low.abs().mean()), 2)
            rec["forward_interpolate_us"] = round(time_device(lambda: ops.forward_interpolate(low), 5), 1)
        print(json.dumps(rec), flush=True)
    eng = RaftEngine(sd, dev, cnet_norm="batch")
    a, b = frames[0:1].contiguous(), frames[1:2].contiguous()
    _, low = eng.forward(a, b, want_low=True)
    cold = time_device(lambda: eng.forward(a, b, want_low=True), 20)
    warm = time_device(lambda: eng.forward(a, b, want_low=True, flow_init=ops.forward_interpolate(low)), 20)
    print(json.dumps({"what": "engine forward, device time", "size": f"{W}x{H}", "cold_ms": round(cold / 1e3, 3),
                      "warm_ms_incl_forward_interpolate": round(warm / 1e3, 3)}), flush=True)


if __name__ == "__main__":
    main()
