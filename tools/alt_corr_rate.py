#!/usr/bin/env python3
"""Volume-free correlation: the LDS-tiled lookup kernel against the per-pixel one, and local mode against volume mode end to end.

One process; every measurement runs under a watchdog of its own (a step that exceeds its limit ends the process with status 124
instead of holding the device).  Prints one JSON line per measurement and a summary line.

  kernels   microseconds per lookup (= per refinement iteration: all four levels) of `ops.local_corr_rows(tiled=False / True)` in the
            same run, on unit-variance features and a smooth sub-pixel flow field, basic network shape (C = 256, r = 4, 336-float
            rows): 512x768 at B = 1, 16, 64 and 1088x1920 at B = 1, 4.  Also the bytes the tiled kernel has to fetch by its design
            (every tile's box once per level + fmap1 once per level) against the algorithmic minimum (each map once).
  forward   pairs/s of `RaftEngine.forward(frames, shared key)` with corr='local' against corr='volume': 512x768 at B = 64 and
            1088x1920 at B = 16, both under the same workspace budget (--budget-gb, default 32: modest on a shared machine; the
            volume layout of 16 pairs at 1088x1920 is 110 GB, so that mode slices the batch, local mode does not).

    python tools/alt_corr_rate.py [--only kernels|forward] [--one-step]      # --one-step: ONE local-mode forward (a rocprofv3 target)
"""
import argparse
import json
import os
import sys
import threading
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                                 # noqa: E402
from sd_animation_optical_flow_amd import ops                                # noqa: E402
from sd_animation_optical_flow_amd.raft import RaftEngine                    # noqa: E402
from sd_animation_optical_flow_amd.weights import random_state_dict          # noqa: E402

C, R, LD, LEVELS = 256, 4, 336, 4
KERNEL_SHAPES = [(512, 768, 1), (512, 768, 16), (512, 768, 64), (1088, 1920, 1), (1088, 1920, 4)]      # (W, H) as named, B
FORWARD_SHAPES = [(512, 768, 64), (1088, 1920, 16)]


class Watchdog:
    """`with Watchdog(seconds, what):` -- the process exits with status 124 when the block runs longer."""

    def __init__(self, seconds, what):
        self.t = threading.Timer(seconds, self._fire)
        self.t.daemon = True
        self.what, self.seconds = what, seconds

    def _fire(self):
        print(json.dumps({"timeout": self.what, "limit_s": self.seconds}), flush=True)
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()


def _event_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernel_case(name_w, name_h, B, reps):
    """name_w x name_h as the shapes are named (512x768 = 768 rows of 512): the 1/8 grid is (name_h/8) x (name_w/8)."""
    h, w = name_h // 8, name_w // 8
    g = torch.Generator(device="cuda").manual_seed(3)
    f1 = torch.randn((B, h, w, C), generator=g, device="cuda")
    lv = [torch.randn((B, h, w, C), generator=g, device="cuda")]
    for _ in range(1, LEVELS):
        lv.append(ops.avgpool2_nhwc(lv[-1]))
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda").float(), torch.arange(w, device="cuda").float(), indexing="ij")
    flow = torch.stack([2.3 + 1.5 * torch.sin(yy / 9.0) + 0.5 * torch.cos(xx / 5.0), -1.1 + 1.2 * torch.cos(xx / 11.0 + yy / 13.0)], -1)
    coords = (torch.stack([xx, yy], -1) + flow)[None].repeat(B, 1, 1, 1).contiguous()
    rows = torch.zeros((B * h * w, LD), device="cuda")
    old = _event_us(lambda: ops.local_corr_rows(f1, lv, coords, R, rows=rows, tiled=False), reps)
    want = rows[:, :324].clone()
    rows.zero_()
    new = _event_us(lambda: ops.local_corr_rows(f1, lv, coords, R, rows=rows, tiled=True), reps)
    err = (rows[:, :324] - want).abs().max().item()
    # bytes by design: per level, every 8x8 tile fetches the bounding box of its windows (8/2^l + 2r + 2 + flow spread per side,
    # clipped to the map) and its pixels' fmap1 rows; algorithmic minimum: fmap1 and the level's map once
    tiled_b = algo_b = 0
    for l in range(LEVELS):
        hl, wl = h >> l, w >> l
        side = 8 / 2 ** l + 2 * R + 2 + 1
        tiles = -(-h // 8) * -(-w // 8)
        tiled_b += B * (tiles * min(side, hl) * min(side, wl) + h * w) * C * 4
        algo_b += B * (hl * wl + h * w) * C * 4
    out_b = B * h * w * 324 * 4
    return {"kernel": "local_corr", "shape": f"{name_w}x{name_h}", "B": B, "per_pixel_us": round(old, 1), "tiled_us": round(new, 1),
            "speedup": round(old / new, 2), "max_abs_diff": float(f"{err:.2e}"), "tiled_fetch_MB_by_design": round(tiled_b / 1e6, 1),
            "algorithmic_fetch_MB": round(algo_b / 1e6, 1), "fetch_ratio": round(tiled_b / algo_b, 2), "write_MB": round(out_b / 1e6, 1),
            "tiled_GFLOPs": round(B * h * w * LEVELS * 100 * C * 2 / new / 1e3, 1)}


def forward_case(name_w, name_h, B, corr, budget, steps, warmup):
    H, W = name_h, name_w
    eng = RaftEngine(random_state_dict(0), torch.device("cuda"), corr=corr)
    eng.ws_budget_bytes = budget
    frames, key, _key_ai, _conf = bench.make_clip(B, H, W, torch.device("cuda"))
    fits = eng.pairs_that_fit(min(B, eng.pairs_per_call(H, W)), H, W, alternate_corr=corr == "local")
    for _ in range(warmup):
        eng.forward(frames, key, iters=bench.ITERS)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.forward(frames, key, iters=bench.ITERS)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    ws = eng._ws.numel()
    eng._ws = None
    del eng
    torch.cuda.empty_cache()
    return {"forward": corr, "shape": f"{name_w}x{name_h}", "B": B, "iters": bench.ITERS, "pairs_per_call": fits, "workspace_GB": round(ws / 1e9, 2),
            "ms_per_step": round(dt * 1e3, 2), "pairs_per_s": round(B / dt, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["kernels", "forward"])
    ap.add_argument("--one-step", action="store_true")
    ap.add_argument("--budget-gb", type=float, default=32.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    budget = int(a.budget_gb * 1e9)
    if a.one_step:
        with Watchdog(240, "one local-mode step"):
            eng = RaftEngine(random_state_dict(0), torch.device("cuda"), corr="local")
            frames, key, _, _ = bench.make_clip(64, 768, 512, torch.device("cuda"))
            eng.forward(frames, key, iters=bench.ITERS)
            torch.cuda.synchronize()
        return
    summary = {}
    if a.only in (None, "kernels"):
        for (nw, nh, B) in KERNEL_SHAPES:
            with Watchdog(120, f"kernels {nw}x{nh} B={B}"):
                r = kernel_case(nw, nh, B, a.reps)
            print(json.dumps(r), flush=True)
            summary[f"kernel {nw}x{nh} B={B}"] = r["speedup"]
            torch.cuda.empty_cache()
    if a.only in (None, "forward"):
        for (nw, nh, B) in FORWARD_SHAPES:
            res = {}
            for corr in ("volume", "local"):
                with Watchdog(420, f"forward {corr} {nw}x{nh} B={B}"):
                    res[corr] = forward_case(nw, nh, B, corr, budget, a.steps, a.warmup)
                print(json.dumps(res[corr]), flush=True)
            summary[f"forward {nw}x{nh} B={B} local/volume"] = round(res["local"]["pairs_per_s"] / res["volume"]["pairs_per_s"], 3)
    print(json.dumps({"summary": summary, "budget_GB": a.budget_gb}))


if __name__ == "__main__":
    main()
