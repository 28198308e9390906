"""Rate of `ops.canny` (ofx_canny_u8) on the GPU box at 512x768, 1 and 3 channels, B = 1 and B = 16, beside `ops.detect_edges` at the
same size and batch (the same map and hysteresis kernels plus a value channel, a histogram and a dilation).  The three alternate
in rounds of one process; a call ends in the library's own stream synchronisation, and the host clock is read after a device
synchronise.  Median of the rounds with [fastest .. slowest], and the number of hysteresis batches (8 sweeps and one 4-byte
read-back each) every input took, counted by the library's profiler scopes in a call outside the timed rounds.
    python tools/canny_rate.py [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sd_animation_optical_flow_amd import keyframes, ops

H, W, ROUNDS, CALLS = 512, 768, 7, 20
LOW, HIGH = 100, 200           # the live driver's Canny net


def content(B, kind):
    """smooth: moving sinusoid content (a video-like frame); random: a random field, an edge at every pixel; contours: weak paths
    through 25 tiles each that are strong at one end, the hysteresis' many-sweeps case."""
    if kind == "random":
        return np.random.default_rng(0).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    if kind == "contours":                                       # tests/canny_check.serpentine tiled: long weak paths, strong at one end
        s = np.zeros((160, 160), dtype=np.uint8)
        for r in range(5):
            s[32 * r + 16:32 * r + 22, 8:152] = 30
            if r < 4:
                s[32 * r + 16:32 * (r + 1) + 22, (slice(146, 152) if r % 2 == 0 else slice(8, 14))] = 30
        s[16:22, 8:20] = 60
        frame = np.tile(s, (H // 160 + 1, W // 160 + 1))[:H, :W]
        return np.ascontiguousarray(np.broadcast_to(frame[None, :, :, None], (B, H, W, 3)))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    return np.stack([np.stack([(127 + 120 * np.sin((xx + 3 * t) / (17 + c)) * np.cos((yy - 2 * t) / (23 - c))) for c in range(3)], -1)
                     for t in range(B)]).astype(np.uint8)


def batches(fn):
    ops.prof_enable(1)
    ops.prof_collect()
    fn()
    n = ops.prof_collect().get("hysteresis_batch", {}).get("calls", 0)
    ops.prof_enable(0)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "canny_rate needs a GPU"
    lines = [f"ops.canny and ops.detect_edges, {W}x{H} uint8 frames on the device, thresholds {LOW}/{HIGH} (detect_edges: its median-derived "
             f"ones, ksize {keyframes.estimated_kernel_size(W, H)}); ms per call, host clock after a device synchronise around {CALLS} calls, "
             f"median of {ROUNDS} rounds [fastest .. slowest], the three alternating within every round after one warm-up call of each; "
             "batches = hysteresis batches of 8 sweeps + one 4-byte read-back the input took"]
    ks = keyframes.estimated_kernel_size(W, H)
    for kind in ("smooth", "random", "contours"):
        for B in (1, 16):
            bgr = torch.from_numpy(content(B, kind)).cuda()
            grey = bgr[..., 1].contiguous()
            fns = {"canny 1ch": lambda: ops.canny(grey, LOW, HIGH), "canny 3ch": lambda: ops.canny(bgr, LOW, HIGH),
                   "detect_edges": lambda: ops.detect_edges(bgr, ks)}
            nb = {k: batches(f) for k, f in fns.items()}              # also the warm-up call
            times = {k: [] for k in fns}
            for _ in range(ROUNDS):
                for k, f in fns.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(CALLS):
                        f()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t) / CALLS * 1e3)
            lines.append(f"\n  {kind} content, B = {B}")
            for k, v in times.items():
                med = statistics.median(v)
                lines.append(f"    {k:13s} {med:8.3f} [{min(v):8.3f} .. {max(v):8.3f}] ms per call = {med / B:7.3f} ms per frame; batches {nb[k]}")
            m3, md = statistics.median(times["canny 3ch"]), statistics.median(times["detect_edges"])
            over = min(times["canny 3ch"]) > max(times["detect_edges"]) or max(times["canny 3ch"]) < min(times["detect_edges"])
            lines.append(f"    canny 3ch - detect_edges = {m3 - md:+.3f} ms per call ({(m3 - md) / md * 100:+.1f} %)"
                         + ("" if over else "; the brackets overlap: inside the round-to-round spread"))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
