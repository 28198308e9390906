"""Rate of the greedy multi-reference composition on the GPU box, three routes side by side at 512x768, N = 1, 2, 3:
  (a) `ops.compose_refs`: two launches, one warp sample per pixel, nothing read back (device events);
  (b) the existing round loop of `ofgen.compose_warp_and_mask` on tensors that are already resident: per round `ops.conf_sum`, the
      `.item()` read-back of the arg-max, a full-frame `ops.warp`, a clone or `ops.merge_images`, two in-place updates (host clock
      around a device synchronise: the loop synchronises by itself);
  (c) `ofgen.compose_warp_and_mask` from numpy: (b) plus the uploads and the three copies back (host clock).
None of the three has been measured before; the file states whichever way each comparison comes out.  One warm-up call of each, then
ROUNDS rounds in which the routes alternate; mean of the rounds with [fastest .. slowest].
    python tools/compose_rate.py [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from sd_animation_optical_flow_amd import ofgen, ops

H, W = 768, 512
ROUNDS, CALLS, HOST_CALLS = 3, 20, 5
THRES = 0.95
MODE = "cv2_cubic"


def device_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def host_ms(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / calls * 1e3


def rounds(fns):
    for f, _, _ in fns.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, (f, timer, calls) in fns.items():
            times[k].append(timer(f, calls))
    return times


def fmt(v):
    return f"{sum(v) / len(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}] ms"


def verdict(new, old):
    if max(new) < min(old):
        return "below"
    if min(new) > max(old):
        return "ABOVE"
    return "overlap"


def scene(n):
    """Smooth flows of a few pixels, confidences in blobs so that every reference wins somewhere (long runs of one pattern, as in
    a frame), random AI frames."""
    rng = np.random.default_rng(n)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    flow = np.stack([np.stack([3 * np.sin(yy / (40 + 7 * s)) + s, 2 * np.cos(xx / (55 - 5 * s)) - s], -1) for s in range(n)]).astype(np.float32)
    conf = np.stack([0.5 + 0.5 * np.sin(xx / (90 + 30 * s) + s) * np.cos(yy / (120 - 20 * s)) for s in range(n)]).astype(np.float32)
    conf = np.clip(conf + 0.46, 0, 1).astype(np.float32)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return flow, conf, frames


def round_loop(flow, conf, frames):
    """`ofgen.compose_warp_and_mask`'s loop on resident tensors (expand=False), restated."""
    n = flow.shape[0]
    c = (conf > THRES).to(torch.float32)
    mask = torch.zeros((1, H, W), dtype=torch.uint8, device=flow.device)
    ret = None
    order = []
    for _ in range(n):
        scores = ops.conf_sum(c[..., None].contiguous(), 0)
        s = int(torch.argmax(scores).item())
        order.append(s)
        warped = ops.warp(frames[s], flow[s][None], mode=MODE, sign=1.0)
        last = c[s].clone()
        cur = (last * 255).to(torch.uint8)[None]
        mask = mask | cur
        ret = warped.clone() if ret is None else ops.merge_images(ret, warped, cur)
        c -= last[None]
        c.clamp_(0, 1)
    return ret[0], mask[0], order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "compose_rate needs a GPU"
    lines = [f"greedy multi-reference composition at {W}x{H}, {MODE}, thres {THRES}; ms per call, one warm-up call of each, mean of {ROUNDS} "
             "rounds [fastest .. slowest], the routes alternating inside every round",
             f"  compose_refs: device events around {CALLS} calls; round loop (resident) and compose_warp_and_mask (numpy): host clock around "
             f"{HOST_CALLS} calls and a device synchronise (both synchronise by themselves, once per round)", ""]
    for n in (1, 2, 3):
        flow, conf, frames = scene(n)
        dflow, dconf, dframes = (torch.from_numpy(a).cuda() for a in (flow, conf, frames))
        fm = np.concatenate([flow, conf[..., None]], -1)[:, None].copy()
        orig = frames[0]
        fns = {"compose_refs": (lambda: ops.compose_refs(dflow, dconf, dframes, THRES, MODE), device_ms, CALLS),
               "loop": (lambda: round_loop(dflow, dconf, dframes), host_ms, HOST_CALLS),
               "numpy": (lambda: ofgen.compose_warp_and_mask(fm.copy(), list(frames), orig, THRES, MODE, expand=False), host_ms, HOST_CALLS)}
        t = rounds(fns)
        ret, mask, select, order, counts = ops.compose_refs(dflow, dconf, dframes, THRES, MODE)
        lret, lmask, lorder = round_loop(dflow, dconf, dframes)
        same = bool(torch.equal(ret, lret)) and bool(torch.equal(mask, lmask)) and order.tolist() == lorder
        share = [round(float((select == s).float().mean()), 3) for s in range(n)]
        lines += [f"N = {n}   order {order.tolist()}   counts {counts.tolist()}   share of pixels sampled per reference {share}   covered "
                  f"{float((mask == 255).float().mean()):.3f}   equal to the round loop: {same}",
                  f"    compose_refs                      {fmt(t['compose_refs'])}",
                  f"    round loop, resident tensors      {fmt(t['loop'])}   compose_refs is {verdict(t['compose_refs'], t['loop'])}",
                  f"    compose_warp_and_mask from numpy  {fmt(t['numpy'])}   compose_refs is {verdict(t['compose_refs'], t['numpy'])}", ""]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
