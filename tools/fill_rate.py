"""Rate of the 4-channel Gaussian blur and of `ops.fill_mask_input` on the GPU box, each beside a baseline that is not the code
under test:
  (a) `ops.gaussian_blur_rgba_u8` on a [1,H,W,4] image against `ops.gaussian_blur_u8` (the tap-summing kernel) on its four planes
      [4,H,W], at 512x768 (one frame) and 1536x768 (a strip of three), radii 2, 4, 16, 64, 256;
  (b) `ops.fill_mask_input` against the host route the reference takes: device-to-host copy of frame and mask, the Pillow chain,
      upload of the result (measured only where Pillow is importable; host clock around a device synchronise).
Device events around CALLS calls after one warm-up call of each; the two sides alternate inside every round; mean of the rounds
with [fastest .. slowest].
    python tools/fill_rate.py [--out FILE]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

from sd_animation_optical_flow_amd import ops

SIZES = ((768, 512), (768, 1536))            # (H, W): one 512-wide frame, a strip of three
RADII = (2, 4, 16, 64, 256)
ROUNDS, CALLS, HOST_CALLS = 3, 20, 2


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
    """fns: name -> (callable, timer, calls).  One warm-up call each, then ROUNDS rounds in which the entries alternate."""
    for f, _, _ in fns.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, (f, timer, calls) in fns.items():
            times[k].append(timer(f, calls))
    return times


def fmt(v):
    return f"{sum(v) / len(v):9.3f} [{min(v):9.3f} .. {max(v):9.3f}] ms"


def verdict(new, old):
    if max(new) < min(old):
        return "below"
    if min(new) > max(old):
        return "ABOVE"
    return "overlap"


def frame(H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([127 + 120 * np.sin(xx / (17 + c)) * np.cos(yy / (23 - c)) for c in range(3)], -1).astype(np.uint8)
    mask = np.zeros((H, W), np.uint8)
    mask[H // 4:H // 2, W // 8:W // 3] = 255
    mask[np.random.default_rng(0).random((H, W)) < 0.002] = 255
    return img, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fill_rate needs a GPU"
    lines = [f"ops.gaussian_blur_rgba_u8 and ops.fill_mask_input; ms per call, device events around {CALLS} calls after one warm-up call of "
             f"each, mean of {ROUNDS} rounds [fastest .. slowest], the two sides alternating inside every round",
             "", "(a) GaussianBlur of one [1,H,W,4] image: the prefix-sum kernel (rgba) against ops.gaussian_blur_u8 on its four planes [4,H,W]"]
    for H, W in SIZES:
        img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (1, H, W, 4), dtype=np.uint8)).cuda()
        planes = img.permute(0, 3, 1, 2).reshape(4, H, W).contiguous()
        lines.append(f"\n  {W}x{H}")
        for radius in RADII:
            t = rounds({"rgba": (lambda: ops.gaussian_blur_rgba_u8(img, radius), device_ms, CALLS),
                        "planes": (lambda: ops.gaussian_blur_u8(planes, radius), device_ms, CALLS)})
            lines.append(f"    radius {radius:3d}   rgba {fmt(t['rgba'])}   four planes {fmt(t['planes'])}   rgba is {verdict(t['rgba'], t['planes'])}")
    lines += ["", "(b) fill_mask_input of one frame: the device chain against device-to-host copy + Pillow + upload (host clock, "
              f"{HOST_CALLS} calls per round)"]
    try:
        import PIL
        import fill_check as FC
    except ImportError:
        PIL = None
    for H, W in SIZES:
        image, mask0 = frame(H, W)
        img = torch.from_numpy(image).cuda()[None]
        m = ops.gaussian_blur_u8(torch.from_numpy(mask0).cuda()[None], 4.0)
        fns = {"device": (lambda: ops.fill_mask_input(img, m), device_ms, CALLS)}
        if PIL is not None:
            fns["host"] = (lambda: torch.from_numpy(FC.pil_fill_mask_input(img[0].cpu().numpy(), m[0].cpu().numpy())).cuda(), host_ms, HOST_CALLS)
        t = rounds(fns)
        line = f"\n  {W}x{H}   device {fmt(t['device'])}"
        if PIL is not None:
            same = bool(torch.equal(fns["device"][0](), fns["host"][0]()[None]))
            line += f"   host route {fmt(t['host'])}   device is {verdict(t['device'], t['host'])}; results equal: {same}"
        else:
            line += "   host route not measured: Pillow is not importable here"
        lines.append(line)
    if PIL is not None:
        lines.append(f"\n  Pillow {PIL.__version__}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
