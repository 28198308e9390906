#!/usr/bin/env python3
"""First-stage decoder rate: the fused nearest-2x upsample convolution against the unfused pair, per layer and end to end.

One process, seeded weights, one 512x768 frame (latent 96x64).  Every figure is device-event time over `--reps` back-to-back calls
after a warm-up of the same shape; the two variants alternate for `--rounds` rounds so that drift and other tenants hit both, and
each line gives the mean over rounds with the fastest and slowest round behind it.

  layers    the three `Upsample` layers of the SD-v1 decoder (512 -> 512 at 96x64 and 192x128, 256 -> 256 at 384x256):
            `ops.upconv2x` against `ops.upsample2x_nearest` + the 3x3 `ops.conv2d_nhwc` of the same build, the largest output
            difference between the two, and TFLOP/s by the layer's nominal arithmetic (9 taps per output; the fused kernel executes
            4/9 of it).
  decoder   milliseconds per frame of `VaeDecoder.decode`, every Upsample fused against every Upsample unfused (what
            OFX_VAE_NO_UPCONV=1 selects), and of `decode_latent` (the byte exit included).

  --precision fp32,fp16   the precision arms instead: per Upsample layer `ops.upconv2x(precision=)` and the unfused pair in every arm,
            then `VaeDecoder.decode` (fused and unfused), `decode_latent` and `VaeEncoder.encode_moments` on the same frame with one
            object per arm.  Every arm of a section alternates inside every round; the first arm is the yardstick (the fp32 path
            of the same build in the same session).

    python tools/vae_decode_rate.py [--out profiles/r16_vae_decode_rate.txt] [--only layers|decoder] [--precision fp32,fp16]
"""
import argparse
import json
import os
import sys
import threading

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sd_animation_optical_flow_amd import ops                                              # noqa: E402
from sd_animation_optical_flow_amd.vae import VaeDecoder, random_vae_decoder_state_dict    # noqa: E402

LAYERS = [(3, 512, 96, 64), (2, 512, 192, 128), (1, 256, 384, 256)]      # decoder level, channels, low-resolution H, W


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


def _event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, rounds):
    """{name: fn} -> {name: (mean, fastest, slowest)} in ms per call, the variants taking turns inside every round."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(_event_ms(fn, reps))
    return {k: (sum(v) / len(v), min(v), max(v)) for k, v in t.items()}


def fmt(r):
    return f"{r[0]:8.3f} ms  (rounds {r[1]:.3f} .. {r[2]:.3f})"


def layer_case(lvl, c, H, W, reps, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(lvl)
    x = torch.randn((1, H, W, c), generator=g, device="cuda")
    w = torch.randn((c, c, 3, 3), generator=torch.Generator().manual_seed(lvl)) / (9 * c) ** 0.5
    b = torch.randn((c,), generator=g, device="cuda") * 0.1
    wf, wp = ops.upconv2x_weight(w).cuda(), ops.pack_conv_weight(w).cuda()
    fused = lambda: ops.upconv2x(x, wf, b)
    unfused = lambda: ops.conv2d_nhwc(ops.upsample2x_nearest(x), wp, 3, 3, c, shift=b)
    up_only = lambda: ops.upsample2x_nearest(x)
    diff = float((fused() - unfused()).abs().max())
    r = alternate({"fused": fused, "unfused": unfused, "upsample": up_only}, reps, rounds)
    nominal = 2.0 * 4 * H * W * c * 9 * c
    lines.append(f"up.{lvl}.upsample  {c} -> {c}, {H}x{W} -> {2 * H}x{2 * W}   (nominal {nominal / 1e9:.1f} GFLOP, fused executes 4/9)")
    lines.append(f"    ofx_upconv2x                        {fmt(r['fused'])}   {nominal / r['fused'][0] / 1e9:7.1f} nominal TFLOP/s, "
                 f"{nominal * 4 / 9 / r['fused'][0] / 1e9:.1f} executed")
    lines.append(f"    ofx_upsample2x_nearest + ofx_conv2d {fmt(r['unfused'])}   {nominal / r['unfused'][0] / 1e9:7.1f} nominal TFLOP/s")
    lines.append(f"      of which the upsample alone       {fmt(r['upsample'])}")
    lines.append(f"    unfused / fused = {r['unfused'][0] / r['fused'][0]:.3f}     max |fused - unfused| = {diff:.2e}")
    return r["unfused"][0] / r["fused"][0]


def decoder_case(reps, rounds, lines):
    dec = VaeDecoder(random_vae_decoder_state_dict(0))
    z = torch.randn((1, 4, 96, 64), generator=torch.Generator().manual_seed(1)).cuda()
    lv = list(dec.fused_upsample)

    def run(fused, fn):
        def f():
            dec.fused_upsample = {k: fused for k in lv}
            return fn(z)
        return f
    diff = float((run(True, dec.decode)() - run(False, dec.decode)()).abs().max())
    r = alternate({"fused": run(True, dec.decode), "unfused": run(False, dec.decode), "bytes": run(True, dec.decode_latent)}, reps, rounds)
    lines.append("VaeDecoder, one 512x768 frame (latent 96x64), ms per frame")
    lines.append(f"    decode, Upsample layers fused               {fmt(r['fused'])}")
    lines.append(f"    decode, unfused (OFX_VAE_NO_UPCONV=1)       {fmt(r['unfused'])}")
    lines.append(f"    decode_latent (fused, to BGR bytes)         {fmt(r['bytes'])}")
    lines.append(f"    unfused / fused = {r['unfused'][0] / r['fused'][0]:.3f}     max |fused - unfused| over the image = {diff:.2e}")


def precision_layer_case(lvl, c, H, W, precs, reps, rounds, lines):
    """One Upsample layer in every precision of `precs`, fused and unfused, all arms alternating inside every round."""
    g = torch.Generator(device="cuda").manual_seed(lvl)
    x = torch.randn((1, H, W, c), generator=g, device="cuda")
    w = torch.randn((c, c, 3, 3), generator=torch.Generator().manual_seed(lvl)) / (9 * c) ** 0.5
    b = torch.randn((c,), generator=g, device="cuda") * 0.1
    wf, wp = ops.upconv2x_weight(w).cuda(), ops.pack_conv_weight(w).cuda()
    fns = {}
    for p in precs:
        fns[f"fused {p}"] = lambda p=p: ops.upconv2x(x, wf, b, precision=p)
        fns[f"unfused {p}"] = lambda p=p: ops.conv2d_nhwc(ops.upsample2x_nearest(x), wp, 3, 3, c, shift=b, precision=p)
    r = alternate(fns, reps, rounds)
    nominal = 2.0 * 4 * H * W * c * 9 * c
    lines.append(f"up.{lvl}.upsample  {c} -> {c}, {H}x{W} -> {2 * H}x{2 * W}   (nominal {nominal / 1e9:.1f} GFLOP, fused executes 4/9; "
                 f"BN {ops.upconv2x_bn(c)})")
    for p in precs:
        lines.append(f"    ofx_upconv2x {p:4s}                        {fmt(r[f'fused {p}'])}   {nominal * 4 / 9 / r[f'fused {p}'][0] / 1e9:7.1f} executed TFLOP/s")
        lines.append(f"    ofx_upsample2x_nearest + ofx_conv2d {p:4s} {fmt(r[f'unfused {p}'])}")
    base = precs[0]
    for p in precs[1:]:
        lines.append(f"    fused {base} / fused {p} = {r[f'fused {base}'][0] / r[f'fused {p}'][0]:.3f}     unfused {p} / fused {p} = "
                     f"{r[f'unfused {p}'][0] / r[f'fused {p}'][0]:.3f}     max |fused {p} - fused {base}| = "
                     f"{float((fns[f'fused {p}']() - fns[f'fused {base}']()).abs().max()):.2e}")


def precision_model_case(precs, reps, rounds, lines):
    """`VaeDecoder.decode` / `decode_latent` and `VaeEncoder.encode_moments` on one 512x768 frame, one object per precision."""
    from sd_animation_optical_flow_amd.vae import VaeEncoder, random_vae_state_dict
    dsd, esd = random_vae_decoder_state_dict(0), random_vae_state_dict(0)
    z = torch.randn((1, 4, 96, 64), generator=torch.Generator().manual_seed(1)).cuda()
    image = (torch.rand((1, 3, 768, 512), generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    decs = {p: VaeDecoder(dsd, precision=p) for p in precs}
    encs = {p: VaeEncoder(esd, precision=p) for p in precs}

    def unfused(dec):
        def f():
            keep = dec.fused_upsample
            dec.fused_upsample = {k: False for k in keep}
            try:
                return dec.decode(z)
            finally:
                dec.fused_upsample = keep
        return f
    fns = {}
    for p in precs:
        fns[f"decode {p}"] = lambda p=p: decs[p].decode(z)
        fns[f"decode unfused {p}"] = unfused(decs[p])
        fns[f"decode_latent {p}"] = lambda p=p: decs[p].decode_latent(z)
        fns[f"encode_moments {p}"] = lambda p=p: encs[p].encode_moments(image)
    r = alternate(fns, reps, rounds)
    lines.append("VaeDecoder / VaeEncoder, one 512x768 frame (latent 96x64), ms per frame")
    for what in ("decode", "decode unfused", "decode_latent", "encode_moments"):
        for p in precs:
            lines.append(f"    {what + ' ' + p:28s} {fmt(r[f'{what} {p}'])}")
        base = precs[0]
        for p in precs[1:]:
            lines.append(f"      {base} / {p} = {r[f'{what} {base}'][0] / r[f'{what} {p}'][0]:.3f}")
    for p in precs[1:]:
        lines.append(f"    max |decode {p} - decode {precs[0]}| = {float((decs[p].decode(z) - decs[precs[0]].decode(z)).abs().max()):.2e}     "
                     f"max |encode_moments {p} - {precs[0]}| = {float((encs[p].encode_moments(image) - encs[precs[0]].encode_moments(image)).abs().max()):.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r16_vae_decode_rate.txt"))
    ap.add_argument("--only", choices=["layers", "decoder"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--precision", help='comma-separated arms, e.g. "fp32,fp16": the first is the yardstick; the Upsample layers, '
                    "VaeDecoder.decode / decode_latent and VaeEncoder.encode_moments in every arm instead of the fused / unfused report")
    a = ap.parse_args()
    precs = [ops.check_upconv_precision(p) for p in a.precision.split(",")] if a.precision else None
    if precs and a.rounds < 3:
        sys.exit("--precision: at least 3 rounds")
    if not torch.cuda.is_available():
        sys.exit("vae_decode_rate.py needs a GPU: nothing is measured without one")
    lines = [f"tools/vae_decode_rate.py --reps {a.reps} --rounds {a.rounds}{' --precision ' + a.precision if a.precision else ''}   "
             f"({torch.cuda.get_device_name(0)})",
             "device-event time per call, mean over rounds (fastest .. slowest round); the variants alternate inside every round", ""]
    if a.only in (None, "layers"):
        for (lvl, c, H, W) in LAYERS:
            with Watchdog(120, f"layer up.{lvl}"):
                if precs:
                    precision_layer_case(lvl, c, H, W, precs, a.reps, a.rounds, lines)
                else:
                    layer_case(lvl, c, H, W, a.reps, a.rounds, lines)
            lines.append("")
    if a.only in (None, "decoder"):
        with Watchdog(300, "decoder"):
            if precs:
                precision_model_case(precs, max(2, a.reps // 2), a.rounds, lines)
            else:
                decoder_case(max(2, a.reps // 2), a.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
