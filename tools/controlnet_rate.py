#!/usr/bin/env python3
"""ControlNet rate on the full SD v1.5 configuration: the hint stem's `ofx_conv3x3_silu` layers against the torch layers they
replace (torch.nn.functional.conv2d + F.silu on NCHW, what OFX_CNET_TORCH_GLUE=1 runs), the whole stem at hint batch 1 and 2,
`ControlNet.forward` whole and, for scale, one `UNetModel.forward` in the same session.

Workload: `SD_V15_CONTROLNET` with seeded weights, UNet batch 2 (cond / uncond), a 64 x 96 latent, a 512 x 768 hint, 77 x 768
context.  The reference computes the residuals once per frame (controlnet.py:413-419), so none of this is on the sampler's
per-step path: the figures are recorded, not gated.

One process; after `--warmup` calls of everything, `--rounds` rounds in which the variants alternate (so that drift and other
tenants hit all of them), each timing `--reps` back-to-back calls between two device events.  A figure is the median over rounds
with the fastest and slowest round behind it.  TFLOP/s of a layer: 2 * pixels * 9 * Cin * Cout executed FLOPs (Cin = 3 counted as
the 4 the kernel runs) over the median.

    python tools/controlnet_rate.py [--out profiles/r27_controlnet_rate.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, LAT_H, LAT_W, CTX_TOKENS = 2, 64, 96, 77


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-unet", action="store_true", help="skip the UNetModel.forward line")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from sd_animation_optical_flow_amd import controlnet as CN, ops
    from sd_animation_optical_flow_amd import unet as UN
    assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
    cfg = CN.SD_V15_CONTROLNET
    sd = CN.random_controlnet_state_dict(0, cfg)
    net = CN.ControlNet(sd, cfg, prefix="")
    assert not net.stem_glue, "unset OFX_CNET_TORCH_GLUE: the tool times the torch layers itself"
    lay = net.layout["hint"]
    g = torch.Generator().manual_seed(27)
    x = torch.randn((BATCH, cfg["in_channels"], LAT_H, LAT_W), generator=g).cuda()
    hint2 = torch.rand((BATCH, 3, 8 * LAT_H, 8 * LAT_W), generator=g).cuda()
    hint1 = hint2[:1].contiguous()
    t = torch.tensor([981.0, 981.0]).cuda()
    ctx = torch.randn((BATCH, CTX_TOKENS, cfg["context_dim"]), generator=g).cuda()
    oihw = {name: sd[f"{name}.weight"].cuda() for name, _, _, _ in lay}

    def glue_stem(h):
        for i, (name, _, _, stride) in enumerate(lay):
            h = F.conv2d(h, oihw[name], net.w[f"{name}.bias"], stride=stride, padding=1)
            if i != len(lay) - 1:
                h = F.silu(h)
        return h

    # per layer: its input at hint batch 1 in both layouts, from one run of the stem
    variants, flops = [], {}
    nhwc = torch.zeros((1, 8 * LAT_H, 8 * LAT_W, net.hint_pad), device="cuda")
    nhwc[..., :3] = hint1.permute(0, 2, 3, 1)
    nchw = hint1
    for i, (name, cin, cout, stride) in enumerate(lay):
        silu = i != len(lay) - 1
        w, b, wo = net.w[f"{name}.weight"], net.w[f"{name}.bias"], oihw[name]
        variants.append((f"{name} kernel", lambda xi=nhwc, w=w, b=b, cout=cout, stride=stride, silu=silu: ops.conv3x3_silu(xi, w, b, cout, stride=stride, silu=silu)))
        variants.append((f"{name} torch", lambda xi=nchw, wo=wo, b=b, stride=stride, silu=silu:
                         F.silu(F.conv2d(xi, wo, b, stride=stride, padding=1)) if silu else F.conv2d(xi, wo, b, stride=stride, padding=1)))
        nhwc = ops.conv3x3_silu(nhwc, w, b, cout, stride=stride, silu=silu)
        nchw = variants[-1][1]()
        flops[name] = 2.0 * nhwc.shape[1] * nhwc.shape[2] * 9 * ((cin + 3) // 4 * 4) * cout
        err = float((nhwc.permute(0, 3, 1, 2) - nchw).abs().max())
        assert err <= 1e-3 * max(1.0, float(nchw.abs().max())), (name, err)         # the two really compute the same layer
    variants += [("stem kernel, hint batch 1", lambda: net.hint_stem(hint1)), ("stem torch, hint batch 1", lambda: glue_stem(hint1)),
                 ("stem kernel, hint batch 2", lambda: net.hint_stem(hint2)), ("stem torch, hint batch 2", lambda: glue_stem(hint2)),
                 ("ControlNet.forward, hint batch 1", lambda: net(x, hint1, t, ctx)),
                 ("ControlNet.forward, hint batch 2", lambda: net(x, hint2, t, ctx))]
    if not a.no_unet:
        ucfg = UN.SD_V15_UNET
        unet = UN.UNetModel(UN.random_unet_state_dict(0, ucfg), ucfg, prefix="")
        ux = torch.randn((BATCH, ucfg["in_channels"], LAT_H, LAT_W), generator=g).cuda()
        control = net(x, hint1, t, ctx)
        variants.append(("UNetModel.forward(control=), for scale", lambda: unet(ux, t, ctx, control=control)))

    for _, fn in variants:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in variants}
    for _ in range(a.rounds):
        for label, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1) / a.reps)

    def fig(label):
        v = times[label]
        return statistics.median(v), min(v), max(v)

    lines = [f"ControlNet rate: SD_V15_CONTROLNET, seeded weights, UNet batch {BATCH}, {LAT_H} x {LAT_W} latent, {8 * LAT_H} x {8 * LAT_W} hint, "
             f"{CTX_TOKENS} x {cfg['context_dim']} context",
             f"device: {torch.cuda.get_device_name(0)}; one process, {a.warmup} warm-up calls, {a.rounds} alternating rounds of {a.reps} "
             f"back-to-back calls; ms per call: median over rounds [fastest, slowest]", "",
             "hint stem, layer by layer at hint batch 1: ofx_conv3x3_silu (NHWC) against F.conv2d + F.silu (NCHW)",
             f"  {'layer':22s} {'shape':26s} {'kernel ms':>26s} {'TFLOP/s':>8s} {'torch ms':>26s} {'kernel / torch':>15s}"]
    hh, ww = 8 * LAT_H, 8 * LAT_W
    losses = []
    for name, cin, cout, stride in lay:
        k, kl, kh = fig(f"{name} kernel")
        tt, tl, th = fig(f"{name} torch")
        shape = f"{cin}->{cout} s{stride} {hh}x{ww}"
        hh, ww = (hh - 1) // stride + 1, (ww - 1) // stride + 1
        lines.append(f"  {name:22s} {shape:26s} {k:9.3f} [{kl:.3f}, {kh:.3f}] {flops[name] / k / 1e9:8.2f} {tt:9.3f} [{tl:.3f}, {th:.3f}] {k / tt:15.2f}")
        if k > tt:
            losses.append(name)
    lines.append("  the kernel loses to the torch layer on: " + (", ".join(losses) if losses else "no layer"))
    lines.append("")
    for label, _ in variants[2 * len(lay):]:
        m, lo, hi = fig(label)
        lines.append(f"{label:44s} {m:9.3f} ms [{lo:.3f}, {hi:.3f}]")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
