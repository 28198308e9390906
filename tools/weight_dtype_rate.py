#!/usr/bin/env python3
"""What `weight_dtype="fp16"` (the convolution / GEMM operands stored in half, OFX_PREC_F16_W) does to time and memory, against
`precision="fp16"` with fp32 weights -- always the baseline, measured in the same session from the same library, never copied.

Every arm runs in a fresh child process; the arms alternate for `--rounds` rounds so that drift and other tenants hit both; a figure
is device-event time over back-to-back calls after a warm-up; each line gives the mean over rounds with [fastest .. slowest].  A
bracket wholly above the baseline's is "slower", wholly below "faster", anything else is inside the run-to-run spread.

Sections (--sections, comma separated, default all):
  layers      the 207 ofx_conv2d launches of one SD v1.5 UNet forward (batch 2, 64x96 latent; tests/test_conv_f16_host.py walks them)
              as their distinct shapes, each timed alone over 10 back-to-back launches after 3 and weighted by its launches per
              forward: ms per forward by family (what the plan makes of a layer), and the 1280-channel levels (8x12 and 16x24) apart.
              Back-to-back launches of one layer find its weights in the last-level cache; the whole forward below does not.
  unet        `UNetModel.forward_nhwc` at that workload with attention_precision fp32 and fp16
  controlnet  `ControlNet.forward` at the same latent with a 512x768 hint
  vae         `VaeEncoder.encode_moments` / `VaeDecoder.decode` of one 512x768 frame, and the decoder's three Upsample layers alone
Every model section also prints the bytes of weights each arm holds on the device.

    python tools/weight_dtype_rate.py [--sections layers,unet] [--out profiles/r39_weight_half_rate.txt]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, LAT_H, LAT_W, CTX_TOKENS = 2, 64, 96, 77
ARMS = ("fp32 weights", "half weights")                               # the baseline first
FAMILIES = ("3x3 s1 patch", "3x3 s1 off-patch", "3x3 s2", "1x1 / GEMM", "all", "1280-ch @ 8x12", "1280-ch @ 16x24")
SECTIONS = ("layers", "unet", "controlnet", "vae")


def _events(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _weight_bytes(models):
    return sum(t.numel() * t.element_size() for m in models for t in m.w.values())


def child_layers(half: bool) -> dict:
    import torch
    from sd_animation_optical_flow_amd import _lib, ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_conv_f16_host import v15_conv_layers
    shapes = {}
    for _, B, h, w, c0, c1, cout, k, stride in v15_conv_layers(BATCH, LAT_H, LAT_W, CTX_TOKENS):
        shapes[(B, h, w, c0, c1, cout, k, stride)] = shapes.get((B, h, w, c0, c1, cout, k, stride), 0) + 1
    ms = {f: 0.0 for f in FAMILIES}
    g = torch.Generator(device="cuda").manual_seed(5)
    for (B, h, w, c0, c1, cout, k, stride), count in sorted(shapes.items()):
        cin = c0 + c1
        kpad = (k * k * cin + 31) // 32 * 32
        x = torch.randn((B, h, w, c0), device="cuda", generator=g)
        x2 = torch.randn((B, h, w, c1), device="cuda", generator=g) if c1 else None
        wp = torch.randn((cout, kpad), device="cuda", generator=g) * (1.0 / (k * k * cin) ** 0.5)
        bias = torch.randn((cout,), device="cuda", generator=g)
        if half:
            wp = wp.half()
        d = _lib.ConvDesc()
        d.in0, d.ld0, d.c0, d.w, d.out, d.ldo = 0x10000, c0, c0, 0x10000, 0x10000, cout
        if c1:
            d.in1, d.ld1, d.c1 = 0x10000, c1, c1
        d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, h, w, (h - 1) // stride + 1, (w - 1) // stride + 1, cout
        d.KH, d.KW, d.stride, d.padH, d.padW, d.precision = k, k, stride, k // 2, k // 2, 7 if half else 5
        p = _lib.ConvPlan()
        assert _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 0, C.byref(p)) == 0
        fam = "1x1 / GEMM" if k == 1 else "3x3 s2" if stride == 2 else "3x3 s1 patch" if p.mode == 2 else "3x3 s1 off-patch"
        out = torch.empty((B, d.Hout, d.Wout, cout), device="cuda")
        run = lambda: ops.conv2d_nhwc(x, wp, k, k, cout, stride=stride, shift=bias, x2=x2, out=out, precision="fp16_w" if half else "fp16")
        t = _events(run, 10, 3) * count
        ms[fam] += t
        ms["all"] += t
        pixels = h * w
        if max(cin, cout) >= 1280 and pixels in (8 * 12, 16 * 24):
            ms["1280-ch @ 8x12" if pixels == 96 else "1280-ch @ 16x24"] += t
    return dict(ms=ms, shapes=len(shapes), launches=sum(shapes.values()))


def _unet_inputs(cfg):
    import torch
    g = torch.Generator().manual_seed(20)
    x = torch.randn((BATCH, LAT_H, LAT_W, cfg["in_channels"]), generator=g).cuda()
    return x, torch.tensor([981.0, 981.0]).cuda(), torch.randn((BATCH, CTX_TOKENS, cfg["context_dim"]), generator=g).cuda()


def child_unet(half: bool, reps: int, warmup: int) -> dict:
    import torch
    from sd_animation_optical_flow_amd import unet as UN
    cfg = UN.SD_V15_UNET
    sd = UN.random_unet_state_dict(0, cfg)
    x, t, ctx = _unet_inputs(cfg)
    res = {"ms": {}}
    for ap in ("fp32", "fp16"):
        model = UN.UNetModel(sd, cfg, prefix="", precision="fp16", attention_precision=ap, weight_dtype="fp16" if half else "fp32")
        out, _ = model.forward_nhwc(x, t, ctx)
        res["ms"][f"UNetModel.forward_nhwc, attention_precision={ap}"] = _events(lambda: model.forward_nhwc(x, t, ctx), reps, warmup)
        res.setdefault("checksum", {})[ap] = float(out.double().abs().mean())
        res["bytes"] = _weight_bytes([model] + list(model.st.values()))
        del model
        torch.cuda.empty_cache()
    return res


def child_controlnet(half: bool, reps: int, warmup: int) -> dict:
    import torch
    from sd_animation_optical_flow_amd import controlnet as CN
    cfg = CN.SD_V15_CONTROLNET
    net = CN.ControlNet(CN.random_controlnet_state_dict(0, cfg), cfg, prefix="", precision="fp16", weight_dtype="fp16" if half else "fp32")
    g = torch.Generator().manual_seed(21)
    x = torch.randn((BATCH, cfg["in_channels"], LAT_H, LAT_W), generator=g).cuda()
    hint = torch.rand((BATCH, cfg["hint_channels"], 8 * LAT_H, 8 * LAT_W), generator=g).cuda()
    t = torch.tensor([981.0, 981.0]).cuda()
    ctx = torch.randn((BATCH, CTX_TOKENS, cfg["context_dim"]), generator=g).cuda()
    outs = net(x, hint, t, ctx)
    return dict(ms={"ControlNet.forward": _events(lambda: net(x, hint, t, ctx), reps, warmup)},
                checksum=float(sum(o.double().abs().mean() for o in outs)), bytes=_weight_bytes([net] + list(net.st.values())))


def child_vae(half: bool, reps: int, warmup: int) -> dict:
    import torch
    from sd_animation_optical_flow_amd import ops
    from sd_animation_optical_flow_amd.vae import VaeDecoder, VaeEncoder, random_vae_decoder_state_dict, random_vae_state_dict
    wd = "fp16" if half else "fp32"
    enc = VaeEncoder(random_vae_state_dict(0), precision="fp16", weight_dtype=wd)
    dec = VaeDecoder(random_vae_decoder_state_dict(0), precision="fp16", weight_dtype=wd)
    g = torch.Generator().manual_seed(22)
    image = (torch.rand((1, 3, 8 * LAT_H, 8 * LAT_W), generator=g) * 2 - 1).cuda()
    z = torch.randn((1, 4, LAT_H, LAT_W), generator=g).cuda()
    ms = {"VaeEncoder.encode_moments 512x768": _events(lambda: enc.encode_moments(image), reps, warmup),
          "VaeDecoder.decode 512x768": _events(lambda: dec.decode(z), reps, warmup)}
    mult, ch = dec.cfg["ch_mult"], dec.cfg["ch"]
    for lvl in range(len(mult) - 1, 0, -1):                              # the Upsample after level lvl: ch * mult[lvl] channels, latent << (top - lvl)
        c, s = ch * mult[lvl], 1 << (len(mult) - 1 - lvl)
        xu = torch.randn((1, LAT_H * s, LAT_W * s, c), device="cuda")
        name = f"decoder.up.{lvl}.upsample.conv"
        wf, b = dec.w[f"{name}.weight.folded"], dec.w[f"{name}.bias"]
        out = torch.empty((1, 2 * LAT_H * s, 2 * LAT_W * s, c), device="cuda")
        ms[f"Upsample {c} ch, {LAT_H * s}x{LAT_W * s} -> {2 * LAT_H * s}x{2 * LAT_W * s}"] = _events(
            lambda: ops.upconv2x(xu, wf, b, out=out, precision="fp16"), 10, 3)
    return dict(ms=ms, checksum=float(dec.decode(z).double().abs().mean()), bytes=_weight_bytes([enc, dec]))


def run_child(section: str, half: bool, a) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", section, "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--half"] if half else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f"child failed ({r.returncode}); nothing further is started\n{r.stdout}\n{r.stderr}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def verdict(base, other):
    if min(other) > max(base):
        return "SLOWER (bracket wholly above the baseline's)"
    if max(other) < min(base):
        return "faster (bracket wholly below the baseline's)"
    return "inside the run-to-run spread (the brackets overlap)"


def section_text(section: str, a) -> str:
    runs = {arm: [] for arm in ARMS}
    for rnd in range(a.rounds):
        for arm in ARMS:
            runs[arm].append(run_child(section, arm == ARMS[1], a))
            print(f"{section} round {rnd} {arm}: " + ", ".join(f"{v:.3f}" for v in runs[arm][-1]["ms"].values()), flush=True)
    stat = lambda v: f"{sum(v) / len(v):9.3f} [{min(v):8.3f} .. {max(v):8.3f}]"
    lines = [f"== {section} ==  ms, device events, mean of {a.rounds} rounds [fastest .. slowest], arms in alternating fresh processes; "
             f"both arms precision=\"fp16\"", ""]
    if section == "layers":
        r0 = runs[ARMS[0]][0]
        lines.append(f"the {r0['launches']} ofx_conv2d launches of one SD v1.5 forward (batch {BATCH}, latent {LAT_H}x{LAT_W}) as {r0['shapes']} distinct "
                     f"shapes, each alone over 10 back-to-back launches after 3, weighted by its launches per forward: ms per forward")
    for key in runs[ARMS[0]][0]["ms"]:
        v = {arm: [r["ms"][key] for r in runs[arm]] for arm in ARMS}
        lines.append(f"  {key}")
        for arm in ARMS:
            lines.append(f"    {arm:14s} {stat(v[arm])}")
        m0, m1 = (sum(v[arm]) / len(v[arm]) for arm in ARMS)
        lines.append(f"    half / fp32 = {m1 / m0:.3f}: {verdict(v[ARMS[0]], v[ARMS[1]])}")
    if "bytes" in runs[ARMS[0]][0]:
        b0, b1 = runs[ARMS[0]][0]["bytes"], runs[ARMS[1]][0]["bytes"]
        lines.append(f"  weights on the device: {b0} bytes ({b0 / 2 ** 30:.3f} GiB) with fp32 weights, {b1} bytes ({b1 / 2 ** 30:.3f} GiB) with "
                     f"weight_dtype=\"fp16\" ({b1 / b0:.3f})")
        same = runs[ARMS[0]][0]["checksum"] == runs[ARMS[1]][0]["checksum"]
        lines.append(f"  mean |out| of both arms {'equal' if same else 'DIFFERENT'}: {runs[ARMS[0]][0]['checksum']} / {runs[ARMS[1]][0]['checksum']}")
    lines.append("")
    return "\n".join(lines)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--out")
    ap.add_argument("--child", choices=SECTIONS)
    ap.add_argument("--half", action="store_true")
    a = ap.parse_args()
    if a.child:
        import torch
        assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
        fn = dict(layers=lambda: child_layers(a.half), unet=lambda: child_unet(a.half, a.reps, a.warmup),
                  controlnet=lambda: child_controlnet(a.half, a.reps, a.warmup), vae=lambda: child_vae(a.half, a.reps, a.warmup))[a.child]
        print("RESULT " + json.dumps(fn()))
        return
    sections = [s.strip() for s in a.sections.split(",") if s.strip()]
    assert all(s in SECTIONS for s in sections), sections
    text = ""
    for s in sections:
        text += section_text(s, a) + "\n"
        if a.out:                                                        # written section by section: a later failure keeps the earlier ones
            with open(a.out, "w") as f:
                f.write(text)
    print(text)


if __name__ == "__main__":
    main()
