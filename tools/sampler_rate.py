#!/usr/bin/env python3
"""`GuidedDDIMSampler.decode` rate on the full SD v1.5 configuration against the same loop written from torch ops.

Workload: `SD_V15_UNET` (in_channels 9) with seeded weights, B = 1 with classifier-free guidance (UNet batch 2), a 64 x 96 latent (a
512 x 768 frame), 77 x 768 context, a 50-step schedule, t_start 20, the mask blend on in every step (eta 0): img2img_inpaint's loop
at denoising strength 0.4.

fused = `GuidedDDIMSampler.decode`: one padded NHWC buffer, per step `UNetModel.forward_nhwc(padded=True)` and ONE `ofx_ddim_step`.
torch = the loop the library did not have: the reference's expressions (guided_ldm_inpainting.py:39-64, :80-103, :127-129; ddpm.py:
356-359, :1405) as torch ops on NCHW tensors around `UNetModel.forward` -- torch.cat with c_concat, torch.cat x2, the permutes and the
pad inside `forward`, chunk, the guidance combination, pred_x0, dir_xt, x_prev, q_sample and the blend.  It lives here, not in the
library: there is no switch that selects it.

Both loops run in ONE process on the same model and the same noise, alternating, `--rounds` rounds each after one warm-up run of
each; a figure is device-event time around the whole loop (ending in a synchronise) divided by the steps: median over rounds
[fastest .. slowest].  Before timing, the two results are compared: the bar is four times the stored yardstick (the reference's fp32
run against float64 on configuration u0, case "a" of tests/golden/sampler_ref_u0.npz) relative to that case's largest value, scaled
to the largest value here; the distance is printed either way.

--bench-json A.json B.json ...: also quote `bench.py --gpus 1` result lines recorded in the same session (name=path, e.g.
parent=/tmp/bench_parent.json), value and unit as bench.py printed them.

    python tools/sampler_rate.py [--rounds 5] [--out profiles/r26_sampler_rate.txt] [--bench-json parent=a.json this=b.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAT_H, LAT_W, CTX_TOKENS, STEPS, T_START, CFG_SCALE = 64, 96, 77, 50, 20, 7.0


def torch_loop(model, sched, plan, x_latent, context, uncond, c_concat, init_latent, nmask, q_noise, scale):
    """The reference's loop from torch ops around `UNetModel.forward` (NCHW)."""
    import torch
    x_dec = x_latent
    b = x_latent.shape[0]
    dev = x_latent.device
    for i, (p, index, step, gs) in enumerate(plan):
        ts = torch.full((b,), float(step), device=dev)
        if gs > 0:
            noised = float(sched["sqrt_alphas_cumprod"][step]) * init_latent + float(sched["sqrt_one_minus_alphas_cumprod"][step]) * q_noise[i]
            x_dec = (1 - nmask) * noised + nmask * x_dec
        x_in = torch.cat([torch.cat([x_dec, c_concat], dim=1)] * 2)
        out, _ = model.forward(x_in, torch.cat([ts] * 2), torch.cat([uncond, context]))
        e_u, e_c = out.chunk(2)
        e_t = e_u + scale * (e_c - e_u)
        full = lambda v: torch.full((b, 1, 1, 1), float(v), device=dev)
        a_t, a_prev = full(sched["ddim_alphas"][index]), full(sched["ddim_alphas_prev"][index])
        sigma_t, s1m = full(sched["ddim_sigmas"][index]), full(sched["ddim_sqrt_one_minus_alphas"][index])
        pred_x0 = (x_dec - s1m * e_t) / a_t.sqrt()
        dir_xt = (1. - a_prev - sigma_t ** 2).sqrt() * e_t
        x_dec = a_prev.sqrt() * pred_x0 + dir_xt
    return x_dec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--bench-json", nargs="*", default=[])
    a = ap.parse_args()
    import numpy as np
    import torch
    from sd_animation_optical_flow_amd import unet as UN
    from sd_animation_optical_flow_amd.sampler import GuidedDDIMSampler, decode_plan
    assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
    cfg = UN.SD_V15_UNET
    model = UN.UNetModel(UN.random_unet_state_dict(0, cfg), cfg, prefix="")
    g = torch.Generator().manual_seed(26)
    r = lambda *s: torch.randn(s, generator=g).cuda()
    x1, init_latent = r(1, 4, LAT_H, LAT_W), r(1, 4, LAT_H, LAT_W)
    context, uncond = r(1, CTX_TOKENS, cfg["context_dim"]), r(1, CTX_TOKENS, cfg["context_dim"])
    c_concat = r(1, 5, LAT_H, LAT_W)
    nmask = torch.zeros((1, 4, LAT_H, LAT_W))
    nmask[:, :, 16:48, 24:72] = 1.0
    nmask = nmask.cuda()
    q_noise = r(T_START, 1, 4, LAT_H, LAT_W)
    sampler = GuidedDDIMSampler(model)
    sched = sampler.make_schedule(STEPS, 0.0)
    plan = decode_plan(sched, T_START)

    def fused():
        return sampler.decode(x1, context, T_START, unconditional_context=uncond, unconditional_guidance_scale=CFG_SCALE, c_concat=c_concat,
                              init_latent=init_latent, nmask=nmask, step_noise=q_noise)[0]

    def plain():
        return torch_loop(model, sched, plan, x1, context, uncond, c_concat, init_latent, nmask, q_noise, CFG_SCALE)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / T_START

    with torch.no_grad():
        xf, xt = fused(), plain()                                  # the warm-up run of each, and the agreement check
        gold = np.load(os.path.join(ROOT, "tests", "golden", "sampler_ref_u0.npz"))
        yard = dict(zip([str(k) for k in gold["dist_keys"]], gold["ref_vs_f64"]))["a"]
        rel = 4.0 * float(yard) / float(np.abs(gold["a.out"]).max())
        big = float(xt.abs().max())
        dist = float((xf - xt).abs().max())
        ms = {"fused": [], "torch": []}
        for rnd in range(a.rounds):
            for name, fn in (("fused", fused), ("torch", plain)):
                ms[name].append(timed(fn))
                print(f"round {rnd} {name}: {ms[name][-1]:.3f} ms per step", flush=True)
    stat = lambda v: f"{statistics.median(v):8.3f} [{min(v):7.3f} .. {max(v):7.3f}]"
    mf, mt = statistics.median(ms["fused"]), statistics.median(ms["torch"])
    spread = max(max(v) - min(v) for v in ms.values())
    overlap = not (max(ms["fused"]) < min(ms["torch"]) or min(ms["fused"]) > max(ms["torch"]))
    lines = [f"GuidedDDIMSampler.decode, SD v1.5 configuration (in_channels 9), seeded weights, B = 1 with classifier-free guidance (UNet batch "
             f"2), latent {LAT_H} x {LAT_W}, context {CTX_TOKENS} x 768, {STEPS}-step schedule, t_start {T_START}, mask blend in every step, eta 0; "
             f"ms per step, device events around the whole loop of {T_START} steps, median of {a.rounds} rounds [fastest .. slowest], the two loops "
             "alternating in one process after one warm-up run of each",
             "fused = one padded NHWC buffer, forward_nhwc(padded=True) + one ofx_ddim_step per step; torch = the reference's expressions as "
             "torch ops on NCHW around UNetModel.forward (written in tools/sampler_rate.py)", "",
             f"  fused {stat(ms['fused'])} ms per step", f"  torch {stat(ms['torch'])} ms per step",
             f"  torch - fused = {mt - mf:+.3f} ms per step ({100.0 * (mt - mf) / mt:+.2f} %); widest round-to-round spread {spread:.3f} ms; "
             + ("THE BRACKETS OVERLAP: the difference is inside the round-to-round spread" if overlap else "the brackets do not overlap"),
             f"  agreement of the two results: max |fused - torch| = {dist:.3e} at max |x| = {big:.3f}; bar {rel * big:.3e} (four times the stored "
             f"yardstick of case a, {float(yard):.3e}, relative to that case's largest value) -> {'inside' if dist <= rel * big else 'OUTSIDE'}", ""]
    if a.bench_json:
        lines.append("bench.py --gpus 1 in the same session (the flow path, which this change does not touch), one line per run as bench.py printed it:")
        for item in a.bench_json:
            name, path = item.split("=", 1)
            with open(path) as f:
                res = json.loads([ln for ln in f.read().splitlines() if ln.startswith("{")][-1])
            keep = {k: res[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup") if k in res}
            lines.append(f"  {name:10s} {json.dumps(keep)}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
