#!/usr/bin/env python3
"""One `warp_and_inpaint_crossattn` frame of `render.SdRenderer` at SD v1.5 sizes, broken down by stage.

Workload: a 512 x 768 frame, two reference frames, `SD_V15_UNET` (in_channels 9), the SD v1 VAE, two `SD_V15_CONTROLNET`s (the
driver's hed / canny pair; the "hed" detector is a stand-in threshold, HED is the caller's), seeded weights, random 77 x 768
contexts, 50 DDIM steps at denoising strength 0.6 (30 UNet calls at batch 2), one K/V history of a previous frame as reference_kv.

The frame is timed whole (`generate_ai_frame_with_ref`), then the same stages are run one by one as the renderer composes them, each
between device synchronisations on the host clock.  The figure of interest is the share of a frame that is NOT the `decode` loop:
everything this library adds around the UNet calls.  No speed is claimed; the file states what was measured.

    python tools/render_rate.py [--rounds 3] [--out profiles/r34_render_rate.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, N, STEPS, DS, THRES = 768, 512, 2, 50, 0.6, 0.95


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from sd_animation_optical_flow_amd import controlnet as CN
    from sd_animation_optical_flow_amd import ofgen, ops, render
    from sd_animation_optical_flow_amd import sampler as S
    from sd_animation_optical_flow_amd import unet as UN
    from sd_animation_optical_flow_amd.handoff import prepare_inpaint_inputs
    from sd_animation_optical_flow_amd.vae import VaeDecoder, VaeEncoder, random_vae_decoder_state_dict, random_vae_state_dict
    assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
    unet = UN.UNetModel(UN.random_unet_state_dict(0, UN.SD_V15_UNET), UN.SD_V15_UNET, prefix="")
    enc, dec = VaeEncoder(random_vae_state_dict(0)), VaeDecoder(random_vae_decoder_state_dict(0))
    nets = [CN.ControlNet(CN.random_controlnet_state_dict(s, CN.SD_V15_CONTROLNET), CN.SD_V15_CONTROLNET, prefix="") for s in (0, 1)]
    g = torch.Generator().manual_seed(34)
    ctx, uc = torch.randn((1, 77, 768), generator=g).cuda(), torch.randn((1, 77, 768), generator=g).cuda()
    stand_in = lambda f: ((f[..., 1] > 128).to(torch.uint8) * 255).contiguous()
    controls = render.driver_controls(nets[0], stand_in, nets[1], "warp_and_inpaint_crossattn")
    rd = render.SdRenderer(unet, enc, dec, (ctx, uc), controls, ddim_steps=STEPS, ds=DS)
    rng = np.random.default_rng(34)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    smooth = lambda s: np.stack([127 + 120 * np.sin(xx / (17 + c + s)) * np.cos(yy / (23 - c + s)) for c in range(3)], -1).astype(np.uint8)
    raw = torch.from_numpy(smooth(0)).cuda()
    ai = [torch.from_numpy(smooth(3 * (s + 1))).cuda() for s in range(N)]
    flow = torch.from_numpy(np.stack([np.stack([3 * np.sin(yy / (40 + 7 * s)) + s, 2 * np.cos(xx / (55 - 5 * s)) - s], -1) for s in range(N)]).astype(np.float32)).cuda()
    conf = np.stack([0.5 + 0.5 * np.sin(xx / (90 + 30 * s) + s) * np.cos(yy / (120 - 20 * s)) for s in range(N)])
    conf = torch.from_numpy(np.clip(conf + 0.46 + 0.01 * rng.random(conf.shape), 0, 1).astype(np.float32)).cuda()

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    mode = "warp_and_inpaint_crossattn"
    _, (_, kv_prev) = clock(lambda: rd.generate_ai_frame_with_ref(flow, conf, ai, raw, mode, thres=THRES))      # warm-up; its K/V is the reference
    whole, stages = [], {}

    def stage(name, fn):
        ms, out = clock(fn)
        stages.setdefault(name, []).append(ms)
        return out

    with torch.no_grad():
        for rnd in range(a.rounds):
            ms, (frame, _) = clock(lambda: rd.generate_ai_frame_with_ref(flow, conf, ai, raw, mode, thres=THRES, reference_kv=[kv_prev]))
            whole.append(ms)
            print(f"round {rnd}: whole frame {ms:.1f} ms", flush=True)
            # the same frame, stage by stage
            ret, mask2, _ = stage("compose_refs + expand_mask", lambda: ofgen.compose_warp_and_mask_device(flow, conf, ai, raw, THRES, expand=True))
            cnets = stage("control conditions (detectors)", lambda: rd.control_nets(raw))
            inp = stage("prepare_inpaint_inputs", lambda: prepare_inpaint_inputs(ret, raw, mask2, mask_blur=4, device=unet.device))
            gen = torch.Generator(device="cuda").manual_seed(1234)
            t_enc = int(min(DS, 0.999) * STEPS)
            lat = (1, 4, H // 8, W // 8)
            n_init, n_cond, n_x1 = (torch.randn(lat, generator=gen, device="cuda") for _ in range(3))
            n_step = torch.randn((t_enc,) + lat, generator=gen, device="cuda")
            init_latent, cond_latent = stage("VAE encode x2", lambda: (enc.get_first_stage_encoding(inp["image"], n_init),
                                                                       enc.get_first_stage_encoding(inp["conditioning_image"], n_cond)))
            c_concat = torch.cat([inp["conditioning_mask_latent"], cond_latent], dim=1)
            smp = S.GuidedDDIMSampler(unet)
            smp.make_schedule(STEPS, 0.0)
            x1 = smp.stochastic_encode(init_latent, t_enc, n_x1)
            p0, _, step0, _ = S.decode_plan(smp.schedule, t_enc)[0]
            # the nets see the first UNet call's latent: x1 after the opening blend (decode's own kernel, blend only)
            nh = lambda t: t.permute(0, 2, 3, 1).contiguous()
            sc = smp.schedule
            xb = ops.ddim_step(nh(x1), dict(sa=float(sc["sqrt_alphas_cumprod"][step0]), s1=float(sc["sqrt_one_minus_alphas_cumprod"][step0])),
                               init=nh(init_latent), nmask=nh(inp["latmask"]), blend_noise=nh(n_step[0]), blend_only=True).permute(0, 3, 1, 2).contiguous()
            stage("ControlNets, first call (2 nets + hints)", lambda: CN.apply_multi_controlnet(
                torch.cat([xb, xb]), torch.full((2,), float(step0), device="cuda"), torch.cat([uc, ctx]), p0, cnets))
            sched = CN.ControlSchedule(cnets)
            decoded, last_gs = stage(f"decode loop ({t_enc} UNet calls, residuals cached)", lambda: smp.decode(
                x1, ctx, t_enc, unconditional_context=uc, unconditional_guidance_scale=7.0, c_concat=c_concat, init_latent=init_latent,
                nmask=inp["latmask"], step_noise=n_step, control=sched, reference_kv=[kv_prev]))
            x = stage("final blend + VAE decode", lambda: torch.clip(dec.decode_first_stage(S.final_blend(init_latent, decoded, inp["latmask"])
                                                                                            if last_gs > 0 else decoded), -1, 1))
            by_hand = stage("decode_to_u8", lambda: ops.decode_to_u8(x.permute(0, 2, 3, 1).contiguous())[0])
            same = bool(torch.equal(by_hand, frame))
    fmt = lambda v: f"{sum(v) / len(v):9.1f} [{min(v):9.1f} .. {max(v):9.1f}] ms"
    mean = lambda v: sum(v) / len(v)
    total = sum(mean(v) for v in stages.values())
    loop = mean(next(v for k, v in stages.items() if k.startswith("decode loop")))
    kv_mb = sum(k.numel() + v.numel() for k, v in kv_prev) * 4 / 1e6
    lines = [f"render.SdRenderer, one {mode} frame at {W}x{H}: {N} reference frames, SD v1.5 UNet (in_channels 9) + SD v1 VAE + two SD v1.5 "
             f"ControlNets, seeded weights, {STEPS} DDIM steps at strength {DS} ({int(DS * STEPS)} UNet calls at batch 2), one K/V history as "
             f"reference_kv; host clock between device synchronisations, mean of {a.rounds} rounds [fastest .. slowest] after one warm-up frame",
             "", f"  whole frame (generate_ai_frame_with_ref)        {fmt(whole)}", "", "  the same stages one by one:"]
    lines += [f"    {k:48s} {fmt(v)}   {100.0 * mean(v) / total:5.1f} %" for k, v in stages.items()]
    lines += [f"    {'sum of the stages':48s} {total:9.1f} ms", "",
              f"  share of the frame that is not the decode loop: {100.0 * (total - loop) / total:.1f} % of the stage sum "
              f"({total - loop:.1f} of {total:.1f} ms); against the whole-frame time: {100.0 * (mean(whole) - loop) / mean(whole):.1f} %",
              f"  the stage-by-stage frame equals the renderer's: {same}",
              f"  K/V history of this frame: {kv_mb:.0f} MB at UNet batch 2 ({len(kv_prev)} transformer blocks, fp32)", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
