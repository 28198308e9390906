"""-m gpu: `decode(control_nets=)` and `render.SdRenderer` as wiring of stages that have their own tests: every result is
`torch.equal` to the same stages composed by hand from the public pieces.  Configurations u0 (the 9-channel inpainting UNet), u0
with in_channels=4 (the seed UNet) and c0 (two ControlNets), frames of 64x64 (strips of 64x128 and 64x192), 10 steps, seeded
weights, explicit contexts."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import controlnet_check as CK   # noqa: E402
import unet_check as UC   # noqa: E402

pytestmark = pytest.mark.gpu
U4 = dict(UC.U0, in_channels=4)
H, W, STEPS, N = 64, 64, 10, 2
THRES = 0.5


@pytest.fixture(scope="module")
def M(cuda):
    """Models, contexts and one scene, built once."""
    from types import SimpleNamespace

    from sd_animation_optical_flow_amd import controlnet as CN
    from sd_animation_optical_flow_amd import render
    from sd_animation_optical_flow_amd import unet as UN
    from sd_animation_optical_flow_amd.vae import VaeDecoder, VaeEncoder, random_vae_decoder_state_dict, random_vae_state_dict
    sg = np.load(os.path.join(HERE, "golden", "sampler_ref_u0.npz"))
    m = SimpleNamespace()
    m.ctx, m.uc = torch.from_numpy(sg["in.context"][:1]).cuda(), torch.from_numpy(sg["in.uncond"][:1]).cuda()
    m.u0 = UN.UNetModel(UN.random_unet_state_dict(0, UC.U0), UC.U0, prefix="")
    m.u4 = UN.UNetModel(UN.random_unet_state_dict(0, U4), U4, prefix="")
    m.enc, m.dec = VaeEncoder(random_vae_state_dict(0)), VaeDecoder(random_vae_decoder_state_dict(0))
    m.nets = [CN.ControlNet(CN.random_controlnet_state_dict(seed, CK.C0), CK.C0, prefix="") for seed in (0, 1)]
    m.green = lambda frame: ((frame[..., 1] > 128).to(torch.uint8) * 255).contiguous()       # the caller's "hed" detector
    m.controls = render.driver_controls(m.nets[0], m.green, m.nets[1], "warp_and_inpaint")
    m.prompted = []

    def conditioning(frame):
        m.prompted.append(frame)
        return m.ctx, m.uc

    m.renderer = render.SdRenderer(m.u0, m.enc, m.dec, conditioning, m.controls, unet_seed=m.u4, ddim_steps=STEPS)
    rng = np.random.default_rng(2024)
    m.flow = torch.from_numpy((rng.standard_normal((N, H, W, 2)) * 2).astype(np.float32)).cuda()
    conf = rng.random((N, H, W)).astype(np.float32)
    conf[1, 10:40, 8:56] = 0.99
    m.conf = torch.from_numpy(conf).cuda()
    m.ai = [torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda() for _ in range(N)]
    # the raw frame: smooth with one sharp rectangle, so that expand_mask's Laplacian edges and cv2.Canny mark its border only
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    raw = np.stack([100 + 60 * np.sin(xx / (9 + c)) * np.cos(yy / (11 - c)) for c in range(3)], -1)
    raw[20:44, 12:30] += 90
    m.raw = torch.from_numpy(raw.astype(np.uint8)).cuda()
    return m


def _nets(m, frame, canny_end=0.9):
    """The driver's `cnets` by hand."""
    from sd_animation_optical_flow_amd import controlnet as CN
    return [CN.SingleControlNet(weight=0.7, model="hed", args={}, condition=m.green(frame), guidance_start=0.0, guidance_end=1.0, net=m.nets[0]),
            CN.SingleControlNet(weight=0.3, model="canny", args={"low_threshold": 100, "high_threshold": 200},
                                condition=CN.canny_condition(frame, 100, 200), guidance_start=0.0, guidance_end=canny_end, net=m.nets[1])]


def _inpaint_by_hand(m, image, reference, mask, condition_frame, reference_kv=(), canny_end=0.9, ds=0.6):
    from sd_animation_optical_flow_amd import ops
    from sd_animation_optical_flow_amd import sampler as S
    smp = S.GuidedDDIMSampler(m.u0)
    x, _, third = S.img2img_inpaint(m.u0, m.enc, m.dec, image, reference, mask, m.ctx, m.uc, denoising_strength=ds, ddim_steps=STEPS, mask_blur=4,
                                    unconditional_guidance_scale=7.0, generator=torch.Generator(device="cuda").manual_seed(1234),
                                    control_nets=_nets(m, condition_frame, canny_end), reference_kv=reference_kv, sampler=smp,
                                    fill_masked=reference is None, want_init_decoded=False)
    assert third is None
    return ops.decode_to_u8(x.permute(0, 2, 3, 1).contiguous())[0], smp.last_kv_hists


def _same_kv(a, b):
    return len(a) == len(b) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------------------
# the sampler's control_nets=

def test_decode_control_nets_is_the_first_call_plus_the_schedule(M):
    from sd_animation_optical_flow_amd import controlnet as CN
    from sd_animation_optical_flow_amd import sampler as S
    g = torch.Generator().manual_seed(5)
    x1 = torch.randn((1, 4, 8, 8), generator=g).cuda()
    t_start = 6
    smp = S.GuidedDDIMSampler(M.u4)
    smp.make_schedule(STEPS, 0.0)
    kw = dict(unconditional_context=M.uc, unconditional_guidance_scale=7.0)
    nets = _nets(M, M.raw, canny_end=0.5)                                # the canny window closes inside the loop
    nets[0].result = "stale"                                             # decode resets every net
    got, _ = smp.decode(x1, M.ctx, t_start, control_nets=nets, **kw)
    kv_got = smp.last_kv_hists
    # by hand: the first UNet call's inputs
    plan = S.decode_plan(smp.schedule, t_start)
    hand = _nets(M, M.raw, canny_end=0.5)
    CN.apply_multi_controlnet(torch.cat([x1, x1]), torch.full((2,), float(plan[0][2]), device="cuda"), torch.cat([M.uc, M.ctx]), plan[0][0], hand)
    assert all(torch.equal(a, b) for c, d in zip(nets, hand) for a, b in zip(c.result, d.result))
    sched = CN.ControlSchedule(hand)
    want, _ = smp.decode(x1, M.ctx, t_start, control=sched, **kw)
    assert torch.equal(got, want) and _same_kv(kv_got, smp.last_kv_hists)
    assert sched.mixes == 2                                              # both nets, then hed alone
    plain, _ = smp.decode(x1, M.ctx, t_start, **kw)
    assert not torch.equal(got, plain)
    # control_nets=None is the call without the argument, bit for bit
    none, _ = smp.decode(x1, M.ctx, t_start, control_nets=None, **kw)
    assert torch.equal(none, plain)
    with pytest.raises(ValueError, match="mutually exclusive"):
        smp.decode(x1, M.ctx, t_start, control=sched, control_nets=nets, **kw)
    # a condition of the wrong size is refused before anything runs: no net has been reset
    bad = _nets(M, M.raw)
    bad[0].result, bad[1].condition = "kept", bad[1].condition[:32].contiguous()
    with pytest.raises(ValueError, match="condition must be uint8"):
        smp.decode(x1, M.ctx, t_start, control_nets=bad, **kw)
    assert bad[0].result == "kept"


def test_decode_control_nets_on_the_hybrid_unet_after_the_opening_blend(M):
    """With nmask the nets see the latent AFTER the opening blend, (1 - nmask) * q_sample(init_latent) + nmask * x1, not x1."""
    from sd_animation_optical_flow_amd import controlnet as CN
    from sd_animation_optical_flow_amd import ops
    from sd_animation_optical_flow_amd import sampler as S
    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(s, generator=g).cuda()
    x1, init, cc, noise = r(1, 4, 8, 8), r(1, 4, 8, 8), r(1, 5, 8, 8), r(6, 1, 4, 8, 8)
    nmask = torch.rand((1, 1, 8, 8), generator=g).cuda().round().expand(1, 4, 8, 8).contiguous()
    nmask[:, :, 0, :4] = 0.25
    smp = S.GuidedDDIMSampler(M.u0)
    sched = smp.make_schedule(STEPS, 0.0)
    nets = _nets(M, M.raw)
    kw = dict(unconditional_context=M.uc, unconditional_guidance_scale=7.0, c_concat=cc, init_latent=init, nmask=nmask, step_noise=noise)
    got, _ = smp.decode(x1, M.ctx, 6, control_nets=nets, **kw)
    p0, _, step, _ = S.decode_plan(sched, 6)[0]
    nh = lambda t: t.permute(0, 2, 3, 1).contiguous()
    blended = ops.ddim_step(nh(x1), dict(sa=float(sched["sqrt_alphas_cumprod"][step]), s1=float(sched["sqrt_one_minus_alphas_cumprod"][step])),
                            init=nh(init), nmask=nh(nmask), blend_noise=nh(noise[0]), blend_only=True).permute(0, 3, 1, 2).contiguous()
    assert not torch.equal(blended, x1)
    hand = _nets(M, M.raw)
    ts, ctx2 = torch.full((2,), float(step), device="cuda"), torch.cat([M.uc, M.ctx])
    CN.apply_multi_controlnet(torch.cat([blended, blended]), ts, ctx2, p0, hand)
    assert all(torch.equal(a, b) for c, d in zip(nets, hand) for a, b in zip(c.result, d.result))
    from_x1 = _nets(M, M.raw)
    CN.apply_multi_controlnet(torch.cat([x1, x1]), ts, ctx2, p0, from_x1)
    assert not torch.equal(from_x1[0].result[0], hand[0].result[0])
    want, _ = smp.decode(x1, M.ctx, 6, control=CN.ControlSchedule(hand), **kw)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# run_inpainting, the four modes, the seed frames

def test_run_inpainting_is_its_stages(M):
    from sd_animation_optical_flow_amd import ops
    mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    mask[8:40, 16:56] = 255
    M.prompted.clear()
    frame, kv = M.renderer.run_inpainting(M.ai[0], M.raw, mask, condition_frame=M.raw)
    assert frame.is_cuda and frame.dtype == torch.uint8 and tuple(frame.shape) == (H, W, 3)
    assert len(M.prompted) == 1 and torch.equal(M.prompted[0], M.raw)                       # the prompt is the reference frame's
    want, want_kv = _inpaint_by_hand(M, M.ai[0], M.raw, mask, M.raw)
    assert torch.equal(frame, want) and _same_kv(kv, want_kv) and len(kv) == M.u0.n_transformers
    again, _ = M.renderer.run_inpainting(M.ai[0].cpu().numpy(), M.raw.cpu().numpy(), mask.cpu().numpy(), condition_frame=M.raw.cpu().numpy())
    assert torch.equal(again, frame)                                                        # seeded per call; arrays are uploaded
    # without a reference: fill_masked, the prompt frame named
    M.prompted.clear()
    filled, _ = M.renderer.run_inpainting(M.ai[0], None, mask, condition_frame=M.ai[1], prompt_frame=M.raw)
    assert torch.equal(M.prompted[0], M.raw)
    assert torch.equal(filled, _inpaint_by_hand(M, M.ai[0], None, mask, M.ai[1])[0]) and not torch.equal(filled, frame)
    del ops


@pytest.mark.parametrize("mode", ["warp_and_inpaint", "warp_and_inpaint_crossattn"])
def test_warp_modes_are_their_stages(M, mode):
    from sd_animation_optical_flow_amd import ops
    frames = torch.stack(M.ai)
    ret, mask, select, order, _ = ops.compose_refs(M.flow, M.conf, frames, THRES, "cv2_cubic")
    assert len(torch.unique(select)) == 2                                                   # both references are sampled
    if mode == "warp_and_inpaint":
        mask2 = ops.dilate((255 - mask)[None], 7)[0]
    else:
        mask2 = ops.expand_mask((255 - mask)[None], M.raw[None], 20, 7)[0]
    assert 0 < int((mask2 == 255).sum()) < H * W
    got, kv = M.renderer.generate_ai_frame_with_ref(M.flow, M.conf, M.ai, M.raw, mode, thres=THRES)
    want, want_kv = _inpaint_by_hand(M, ret, M.raw, mask2, M.raw)
    assert torch.equal(got, want) and _same_kv(kv, want_kv)
    # a kv_hist handed back as reference_kv: used by the crossattn mode only
    got2, _ = M.renderer.generate_ai_frame_with_ref(M.flow, M.conf, M.ai, M.raw, mode, thres=THRES, reference_kv=[kv])
    if mode == "warp_and_inpaint":
        assert torch.equal(got2, got)
    else:
        assert not torch.equal(got2, got)
        assert torch.equal(got2, _inpaint_by_hand(M, ret, M.raw, mask2, M.raw, reference_kv=[want_kv])[0])


def test_self_attn_mode_is_its_stages(M):
    from sd_animation_optical_flow_amd import ofgen
    M.prompted.clear()
    got, kv = M.renderer.generate_ai_frame_with_ref(M.flow, M.conf, M.ai, M.raw, "self_attn")
    assert tuple(got.shape) == (H, W, 3) and got.is_contiguous()
    assert torch.equal(M.prompted[0], M.raw)                                                # tagger_frame = all_frames[:, :w]
    all_frames, mask = ofgen.strip_inputs_self_attn(M.raw, M.ai)
    assert tuple(all_frames.shape) == (H, W * (N + 1), 3)
    want, want_kv = _inpaint_by_hand(M, all_frames, None, mask, all_frames, canny_end=1.0)    # the canny window ends at 1 here
    assert tuple(want.shape) == (H, W * (N + 1), 3)
    assert torch.equal(got, want[:, :W]) and _same_kv(kv, want_kv)
    assert not torch.equal(got, _inpaint_by_hand(M, all_frames, None, mask, all_frames, canny_end=0.9)[0][:, :W])


def test_both_mode_is_its_stages_and_samples_the_first_draw_only(M):
    from sd_animation_optical_flow_amd import ofgen, ops
    frames = torch.stack(M.ai)
    ret, mask, select, order, _ = ops.compose_refs(M.flow, M.conf, frames, THRES, "cv2_cubic", first_only=True)
    first = int(order[0])
    assert bool((select == first).all())
    assert torch.equal(ret, ops.warp(M.ai[first], M.flow[first][None], mode="cv2_cubic", sign=1.0)[0])   # the first warp, whole
    _, full_mask, full_select, _, _ = ops.compose_refs(M.flow, M.conf, frames, THRES, "cv2_cubic")
    assert torch.equal(mask, full_mask) and len(torch.unique(full_select)) == 2             # the mask still covers every reference
    flipped = M.ai[0].flip(0).contiguous()
    for prev, pos in ((None, None), (flipped, None), (flipped, 0)):        # the previous frame behind the references, or where its index puts it
        M.prompted.clear()
        got, kv = M.renderer.generate_ai_frame_with_ref(M.flow, M.conf, M.ai, M.raw, "both", thres=THRES, prev_ai_frame=prev, prev_position=pos)
        refs = list(M.ai)
        if prev is not None:
            refs.insert(len(refs) if pos is None else pos, prev)
        a, b, m = ofgen.strip_inputs_both(ret, M.raw, 255 - mask, refs)                     # no dilation in this mode
        assert tuple(a.shape) == (H, W * (len(refs) + 1), 3)
        want, want_kv = _inpaint_by_hand(M, a, None, m, b)                                  # the ControlNets see the raw-frame strip
        assert tuple(got.shape) == (H, W, 3) and torch.equal(got, want[:, :W]) and _same_kv(kv, want_kv)
        assert torch.equal(M.prompted[0], M.raw)


def test_generate_seed_frames_is_one_img2img_on_the_wide_image(M):
    from sd_animation_optical_flow_amd import ops
    from sd_animation_optical_flow_amd import sampler as S
    M.prompted.clear()
    frames, kv = M.renderer.generate_seed_frames([M.raw, M.ai[0].cpu().numpy()], ds=0.8)
    assert len(frames) == 2 and all(tuple(f.shape) == (H, W, 3) and f.is_contiguous() for f in frames)
    assert len(M.prompted) == 1 and torch.equal(M.prompted[0], M.raw)                       # the first frame's prompt
    wide = torch.cat([M.raw, M.ai[0]], dim=1)
    smp = S.GuidedDDIMSampler(M.u4)
    x = S.img2img(M.u4, M.enc, M.dec, wide, M.ctx, M.uc, denoising_strength=0.8, ddim_steps=STEPS,
                  generator=torch.Generator(device="cuda").manual_seed(1234), control_nets=_nets(M, wide), sampler=smp)
    want = ops.decode_to_u8(x.permute(0, 2, 3, 1).contiguous())[0]
    assert torch.equal(torch.cat(frames, dim=1), want) and _same_kv(kv, smp.last_kv_hists)
    key = M.renderer.render_key(M.raw)                                                      # ClipPipeline's hook: one seed frame
    assert tuple(key.shape) == (H, W, 3) and torch.equal(key, M.renderer.generate_seed_frames([M.raw])[0][0])


def test_renderer_is_clip_pipelines_render_hook(M):
    from sd_animation_optical_flow_amd.pipeline import FramePacket
    mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    mask[:20] = 255
    pkt = FramePacket(index=1, key_index=0, flow=M.flow[0], confidence=M.conf[0], warped=M.ai[0], mask=mask)
    assert torch.equal(M.renderer(pkt, M.raw), M.renderer.run_inpainting(M.ai[0], M.raw, mask, condition_frame=M.raw)[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# run_exp over a six-frame workspace

def test_run_exp_renders_every_frame_and_keeps_no_dropped_kv(M, raft_sd, tmp_path):
    from sd_animation_optical_flow_amd import ofgen, pdcnet_of, render
    from sd_animation_optical_flow_amd.workspace import VideoData
    g = torch.Generator().manual_seed(31)
    base = torch.nn.functional.avg_pool2d(torch.rand((1, 3, 96, 96), generator=g), 5, 1, 2)
    base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)
    clip = [base[0, :, 8 + i:8 + i + H, 12 - i:12 - i + W].permute(1, 2, 0).contiguous().numpy() for i in range(6)]
    video = VideoData(clip, (W, H), str(tmp_path))
    assert video.num_frames == 6
    pdc = ofgen.PDCNetAux(pdcnet_of.create_of_algo(raft_sd), str(tmp_path), batch_size=4)
    kv_map = render.run_exp(video, pdc, M.renderer, num_ref_for_generation=1, ds=0.6, persist_kv=True)
    assert all(video.generated(i) for i in range(6))
    key = [int(f.split(".")[0]) for f in os.listdir(tmp_path / "d01")]
    assert len(key) == 1
    seeds = sorted({0, key[0]})
    plan = render.generation_plan([list(range(6)), seeds], 1)
    assert sorted(seeds + [p[1] for p in plan]) == list(range(6))
    dropped = {p[4] for p in plan if p[4] is not None}
    assert dropped and sorted(kv_map) == sorted(set(range(6)) - dropped)
    assert sorted(int(f.split(".")[0]) for f in os.listdir(tmp_path / "crossattn")) == sorted(kv_map)     # put_kv / remove_kv followed
    assert os.listdir(tmp_path / "pdcnet") == []                                            # purged, as the reference does
    # the first frame of the plan again, by hand, from what the run left behind: its references are seed frames
    _, idx, refs, kv_refs, drop = plan[0]
    assert drop is None and kv_refs == refs and set(refs) <= set(seeds)
    flow, conf = pdc.multiple_to_one_device(video, refs, idx)
    ai = [torch.from_numpy(video.get_ai_frame(r)).cuda() for r in refs]
    want, _ = M.renderer.generate_ai_frame_with_ref(flow, conf, ai, video.get_raw_frame(idx), "warp_and_inpaint_crossattn",
                                                   reference_kv=[video.get_kv(r) for r in kv_refs], ds=0.6)
    assert np.array_equal(want.cpu().numpy(), video.get_ai_frame(idx))
