"""-m gpu: `sampler.img2img` (the seed-frame path and the latent-guided path) as wiring of stages that have their own tests, and
`decode(control=<callable>)` with `controlnet.ControlSchedule`: guidance windows inside the loop against a float64 loop that takes
the control of each step.  Configuration u0 at its golden sizes; every test prints its figures (-s)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sampler_check as SK   # noqa: E402
import transformer_check as TC   # noqa: E402
import unet_check as UC   # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "sampler_ref_u0.npz")
U4 = dict(UC.U0, in_channels=4)                                  # u0 without the hybrid conditioning: img2img has no c_concat
H, W, STEPS, STRENGTH, T_ENC = 64, 96, 10, 0.4, 4


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def u0(cuda):
    from sd_animation_optical_flow_amd import unet as UN
    sd = UN.random_unet_state_dict(0, UC.U0)
    return UN.UNetModel(sd, UC.U0, prefix=""), TC.to64(sd)


@pytest.fixture(scope="module")
def u4(cuda):
    from sd_animation_optical_flow_amd import unet as UN
    return UN.UNetModel(UN.random_unet_state_dict(0, U4), U4, prefix="")


@pytest.fixture(scope="module")
def vaes(cuda):
    from sd_animation_optical_flow_amd.vae import VaeDecoder, VaeEncoder, random_vae_decoder_state_dict, random_vae_state_dict
    return VaeEncoder(random_vae_state_dict(0)), VaeDecoder(random_vae_decoder_state_dict(0))


@pytest.fixture(scope="module")
def frames():
    g = torch.Generator().manual_seed(1234)
    image = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    target = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    r = lambda: torch.randn((1, 4, H // 8, W // 8), generator=g).cuda()
    return image, target, dict(init=r(), target=r(), x1=r())


def _to_image(bgr):
    """frame_rgb.astype(np.float32) / 127.5 - 1. on the device, [1,3,H,W]."""
    return bgr.cuda().flip(-1).permute(2, 0, 1)[None].float() / 127.5 - 1.0


def test_img2img_is_its_stages(u4, vaes, gold, frames):
    from sd_animation_optical_flow_amd import sampler as S
    enc, dec = vaes
    image, target, noise = frames
    ctx, uc = torch.from_numpy(gold["in.context"][:1]).cuda(), torch.from_numpy(gold["in.uncond"][:1]).cuda()
    assert int(min(STRENGTH, 0.999) * STEPS) == T_ENC
    kw = dict(denoising_strength=STRENGTH, ddim_steps=STEPS)
    gmap = (0.1 + 0.4 * torch.rand((1, 1, H // 8, W // 8), generator=torch.Generator().manual_seed(77))).cuda()
    init_latent = enc.get_first_stage_encoding(_to_image(image), noise["init"])
    target_latent = enc.get_first_stage_encoding(_to_image(target), noise["target"])
    outs = {}
    for name, tgt, func in (("seed", None, None), ("scalar", target, lambda p: 0.3), ("map", target, lambda p: gmap)):
        smp = S.GuidedDDIMSampler(u4)
        call = dict(kw, sampler=smp, noise={k: v for k, v in noise.items() if tgt is not None or k != "target"})
        if tgt is not None:
            call.update(target_bgr=tgt.numpy() if name == "map" else tgt, guidance_schedule_func=func)       # numpy and tensor frames
        got = S.img2img(u4, enc, dec, image, ctx, uc, **call)
        assert tuple(got.shape) == (1, 3, H, W) and bool(torch.isfinite(got).all()) and float(got.abs().max()) <= 1.0
        assert len(smp.last_kv_hists) == u4.n_transformers and smp.last_kv_hists[0][0].shape[0] == 2
        # the same stages composed by hand from the public pieces
        s2 = S.GuidedDDIMSampler(u4)
        s2.make_schedule(STEPS, 0.0)
        x1 = s2.stochastic_encode(init_latent, T_ENC, noise["x1"])
        dkw = dict(unconditional_context=uc, unconditional_guidance_scale=7.0)
        if tgt is not None:
            dkw.update(guidance=target_latent, guidance_schedule_func=func)
        decoded, _ = s2.decode(x1, ctx, T_ENC, **dkw)
        assert torch.equal(got, torch.clip(dec.decode_first_stage(decoded), -1, 1)), name
        outs[name] = got
    d = {n: float((outs[n] - outs["seed"]).abs().max()) for n in ("scalar", "map")}
    print(f"img2img: guided runs differ from the seed run by {d}, map from scalar by {float((outs['map'] - outs['scalar']).abs().max()):.3e}")
    assert d["scalar"] > 1e-3 and d["map"] > 1e-3 and not torch.equal(outs["map"], outs["scalar"])
    # a batch of one given as [1,H,W,3] is the same call
    assert torch.equal(S.img2img(u4, enc, dec, image[None], ctx, uc, noise={k: noise[k] for k in ("init", "x1")}, **kw), outs["seed"])


def test_img2img_draws_its_noise_from_the_generator(u4, vaes, gold, frames):
    from sd_animation_optical_flow_amd import sampler as S
    enc, dec = vaes
    image, target, _ = frames
    ctx, uc = torch.from_numpy(gold["in.context"][:1]).cuda(), torch.from_numpy(gold["in.uncond"][:1]).cuda()
    kw = dict(denoising_strength=STRENGTH, ddim_steps=STEPS, target_bgr=target)
    gen = lambda s: torch.Generator(device="cuda").manual_seed(s)
    runs = [S.img2img(u4, enc, dec, image, ctx, uc, generator=gen(s), **kw) for s in (3, 3, 4)]
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    # the order of the draws: init, target, x1, one torch.randn each
    g = gen(3)
    drawn = {k: torch.randn((1, 4, H // 8, W // 8), generator=g, device="cuda") for k in ("init", "target", "x1")}
    assert torch.equal(S.img2img(u4, enc, dec, image, ctx, uc, noise=drawn, **kw), runs[0])
    g = gen(3)
    part = {k: torch.randn((1, 4, H // 8, W // 8), generator=g, device="cuda") for k in ("init", "target")}
    assert torch.equal(S.img2img(u4, enc, dec, image, ctx, uc, noise=part, generator=g, **kw), runs[0])


def test_img2img_hands_control_to_decode(u4, vaes, gold, frames):
    from sd_animation_optical_flow_amd import controlnet as CN
    from sd_animation_optical_flow_amd import sampler as S
    enc, dec = vaes
    image, _, noise = frames
    ctx, uc = torch.from_numpy(gold["in.context"][:1]).cuda(), torch.from_numpy(gold["in.uncond"][:1]).cuda()
    ctl = [c.cuda() for c in UC.control_residuals(u4.layout, 2, H // 8, W // 8)]
    kw = dict(denoising_strength=STRENGTH, ddim_steps=STEPS, noise={k: noise[k] for k in ("init", "x1")})
    plain = S.img2img(u4, enc, dec, image, ctx, uc, **kw)
    fixed = S.img2img(u4, enc, dec, image, ctx, uc, control=ctl, **kw)
    cs = CN.ControlSchedule([CN.SingleControlNet(1.0, "canny", {}, None, result=ctl)])
    sched = S.img2img(u4, enc, dec, image, ctx, uc, control=cs, **kw)
    assert torch.equal(sched, fixed) and not torch.equal(fixed, plain) and cs.mixes == 1


def test_img2img_refusals(u0, u4, vaes, gold, frames):
    from sd_animation_optical_flow_amd import sampler as S
    enc, dec = vaes
    image, target, noise = frames
    ctx, uc = torch.from_numpy(gold["in.context"][:1]).cuda(), torch.from_numpy(gold["in.uncond"][:1]).cuda()
    with pytest.raises(ValueError):                                        # t_enc == 0
        S.img2img(u4, enc, dec, image, ctx, uc, denoising_strength=0.05, ddim_steps=10)
    with pytest.raises(ValueError):                                        # the hybrid UNet is img2img_inpaint's
        S.img2img(u0[0], enc, dec, image, ctx, uc, denoising_strength=STRENGTH, ddim_steps=STEPS)
    with pytest.raises(ValueError):
        S.img2img(u4, enc, dec, image, ctx, uc, denoising_strength=STRENGTH, ddim_steps=STEPS, noise=dict(step=noise["x1"]))
    with pytest.raises(RuntimeError):
        S.img2img(u4, enc, dec, image.float(), ctx, uc, denoising_strength=STRENGTH, ddim_steps=STEPS)
    with pytest.raises(RuntimeError):
        S.img2img(u4, enc, dec, image, ctx, uc, denoising_strength=STRENGTH, ddim_steps=STEPS, target_bgr=target[:32])
    with pytest.raises(NotImplementedError):                               # what decode refuses is still refused
        S.img2img(u4, enc, dec, image, ctx, uc, denoising_strength=STRENGTH, ddim_steps=STEPS, target_bgr=target, noise=noise,
                  guidance_schedule_func=lambda p: np.full((8, 12), 0.3, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# windowed control, with case f's inputs

def _loop64_windowed(sd64, layout, sched, case, inp, x1, plan, coef_of, control_of, reference_kv):
    """`sampler_check.loop64` for a case with CFG and the mask blend and without latent guidance or eta, the control of every UNet
    call given by control_of(i, p) (float64 NCHW residuals or None)."""
    assert case["cfg"] is not None and case["mask"] and not case["guide"] and case["eta"] == 0.0
    B = case["B"]
    sl = lambda name: inp[name][:B].double()
    x = x1[:B].double()
    ctx = torch.cat([sl("uncond"), sl("context")])
    cc = sl("c_concat")
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    for i, (p, index, step, gs) in enumerate(plan):
        if gs > 0:
            q = float(sched["sqrt_alphas_cumprod"][step]) * sl("init_latent") + \
                float(sched["sqrt_one_minus_alphas_cumprod"][step]) * inp["q_noise"][i, :B].double()
            x = (1.0 - sl("nmask")) * q + sl("nmask") * x
        xc = torch.cat([x, cc], dim=1)
        eps = UC.unet64(sd64, layout, torch.cat([xc] * 2), torch.full((2 * B,), float(step)), ctx, control=control_of(i, p),
                        reference_kv=reference_kv)[0]
        k = dict(coef_of(index))
        k["cfg"] = case["cfg"]
        xp, _, _ = SK.step64(k, nhwc(x), eps_c=nhwc(eps[B:]), eps_u=nhwc(eps[:B]))
        x = xp.permute(0, 3, 1, 2)
    return x


@pytest.fixture(scope="module")
def case_f(gold, u0):
    model, _ = u0
    case = SK.DECODE_CASES["f"]
    inp = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("in.")}
    control, _, frames = SK.decode_extras(model.layout)
    dev = lambda t: t[:1].cuda()
    kw = dict(unconditional_context=dev(inp["uncond"]), unconditional_guidance_scale=case["cfg"], c_concat=dev(inp["c_concat"]),
              init_latent=dev(inp["init_latent"]), nmask=dev(inp["nmask"]), step_noise=inp["q_noise"][:, :1].contiguous().cuda(),
              reference_kv=[[(k.cuda(), v.cuda()) for k, v in f] for f in frames], guidance_schedule_func=case["func"])
    return case, inp, dev(torch.from_numpy(gold["x1"])), dev(inp["context"]), kw, control


def test_a_callable_that_returns_the_list_is_the_list(u0, case_f):
    from sd_animation_optical_flow_amd.sampler import GuidedDDIMSampler
    model, _ = u0
    case, _, x1, ctx, kw, control = case_f
    ctl = [c.cuda() for c in control]
    s = GuidedDDIMSampler(model)
    s.make_schedule(case["steps"], case["eta"])
    fixed, _ = s.decode(x1, ctx, case["t_start"], control=ctl, **kw)
    calls = []

    def fn(i, p):
        calls.append((i, p))
        return ctl

    got, _ = s.decode(x1, ctx, case["t_start"], control=fn, **kw)
    assert torch.equal(got, fixed)
    assert calls == [(i, (i + 1) / 4) for i in range(4)]
    none, _ = s.decode(x1, ctx, case["t_start"], control=lambda i, p: None, **kw)
    plain, _ = s.decode(x1, ctx, case["t_start"], **kw)
    assert torch.equal(none, plain) and not torch.equal(plain, fixed)
    with pytest.raises(ValueError):                                        # what the callable returns is validated before it is used
        s.decode(x1, ctx, case["t_start"], control=lambda i, p: ctl[:-1], **kw)
    with pytest.raises(ValueError):
        s.decode(x1, ctx, case["t_start"], control=lambda i, p: ctl if i < 2 else [c[:1] for c in ctl], **kw)


def test_control_schedule_closes_a_window_inside_the_loop(gold, u0, case_f):
    from sd_animation_optical_flow_amd import controlnet as CN
    from sd_animation_optical_flow_amd.sampler import GuidedDDIMSampler, ddim_schedule, decode_plan, step_coefficients
    model, sd64 = u0
    case, inp, x1, ctx, kw, control = case_f
    second = UC.control_residuals(model.layout, 2, SK.LAT_H, SK.LAT_W, seed=777)
    W1, W2, END = 1.0, 0.75, 0.5                                  # p = 0.25, 0.5, 0.75, 1: the second window closes after step 1 of 4
    nets = lambda end: [CN.SingleControlNet(W1, "canny", {}, None, result=[c.cuda() for c in control]),
                        CN.SingleControlNet(W2, "hed", {}, None, guidance_end=end, result=[c.cuda() for c in second])]
    with pytest.raises(ValueError):
        CN.ControlSchedule([CN.SingleControlNet(1.0, "canny", {}, None)])          # no cached result
    with pytest.raises(ValueError):
        CN.ControlSchedule([])
    sched = ddim_schedule(case["steps"], case["eta"])
    plan = decode_plan(sched, case["t_start"], case["func"])
    assert [p for p, _, _, _ in plan] == [0.25, 0.5, 0.75, 1.0]
    _, _, last = SK.decode_extras(model.layout)
    ref_kv = [[(k.double(), v.double()) for k, v in f] for f in last]
    mix64 = lambda w2: [W1 * a.double() + w2 * b.double() for a, b in zip(control, second)]
    coef = lambda index: step_coefficients(sched, index)
    ref = _loop64_windowed(sd64, model.layout, sched, case, inp, torch.from_numpy(gold["x1"]), plan, coef,
                           lambda i, p: mix64(W2 if p <= END else 0.0), ref_kv)
    ref_open = _loop64_windowed(sd64, model.layout, sched, case, inp, torch.from_numpy(gold["x1"]), plan, coef, lambda i, p: mix64(W2), ref_kv)
    s = GuidedDDIMSampler(model)
    s.make_schedule(case["steps"], case["eta"])
    cs = CN.ControlSchedule(nets(END))
    got, _ = s.decode(x1, ctx, case["t_start"], control=cs, **kw)
    yard = dict(zip([str(k) for k in gold["dist_keys"]], gold["ref_vs_f64"]))["f"]
    bar = UC.bar4(yard)
    d = float((got.double().cpu() - ref).abs().max())
    d_open = float((got.double().cpu() - ref_open).abs().max())
    print(f"windowed control: device vs float64 {d:.3e}, bar {bar:.3e} (yardstick {yard:.3e}); from the loop whose window never closes "
          f"{d_open:.3e}; mixes {cs.mixes}")
    assert d <= bar
    assert d_open > 1e2 * bar                                     # a schedule that is ignored fails
    assert cs.mixes == 2                                          # one per distinct weight tuple: (1, 0.75) and (1, 0)
    # the schedule's values are apply_multi_controlnet's, bit for bit, and None once every window is shut
    both = CN.ControlSchedule(nets(END))
    for p, w2 in ((0.25, W2), (0.75, 0.0)):
        want = CN.apply_multi_controlnet(None, None, None, p, nets(END))
        assert all(torch.equal(a, b) for a, b in zip(both(0, p), want))
    shut = nets(END)
    shut[0].guidance_end = 0.6
    cs2 = CN.ControlSchedule(shut)
    assert cs2(0, 0.25) is cs2(1, 0.5) and cs2(2, 0.55) is not None and cs2.mixes == 2      # (1, 0.75), then (1, 0)
    assert cs2(3, 0.75) is None and cs2(3, 1.0) is None and cs2.mixes == 2                  # (0, 0): no mix
    # a never-closing schedule is the fixed mix
    open_cs = CN.ControlSchedule(nets(1.0))
    a, _ = s.decode(x1, ctx, case["t_start"], control=open_cs, **kw)
    b, _ = s.decode(x1, ctx, case["t_start"], control=CN.apply_multi_controlnet(None, None, None, 0.25, nets(1.0)), **kw)
    assert torch.equal(a, b) and open_cs.mixes == 1
