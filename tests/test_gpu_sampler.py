"""The guided DDIM sampler on the device: `ofx_ddim_step` against float64 with the running-error bound of tests/sampler_check.py
(every element), its refusals, `GuidedDDIMSampler.decode` on configuration u0 against the float64 restatement with the bar of four
times the reference's own distance (tests/golden/sampler_ref_u0.npz), `forward_nhwc(padded=True)`, and the wiring of
`img2img_inpaint`.  Every test prints its figures (-s)."""
import ctypes as C
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
EINVAL, EALIGN = -1, -2
SENTINELS = (float("nan"), -3.5, float("inf"), 1e30, -0.0, 7.25, float("nan"), 2.0)


@pytest.fixture(scope="module")
def ops(cuda):
    from sd_animation_optical_flow_amd import ops as O
    return O


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def u0(cuda):
    from sd_animation_optical_flow_amd import unet as UN
    sd = UN.random_unet_state_dict(0, UC.U0)
    return UN.UNetModel(sd, UC.U0, prefix=""), TC.to64(sd)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel

def _wide_out(lead):
    """A 12-wide buffer of sentinels (NaN among them) and its channels 0..3."""
    w = torch.empty(lead + (12,), device="cuda")
    w[..., 4:] = torch.tensor(SENTINELS, device="cuda")
    w[..., :4] = 123.0
    return w, w[..., :4]


def _check(what, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    assert bool(torch.isfinite(got).all()), what
    ratio = float((err / bound).max())
    return ratio


@pytest.mark.parametrize("shape", SK.KERNEL_SHAPES, ids=[f"rows{b * h * w}" for b, h, w in SK.KERNEL_SHAPES])
@pytest.mark.parametrize("wide", [False, True], ids=["dense", "cols0-3of12"])
def test_ddim_step_against_float64(ops, shape, wide):
    t = SK.kernel_inputs(shape)
    d = {k: v.cuda() for k, v in t.items()}
    lead = tuple(shape)
    worst = 0.0
    for f in SK.kernel_features():
        k, kw, only = SK.kernel_call(f, d)
        if f["guide"] == "map":
            kw["gmap"] = d["gmap"]
        xp64, pred64, plain64, bx, bp = SK.kernel_reference(f, t)
        bufs = []
        outs = {}
        for name in ("out0",) + (("out1", "pred_out") if f["two"] and not only else ("out1",) if f["two"] else ()):
            if wide:
                w, v = _wide_out(lead)
                bufs.append(w)
            else:
                v = torch.full(lead + (4,), 123.0, device="cuda")
            outs[name] = v
        ret = ops.ddim_step(d["x"], k, blend_only=only, **kw, **outs)
        assert ret.data_ptr() == outs["out0"].data_ptr()
        fid = SK.feature_id(f)
        r = _check(fid, outs["out0"], xp64, bx)
        worst = max(worst, r)
        assert r <= 1.0, (fid, r)
        if "out1" in outs:
            assert torch.equal(outs["out1"], outs["out0"]), fid
        if "pred_out" in outs:
            rp = _check(fid + " pred", outs["pred_out"], pred64, bp)
            worst = max(worst, rp)
            assert rp <= 1.0, (fid, rp)
        for w in bufs:                                             # the other columns come back bitwise unchanged
            want = torch.tensor(SENTINELS, device="cuda").expand(lead + (8,))
            assert torch.equal(w[..., 4:].contiguous().view(torch.int32), want.contiguous().view(torch.int32)), fid
        if f["blend"] != "off":
            got = outs["out0"].cpu()
            m = t["nmask"]
            zero, one = m == 0, m == 1
            assert bool(zero.any()) and bool(one.any())
            if only:
                assert torch.equal(got[zero], t["init"][zero]), fid           # init exactly
                assert torch.equal(got[one], t["x"][one]), fid
            else:
                q64 = k["sa"] * t["init"].double() + k["s1"] * t["blend_noise"].double()
                assert bool(((got.double() - q64).abs()[zero] <= bx[zero]).all()), fid
                # where nmask == 1: the bits of the same call without the blend
                plain = ops.ddim_step(d["x"], k, **{a: b for a, b in kw.items() if a not in ("init", "nmask", "blend_noise")})
                assert torch.equal(got[one], plain.cpu()[one]), fid
    print(f"rows {shape[0] * shape[1] * shape[2]} {'12-wide' if wide else 'dense'}: worst |error| / bound {worst:.3f} over "
          f"{len(SK.kernel_features())} feature sets")


def test_ddim_step_in_place_on_the_unet_input_buffer(ops):
    """out0 is x itself (channels 0..3 of half 0 of a [2B,h,w,12] buffer), out1 the same channels of half 1; columns 4..11 hold
    c_concat and the pad and must not change."""
    B, h, w = 2, 8, 12
    t = SK.kernel_inputs((B, h, w))
    f = dict(cfg=True, guide="scalar", sigma=True, blend="on", two=True)
    xp64, _, _, bx, _ = SK.kernel_reference(f, t)
    buf = torch.randn((2 * B, h, w, 12), device="cuda")
    buf[..., 9:] = 0.0
    buf[:B, ..., :4] = t["x"].cuda()
    before = buf.clone()
    d = {k: v.cuda() for k, v in t.items()}
    k, kw, _ = SK.kernel_call(f, d)
    x0v, x1v = buf[:B, ..., :4], buf[B:, ..., :4]
    ops.ddim_step(x0v, k, out0=x0v, out1=x1v, **kw)
    assert _check("in place", x0v, xp64, bx) <= 1.0
    assert torch.equal(x0v, x1v)
    assert torch.equal(buf[..., 4:], before[..., 4:])


def test_ddim_step_rejects_before_any_launch(ops):
    from sd_animation_optical_flow_amd import _lib
    L = _lib.lib()
    rows, Cn = 24, 4
    POISON = 7.25
    x = torch.randn((rows, 12), device="cuda")
    eps = torch.randn((2 * rows, Cn), device="cuda")
    init, nmask, noise = (torch.rand((rows, Cn), device="cuda") for _ in range(3))
    out = torch.full((2 * rows + 1, 12), POISON, device="cuda")
    x_before = x.clone()
    coef = _lib.DdimCoef(cfg=7.0, sqrt_at=0.8, sqrt_1m_at=0.6, sqrt_aprev=0.9, dir_coef=0.4, sigma_t=0.0, g=0.0, sa=0.9, s1=0.4)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    NULL = C.c_void_p(0)

    def call(xp=None, ldx=12, ec="eps", eu="eps", lde=Cn, o0=None, ldo0=12, o1=None, ldo1=12, c=Cn, mode=0, n=rows, bn="noise", k=coef):
        return L.ofx_ddim_step(p(x) if xp is None else xp, ldx, p(eps, 4 * rows * Cn) if ec == "eps" else ec, p(eps) if eu == "eps" else eu, lde,
                               NULL, 0, NULL, NULL, 0, p(init), Cn, p(nmask), Cn, p(noise) if bn == "noise" else bn, Cn,
                               p(out) if o0 is None else o0, ldo0, NULL if o1 is None else o1, ldo1, NULL, 0,
                               C.byref(k) if k is not None else None, mode, n, c, None)

    cases = [
        ("x not 16-byte aligned", call(xp=p(x, 4)), EALIGN),
        ("out0 not 16-byte aligned", call(o0=p(out, 8)), EALIGN),
        ("ldx % 4", call(ldx=14), EALIGN),
        ("ldo0 % 4", call(ldo0=6), EALIGN),
        ("ld < C", call(c=8, lde=8, ldo0=4), EINVAL),
        ("lde < C", call(c=8), EINVAL),
        ("C % 4", call(c=2), EALIGN),
        ("eps_c NULL", call(ec=NULL), EINVAL),
        ("x NULL", call(xp=NULL), EINVAL),
        ("coef NULL", call(k=None), EINVAL),
        ("rows <= 0", call(n=0), EINVAL),
        ("unknown mode", call(mode=2), EINVAL),
        ("blend-only with eps", call(mode=1), EINVAL),
        ("s1 != 0 without blend noise", call(bn=NULL), EINVAL),
        ("out0 overlaps eps", call(o0=p(eps), ldo0=Cn), EINVAL),
        ("out0 overlaps init", call(o0=p(init), ldo0=Cn), EINVAL),
        ("out0 == out1", call(o1=p(out)), EINVAL),
        ("out1 overlaps out0 partially", call(o1=p(out, 4 * 12 * 3)), EINVAL),
        ("out0 overlaps x partially", call(o0=p(x, 16)), EINVAL),
        ("out0 == x with another row stride", call(o0=p(x), ldo0=8), EINVAL),
    ]
    torch.cuda.synchronize()
    for what, got, want in cases:
        assert got == want, (what, got, want)
    assert bool((out == POISON).all()) and torch.equal(x, x_before)               # nothing was launched
    # the valid call on the same buffers runs: out0 and out1 the two halves of `out`
    assert call(o1=p(out, 4 * 12 * rows)) == 0
    torch.cuda.synchronize()
    got = out[:rows, :4]
    assert torch.equal(got, out[rows:2 * rows, :4]) and bool((out[:, 4:] == POISON).all()) and bool((out[2 * rows] == POISON).all())
    k = {f: getattr(coef, f) for f in SK.COEF_FIELDS}
    ref, _, _ = SK.step64(k, x[:, :4].cpu(), eps_c=eps[rows:].cpu(), eps_u=eps[:rows].cpu(), init=init.cpu(), nmask=nmask.cpu(), blend_noise=noise.cpu())
    bound, _ = SK.step_bound(k, x[:, :4].cpu(), eps_c=eps[rows:].cpu(), eps_u=eps[:rows].cpu(), init=init.cpu(), nmask=nmask.cpu(),
                             blend_noise=noise.cpu())
    assert bool(((got.cpu().double() - ref).abs() <= bound).all())
    # and x itself is a legal out0
    assert call(o0=p(x), o1=p(out, 4 * 12 * rows)) == 0
    torch.cuda.synchronize()
    assert torch.equal(x[:, :4], got) and torch.equal(x[:, 4:], x_before[:, 4:])


# ---------------------------------------------------------------------------------------------------------------------------------
# forward_nhwc(padded=True)

def test_forward_nhwc_padded_is_the_default_call_bit_for_bit(u0):
    model, _ = u0
    x, t, ctx = (v.cuda() for v in UC.u0_inputs())
    xh = x.permute(0, 2, 3, 1).contiguous()
    want, kv_want = model.forward_nhwc(xh, t, ctx)
    xp = torch.zeros((xh.shape[0], xh.shape[1], xh.shape[2], model.in_pad), device="cuda")
    xp[..., :model.in_channels] = xh
    before = xp.clone()
    got, kv = model.forward_nhwc(xp, t, ctx, padded=True)
    assert torch.equal(got, want) and torch.equal(xp, before)
    for (k0, v0), (k1, v1) in zip(kv_want, kv):
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
    with pytest.raises(RuntimeError):
        model.forward_nhwc(xh, t, ctx, padded=True)                       # 9 channels where in_pad = 12 are expected
    with pytest.raises(RuntimeError):
        model.forward_nhwc(torch.zeros((2, 8, 12, 24), device="cuda")[..., :12], t, ctx, padded=True)     # not contiguous


# ---------------------------------------------------------------------------------------------------------------------------------
# decode

@pytest.fixture(scope="module")
def decode_refs(gold, u0):
    """The float64 restatement of every case, computed once."""
    from sd_animation_optical_flow_amd.sampler import ddim_schedule, decode_plan, step_coefficients
    model, sd64 = u0
    inp = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("in.")}
    x1 = torch.from_numpy(gold["x1"])
    refs = {}
    for name, case in SK.DECODE_CASES.items():
        sched = ddim_schedule(case["steps"], case["eta"])
        plan = decode_plan(sched, case["t_start"], case["func"])
        refs[name] = SK.loop64(sd64, model.layout, sched, case, inp, x1, plan, lambda index, s=sched: step_coefficients(s, index))
    return inp, x1, refs


def test_stochastic_encode_is_the_reference(gold, u0):
    from sd_animation_optical_flow_amd.sampler import GuidedDDIMSampler
    s = GuidedDDIMSampler(u0[0])
    s.make_schedule(10)
    got = s.stochastic_encode(torch.from_numpy(gold["in.init_latent"]).cuda(), SK.MAX_T, torch.from_numpy(gold["in.x1_noise"]).cuda())
    d = float((got.cpu() - torch.from_numpy(gold["x1"])).abs().max())
    print(f"stochastic_encode vs the reference's: {d:.3e}")
    assert d <= 2.0 ** -23 * float(np.abs(gold["x1"]).max())              # two products and a sum; a fused multiply-add may differ by an ulp


@pytest.mark.parametrize("name", sorted(SK.DECODE_CASES))
def test_decode_against_float64(gold, u0, decode_refs, name):
    from sd_animation_optical_flow_amd.sampler import GuidedDDIMSampler
    model, _ = u0
    inp, x1, refs = decode_refs
    case = SK.DECODE_CASES[name]
    B = case["B"]
    dev = lambda t: t[:B].cuda()
    sampler = GuidedDDIMSampler(model)
    sampler.make_schedule(case["steps"], case["eta"])
    kw = dict(c_concat=dev(inp["c_concat"]), guidance_schedule_func=case["func"])
    if case["cfg"] is not None:
        kw.update(unconditional_context=dev(inp["uncond"]), unconditional_guidance_scale=case["cfg"])
    if case["mask"]:
        kw.update(init_latent=dev(inp["init_latent"]), nmask=dev(inp["nmask"]))
    if case["guide"]:
        kw["guidance"] = dev(inp["guidance"])
    qn, dn = inp["q_noise"][:, :B].contiguous().cuda(), inp["ddim_noise"][:, :B].contiguous().cuda()
    if case["eta"] != 0.0:
        kw["step_noise"] = (qn if case["mask"] else None, dn)
    elif case["mask"]:
        kw["step_noise"] = qn
    seen = []
    kw["callback"] = seen.append
    UB = 2 * B if case["cfg"] is not None else B
    extras, extras_before = {}, []
    if case.get("extras"):                                                 # non-zero control and a reference frame at the UNet's batch
        control, _, frames = SK.decode_extras(model.layout)
        extras = dict(control=[c.cuda() for c in control], reference_kv=[[(k.cuda(), v.cuda()) for k, v in f] for f in frames])
        assert all(c.shape[0] == UB for c in extras["control"]) and all(k.shape[0] == UB for f in extras["reference_kv"] for k, _ in f)
        extras_before = [t.clone() for t in extras["control"]] + [t.clone() for f in extras["reference_kv"] for kv in f for t in kv]
    x_in = dev(x1)
    held = {k: v.clone() for k, v in kw.items() if torch.is_tensor(v)}
    x_before = x_in.clone()
    got, last_gs = sampler.decode(x_in, dev(inp["context"]), case["t_start"], **extras, **kw)
    assert seen == list(range(case["t_start"]))
    assert float(last_gs) == float(gold[f"{name}.last_gs"])
    assert torch.equal(x_in, x_before) and all(torch.equal(kw[k], v) for k, v in held.items())           # the caller's tensors are not written to
    if extras:                                                             # every control and K/V tensor: the bits of before the call
        after = list(extras["control"]) + [t for f in extras["reference_kv"] for kv in f for t in kv]
        assert len(after) == len(extras_before) == len(extras["control"]) + 2 * model.n_transformers
        assert all(torch.equal(a, b) for a, b in zip(after, extras_before))
    yard = dict(zip([str(k) for k in gold["dist_keys"]], gold["ref_vs_f64"]))[name]
    d = float((got.double().cpu() - refs[name]).abs().max())
    d_ref = float((got.cpu() - torch.from_numpy(gold[f"{name}.out"])).abs().max())
    print(f"case {name}: device vs float64 {d:.3e}, bar {UC.bar4(yard):.3e} (yardstick {yard:.3e}); vs the reference's fp32 {d_ref:.3e}")
    assert tuple(got.shape) == (B, 4, SK.LAT_H, SK.LAT_W) and got.is_contiguous()
    assert d <= UC.bar4(yard)
    if extras:                                                             # f is a with the two: they reached the UNet, and changed the result
        d_plain = float((got.double().cpu() - refs["a"]).abs().max())
        print(f"case {name}: distance from the float64 loop WITHOUT control / reference_kv {d_plain:.3e}")
        assert d_plain > 1e2 * UC.bar4(yard)
    assert len(sampler.last_kv_hists) == model.n_transformers and sampler.last_kv_hists[0][0].shape[0] == UB


def test_decode_with_a_strength_map_against_float64(gold, u0, decode_refs):
    """Case d with a per-pixel strength: `guidance_schedule_func` returns a device map [B,1,h,w] already at latent size, against the
    float64 loop with the same map.  The bar is case d's: the same loop at the same shapes with the same operations, the scalar g
    replaced by one value per pixel out of [0.1, 0.5) around d's 0.3 (the reference's own map branch needs cv2 and cannot run on the
    host that makes the golden file)."""
    from sd_animation_optical_flow_amd.sampler import GuidedDDIMSampler, ddim_schedule, decode_plan, step_coefficients
    model, sd64 = u0
    inp, x1, refs = decode_refs
    case = SK.DECODE_CASES["d"]
    gmap = 0.1 + 0.4 * torch.rand((1, 1, SK.LAT_H, SK.LAT_W), generator=torch.Generator().manual_seed(77))
    gdev = gmap.cuda()
    sched = ddim_schedule(case["steps"], case["eta"])
    plan = decode_plan(sched, case["t_start"], lambda p: gmap)
    ref = SK.loop64(sd64, model.layout, sched, case, inp, x1, plan, lambda index: step_coefficients(sched, index))
    dev = lambda t: t[:1].cuda()
    s = GuidedDDIMSampler(model)
    s.make_schedule(case["steps"], case["eta"])
    kw = dict(unconditional_context=dev(inp["uncond"]), unconditional_guidance_scale=case["cfg"], c_concat=dev(inp["c_concat"]),
              guidance=dev(inp["guidance"]))
    got, last_gs = s.decode(dev(x1), dev(inp["context"]), case["t_start"], guidance_schedule_func=lambda p: gdev, **kw)
    assert last_gs is gdev and torch.equal(gdev.cpu(), gmap)
    yard = dict(zip([str(k) for k in gold["dist_keys"]], gold["ref_vs_f64"]))["d"]
    d = float((got.double().cpu() - ref).abs().max())
    d_scalar = float((got.double().cpu() - refs["d"]).abs().max())
    print(f"strength map: device vs float64 {d:.3e}, bar {UC.bar4(yard):.3e}; from the scalar-strength loop {d_scalar:.3e}")
    assert d <= UC.bar4(yard) and d_scalar > 1e2 * UC.bar4(yard)
    flat, _ = s.decode(dev(x1), dev(inp["context"]), case["t_start"], guidance_schedule_func=lambda p: gdev[:, 0], **kw)     # [B,h,w]
    assert torch.equal(flat, got)
    with pytest.raises(RuntimeError):
        s.decode(dev(x1), dev(inp["context"]), case["t_start"], guidance_schedule_func=lambda p: gdev[..., :4], **kw)
    with pytest.raises(ValueError):                                        # a map gates no blend
        s.decode(dev(x1), dev(inp["context"]), case["t_start"], guidance_schedule_func=lambda p: gdev, init_latent=dev(inp["init_latent"]),
                 nmask=dev(inp["nmask"]), **kw)


def test_decode_draws_all_noise_up_front_from_the_generator(u0, decode_refs):
    from sd_animation_optical_flow_amd.sampler import GuidedDDIMSampler
    model, _ = u0
    inp, x1, _ = decode_refs
    dev = lambda t: t[:1].cuda()
    s = GuidedDDIMSampler(model)
    s.make_schedule(10, 0.5)
    kw = dict(unconditional_context=dev(inp["uncond"]), unconditional_guidance_scale=7.0, c_concat=dev(inp["c_concat"]),
              init_latent=dev(inp["init_latent"]), nmask=dev(inp["nmask"]))
    g = torch.Generator(device="cuda").manual_seed(5)
    a, _ = s.decode(dev(x1), dev(inp["context"]), 3, generator=g, **kw)
    drawn = torch.randn((2, 3, 1, 4, SK.LAT_H, SK.LAT_W), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    b, _ = s.decode(dev(x1), dev(inp["context"]), 3, step_noise=(drawn[0], drawn[1]), **kw)
    assert torch.equal(a, b)
    # temperature is folded into sigma_t: 0.5 sigma_t n and sigma_t (0.5 n) are the same fp32 product, a halving being exact
    half, _ = s.decode(dev(x1), dev(inp["context"]), 3, step_noise=(drawn[0], drawn[1]), temperature=0.5, **kw)
    c, _ = s.decode(dev(x1), dev(inp["context"]), 3, step_noise=(drawn[0], 0.5 * drawn[1]), **kw)
    assert torch.equal(half, c) and not torch.equal(half, b)
    with pytest.raises(ValueError):
        s.decode(dev(x1), dev(inp["context"]), 3, step_noise=drawn[0], **kw)         # eta > 0 needs the 2-tuple
    with pytest.raises(ValueError):
        s.decode(dev(x1), dev(inp["context"]), 3, **{**kw, "c_concat": None})
    with pytest.raises(ValueError):
        s.decode(dev(x1), dev(inp["context"]), 3, control=[torch.zeros(1, device="cuda")], **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# img2img_inpaint

@pytest.fixture(scope="module")
def vaes(cuda):
    from sd_animation_optical_flow_amd.vae import VaeDecoder, VaeEncoder, random_vae_decoder_state_dict, random_vae_state_dict
    return VaeEncoder(random_vae_state_dict(0)), VaeDecoder(random_vae_decoder_state_dict(0))


def test_img2img_inpaint_wiring(u0, vaes, gold):
    from sd_animation_optical_flow_amd import sampler as S
    from sd_animation_optical_flow_amd.handoff import prepare_inpaint_inputs
    model, _ = u0
    enc, dec = vaes
    H, W, steps, strength = 64, 96, 10, 0.4
    g = torch.Generator().manual_seed(99)
    image = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    reference = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    mask = torch.zeros((H, W), dtype=torch.uint8)
    mask[8:40, 16:72] = 255
    ctx, uc = torch.from_numpy(gold["in.context"][:1]).cuda(), torch.from_numpy(gold["in.uncond"][:1]).cuda()
    t_enc = int(min(strength, 0.999) * steps)
    assert t_enc == 4
    r = lambda *s: torch.randn(s, generator=g).cuda()
    noise = dict(init=r(1, 4, 8, 12), cond=r(1, 4, 8, 12), x1=r(1, 4, 8, 12), step=r(t_enc, 1, 4, 8, 12))
    smp = S.GuidedDDIMSampler(model)
    kw = dict(denoising_strength=strength, ddim_steps=steps, mask_blur=4, unconditional_guidance_scale=7.0)
    x_samples, img, init_dec = S.img2img_inpaint(model, enc, dec, image, reference, mask, ctx, uc, noise=noise, sampler=smp, **kw)
    assert tuple(x_samples.shape) == (1, 3, H, W) and bool(torch.isfinite(x_samples).all()) and float(x_samples.abs().max()) <= 1.0
    assert len(smp.last_kv_hists) == model.n_transformers
    # the same stages composed by hand from the public pieces
    inp = prepare_inpaint_inputs(image, reference, mask, mask_blur=4)
    latmask = inp["latmask"]
    assert bool((latmask == 0).any()) and bool((latmask == 1).any())
    init_latent = enc.get_first_stage_encoding(inp["image"], noise["init"])
    c_concat = torch.cat([inp["conditioning_mask_latent"], enc.get_first_stage_encoding(inp["conditioning_image"], noise["cond"])], dim=1)
    s2 = S.GuidedDDIMSampler(model)
    s2.make_schedule(steps, 0.0)
    x1 = s2.stochastic_encode(init_latent, t_enc, noise["x1"])
    decoded, last_gs = s2.decode(x1, ctx, t_enc, unconditional_context=uc, unconditional_guidance_scale=7.0, c_concat=c_concat,
                                 init_latent=init_latent, nmask=latmask, step_noise=noise["step"])
    assert last_gs == 0.1
    blended = S.final_blend(init_latent, decoded, latmask)
    zero, one = latmask == 0, latmask == 1
    assert torch.equal(blended[zero], init_latent[zero])                        # unmasked latent pixels are init_latent exactly
    assert torch.equal(blended[one], decoded[one]) and not torch.equal(blended[one], init_latent[one])
    # in between, guided_ldm_inpainting.py:338 in float64 to the kernel's bound (its products may be fused where torch rounds each)
    c64 = lambda t: t.double().cpu()
    ref = c64(init_latent) * (1 - c64(latmask)) + c64(decoded) * c64(latmask)
    bound, _ = SK.step_bound(dict(sa=1.0, s1=0.0), decoded.cpu(), init=init_latent.cpu(), nmask=latmask.cpu(), blend_only=True)
    assert bool(((c64(blended) - ref).abs() <= bound).all())
    assert torch.equal(x_samples, torch.clip(dec.decode_first_stage(blended), -1, 1))
    assert torch.equal(img, inp["image"])
    assert torch.equal(init_dec, dec.decode_first_stage(init_latent).clip(-1, 1))
    # noise from a generator: two calls with one seed agree bit for bit, and differ from another seed
    runs = [S.img2img_inpaint(model, enc, dec, image, reference, mask, ctx, uc, generator=torch.Generator(device="cuda").manual_seed(sd), **kw)[0]
            for sd in (3, 3, 4)]
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
