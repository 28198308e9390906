"""-m gpu: the radius-independent 4-channel Gaussian blur and the `fill_mask_input` chain against the numpy restatement
(tests/fill_check.py) and the Pillow vectors (tests/golden/fill_mask_pil.npz), bit for bit; `prepare_inpaint_inputs(fill_masked=True)`
and `img2img_inpaint(fill_masked=True)` as wiring of stages that have their own tests; the strip helpers of the `self_attn` and
`both` modes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fill_check as FC   # noqa: E402
import unet_check as UC   # noqa: E402

pytestmark = pytest.mark.gpu
OFX_EINVAL = -1

# (H, W, radius): 1x1; single columns and rows; box radius 255 past both sides; more pixels than threads (a chunk of 3 per thread,
# carries across the four waves); one pixel past a block (256 threads) and past 4 per thread; ragged sizes at small radii and a
# fractional one; the sampler's test frame; the copy; rows at 4096 and at the stated limit of the LDS layout (6144)
BLUR_CASES = [(1, 1, 256), (9, 1, 2), (1, 9, 2), (8, 8, 256), (40, 24, 256), (17, 300, 16), (1, 257, 64), (3, 1025, 64), (50, 70, 2),
              (50, 70, 4), (50, 70, 7.5), (64, 96, 64), (33, 47, 0), (2, 4096, 64), (1, 6144, 256)]


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def _rgba(seed, B, H, W):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 4), dtype=np.uint8)


@pytest.fixture(scope="module")
def gold():
    return np.load(FC.GOLDEN)


@pytest.mark.parametrize("H,W,radius", BLUR_CASES)
def test_rgba_blur_matches_restatement_and_the_plane_blur(cuda, H, W, radius):
    ops = _ops()
    a = _rgba(H * 7919 + W, 2, H, W)                                          # B = 2, different items
    a[1, ..., 3] = 255 - a[1, ..., 0]
    t = torch.from_numpy(a).cuda()
    out = ops.gaussian_blur_rgba_u8(t, radius)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, H, W, 4)
    got = out.cpu().numpy()
    for b in range(2):
        assert np.array_equal(got[b], FC.blur_rgba(a[b], radius)), b
    planes = ops.gaussian_blur_u8(t.permute(0, 3, 1, 2).reshape(8, H, W).contiguous(), radius)
    assert torch.equal(out, planes.reshape(2, 4, H, W).permute(0, 2, 3, 1))
    assert torch.equal(t, torch.from_numpy(a).cuda())                         # the input is left alone


def test_rgba_blur_reproduces_the_pillow_vector(cuda, gold):
    pasted = FC.paste(gold["a_image"], gold["a_mask"])
    out = _ops().gaussian_blur_rgba_u8(torch.from_numpy(pasted).cuda()[None], 256)
    assert np.array_equal(out[0].cpu().numpy(), gold["a_pil_blur256"])


def test_rgba_blur_keeps_a_constant_image(cuda):
    """255 everywhere at box radius 255: the accumulator (511 taps of 255, times ww) stays inside uint32 and the result is 255."""
    a = torch.full((1, 3, 700, 4), 255, dtype=torch.uint8, device="cuda")
    assert torch.equal(_ops().gaussian_blur_rgba_u8(a, 256), a)
    assert torch.equal(_ops().gaussian_blur_u8(a.permute(0, 3, 1, 2).reshape(4, 3, 700).contiguous(), 256), a.reshape(4, 3, 700))


def test_blur_refusals(cuda):
    from sd_animation_optical_flow_amd import _lib
    ops, L = _ops(), _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = torch.zeros((1, 4, 8, 4), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(a)
    assert L.ofx_gaussian_blur_rgba_u8(p(a), p(out), p(a), 1, 4, 8, 2.0, s) == OFX_EINVAL        # scratch aliases the input
    assert L.ofx_gaussian_blur_rgba_u8(p(a), p(out), p(out), 1, 4, 8, 2.0, s) == OFX_EINVAL      # ... the output
    long_row = torch.zeros((1, 1, 6145, 4), dtype=torch.uint8, device="cuda")                     # one past the LDS layout's limit
    with pytest.raises(_lib.OfxError) as e:
        ops.gaussian_blur_rgba_u8(long_row, 2.0)
    assert e.value.code == OFX_EINVAL
    with pytest.raises(_lib.OfxError):
        ops.gaussian_blur_rgba_u8(long_row.reshape(1, 6145, 1, 4), 2.0)
    with pytest.raises(RuntimeError):
        ops.gaussian_blur_rgba_u8(a[..., :3].contiguous(), 2.0)
    img = torch.zeros((1, 4, 8, 3), dtype=torch.uint8, device="cuda")
    m = torch.zeros((1, 4, 8), dtype=torch.uint8, device="cuda")
    n = L.ofx_fill_mask_input_scratch_bytes(1, 4, 8)
    assert n >= 4 * 4 * 8 * 4 and L.ofx_fill_mask_input_scratch_bytes(0, 4, 8) == 0
    assert L.ofx_fill_mask_input(p(img), p(m), p(out), p(img), 1, 4, 8, s) == OFX_EINVAL           # scratch aliases the frame
    assert L.ofx_fill_mask_input(p(img), p(m), p(out), p(out), 1, 4, 8, s) == OFX_EINVAL
    with pytest.raises(_lib.OfxError):
        ops.fill_mask_input(torch.zeros((1, 1, 6145, 3), dtype=torch.uint8, device="cuda"), torch.zeros((1, 1, 6145), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()


def test_fill_mask_input_reproduces_pillow(cuda, gold):
    from sd_animation_optical_flow_amd import handoff
    ops = _ops()
    for n in [str(x) for x in gold["names"]]:
        image, mask, want = gold[f"{n}_image"], gold[f"{n}_mask"], gold[f"{n}_pil_fill"]
        got = ops.fill_mask_input(torch.from_numpy(image).cuda()[None], torch.from_numpy(mask).cuda()[None])
        assert np.array_equal(got[0].cpu().numpy(), want), n
        assert np.array_equal(handoff.fill_mask_input(image, mask).cpu().numpy(), want), n       # numpy in, [H,W,3]
    # B = 2 with different items, against the restatement: a ragged frame, one item blobs, the other every mask value
    i0, m0 = FC.random_case(31, 37, 53, "blobs")
    i1, m1 = FC.random_case(32, 37, 53, "noise")
    got = ops.fill_mask_input(torch.from_numpy(np.stack([i0, i1])).cuda(), torch.from_numpy(np.stack([m0, m1])).cuda()).cpu().numpy()
    assert np.array_equal(got[0], FC.fill_mask_input(i0, m0)) and np.array_equal(got[1], FC.fill_mask_input(i1, m1))
    keep = m0 == 0
    assert keep.any() and np.array_equal(got[0][keep], i0[keep])


def test_prepare_inpaint_inputs_fill_masked(cuda, gold):
    from sd_animation_optical_flow_amd import handoff
    rng = np.random.default_rng(77)
    H, W = 64, 96
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = np.zeros((H, W), np.uint8)
    mask[8:40, 16:72] = 255
    out = handoff.prepare_inpaint_inputs(image, None, mask, mask_blur=4.0, fill_masked=True)
    image_mask = FC.HO.gaussian_blur_u8(mask, 4.0)
    assert np.array_equal(out["image_mask"][0].cpu().numpy(), image_mask)
    filled = FC.fill_mask_input(image, image_mask)
    assert not np.array_equal(filled, image)
    want = np.moveaxis(filled[..., ::-1].astype(np.float32) / 127.5 - 1.0, 2, 0)              # RGB planar, as the composite path
    assert np.array_equal(out["image"][0].cpu().numpy(), want)
    # the existing path fed the filled frame as both image and reference gives every tensor
    same = handoff.prepare_inpaint_inputs(filled, filled, mask, mask_blur=4.0)
    assert set(same) == set(out)
    for k in out:
        assert torch.equal(out[k], same[k]), k
    # the fixture's frame through the whole preparation: its mask is already blurred, so mask_blur 0
    g_img, g_mask = gold["c_image"], gold["c_mask"]
    o2 = handoff.prepare_inpaint_inputs(g_img, None, g_mask, mask_blur=0.0, fill_masked=True)
    rgb = ((o2["image"][0].permute(1, 2, 0) + 1.0) * 127.5).round().to(torch.uint8).flip(-1).cpu().numpy()
    assert np.array_equal(rgb, gold["c_pil_fill"])
    with pytest.raises(ValueError):
        handoff.prepare_inpaint_inputs(image, image, mask, fill_masked=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# img2img_inpaint(fill_masked=True), configuration u0 at 64 x 96 as tests/test_gpu_img2img.py

H, W, STEPS = 64, 96, 10
T_ENC = 9                                                                     # int(0.999 * 10): denoising_strength becomes 1


@pytest.fixture(scope="module")
def models(cuda):
    from sd_animation_optical_flow_amd import unet as UN
    from sd_animation_optical_flow_amd.vae import VaeDecoder, VaeEncoder, random_vae_decoder_state_dict, random_vae_state_dict
    sg = np.load(os.path.join(HERE, "golden", "sampler_ref_u0.npz"))
    ctx, uc = torch.from_numpy(sg["in.context"][:1]).cuda(), torch.from_numpy(sg["in.uncond"][:1]).cuda()
    g = torch.Generator().manual_seed(4321)
    image = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    mask = torch.zeros((H, W), dtype=torch.uint8)
    mask[8:40, 16:72] = 255
    return (UN.UNetModel(UN.random_unet_state_dict(0, UC.U0), UC.U0, prefix=""), VaeEncoder(random_vae_state_dict(0)),
            VaeDecoder(random_vae_decoder_state_dict(0)), ctx, uc, image, mask)


def test_img2img_inpaint_fill_masked_is_its_stages(models):
    from sd_animation_optical_flow_amd import sampler as S
    from sd_animation_optical_flow_amd.handoff import prepare_inpaint_inputs
    model, enc, dec, ctx, uc, image, mask = models
    g = torch.Generator().manual_seed(99)
    r = lambda *s: torch.randn(s, generator=g).cuda()
    noise = dict(init=r(1, 4, 8, 12), fill=r(1, 4, 8, 12), cond=r(1, 4, 8, 12), x1=r(1, 4, 8, 12), step=r(T_ENC, 1, 4, 8, 12))
    kw = dict(denoising_strength=0.05, ddim_steps=STEPS, mask_blur=4, unconditional_guidance_scale=7.0, fill_masked=True)
    smp = S.GuidedDDIMSampler(model)
    x_samples, img, init_dec = S.img2img_inpaint(model, enc, dec, image, None, mask, ctx, uc, noise=noise, sampler=smp, **kw)
    assert tuple(x_samples.shape) == (1, 3, H, W) and bool(torch.isfinite(x_samples).all()) and float(x_samples.abs().max()) <= 1.0
    # the same stages composed by hand
    inp = prepare_inpaint_inputs(image, None, mask, mask_blur=4, fill_masked=True)
    latmask = inp["latmask"]
    assert bool((latmask == 0).any()) and bool((latmask == 1).any())
    encoded = enc.get_first_stage_encoding(inp["image"], noise["init"])
    init_latent = S.final_blend(encoded, noise["fill"], latmask)             # (1 - nmask) * init_latent + nmask * noise
    one, zero = latmask == 1, latmask == 0
    assert torch.equal(init_latent[one], noise["fill"][one]) and torch.equal(init_latent[zero], encoded[zero])
    c_concat = torch.cat([inp["conditioning_mask_latent"], enc.get_first_stage_encoding(inp["conditioning_image"], noise["cond"])], dim=1)
    s2 = S.GuidedDDIMSampler(model)
    s2.make_schedule(STEPS, 0.0)
    x1 = s2.stochastic_encode(init_latent, T_ENC, noise["x1"])
    decoded, last_gs = s2.decode(x1, ctx, T_ENC, unconditional_context=uc, unconditional_guidance_scale=7.0, c_concat=c_concat,
                                 init_latent=init_latent, nmask=latmask, step_noise=noise["step"])
    assert last_gs == 0.1
    blended = S.final_blend(init_latent, decoded, latmask)                    # the final blend uses the noised init_latent
    assert torch.equal(x_samples, torch.clip(dec.decode_first_stage(blended), -1, 1))
    assert torch.equal(img, inp["image"])
    assert torch.equal(init_dec, dec.decode_first_stage(init_latent).clip(-1, 1))
    # step noise of the strength the caller passed (t_enc would be 0) is refused: the path runs int(0.999 * steps) steps
    with pytest.raises(RuntimeError):
        S.img2img_inpaint(model, enc, dec, image, None, mask, ctx, uc, noise=dict(noise, step=noise["step"][:4].contiguous()), **kw)


def test_img2img_inpaint_fill_masked_draws_in_the_reference_order(models):
    from sd_animation_optical_flow_amd import sampler as S
    model, enc, dec, ctx, uc, image, mask = models
    kw = dict(ddim_steps=STEPS, mask_blur=4, fill_masked=True)
    gen = lambda s: torch.Generator(device="cuda").manual_seed(s)
    runs = [S.img2img_inpaint(model, enc, dec, image, None, mask, ctx, uc, generator=gen(s), **kw)[0] for s in (3, 3, 4)]
    assert torch.equal(runs[0], runs[1]) and not torch.equal(runs[0], runs[2])
    g = gen(3)
    drawn = {k: torch.randn((1, 4, 8, 12), generator=g, device="cuda") for k in ("init", "fill", "cond", "x1")}
    drawn["step"] = torch.randn((T_ENC, 1, 4, 8, 12), generator=g, device="cuda")
    assert torch.equal(S.img2img_inpaint(model, enc, dec, image, None, mask, ctx, uc, noise=drawn, **kw)[0], runs[0])
    g = gen(3)
    part = {k: torch.randn((1, 4, 8, 12), generator=g, device="cuda") for k in ("init", "fill")}
    assert torch.equal(S.img2img_inpaint(model, enc, dec, image, None, mask, ctx, uc, noise=part, generator=g, **kw)[0], runs[0])


def test_strip_helpers_match_numpy(cuda):
    from sd_animation_optical_flow_amd import ofgen
    rng = np.random.default_rng(8)
    h, w, n = 10, 14, 3
    fr = lambda: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    raw, ret, original, ai = fr(), fr(), fr(), [fr() for _ in range(n)]
    mask2 = rng.integers(0, 256, (h, w), dtype=np.uint8)
    # ofgen_keyframe_inpaint.py:823-831
    want_frames = np.zeros((h, w * (n + 1), 3), np.uint8)
    want_frames[:, :w] = raw
    for i in range(n):
        want_frames[:, (i + 1) * w:(i + 2) * w] = ai[i]
    want_mask = np.zeros((h, w * (n + 1)), np.uint8)
    want_mask[:, :w] = 255
    frames, mask = ofgen.strip_inputs_self_attn(raw, [torch.from_numpy(ai[0]).cuda()] + ai[1:])       # tensors and arrays
    assert frames.is_cuda and mask.is_cuda and frames.dtype == mask.dtype == torch.uint8
    assert np.array_equal(frames.cpu().numpy(), want_frames) and np.array_equal(mask.cpu().numpy(), want_mask)
    # :929-937
    a, b, m = ofgen.strip_inputs_both(ret, original, mask2, ai)
    wa, wb = want_frames.copy(), want_frames.copy()
    wa[:, :w], wb[:, :w] = ret, original
    wm = np.zeros_like(want_mask)
    wm[:, :w] = mask2
    assert np.array_equal(a.cpu().numpy(), wa) and np.array_equal(b.cpu().numpy(), wb) and np.array_equal(m.cpu().numpy(), wm)
    f1, m1 = ofgen.strip_inputs_self_attn(raw, [])                            # no reference frame: the frame alone
    assert np.array_equal(f1.cpu().numpy(), raw) and bool((m1 == 255).all())
    with pytest.raises(RuntimeError):
        ofgen.strip_inputs_self_attn(raw, [ai[0][:5]])
    with pytest.raises(RuntimeError):
        ofgen.strip_inputs_both(ret, original, mask2[:5], ai)
