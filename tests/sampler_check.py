"""Float64 restatements of the guided DDIM step, the mask blend and the decode loop, the kernel's per-element bound and the case
tables of the sampler tests.  Not a conftest: imported by name, and importable without a device.

    GuidedDDIMSample.p_sample_ddim / decode      guided_ldm_inpainting.py:28-137
    latent guidance                              guided_ldm.py:82-89, :123
    q_sample                                     ldm/models/diffusion/ddpm.py:356-359
    DiffusionWrapper.forward ("hybrid")          ddpm.py:1404-1407
The loop runs over `unet_check.unet64`.  PINNED by tests/test_sampler_host.py against tests/golden/sampler_ref_u0.npz, the output of
the reference's own sampler class and UNet (tests/golden/make_golden_sampler.py).

The kernel's bound.  `ofx_ddim_step` evaluates, per element,
    e = eps_u + cfg (eps_c - eps_u);  pred = (x - s1m e) / sat;  [pred = pred (1 - g) + guidance g;  e = (x - sat pred) / s1m]
    xp = saprev pred + dir e [+ sigma n];  [xp = (1 - m) (sa init + s1 bn) + m xp]
At most 21 roundings lie between an input and the output (3 for CFG, 3 for pred, 4 + 3 for the guidance pair, 3 + 2 for xp, 3 for
q and 3 for the blend, less what a fused multiply-add saves).  Every intermediate t~ of such a chain obeys the running-error bound
|t~ - t| <= n u T, where T is the same expression with every operand replaced by its absolute value and every subtraction by an
addition, and n the number of roundings so far; so the result is within 21 u T(out).  K_STEP = 32 leaves room for a division
that is not correctly rounded (2.5 ulp) and for second-order terms.  u = 2^-24.  No constant is measured.
"""
import itertools
import os

import numpy as np
import torch

import unet_check as UC

U = 2.0 ** -24
K_STEP = 32.0
COEF_FIELDS = ("cfg", "sqrt_at", "sqrt_1m_at", "sqrt_aprev", "dir_coef", "sigma_t", "g", "sa", "s1")


def _chain(k, x, eps_c=None, eps_u=None, guidance=None, g=None, step_noise=None, init=None, nmask=None, blend_noise=None,
           blend_only=False, magnitude=False):
    """The chain in float64 -> (xp, pred or None, xp before the blend).  magnitude=True: every operand's absolute value, every
    subtraction an addition (the T of the header)."""
    d = (lambda t: None if t is None else t.double().abs()) if magnitude else (lambda t: None if t is None else t.double())
    c = {f: (abs(float(k.get(f, 0.0))) if magnitude else float(k.get(f, 0.0))) for f in COEF_FIELDS}
    sub = (lambda a, b: a + b) if magnitude else (lambda a, b: a - b)
    x, eps_c, eps_u, guidance, step_noise, init, nmask, blend_noise = map(d, (x, eps_c, eps_u, guidance, step_noise, init, nmask, blend_noise))
    xp, pred = x, None
    if not blend_only:
        e = eps_c if eps_u is None else eps_u + c["cfg"] * sub(eps_c, eps_u)
        pred = sub(x, c["sqrt_1m_at"] * e) / c["sqrt_at"]
        if guidance is not None:
            gg = c["g"] if g is None else d(g)[..., None]
            pred = pred * sub(1.0, gg) + guidance * gg
            e = sub(x, c["sqrt_at"] * pred) / c["sqrt_1m_at"]
        xp = c["sqrt_aprev"] * pred + c["dir_coef"] * e
        if step_noise is not None:
            xp = xp + c["sigma_t"] * step_noise
    plain = xp
    if nmask is not None:
        q = c["sa"] * init
        if blend_noise is not None:
            q = q + c["s1"] * blend_noise
        xp = sub(1.0, nmask) * q + nmask * xp
    return xp, pred, plain


def step64(k, x, **kw):
    """-> (xp, pred, xp before the blend) in float64."""
    return _chain(k, x, **kw)


def step_bound(k, x, **kw):
    """-> (bound of xp, bound of pred) per element (header)."""
    xp, pred, _ = _chain(k, x, magnitude=True, **kw)
    return K_STEP * U * xp, None if pred is None else K_STEP * U * pred


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel's cases: rows (B, h, w) x feature sets

KERNEL_SHAPES = [(1, 3, 5), (2, 8, 12), (3, 17, 23)]           # 15 rows: less than a wave; 192: the u0 size; 1173: several workgroups, no multiple of a block
KERNEL_COEF = dict(cfg=7.0, sqrt_at=0.7673452496528625, sqrt_1m_at=0.6412341594696045, sqrt_aprev=0.8672620058059692,
                   dir_coef=0.49785199761390686, sigma_t=0.21, g=0.3, sa=0.9317, s1=0.3633)


def kernel_features():
    """Every combination of: CFG off / on; guidance off / scalar / map; sigma term off / on; blend off / on / blend-only (s1 = 0);
    one / two outputs (the second set also writes pred_out).  Blend-only has no DDIM part, so its other switches are off."""
    out = []
    for cfg, guide, sigma, blend, two in itertools.product((False, True), ("off", "scalar", "map"), (False, True), ("off", "on"), (False, True)):
        out.append(dict(cfg=cfg, guide=guide, sigma=sigma, blend=blend, two=two))
    out += [dict(cfg=False, guide="off", sigma=False, blend="only", two=two) for two in (False, True)]
    return out


def feature_id(f):
    return f"{'cfg' if f['cfg'] else 'nocfg'}-g{f['guide']}-{'sig' if f['sigma'] else 'nosig'}-blend{f['blend']}-{'two' if f['two'] else 'one'}"


def kernel_inputs(shape, seed=0):
    """Seeded operands [B,h,w,4] (float32, CPU) for one shape; nmask holds 0, 1 and values in between, with whole rows of 0 and 1."""
    B, h, w = shape
    g = torch.Generator().manual_seed(7700 + seed + 131 * B + 17 * h + w)
    r = lambda s=1.0: torch.randn((B, h, w, 4), generator=g) * s
    t = dict(x=r(), eps_c=r(), eps_u=r(), guidance=r(0.8), step_noise=r(), init=r(), blend_noise=r())
    m = torch.rand((B, h, w, 4), generator=g)
    m[:, 0] = 0.0
    m[:, 1] = 1.0
    m[:, 2:, ::2] = torch.round(m[:, 2:, ::2])
    t["nmask"] = m
    t["gmap"] = torch.rand((B, h, w), generator=g)
    return t


def kernel_call(f, t):
    """(coef, keyword operands, blend_only) of feature set f over the operands t (any device)."""
    k = dict(KERNEL_COEF)
    kw = {}
    only = f["blend"] == "only"
    if not only:
        kw["eps_c"] = t["eps_c"]
        if f["cfg"]:
            kw["eps_u"] = t["eps_u"]
        if f["guide"] != "off":
            kw["guidance"] = t["guidance"]
        if f["sigma"]:
            kw["step_noise"] = t["step_noise"]
    if f["blend"] != "off":
        kw["init"], kw["nmask"] = t["init"], t["nmask"]
        if only:
            k["sa"], k["s1"] = 1.0, 0.0
        else:
            kw["blend_noise"] = t["blend_noise"]
    return k, kw, only


def kernel_reference(f, t):
    """-> (xp64, pred64 or None, plain64, bound_xp, bound_pred) for feature set f."""
    k, kw, only = kernel_call(f, t)
    g = t["gmap"] if f["guide"] == "map" else None
    xp, pred, plain = step64(k, t["x"], g=g, blend_only=only, **kw)
    bx, bp = step_bound(k, t["x"], g=g, blend_only=only, **kw)
    return xp, pred, plain, bx, bp


# ---------------------------------------------------------------------------------------------------------------------------------
# the decode loop in float64

LAT_H, LAT_W, CTX_M, CAT_C = UC.U0_H, UC.U0_W, UC.U0_M, 5


def _gate_last_two(p):
    return 0.1 if p <= 0.5 else 0.0


# name: B, DDIM steps, eta, t_start, CFG scale or None, mask blend, latent guidance, schedule function; extras: case a with the
# non-zero `control` residuals and the reference-frame K/V of `decode_extras` in every UNet call (UNet batch 2)
DECODE_CASES = {
    "a": dict(B=1, steps=10, eta=0.0, t_start=4, cfg=7.0, mask=True, guide=False, func=lambda p: 0.1),
    "b": dict(B=2, steps=10, eta=0.0, t_start=4, cfg=None, mask=False, guide=False, func=lambda p: 0.1),
    "c": dict(B=1, steps=10, eta=0.0, t_start=4, cfg=7.0, mask=True, guide=False, func=_gate_last_two),
    "d": dict(B=1, steps=10, eta=0.0, t_start=4, cfg=7.0, mask=False, guide=True, func=lambda p: 0.3),
    "e": dict(B=1, steps=10, eta=0.5, t_start=4, cfg=7.0, mask=True, guide=False, func=lambda p: 0.1),
    "f": dict(B=1, steps=10, eta=0.0, t_start=4, cfg=7.0, mask=True, guide=False, func=lambda p: 0.1, extras=True),
}
SCHEDULES = ((10, 0.0), (50, 0.0), (10, 0.5))
MAX_B, MAX_T = 2, 4


def decode_inputs():
    """The seeded inputs of every decode case at batch MAX_B (a case with B = 1 takes image 0): float32, CPU, NCHW."""
    g = torch.Generator().manual_seed(31337)
    B, h, w = MAX_B, LAT_H, LAT_W
    r = lambda *s: torch.randn(s, generator=g)
    t = dict(init_latent=r(B, 4, h, w), x1_noise=r(B, 4, h, w), context=r(B, CTX_M, UC.U0["context_dim"]),
             uncond=r(B, CTX_M, UC.U0["context_dim"]), guidance=0.8 * r(B, 4, h, w), q_noise=r(MAX_T, B, 4, h, w),
             ddim_noise=r(MAX_T, B, 4, h, w))
    m = torch.round(torch.rand((B, 1, h, w), generator=g))
    m[:, :, 0] = 0.0                                             # one all-zero and one all-one row of pixels
    m[:, :, 1] = 1.0
    t["nmask"] = m.expand(B, 4, h, w).contiguous()
    cc = r(B, CAT_C, h, w)
    cc[:, :1] = 1.0 - m                                          # channel 0 of c_concat is a mask, as in the reference
    t["c_concat"] = cc
    return t


def decode_extras(layout):
    """What case f hands to every UNet call, at the UNet's batch 2 (B = 1 with classifier-free guidance): the seeded non-zero
    `control` residuals of `unet_check.control_residuals` and one reference frame, the K/V history of tests/golden/unet_ref_u0.npz
    with its two images swapped (`unet_check.reference_frames`, "all").  -> (control NCHW, frames in the reference's [(b h), n, d]
    layout, the same frames as [b, n, heads * d]); float32, CPU."""
    heads = UC.transformer_heads(layout)
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_ref_u0.npz"))
    hist = [(torch.from_numpy(gold[f"k{i}"]), torch.from_numpy(gold[f"v{i}"])) for i in range(len(heads))]
    frames = UC.reference_frames(hist, heads, "all")
    last = [[(UC.TC.heads_last(k, h), UC.TC.heads_last(v, h)) for (k, v), h in zip(f, heads)] for f in frames]
    return UC.control_residuals(layout, 2, LAT_H, LAT_W), frames, last


def loop64(sd64, layout, sched, case, inp, x1, plan, coef_of):
    """`GuidedDDIMSample.decode` in float64 over `unet_check.unet64`.  sched: `sampler.ddim_schedule`'s tables (the fp32 values are
    the ones the reference uses; everything after them is float64); plan: [(p, index, step, gs)], gs a number or, with latent
    guidance, a map [B,h,w]; coef_of(index): the fp32 scalars of `p_sample_ddim` (`sampler.step_coefficients`).  A case with
    `extras` passes `decode_extras` to every UNet call.  -> x_dec float64 [B,4,h,w]."""
    B = case["B"]
    unet_kw = {}
    if case.get("extras"):
        control, _, last = decode_extras(layout)
        unet_kw = dict(control=control, reference_kv=[[(k.double(), v.double()) for k, v in f] for f in last])
    sl = lambda name: inp[name][:B].double()
    x = x1[:B].double()
    ctx = torch.cat([sl("uncond"), sl("context")]) if case["cfg"] is not None else sl("context")
    cc = sl("c_concat")
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    for i, (p, index, step, gs) in enumerate(plan):
        if case["mask"] and gs > 0:                              # guided_ldm_inpainting.py:127-129
            q = float(sched["sqrt_alphas_cumprod"][step]) * sl("init_latent") + \
                float(sched["sqrt_one_minus_alphas_cumprod"][step]) * inp["q_noise"][i, :B].double()
            x = (1.0 - sl("nmask")) * q + sl("nmask") * x
        xc = torch.cat([x, cc], dim=1)                           # ddpm.py:1405
        UB = 2 * B if case["cfg"] is not None else B
        ts = torch.full((UB,), float(step))
        eps = UC.unet64(sd64, layout, torch.cat([xc] * 2) if case["cfg"] is not None else xc, ts, ctx, **unet_kw)[0]
        k = dict(coef_of(index))
        kw = {}
        if case["cfg"] is not None:
            k["cfg"] = case["cfg"]
            kw["eps_u"] = nhwc(eps[:B])
        if case["guide"]:
            if torch.is_tensor(gs):
                kw["g"] = gs.reshape(B, LAT_H, LAT_W).cpu()
            else:
                k["g"] = float(gs)
            kw["guidance"] = nhwc(sl("guidance"))
        if case["eta"] != 0.0:
            kw["step_noise"] = nhwc(inp["ddim_noise"][i, :B])
        xp, _, _ = step64(k, nhwc(x), eps_c=nhwc(eps[B:] if case["cfg"] is not None else eps), **kw)
        x = xp.permute(0, 3, 1, 2)
    return x
