"""The reference's guided DDIM sampler on the device: from (warped frame, mask) to a repainted frame without leaving the library.

    GuidedDDIMSample.p_sample_ddim / decode      guided_ldm_inpainting.py:28-137   (mask blend, guidance only gates it)
    GuidedDDIMSample.p_sample_ddim / decode      guided_ldm.py:30-158              (latent guidance of pred_x0)
    GuidedLDM.img2img_inpaint                    guided_ldm_inpainting.py:262-345
    GuidedLDM.img2img                            guided_ldm_inpainting.py:185-259 (mask None), guided_ldm.py:166-219 (latent guidance)
    DDIMSampler.make_schedule, stochastic_encode ldm/models/diffusion/ddim.py:23-52, :301-314
    DDPM.register_schedule, q_sample             ldm/models/diffusion/ddpm.py:138-160, :356-359
    DiffusionWrapper.forward ("hybrid")          ddpm.py:1404-1407
    make_beta_schedule, make_ddim_timesteps, make_ddim_sampling_parameters      ldm/modules/diffusionmodules/util.py:21-74

The loop's time is the UNet's (`unet.UNetModel.forward_nhwc`).  Around it the reference runs, per step, torch.cat x2, chunk, the
classifier-free-guidance combination, pred_x0, dir_xt, x_prev, then q_sample and the mask blend of the next iteration, torch.cat
with c_concat and torch.cat x2 again.  Here all of that is ONE launch, `ops.ddim_step`: `decode` keeps one NHWC buffer
[2B or B, h, w, unet.in_pad] -- the UNet's own padded input, c_concat and the zero pad written once -- and the kernel reads eps
where `forward_nhwc(padded=True)` left it and writes the next latent into channels 0..3 of both halves.  A step is "UNet, one
kernel": no allocation of the sampler's own, no layout change.  NCHW appears at the public edge only.

Since a step's kernel also performs the blend that OPENS the next iteration, the order of operations is the reference's and only
the grouping into launches differs; the blend before the first step and img2img_inpaint's final blend are the same kernel with the
DDIM part switched off.

Needs no device to import; `ddim_schedule` is pure host code.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .controlnet import ControlSchedule, SingleControlNet, apply_multi_controlnet, check_control_nets
from .handoff import prepare_inpaint_inputs
from .modelbase import is_f32_cuda

_NOT_BUILT = ("use_original_steps", "score_corrector", "quantize_denoised", "noise_dropout", "dynamic_threshold")


def ddim_schedule(ddim_steps: int, eta: float = 0.0, *, timesteps: int = 1000, linear_start: float = 0.00085, linear_end: float = 0.0120,
                  beta_schedule: str = "linear", ddim_discretize: str = "uniform") -> Dict[str, object]:
    """The tables `DDPM.register_schedule` + `DDIMSampler.make_schedule` leave behind, with the dtype and the bits of each (the
    defaults are guided_ldm_inpaint_v15.yaml's).  The reference mixes number formats here, and so does this:
        ddim_timesteps                       int64 numpy: range(0, timesteps, timesteps // ddim_steps) + 1 ("uniform")
        ddim_alphas                          float32 tensor: the float32 `alphas_cumprod` (a float64 cumprod, rounded) at those steps
        ddim_alphas_prev                     float64 NUMPY array of float32 values: alphas_cumprod[0], then ddim_alphas[:-1]
        ddim_sigmas                          float64 tensor: eta * sqrt((1 - a_prev) / (1 - a) * (1 - a / a_prev)), where 1 - a and its
                                             reciprocal are float32 (a tensor on the right of a numpy array: torch's reflected
                                             division) and the rest float64
        ddim_sqrt_one_minus_alphas           float32 tensor: sqrt(1 - a) in float32
        sqrt_alphas_cumprod,                 float32 tensors [timesteps]: the DDPM's own buffers, the float64 square roots rounded,
        sqrt_one_minus_alphas_cumprod        which `q_sample` reads (not the sampler's float32 square roots of the same name)
    Only the "linear" beta schedule and the "uniform" discretisation are built (NotImplementedError)."""
    if beta_schedule != "linear":
        raise NotImplementedError(f"beta_schedule={beta_schedule!r} is not built (only 'linear', what guided_ldm_*_v15.yaml uses)")
    if ddim_discretize != "uniform":
        raise NotImplementedError(f"ddim_discretize={ddim_discretize!r} is not built (only 'uniform', what img2img_inpaint asks for)")
    ddim_steps, timesteps = int(ddim_steps), int(timesteps)
    if not 0 < ddim_steps <= timesteps:
        raise ValueError(f"ddim_steps must be in 1..{timesteps}, got {ddim_steps}")
    ts = np.asarray(list(range(0, timesteps, timesteps // ddim_steps))) + 1
    if int(ts[-1]) >= timesteps:
        raise ValueError(f"ddim_steps={ddim_steps}: the last DDIM step, {int(ts[-1])}, is past the {timesteps} DDPM steps (the reference "
                         "fails indexing alphas_cumprod)")
    betas = (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps, dtype=torch.float64) ** 2).numpy()
    cum64 = np.cumprod(1.0 - betas, axis=0)
    cum32 = torch.tensor(cum64, dtype=torch.float32)
    a = cum32[ts]
    a_prev = np.asarray([float(cum32[0])] + cum32[ts[:-1]].tolist(), dtype=np.float64)
    ratio = (1 - a).reciprocal() * torch.from_numpy(1 - a_prev)                   # float32 reciprocal, float64 product
    sig = float(eta) * torch.from_numpy(np.sqrt((ratio * (1 - a / torch.from_numpy(a_prev))).numpy()))
    return dict(ddim_timesteps=ts, ddim_alphas=a, ddim_alphas_prev=a_prev, ddim_sigmas=sig, ddim_sqrt_one_minus_alphas=torch.sqrt(1.0 - a),
                sqrt_alphas_cumprod=torch.tensor(np.sqrt(cum64), dtype=torch.float32),
                sqrt_one_minus_alphas_cumprod=torch.tensor(np.sqrt(1.0 - cum64), dtype=torch.float32))


def step_coefficients(sched: Dict[str, object], index: int, temperature: float = 1.0) -> Dict[str, float]:
    """The fp32 scalars of `p_sample_ddim` at `index` (guided_ldm_inpainting.py:80-103) as Python floats that hold fp32 values:
    every table entry becomes an fp32 `torch.full`, and `a_t.sqrt()`, `a_prev.sqrt()` and `(1. - a_prev - sigma_t**2).sqrt()` are
    taken in fp32.  `temperature` multiplies sigma_t (sigma_t * noise * temperature, :100)."""
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
    a_t, a_prev, sigma = f32(sched["ddim_alphas"][index]), f32(sched["ddim_alphas_prev"][index]), f32(sched["ddim_sigmas"][index])
    return dict(sqrt_at=float(a_t.sqrt()), sqrt_1m_at=float(f32(sched["ddim_sqrt_one_minus_alphas"][index])), sqrt_aprev=float(a_prev.sqrt()),
                dir_coef=float((1.0 - a_prev - sigma ** 2).sqrt()), sigma_t=float(sigma * f32(temperature)))


def decode_plan(sched: Dict[str, object], t_start: int, guidance_schedule_func: Callable = lambda p: 0.1) -> List[Tuple[float, int, int, object]]:
    """The bookkeeping of `GuidedDDIMSample.decode` (guided_ldm_inpainting.py:110-126): one (p, index, step, gs) per iteration.
    The reference reassigns `total_steps` to the length of the truncated timestep list (:115), so p = (i + 1) / t_start and
    index = t_start - i - 1; `step` is the DDPM timestep the UNet and q_sample see.  Needs no device."""
    n = len(sched["ddim_timesteps"])
    if not isinstance(t_start, (int, np.integer)) or isinstance(t_start, bool) or not 0 < t_start <= n:
        raise ValueError(f"t_start must be an int in 1..{n}, got {t_start!r}")
    steps = np.flip(sched["ddim_timesteps"][:t_start])
    total = int(steps.shape[0])
    plan = []
    for i, step in enumerate(steps):
        p = (i + (total - t_start) + 1) / total
        plan.append((p, total - i - 1, int(step), guidance_schedule_func(p)))
    return plan


def _latent(t, name, shape=None) -> torch.Tensor:
    if not is_f32_cuda(t, 4) or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError(f"{name} must be a CUDA float32 tensor {'[B,C,h,w]' if shape is None else tuple(shape)}")
    return t


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def final_blend(init_latent: torch.Tensor, decoded: torch.Tensor, nmask: torch.Tensor) -> torch.Tensor:
    """`decoded = init_latent * (1 - nmask) + decoded * nmask` (guided_ldm_inpainting.py:338) through `ops.ddim_step` with the DDIM
    part off (sa = 1, s1 = 0).  Three NCHW float32 device tensors of one shape -> a new tensor; where nmask is 0 the result is
    init_latent exactly, where it is 1 decoded exactly."""
    _latent(decoded, "decoded")
    _latent(init_latent, "init_latent", decoded.shape)
    _latent(nmask, "nmask", decoded.shape)
    if decoded.numel() % 4:
        raise RuntimeError("the latents must hold a multiple of 4 elements")
    flat = lambda t: t.contiguous().view(-1, 4)        # elementwise: any layout will do as long as the three share it
    out = ops.ddim_step(flat(decoded), dict(sa=1.0, s1=0.0), init=flat(init_latent), nmask=flat(nmask), blend_only=True)
    return out.view(decoded.shape)


class GuidedDDIMSampler:
    """`GuidedDDIMSample` over a `unet.UNetModel` (the "eps" parameterisation; module docstring)."""

    def __init__(self, unet, parameterization: str = "eps", **schedule_kwargs):
        if parameterization != "eps":
            raise NotImplementedError(f"parameterization={parameterization!r} is not built (only 'eps'; 'v' needs predict_eps_from_z_and_v)")
        self.unet = unet
        self.schedule_kwargs = dict(schedule_kwargs)          # timesteps / linear_start / linear_end of the DDPM
        self.schedule: Optional[Dict[str, object]] = None
        self.eta = 0.0
        self.last_kv_hists: List[Tuple[torch.Tensor, torch.Tensor]] = []

    def make_schedule(self, ddim_num_steps: int, ddim_eta: float = 0.0, ddim_discretize: str = "uniform") -> Dict[str, object]:
        """`DDIMSampler.make_schedule` (ddim.py:23-52): builds and keeps `ddim_schedule(ddim_num_steps, ddim_eta)`."""
        self.schedule = ddim_schedule(ddim_num_steps, ddim_eta, ddim_discretize=ddim_discretize, **self.schedule_kwargs)
        self.eta = float(ddim_eta)
        return self.schedule

    def _sched(self) -> Dict[str, object]:
        if self.schedule is None:
            raise RuntimeError("make_schedule has not been called")
        return self.schedule

    def stochastic_encode(self, x0: torch.Tensor, t: int, noise: torch.Tensor, use_original_steps: bool = False) -> torch.Tensor:
        """`DDIMSampler.stochastic_encode` (ddim.py:301-314): sqrt(ddim_alphas)[t] * x0 + ddim_sqrt_one_minus_alphas[t] * noise, fp32.
        The tables are indexed at `t` itself, as the reference does: `img2img_inpaint` passes t_enc although the first decode step
        is index t_enc - 1.  t: one int for the whole batch; noise is explicit."""
        if use_original_steps:
            raise NotImplementedError("use_original_steps is not built")
        s = self._sched()
        n = len(s["ddim_timesteps"])
        if not isinstance(t, (int, np.integer)) or isinstance(t, bool) or not 0 <= t < n:
            raise ValueError(f"t must be an int in 0..{n - 1}, got {t!r}")
        _latent(x0, "x0")
        _latent(noise, "noise", x0.shape)
        return float(torch.sqrt(s["ddim_alphas"])[t]) * x0 + float(s["ddim_sqrt_one_minus_alphas"][t]) * noise

    @torch.no_grad()
    def decode(self, x_latent: torch.Tensor, context: torch.Tensor, t_start: int, *, unconditional_context: Optional[torch.Tensor] = None,
               unconditional_guidance_scale: float = 1.0, c_concat: Optional[torch.Tensor] = None, init_latent: Optional[torch.Tensor] = None,
               nmask: Optional[torch.Tensor] = None, guidance=None, guidance_schedule_func: Callable = lambda p: 0.1, step_noise=None,
               generator: Optional[torch.Generator] = None, control=None, reference_kv=(), callback: Optional[Callable] = None,
               guidance_space: str = "latent", temperature: float = 1.0, control_nets: Optional[Sequence[SingleControlNet]] = None,
               **not_built) -> Tuple[torch.Tensor, object]:
        """`GuidedDDIMSample.decode`: x_latent f32 [B,4,h,w] on the device (what `stochastic_encode` returned), context [B,M,context_dim]
        -> (x_dec [B,4,h,w], last_gs).  The bookkeeping is `decode_plan`'s; every check runs before the first launch.

        unconditional_context [B,M,context_dim] with a scale other than 1 turns classifier-free guidance on: the UNet runs at batch
        2B, the unconditional rows first (torch.cat([unconditional_conditioning, c]), guided_ldm_inpainting.py:62).
        c_concat [B, unet.in_channels - 4, h, w]: the "hybrid" conditioning, torch.cat([x] + c_concat, dim=1) (ddpm.py:1405).
        nmask + init_latent [B,4,h,w]: before the UNet call of every step whose gs > 0 the latent becomes
            (1 - nmask) * q_sample(init_latent, step) + nmask * x_dec                                   (:127-129)
        and `guidance` None is the inpainting class: gs only gates that blend.  guidance [B,4,h,w] is the latent guidance of
        guided_ldm.py:82-89: pred_x0 = pred_x0 * (1 - gs) + guidance * gs and eps recomputed from it (:123), with gs a float or a
        device map [B,h,w] / [B,1,h,w] already at latent size.  A numpy map needs cv2's resize and guidance_space='pixel' reads an
        undefined name in the reference: both NotImplementedError.  With nmask, gs must be a number.
        Two departures from guided_ldm.py: it recomputes eps from pred_x0 in every step (:123), which without `guidance` only
        rounds eps again; here the recomputation runs only when `guidance` is given.  And it accepts a Python float alone as a
        scalar strength (an int raises, :91); here an int is taken as that number.
        step_noise: the q_sample noise of every step, [t_start,B,4,h,w]; with eta > 0 a 2-tuple whose second tensor is the DDIM
        noise of every step.  None: all of it is drawn up front in ONE torch.randn([1 or 2, t_start, B, 4, h, w]) from `generator`
        on the device (q_sample noise only when nmask is given, first; the DDIM noise only when eta > 0).
        control / reference_kv go to every UNet call unchanged and must be at the UNet's batch (2B with classifier-free guidance);
        neither they nor any latent passed in is written to.  callback(i) runs after step i.
        control may also be a callable control(i, p), called right before the UNet call of iteration i with `decode_plan`'s p: it
        returns what control= takes, a list at the UNet's batch or None, and each distinct object it returns is validated
        (`unet._check_inputs`) before it is used.  `controlnet.ControlSchedule` is one: the nets' guidance windows.
        control_nets: what the reference's driver passes (ofgen_keyframe_inpaint.py:798, :1115), a sequence of
        `controlnet.SingleControlNet`; mutually exclusive with control= (ValueError before any launch), and the nets, their conditions
        (uint8, 8x the latent) and their sizes are checked before any launch too (`controlnet.check_control_nets`).  Every net's `result` is set
        to None, and right before the first UNet call `apply_multi_controlnet(x, t, ctx, p, nets)` runs once on exactly that call's
        inputs -- the latent channels of the loop's buffer as NCHW at the UNet's batch, after the opening blend; the first step's
        timesteps; the doubled context -- which computes and caches the nets' residuals; the loop then reads them through
        `ControlSchedule(nets)`.  The reference tree holds no code that says which step's x_noisy the cached residuals come from:
        the first call of a function that caches on first use is the first step, and that is what this does.
        `self.last_kv_hists` is the K/V history of the LAST UNet call -- the final step (index 0), the least noisy latent, at the
        UNet's batch (unconditional rows first).  The reference's driver stores one history per frame and its tree has no code that
        defines which step's; the last call is what a loop that keeps overwriting one variable leaves behind.
        temperature multiplies the DDIM noise term (sigma_t * noise * temperature); it matters only with eta > 0.
        Not built (NotImplementedError): use_original_steps, score_corrector, quantize_denoised, noise_dropout, dynamic_threshold."""
        for key, val in not_built.items():
            if key not in _NOT_BUILT and key != "corrector_kwargs":
                raise TypeError(f"decode() got an unexpected keyword argument {key!r}")
            if val:
                raise NotImplementedError(f"{key} is not built")
        if guidance_space != "latent":
            raise NotImplementedError(f"guidance_space={guidance_space!r} is not built: the reference's pixel branch reads an undefined name "
                                      "(guided_ldm.py:112)")
        if control_nets is not None:
            if control is not None:
                raise ValueError("control= and control_nets= are mutually exclusive")
            control_nets = list(control_nets)
            if not control_nets or any(c.net is None for c in control_nets):
                raise ValueError("control_nets must be a non-empty sequence of SingleControlNet whose .net is set (None: no ControlNets)")
        sched = self._sched()
        plan = decode_plan(sched, t_start, guidance_schedule_func)
        cfg_on = unconditional_context is not None and unconditional_guidance_scale != 1.0
        blend = nmask is not None
        gs_list = [gs for _, _, _, gs in plan]
        for gs in gs_list:
            if isinstance(gs, np.ndarray):
                raise NotImplementedError("a numpy guidance-strength map goes through cv2.resize in the reference (guided_ldm.py:87): pass a "
                                          "device tensor already at latent size")
            if torch.is_tensor(gs):
                if guidance is None or blend:
                    raise ValueError("a guidance-strength map needs `guidance` and no nmask (gs > 0 gates the blend)")
            elif isinstance(gs, bool) or not isinstance(gs, (int, float)):
                raise NotImplementedError(f"guidance strength of type {type(gs).__name__} (the reference raises too, guided_ldm.py:91)")
        # ---- shapes, dtypes, devices: everything is checked before the first launch
        unet = self.unet
        _latent(x_latent, "x_latent")
        B, Cz, h, w = x_latent.shape
        dev = x_latent.device
        if Cz % 4 or Cz > unet.in_channels or unet.out_channels != Cz:
            raise ValueError(f"the latent has {Cz} channels; the UNet takes {unet.in_channels} and returns {unet.out_channels}")
        ncat = unet.in_channels - Cz
        if (c_concat is None) != (ncat == 0):
            raise ValueError(f"the UNet takes {unet.in_channels} channels: c_concat must have {ncat}")
        if c_concat is not None:
            _latent(c_concat, "c_concat", (B, ncat, h, w))
        if blend != (init_latent is not None):
            raise ValueError("nmask and init_latent go together")
        if blend:
            _latent(init_latent, "init_latent", x_latent.shape)
            _latent(nmask, "nmask", x_latent.shape)
        if guidance is not None:
            _latent(guidance, "guidance", x_latent.shape)
        UB = 2 * B if cfg_on else B
        cd = int(unet.cfg["context_dim"])

        def ctx(t, name):
            if not is_f32_cuda(t, 3) or t.shape[0] != B or t.shape[2] != cd:
                raise RuntimeError(f"{name} must be a CUDA float32 tensor [{B},M,{cd}]")
            return t

        ctx(context, "context")
        if cfg_on and tuple(ctx(unconditional_context, "unconditional_context").shape) != tuple(context.shape):
            raise RuntimeError("unconditional_context must have the shape of context")
        gmaps: List[Optional[torch.Tensor]] = []
        for gs in gs_list:
            if torch.is_tensor(gs):
                if not gs.is_cuda or gs.dtype != torch.float32 or tuple(gs.shape) not in ((B, h, w), (B, 1, h, w)):
                    raise RuntimeError(f"a guidance-strength map must be a CUDA float32 tensor [{B},{h},{w}]")
                gmaps.append(gs.reshape(B, h, w).contiguous())
            else:
                gmaps.append(None)
        eta_on = self.eta != 0.0
        n_noise = int(blend) + int(eta_on)
        qn = dn = None
        if step_noise is not None:
            parts = list(step_noise) if isinstance(step_noise, (tuple, list)) else [step_noise]
            if len(parts) != 1 + int(eta_on) or (not blend and not eta_on):
                raise ValueError("step_noise: one tensor [t_start,B,4,h,w] (the q_sample noise), and with eta > 0 a 2-tuple whose second "
                                 "tensor is the DDIM noise")
            for t in parts:
                if t is not None and (not is_f32_cuda(t, 5) or tuple(t.shape) != (t_start, B, Cz, h, w)):
                    raise RuntimeError(f"step_noise must be CUDA float32 [{t_start},{B},{Cz},{h},{w}]")
            qn = parts[0]
            dn = parts[1] if eta_on else None
            if (blend and qn is None) or (eta_on and dn is None):
                raise ValueError("step_noise lacks a tensor this run needs")
        ts_all = torch.tensor([[float(step)] * UB for _, _, step, _ in plan], dtype=torch.float32)
        control_fn = control if callable(control) else None                           # control(i, p): validated as it is returned
        unet._check_inputs(UB, h, w, ts_all[0], None, None if control_fn else control, reference_kv)   # raises on a bad control / reference_kv / size
        if control_nets is not None:
            check_control_nets(control_nets, UB, Cz, h, w, ts_all[0], cd)             # nets, conditions and sizes: before the opening blend
        # ---- setup: the only allocations and layout changes of the loop
        if step_noise is None and n_noise:
            drawn = torch.randn((n_noise, t_start, B, Cz, h, w), generator=generator, device=dev, dtype=torch.float32)
            qn = drawn[0] if blend else None
            dn = drawn[-1] if eta_on else None
        to_rows = lambda t: None if t is None else t.permute(0, 1, 3, 4, 2).contiguous()          # [t_start,B,h,w,4]
        qn, dn = to_rows(qn if blend else None), to_rows(dn)
        buf = torch.zeros((UB, h, w, unet.in_pad), dtype=torch.float32, device=dev)
        xh = x_latent.permute(0, 2, 3, 1)
        buf[:B, ..., :Cz] = xh
        if c_concat is not None:
            buf[:B, ..., Cz:unet.in_channels] = c_concat.permute(0, 2, 3, 1)
        if cfg_on:
            buf[B:] = buf[:B]
        x0v = buf[:B, ..., :Cz]
        x1v = buf[B:, ..., :Cz] if cfg_on else None
        ctx_in = torch.cat([unconditional_context, context]) if cfg_on else context
        init_r = _nhwc(init_latent) if blend else None
        mask_r = _nhwc(nmask) if blend else None
        guide_r = _nhwc(guidance) if guidance is not None else None
        ts_all = ts_all.to(dev)
        sa_t, s1_t = sched["sqrt_alphas_cumprod"], sched["sqrt_one_minus_alphas_cumprod"]
        gate = [blend and gs > 0 for gs in gs_list]                                   # (:127)

        def blend_args(i):
            """The q_sample + blend that opens iteration i (:128-129)."""
            step = plan[i][2]
            return dict(sa=float(sa_t[step]), s1=float(s1_t[step])), dict(init=init_r, nmask=mask_r, blend_noise=qn[i])

        if gate[0]:
            k, kw = blend_args(0)
            ops.ddim_step(x0v, k, out0=x0v, out1=x1v, blend_only=True, **kw)
        if control_nets is not None:
            for c in control_nets:
                c.result = None
            apply_multi_controlnet(buf[..., :Cz].permute(0, 3, 1, 2).contiguous(), ts_all[0], ctx_in, plan[0][0], control_nets)
            control_fn = ControlSchedule(control_nets)
        kv: List[Tuple[torch.Tensor, torch.Tensor]] = []
        checked: list = []                                                            # the distinct objects control(i, p) has returned
        for i, (p, index, step, gs) in enumerate(plan):
            if control_fn is not None:
                control = control_fn(i, p)
                if control is not None and not any(control is c for c in checked):
                    unet._check_inputs(UB, h, w, ts_all[i], None, control, ())
                    checked.append(control)
            eps, kv = unet.forward_nhwc(buf, ts_all[i], ctx_in, control, False, reference_kv, padded=True)
            k = step_coefficients(sched, index, temperature)
            k["cfg"] = float(unconditional_guidance_scale)
            kw = {}
            if guide_r is not None:
                kw["guidance"] = guide_r
                if gmaps[i] is not None:
                    kw["gmap"] = gmaps[i]
                else:
                    k["g"] = float(gs)
            if eta_on:
                kw["step_noise"] = dn[i]
            if i + 1 < len(plan) and gate[i + 1]:
                k2, kw2 = blend_args(i + 1)
                k.update(k2)
                kw.update(kw2)
            ops.ddim_step(x0v, k, eps_c=eps[B:] if cfg_on else eps, eps_u=eps[:B] if cfg_on else None, out0=x0v, out1=x1v, **kw)
            if callback:
                callback(i)
        self.last_kv_hists = kv
        return x0v.permute(0, 3, 1, 2).contiguous(), gs_list[-1]


@torch.no_grad()
def img2img_inpaint(unet, vae_encoder, vae_decoder, image_bgr, reference_bgr, mask, context: torch.Tensor,
                    unconditional_context: Optional[torch.Tensor], *, denoising_strength: float = 0.05, ddim_steps: int = 50,
                    mask_blur: float = 16, unconditional_guidance_scale: float = 7.0, guidance_schedule_func: Callable = lambda p: 0.1,
                    noise: Optional[Dict[str, torch.Tensor]] = None, generator: Optional[torch.Generator] = None, control=None,
                    reference_kv=(), sampler: Optional[GuidedDDIMSampler] = None, fill_masked: bool = False,
                    control_nets: Optional[Sequence[SingleControlNet]] = None, want_init_decoded: bool = True):
    """`GuidedLDM.img2img_inpaint` (guided_ldm_inpainting.py:262-345), eta = 0.  With a reference frame: image_bgr / reference_bgr
    uint8 [H,W,3] (cv2 channel order) and mask uint8 [H,W] (255 = repaint) as `handoff.prepare_inpaint_inputs` takes them, context /
    unconditional_context [1,M,context_dim] device tensors (`text_encoder.ClipTextEncoder.conditioning` makes both from a prompt pair) ->
        (x_samples clipped to [-1,1] f32 [1,3,H,W],  image f32 [1,3,H,W],  init_latent_decoded clipped)
    The chain: prepare_inpaint_inputs; init_latent = encode(image); c_concat = cat(conditioning_mask_latent, encode(conditioning
    _image)); t_enc = int(min(strength, 0.999) * steps); stochastic_encode(init_latent, t_enc); decode with nmask = latmask; the final
    blend when last_gs > 0; both VAE decodes.
    noise: explicit tensors under the keys "init" and "cond" (the two encoder samples, [B,4,h,w]), "x1" (stochastic_encode's,
    [B,4,h,w]) and "step" (`decode`'s step_noise, [t_enc,B,4,h,w]); a key left out is drawn from `generator` on the device, in that
    order (init, cond, x1, step), each with one torch.randn.
    reference_bgr None with fill_masked=True is the path without a reference (`reference_img is None`, :295-296, :310-312; what the
    `self_attn` and `both` modes of generate_ai_frame_with_ref run on a strip of frames): `image` is `handoff.fill_mask_input` of
    the frame, init_latent = (1 - nmask) * init_latent + nmask * noise["fill"] ([B,4,h,w], drawn between "init" and "cond":
    init, fill, cond, x1, step), denoising_strength becomes 1 (t_enc = int(0.999 * ddim_steps)) and the final blend uses that
    noised init_latent.  reference_bgr None without fill_masked is a NotImplementedError, fill_masked with a reference or
    noise["fill"] without fill_masked a ValueError.  t_enc == 0 (the default strength 0.05 needs at least 20 steps) is a
    ValueError: the reference would run zero steps and index an empty range.  All raise before any launch.
    `sampler`: a GuidedDDIMSampler over `unet` to reuse (its `last_kv_hists` is then the caller's to read).
    control_nets: `decode`'s (exclusive with control=: a ValueError here too, before any launch).  want_init_decoded=False skips
    the second VAE decode, which the reference's driver only writes to its visualisation; the third result is then None."""
    if control is not None and control_nets is not None:
        raise ValueError("control= and control_nets= are mutually exclusive")
    if reference_bgr is None and not fill_masked:
        raise NotImplementedError("reference_bgr=None is the reference's fill_mask_input path: ask for it with fill_masked=True")
    if fill_masked and reference_bgr is not None:
        raise ValueError("fill_masked=True is the path without a reference frame: reference_bgr must be None")
    if fill_masked:
        denoising_strength = 1                                                          # (:312)
    t_enc = int(min(denoising_strength, 0.999) * ddim_steps)
    if t_enc <= 0:
        raise ValueError(f"denoising_strength={denoising_strength} at {ddim_steps} steps gives t_enc = 0: no step to run")
    noise = dict(noise or {})
    unknown = set(noise) - {"init", "fill", "cond", "x1", "step"}
    if unknown:
        raise ValueError(f"noise has unknown keys {sorted(unknown)}")
    if "fill" in noise and not fill_masked:
        raise ValueError("noise['fill'] without fill_masked")
    smp = sampler if sampler is not None else GuidedDDIMSampler(unet)
    smp.make_schedule(ddim_steps, 0.0)
    dev = unet.device
    inp = prepare_inpaint_inputs(image_bgr, reference_bgr, mask, mask_blur=mask_blur, device=dev, fill_masked=fill_masked)
    image, latmask = inp["image"], inp["latmask"]
    B, _, h, w = latmask.shape

    def draw(key, shape):
        if key in noise:
            return _latent(noise[key], f"noise[{key!r}]", shape) if len(shape) == 4 else noise[key]
        return torch.randn(shape, generator=generator, device=dev, dtype=torch.float32)

    n_init = draw("init", (B, 4, h, w))
    n_fill = draw("fill", (B, 4, h, w)) if fill_masked else None
    n_cond = draw("cond", (B, 4, h, w))
    n_x1, n_step = draw("x1", (B, 4, h, w)), draw("step", (t_enc, B, 4, h, w))
    init_latent = vae_encoder.get_first_stage_encoding(image, n_init)
    if fill_masked:
        init_latent = final_blend(init_latent, n_fill, latmask)                         # (:311)
    cond_latent = vae_encoder.get_first_stage_encoding(inp["conditioning_image"], n_cond)
    c_concat = torch.cat([inp["conditioning_mask_latent"], cond_latent], dim=1)
    x1 = smp.stochastic_encode(init_latent, t_enc, n_x1)
    decoded, last_gs = smp.decode(x1, context, t_enc, unconditional_context=unconditional_context,
                                  unconditional_guidance_scale=unconditional_guidance_scale, c_concat=c_concat, init_latent=init_latent,
                                  nmask=latmask, guidance_schedule_func=guidance_schedule_func, step_noise=n_step, control=control,
                                  reference_kv=reference_kv, control_nets=control_nets)
    if last_gs > 0:
        decoded = final_blend(init_latent, decoded, latmask)
    x_samples = vae_decoder.decode_first_stage(decoded)
    init_latent_decoded = vae_decoder.decode_first_stage(init_latent).clip(-1, 1) if want_init_decoded else None
    return torch.clip(x_samples, -1, 1), image, init_latent_decoded


def _bgr_image(frame_bgr, name: str, device) -> torch.Tensor:
    """u8 [H,W,3] or [B,H,W,3] in cv2 channel order, numpy or tensor -> f32 [B,3,H,W] RGB, x / 127.5 - 1, computed on the device
    (`frame_rgb.astype(np.float32) / 127.5 - 1.`, ofgen_keyframe_inpaint.py:204)."""
    t = frame_bgr if torch.is_tensor(frame_bgr) else torch.from_numpy(np.ascontiguousarray(frame_bgr))
    if t.dtype != torch.uint8 or t.dim() not in (3, 4) or t.shape[-1] != 3:
        raise RuntimeError(f"{name} must be uint8 [H,W,3] or [B,H,W,3]")
    t = t.to(device)
    if t.dim() == 3:
        t = t[None]
    return t.flip(-1).permute(0, 3, 1, 2).float().contiguous() / 127.5 - 1.0


@torch.no_grad()
def img2img(unet, vae_encoder, vae_decoder, image_bgr, context: torch.Tensor, unconditional_context: Optional[torch.Tensor], *,
            denoising_strength: float, ddim_steps: int = 50, target_bgr=None, guidance_schedule_func: Callable = lambda p: 0.1,
            unconditional_guidance_scale: float = 7.0, noise: Optional[Dict[str, torch.Tensor]] = None,
            generator: Optional[torch.Generator] = None, control=None, reference_kv=(),
            sampler: Optional[GuidedDDIMSampler] = None, control_nets: Optional[Sequence[SingleControlNet]] = None) -> torch.Tensor:
    """`GuidedLDM.img2img`, eta = 0: the seed key frames of the live driver and the guided frames of `ofgen.py`.  image_bgr /
    target_bgr uint8 [H,W,3] or [B,H,W,3] (cv2 channel order; several frames side by side in one wide image are one image), context
    / unconditional_context [B,M,context_dim] device tensors -> x_samples f32 [B,3,H,W] clipped to [-1,1].
        target_bgr None    guided_ldm_inpainting.py:185-259 with mask None: init_latent = encode(image); t_enc = int(min(strength,
                           0.999) * steps); stochastic_encode; decode without nmask or c_concat; decode_first_stage; clip
        target_bgr given   guided_ldm.py:166-219 with guidance_space='latent': the target's latent is `decode(guidance=)` and
                           guidance_schedule_func returns a float or a device map at latent size, as `decode` takes them
    noise: explicit tensors [B,4,h,w] under the keys "init" and "target" (the encoder samples) and "x1" (stochastic_encode's); a key
    left out is drawn from `generator` on the device, in that order (init, target, x1), each with one torch.randn; "target" is
    drawn only when a target is given.  control (a list or a callable, as `decode` takes) and reference_kv go to `decode`.
    `sampler`: a GuidedDDIMSampler over `unet` to reuse; its `last_kv_hists` is what the driver stores per key frame.
    t_enc == 0 and a UNet whose in_channels is not 4 (there is no c_concat on this path) are ValueErrors before any launch.  No
    launch of its own: the loop is `decode`, around it two (or three) VAE passes.  control_nets is `decode`'s (exclusive with
    control=: a ValueError here too, before any launch)."""
    if control is not None and control_nets is not None:
        raise ValueError("control= and control_nets= are mutually exclusive")
    t_enc = int(min(denoising_strength, 0.999) * ddim_steps)
    if t_enc <= 0:
        raise ValueError(f"denoising_strength={denoising_strength} at {ddim_steps} steps gives t_enc = 0: no step to run")
    if unet.in_channels != 4:
        raise ValueError(f"img2img runs the UNet on the latent alone: in_channels must be 4, got {unet.in_channels} (a hybrid UNet "
                         "is img2img_inpaint's)")
    noise = dict(noise or {})
    unknown = set(noise) - {"init", "target", "x1"}
    if unknown:
        raise ValueError(f"noise has unknown keys {sorted(unknown)}")
    if target_bgr is None and "target" in noise:
        raise ValueError("noise['target'] without target_bgr")
    smp = sampler if sampler is not None else GuidedDDIMSampler(unet)
    smp.make_schedule(ddim_steps, 0.0)
    dev = unet.device
    image = _bgr_image(image_bgr, "image_bgr", dev)
    target = None if target_bgr is None else _bgr_image(target_bgr, "target_bgr", dev)
    if target is not None and tuple(target.shape) != tuple(image.shape):
        raise RuntimeError(f"target_bgr {tuple(target.shape)} does not match image_bgr {tuple(image.shape)}")
    B, _, H, W = image.shape
    shape = (B, 4, H // 8, W // 8)

    def draw(key):
        if key in noise:
            return _latent(noise[key], f"noise[{key!r}]", shape)
        return torch.randn(shape, generator=generator, device=dev, dtype=torch.float32)

    n_init = draw("init")
    n_target = draw("target") if target is not None else None
    n_x1 = draw("x1")
    init_latent = vae_encoder.get_first_stage_encoding(image, n_init)
    target_latent = None if target is None else vae_encoder.get_first_stage_encoding(target, n_target)
    x1 = smp.stochastic_encode(init_latent, t_enc, n_x1)
    decoded, _ = smp.decode(x1, context, t_enc, unconditional_context=unconditional_context,
                            unconditional_guidance_scale=unconditional_guidance_scale, guidance=target_latent,
                            guidance_schedule_func=guidance_schedule_func, control=control, reference_kv=reference_kv,
                            control_nets=control_nets)
    return torch.clip(vae_decoder.decode_first_stage(decoded), -1, 1)
