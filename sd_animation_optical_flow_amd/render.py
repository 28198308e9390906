"""The generative half of the reference's driver, composed from the device modules: from (flow, confidence, reference AI frames,
raw frame) to a rendered frame without leaving HBM.

    run_inpainting                                   ofgen_keyframe_inpaint.py:255-290
    generate_ai_frame_with_ref and its four modes    ofgen_keyframe_inpaint.py:722-1086
    generate_seed_frames                             ofgen_keyframe_inpaint.py:1088-1117
    the generation loop of run_exp                   ofgen_keyframe_inpaint.py:1153-1241

`SdRenderer` holds the models (`unet.UNetModel`, `vae.VaeEncoder` / `VaeDecoder`, `controlnet.ControlNet`s) and the driver's
constants; its methods restate the reference functions line for line over `ofgen.compose_warp_and_mask_device` (one
`ops.compose_refs`), `ofgen.strip_inputs_*`, `sampler.img2img_inpaint` / `img2img` with `control_nets=`, and `ops.decode_to_u8`.
Frames are BGR uint8 [H,W,3] (cv2's order, the reference's) on the device on the way in and out; arrays are uploaded.

What is not built: the tagger that writes the reference's prompt (`conditioning` is the caller's callable, or a fixed pair:
`fixed_prompt`), the HED detector (`ControlSpec.detector` is the caller's, as in `controlnet.make_hint`), `merge_denoise_history`
(the reference's live call passes an empty history) and the `render_vis` images.

A K/V history (`kv_hist`, `GuidedDDIMSampler.last_kv_hists`) holds the self-attention keys and values of every transformer block of
the UNet's last call.  At SD v1.5 and 512x768 that is 139 MB per batch row (16 attention layers: 5 at 6144 tokens x 320 channels,
5 at 1536 x 640, 5 at 384 x 1280, 1 at 96 x 1280, keys and values, fp32), so 277 MB per frame at UNet batch 2 -- derived from
the layer table; `tools/render_rate.py` reports the same figure from the tensors.  `run_exp` keeps them on the device in a dict and drops them as the reference does.
`kv_dtype="fp16"` (`UNetModel`, `SdRenderer`, `run_exp`) keeps them in half, as the reference's autocast does: 139 MB per frame in
memory and in `video.put_kv`'s pickle; the fused attention reads them in place in either dtype (`transformer` module docstring).

Needs no device to import; `generation_plan` is pure Python.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ofgen, ops
from .controlnet import SingleControlNet, canny_condition
from .sampler import GuidedDDIMSampler, img2img, img2img_inpaint

MODES = ("warp_and_inpaint", "warp_and_inpaint_crossattn", "self_attn", "both")


@dataclass
class ControlSpec:
    """One ControlNet of the driver: `SingleControlNet`'s constants plus the detector that makes its condition from a frame.
    detector(frame_bgr u8 [H,W,3] on the device) -> the edge map u8 [H,W] (`controlnet.make_hint` takes it)."""
    model: str
    net: Any
    weight: float
    guidance_start: float = 0.0
    guidance_end: float = 1.0
    args: dict = field(default_factory=dict)
    detector: Optional[Callable] = None


def canny_detector(low: float = 100, high: float = 200) -> Callable:
    """`extract_control`'s 'canny' detector: frame -> `controlnet.canny_condition(frame, low, high)` on the frame's device."""
    return lambda frame_bgr: canny_condition(frame_bgr, low, high, device=frame_bgr.device)


def driver_controls(hed_net, hed_detector: Callable, canny_net, mode: str = "warp_and_inpaint_crossattn") -> List[ControlSpec]:
    """The pair every mode of the driver builds (:775-795, :833-853, :938-958, :1028-1048, :1093-1113): hed at weight 0.7 over
    [0, 1] and canny at weight 0.3 with thresholds 100 / 200 over [0, 0.9] -- [0, 1] in `self_attn` (:842-852)."""
    if mode not in MODES and mode != "seed":
        raise ValueError(f"unknown mode {mode!r}: one of {MODES} or 'seed'")
    args = {"low_threshold": 100, "high_threshold": 200}
    return [ControlSpec("hed", hed_net, 0.7, 0.0, 1.0, {}, hed_detector),
            ControlSpec("canny", canny_net, 0.3, 0.0, 1.0 if mode == "self_attn" else 0.9, args, canny_detector(100, 200))]


def fixed_prompt(text_encoder, tokens_c, tokens_uc) -> Tuple[torch.Tensor, torch.Tensor]:
    """A fixed (context, unconditional_context) pair for `SdRenderer(conditioning=)`: `ClipTextEncoder.conditioning` of one
    prompt pair, encoded once.  The reference prompts every frame with its tagger's labels; the tagger is not built."""
    return text_encoder.conditioning(tokens_c, tokens_uc)


def _frame(a, device) -> torch.Tensor:
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device).contiguous()


def as_kv_dtype(kv, kv_dtype: str):
    """A K/V history (a list of (k, v) pairs) with every tensor in `kv_dtype` ("fp32" / "fp16"): the list itself where every tensor
    already is (no copy), a converted copy otherwise -- to half with round to nearest even and infinities beyond +-65504."""
    dt = ops.KV_DTYPES[ops.check_kv_dtype(kv_dtype)]
    if all((not torch.is_tensor(t)) or t.dtype == dt for e in kv for t in e):
        return kv
    return [tuple(t.to(dt) if torch.is_tensor(t) else t for t in e) for e in kv]


def generation_plan(history: Sequence, num_ref: int) -> List[Tuple[int, int, List[int], List[int], Optional[int]]]:
    """The bookkeeping of run_exp's generation loop (:1173-1240), pure Python.  history: the index sets the analysis left, from
    all frames (level 0) to the seed frames (frame 0 already added); each a `VideoFrameIndices` or any iterable of ints, none is
    modified.  -> one (level, idx, reference indices, kv reference indices, kv index to drop or None) per frame, in the order
    the reference renders them: the seed level is popped as `generated`; every level above it is popped in turn, loses the
    generated frames (`remove`), and each of its frames takes `generated.adjacent_frames(idx, num_ref)` as references.  The K/V
    histories handed in are the references', and at level 0 also the previous frame's of that level, which is dropped once the
    frame is rendered (:1204-1208, :1233-1234).  `generated` grows by the level when the level is done (:1240)."""
    from .workspace import VideoFrameIndices
    hist = [VideoFrameIndices(getattr(h, "indices", h)) for h in history]
    if not hist:
        raise ValueError("generation_plan: history is empty")
    level = len(hist) - 1
    generated = hist.pop()
    plan = []
    while hist:
        level -= 1
        cur = hist.pop()
        cur.remove(generated)
        last = -1
        for idx in cur.indices:
            refs = list(generated.adjacent_frames(idx, num_ref).indices)
            kv_refs = list(refs)
            drop = None
            if last != -1 and level == 0:
                kv_refs.append(last)
                drop = last
            plan.append((level, idx, refs, kv_refs, drop))
            last = idx
        generated.add(cur)
    return plan


class SdRenderer:
    """The driver's models and constants.  unet_inpaint: the 9-channel inpainting `UNetModel` of `run_inpainting`; unet_seed: the
    4-channel one of `generate_seed_frames` (optional).  conditioning: a callable frame_bgr -> (context, unconditional_context),
    or that pair.  controls: `ControlSpec`s (`driver_controls`); their guidance windows are the specs'.  seed: every
    `run_inpainting` / `generate_seed_frames` call draws its noise from a device generator seeded with it, as the reference
    calls torch.manual_seed(1234) per call (:274-275).  An instance is also `ClipPipeline`'s pair of hooks: `render=renderer`,
    `render_key=renderer.render_key`.  kv_dtype: "fp32" (default) or "fp16", the dtype of every K/V history the methods hand back
    (anything else is a ValueError).  UNets built with the same `kv_dtype=` record it directly; a history of the other dtype is
    converted once as it is handed back (`as_kv_dtype`)."""

    def __init__(self, unet_inpaint, vae_encoder, vae_decoder, conditioning, controls: Sequence[ControlSpec] = (), *, unet_seed=None,
                 ddim_steps: int = 50, ds: float = 0.6, mask_blur: float = 4, unconditional_guidance_scale: float = 7.0,
                 guidance_schedule_func: Callable = lambda p: 0.1, seed: int = 1234, warp_mode: Optional[str] = None,
                 kv_dtype: str = "fp32"):
        self.kv_dtype = ops.check_kv_dtype(kv_dtype)               # before anything else is looked at
        self.unet_inpaint, self.unet_seed = unet_inpaint, unet_seed
        self.vae_encoder, self.vae_decoder = vae_encoder, vae_decoder
        self.conditioning = conditioning
        self.controls = list(controls)
        self.ddim_steps, self.ds, self.mask_blur = int(ddim_steps), float(ds), mask_blur
        self.unconditional_guidance_scale = float(unconditional_guidance_scale)
        self.guidance_schedule_func = guidance_schedule_func
        self.seed = int(seed)
        self.warp_mode = warp_mode

    # ---- pieces ----------------------------------------------------------------------------------------------------------
    @property
    def device(self):
        return self.unet_inpaint.device

    def _kv(self, kv):
        return as_kv_dtype(kv, self.kv_dtype)

    def _generator(self) -> torch.Generator:
        return torch.Generator(device=self.device).manual_seed(self.seed)

    def _context(self, frame_bgr) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        return self.conditioning(frame_bgr) if callable(self.conditioning) else tuple(self.conditioning)

    def control_nets(self, condition_frame: torch.Tensor, canny_end: Optional[float] = None) -> Optional[List[SingleControlNet]]:
        """The `cnets` list of a mode: one fresh `SingleControlNet` per spec, its condition the spec's detector on
        `condition_frame`.  canny_end overrides the 'canny' specs' guidance_end (1 in `self_attn`).  None without controls."""
        nets = []
        for s in self.controls:
            if s.detector is None:
                raise ValueError(f"ControlSpec(model={s.model!r}) has no detector")
            end = canny_end if (canny_end is not None and s.model == "canny") else s.guidance_end
            nets.append(SingleControlNet(weight=s.weight, model=s.model, args=dict(s.args), condition=s.detector(condition_frame),
                                         guidance_start=s.guidance_start, guidance_end=end, net=s.net))
        return nets or None

    # ---- run_inpainting (:255-290) ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def run_inpainting(self, image_bgr, reference_bgr, mask, *, condition_frame, prompt_frame=None, reference_kv=(),
                       ds: Optional[float] = None, canny_end: Optional[float] = None):
        """image_bgr u8 [H,W,3], reference_bgr the same or None (then `fill_masked`: the strip modes), mask u8 [H,W] (255 =
        repaint) -> (frame u8 [H,W,3] BGR on the device, kv_hist = the sampler's `last_kv_hists`).  The prompt is
        `conditioning(prompt_frame)`, of the reference frame without one (:266-269); the ControlNets see `condition_frame`.
        `img2img_inpaint(..., mask_blur=4, control_nets=, reference_kv=)` with the second VAE decode (visualisation only) off;
        the frame leaves through `ops.decode_to_u8`, the reference's `(img * 127.5 + 127.5).astype(np.uint8)` and RGB2BGR."""
        dev = self.device
        image = _frame(image_bgr, dev)
        reference = None if reference_bgr is None else _frame(reference_bgr, dev)
        pf = prompt_frame if prompt_frame is not None else (reference if reference is not None else image)
        context, uncond = self._context(pf)
        nets = self.control_nets(_frame(condition_frame, dev), canny_end)
        smp = GuidedDDIMSampler(self.unet_inpaint)
        x, _, _ = img2img_inpaint(self.unet_inpaint, self.vae_encoder, self.vae_decoder, image, reference, _frame(mask, dev), context, uncond,
                                  denoising_strength=self.ds if ds is None else ds, ddim_steps=self.ddim_steps, mask_blur=self.mask_blur,
                                  unconditional_guidance_scale=self.unconditional_guidance_scale,
                                  guidance_schedule_func=self.guidance_schedule_func, generator=self._generator(), control_nets=nets,
                                  reference_kv=reference_kv, sampler=smp, fill_masked=reference is None, want_init_decoded=False)
        return ops.decode_to_u8(x.permute(0, 2, 3, 1).contiguous())[0], self._kv(smp.last_kv_hists)

    # ---- generate_seed_frames (:1088-1117) -------------------------------------------------------------------------------
    @torch.no_grad()
    def generate_seed_frames(self, raw_frames: Sequence, ds: float = 0.8):
        """raw_frames: BGR u8 [H,W,3] frames -> (list of rendered frames u8 [H,W,3] on the device, kv_hist).  The frames go side
        by side into ONE `img2img` on `unet_seed`; the prompt is the first frame's (:1115), the ControlNets see the wide image."""
        if self.unet_seed is None:
            raise ValueError("generate_seed_frames needs unet_seed (the 4-channel UNet of the reference's model_gen)")
        if len(raw_frames) == 0:
            raise ValueError("generate_seed_frames: no frames")
        dev = self.unet_seed.device
        frames = [_frame(f, dev) for f in raw_frames]
        large = torch.cat(frames, dim=1)
        context, uncond = self._context(frames[0])
        smp = GuidedDDIMSampler(self.unet_seed)
        x = img2img(self.unet_seed, self.vae_encoder, self.vae_decoder, large, context, uncond, denoising_strength=ds,
                    ddim_steps=self.ddim_steps, guidance_schedule_func=self.guidance_schedule_func,
                    unconditional_guidance_scale=self.unconditional_guidance_scale, generator=self._generator(),
                    control_nets=self.control_nets(large), sampler=smp)
        wide = ops.decode_to_u8(x.permute(0, 2, 3, 1).contiguous())[0]
        return [p.contiguous() for p in torch.chunk(wide, len(frames), dim=1)], self._kv(smp.last_kv_hists)

    # ---- generate_ai_frame_with_ref (:722-1086) --------------------------------------------------------------------------
    @torch.no_grad()
    def generate_ai_frame_with_ref(self, flow, conf, ai_frames: Sequence, raw_frame, mode: str = "warp_and_inpaint", *, reference_kv=(),
                                   prev_ai_frame=None, prev_position: Optional[int] = None, thres: float = 0.95, ds: Optional[float] = None):
        """flow f32 [N,H,W,2] / conf f32 [N,H,W] (`PDCNetAux.multiple_to_one_device`), ai_frames: the N reference frames' AI
        frames, raw_frame: the frame to render, all BGR u8 [H,W,3] -> (frame u8 [H,W,3] on the device, kv_hist).
            'warp_and_inpaint'            (:741-798)   greedy composition, mask2 = dilate(255 - mask, 7x7 ellipse); reference = raw frame
            'warp_and_inpaint_crossattn'  (:995-1051)  greedy composition, mask2 = expand_mask(255 - mask, raw); reference_kv goes through
            'self_attn'                   (:823-858)   `strip_inputs_self_attn`: no reference, the ControlNets see the strip (canny to
                                                       p = 1), the answer is the strip's first w columns
            'both'                        (:877-962)   composition of order[0] alone (its merge is commented out), no dilation;
                                                       prev_ai_frame joins the references of the strip when given (the caller
                                                       decides, :878) -- behind them, or at index prev_position among them: the
                                                       reference adds frame idx - 1 to a SORTED index set (:921), so it stands where
                                                       its index puts it, which `run_exp` passes; the composition uses ai_frames alone
                                                       `strip_inputs_both`; the ControlNets see the raw-frame strip; first w columns
        reference_kv is used by 'warp_and_inpaint_crossattn' only, as in the reference.  An unknown mode is a ValueError."""
        if mode not in MODES:
            raise ValueError(f"unknown mode {mode!r}: one of {MODES}")
        dev = self.device
        raw = _frame(raw_frame, dev)
        w = raw.shape[1]
        if mode == "self_attn":
            all_frames, mask = ofgen.strip_inputs_self_attn(raw, ai_frames, dev)
            ans, kv = self.run_inpainting(all_frames, None, mask, condition_frame=all_frames, prompt_frame=raw, ds=ds, canny_end=1.0)
            return ans[:, :w].contiguous(), kv
        if mode == "both":
            ret, mask2, _ = ofgen.compose_warp_and_mask_device(flow, conf, ai_frames, raw, thres, self.warp_mode, expand=False,
                                                               first_only=True, device=dev)
            refs = list(ai_frames)
            if prev_ai_frame is not None:
                refs.insert(len(refs) if prev_position is None else int(prev_position), prev_ai_frame)
            frames, ref_frames, mask = ofgen.strip_inputs_both(ret, raw, mask2, refs, dev)
            ans, kv = self.run_inpainting(frames, None, mask, condition_frame=ref_frames, prompt_frame=raw, ds=ds)
            return ans[:, :w].contiguous(), kv
        crossattn = mode == "warp_and_inpaint_crossattn"
        ret, mask2, _ = ofgen.compose_warp_and_mask_device(flow, conf, ai_frames, raw, thres, self.warp_mode, expand=crossattn, device=dev)
        if not crossattn:
            mask2 = ops.dilate(mask2[None].contiguous(), 7)[0]                                  # :773-774
        return self.run_inpainting(ret, raw, mask2, condition_frame=raw, reference_kv=reference_kv if crossattn else (), ds=ds)

    # ---- ClipPipeline's hooks --------------------------------------------------------------------------------------------
    def __call__(self, packet, raw_bgr) -> torch.Tensor:
        """`ClipPipeline(render=)`: the packet's warped key frame repainted where its mask asks, the raw frame as reference."""
        return self.run_inpainting(packet.warped, raw_bgr, packet.mask, condition_frame=raw_bgr)[0]

    def render_key(self, raw_bgr) -> torch.Tensor:
        """`ClipPipeline(render_key=)`: one seed frame."""
        return self.generate_seed_frames([raw_bgr])[0][0]


@torch.no_grad()
def run_exp(video, pdcnet, renderer: SdRenderer, num_ref_for_generation: int = 1, ds: float = 0.6,
            mode: str = "warp_and_inpaint_crossattn", kernel_size: int = 30, stride: int = 15, dilation: int = 2,
            persist_kv: bool = False, kv_dtype: Optional[str] = None) -> Dict[int, list]:
    """The reference's `run_exp` from the analysis on (:1153-1241) over a `workspace.VideoData` and an `ofgen.PDCNetAux`:
    `KeyframeConv` level by level (`d{level:02d}/` under the workspace) down to one seed frame, frame 0 added, the seed frames
    (`generate_seed_frames`, ds 0.8), then `generation_plan`: per frame `multiple_to_one_device`, `generate_ai_frame_with_ref`,
    `put_ai_frame`.  K/V histories stay on the device in a dict keyed by frame index, which is returned; the previous frame's is
    dropped at level 0 as the reference does.  persist_kv also pickles them through `video.put_kv` / `remove_kv` (277 MB per
    frame at v1.5 and 512x768, module docstring; half of that with kv_dtype "fp16").  kv_dtype: "fp32" or "fp16", the dtype of the
    histories in the returned dict and in `video.put_kv`; None (default) is the renderer's own `kv_dtype`, "fp32" unless it was
    built otherwise.  An unknown mode or kv_dtype, or a renderer without `unet_seed`, is a ValueError before anything runs."""
    import os

    from .workspace import VideoFrameIndices
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r}: one of {MODES}")
    kv_dtype = ops.check_kv_dtype(getattr(renderer, "kv_dtype", "fp32") if kv_dtype is None else kv_dtype)
    if renderer.unet_seed is None:
        raise ValueError("run_exp needs a renderer with unet_seed (the seed frames)")
    n_seed_frames = 1
    history = [VideoFrameIndices.from_n(video.num_frames)]
    frame_indices = history[0]
    level = 0
    while len(frame_indices) > n_seed_frames:
        level += 1
        frame_indices = ofgen.KeyframeConv(pdcnet, os.path.join(video.workspace_dir, f"d{level:02d}"), video, frame_indices,
                                           kernel_size=kernel_size, stride=stride, dilation=dilation)
        history.append(frame_indices)
    pdcnet.purge()
    frame_indices.add(0)
    seeds, seed_kv = renderer.generate_seed_frames([video.get_raw_frame(i) for i in frame_indices.indices], ds=0.8)
    kv_map: Dict[int, list] = {}
    ai: Dict[int, torch.Tensor] = {}

    def put(idx, frame, kv):
        kv = as_kv_dtype(kv, kv_dtype)
        ai[idx] = frame
        video.put_ai_frame(idx, frame.cpu().numpy())
        kv_map[idx] = kv
        if persist_kv:
            video.put_kv(idx, kv)

    for i, idx in enumerate(frame_indices.indices):
        put(idx, seeds[i], seed_kv)
    dev = renderer.device
    ai_frame = lambda i: ai[i] if i in ai else _frame(video.get_ai_frame(i), dev)
    for _, idx, refs, kv_refs, drop in generation_plan(history, num_ref_for_generation):
        flow, conf = pdcnet.multiple_to_one_device(video, refs, idx)
        prev, prev_pos = None, None
        if mode == "both" and idx > 0 and (idx - 1) not in refs and video.generated(idx - 1):          # :878
            prev, prev_pos = ai_frame(idx - 1), sorted(refs + [idx - 1]).index(idx - 1)                 # VideoFrameIndices.add sorts (:921)
        frame, kv = renderer.generate_ai_frame_with_ref(flow, conf, [ai_frame(r) for r in refs], _frame(video.get_raw_frame(idx), dev),
                                                        mode, reference_kv=[kv_map[r] for r in kv_refs], prev_ai_frame=prev, prev_position=prev_pos,
                                                        ds=ds)
        put(idx, frame, kv)
        if drop is not None:
            del kv_map[drop]
            if persist_kv:
                video.remove_kv(drop)
    pdcnet.purge()
    return kv_map
