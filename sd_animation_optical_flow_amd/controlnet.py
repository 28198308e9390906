"""The reference's ControlNet on the device: hint stem, trunk, zero convolutions and the mixing of several nets.

    ControlNet.__init__ / forward          controlnet.py:65-322
    input_hint_block                       controlnet.py:164-180
    SingleControlNet                       controlnet.py:326-335
    extract_control (the tensor half)      controlnet.py:342-370   -> `make_hint`
    get_controlnet_instance (the config)   controlnet.py:376-390   -> `SD_V15_CONTROLNET`
    apply_multi_controlnet                 controlnet.py:412-432

The trunk is the encoder half of the UNet -- `unet_layout(cfg)["input"]` and `["middle"]`, with identical state-dict keys -- and
runs through the code `UNetModel` runs (`unet.UNetTrunk`: the weight loading, `emb_projections`, `resblock`, `_block`, the input
checks both share; loading and packing themselves are `modelbase`'s).  What is ControlNet's own:
  * the hint stem, eight 3x3 convolutions with nn.SiLU between them (strides 1,1,2,1,2,1,2,1; 8x down): one `ops.conv3x3_silu`
    launch per layer (csrc/controlnet.hip), the last with silu=False.  The 3-channel hint is padded to 4 channels that meet zero
    weights (`ops.pack_conv_weight`).
  * `h += guided_hint` (:311-314) is the `addend` of `input_blocks.0.0`'s epilogue when the hint's batch equals x's.  A hint of
    batch 1 is legal: the stem runs once and its output is added to every image of x with one broadcast torch add.  The reference
    does this for model == 'inpaint' (:367), and its `einops.repeat(n=2)` of one edge map (:346, :351) is the same thing computed
    twice.
  * the 1x1 `zero_convs` / `middle_block_out` are `conv2d_nhwc` launches; the residuals leave as NCHW, `len(input_blocks) + 1` of
    them: exactly what `UNetModel.forward(control=)` takes.

`apply_multi_controlnet` mixes with torch: `controls[i] = result_0[i] * w_0`, then `controls[i].add_(result_n[i], alpha=w_n)` --
13 small maps per net, once per sampler step; no kernel of its own.  One deliberate difference from the reference: there
`c.net is None` triggers loading a checkpoint by model name and computing the residuals (:414-419); here `c.net` is a `ControlNet`
(or any callable with its `forward` signature) the caller built, and the residuals are computed when `c.result is None`.

The 'canny' detector is `canny_condition`: `cv2.Canny` on a grey or colour frame through `ops.canny` (csrc/keyframe.hip), the edge
map staying on the device.  `ControlSchedule` carries the nets' guidance windows into the sampler's loop.

Not built: `apply_hed` (its module is missing from the reference tree), loading a checkpoint by model name, and everything
`unet._check_cfg` refuses (dims != 2 among it).

OFX_CNET_TORCH_GLUE=1 in the environment (read once per process; the A/B baseline and a diagnostic): the hint stem through
torch.nn.functional.conv2d + F.silu on NCHW.  The trunk is unaffected.

No checkpoint ships with the reference tree: parity is pinned with seeded weights loaded into the reference's own module
(tests/golden/make_golden_controlnet.py).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .modelbase import env_flag, is_f32_cuda, pad_channels4, random_tensors, wb
from .unet import UNetTrunk, route_reference_kv, unet_layout, unet_tensors

# the arguments of `get_controlnet_instance` (controlnet.py:376-390)
SD_V15_CONTROLNET = dict(in_channels=4, hint_channels=3, model_channels=320, attention_resolutions=(4, 2, 1), num_res_blocks=2,
                         channel_mult=(1, 2, 4, 4), num_heads=8, transformer_depth=1, context_dim=768, legacy=False)

# `input_hint_block` (:164-180) as (index in the Sequential, output channels or None = model_channels, stride); SiLU after all but the last
HINT_STEM = ((0, 16, 1), (2, 16, 1), (4, 32, 2), (6, 32, 1), (8, 96, 2), (10, 96, 1), (12, 256, 2), (14, None, 1))
HINT_SCALE = 8                 # the stem's three stride-2 layers: the hint is 8x the latent (the VAE's factor)


def controlnet_layout(cfg: dict = SD_V15_CONTROLNET) -> Dict[str, object]:
    """`unet_layout` of the same arguments without its output half, plus "hint": the stem as (name, cin, cout, stride) and "zero":
    the 1x1 convolutions as (name, channels), `middle_block_out` last.  `out_channels` is not a ControlNet argument; the UNet
    layout is asked with a placeholder and its "output" is dropped."""
    if "hint_channels" not in cfg:
        raise KeyError("ControlNet cfg lacks hint_channels")
    lay = unet_layout(dict(cfg, out_channels=cfg.get("out_channels", cfg.get("in_channels"))))
    c = lay["cfg"]
    hint, cin = [], int(c["hint_channels"])
    for idx, cout, stride in HINT_STEM:
        cout = int(c["model_channels"]) if cout is None else cout
        hint.append((f"input_hint_block.{idx}", cin, cout, stride))
        cin = cout
    zero = [(f"zero_convs.{i}.0", ch) for i, ch in enumerate(lay["skip"])] + [("middle_block_out.0", lay["skip"][-1])]
    return dict(input=lay["input"], middle=lay["middle"], skip=lay["skip"], cfg=c, hint=hint, zero=zero)


def controlnet_tensors(cfg: dict = SD_V15_CONTROLNET) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of every tensor of the reference's `ControlNet(**cfg, use_spatial_transformer=True)` in the module's own order
    (time_embed, input_blocks, zero_convs, input_hint_block, middle_block, middle_block_out), without a prefix.  Needs no device."""
    lay = controlnet_layout(cfg)
    trunk = unet_tensors(lay["cfg"])
    part = lambda p: [(k, s) for k, s in trunk if k.startswith(p)]
    out = part("time_embed.") + part("input_blocks.")
    for name, ch in lay["zero"][:-1]:
        wb(out, name, ch, ch, 1, 1)
    for name, cin, cout, _ in lay["hint"]:
        wb(out, name, cout, cin, 3, 3)
    out += part("middle_block.")
    wb(out, lay["zero"][-1][0], lay["zero"][-1][1], lay["zero"][-1][1], 1, 1)
    return out


def random_controlnet_state_dict(seed: int, cfg: dict = SD_V15_CONTROLNET) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for the absent checkpoints, built like `random_unet_state_dict`: fan-in-scaled normal weights, norm scales
    around 1, small biases.  The convolutions the reference wraps in `zero_module` (`zero_convs.*`, `input_hint_block.14`,
    `middle_block_out`, and the trunk's `out_layers.3` / `proj_out`) are NOT zeroed: zeroed, every residual would be zero (the
    reason unet.py gives)."""
    return random_tensors(controlnet_tensors(cfg), int(seed) + 49979687)


def _torch_glue() -> bool:
    """OFX_CNET_TORCH_GLUE=1 (A/B baseline and diagnostic, read once per process): the hint stem through torch.nn.functional."""
    return env_flag("OFX_CNET_TORCH_GLUE")


class ControlNet(UNetTrunk):
    """`controlnet.ControlNet` (inference) on a HIP device.  `precision` / `attention_precision` are the trunk's, as in `UNetModel`;
    the hint stem is exact fp32 in every mode.  `kv_dtype` is the trunk's too: checked and handed to the transformers, whose K/V a
    ControlNet records and drops (it takes no reference K/V and returns none).  `weight_dtype` ("fp32" default, "fp16" with
    precision="fp16" only) stores the trunk's and the zero convolutions' operands in half, as in `UNetModel`; the hint stem's
    weights stay fp32."""
    _what = "ControlNet"
    _fp32_weight_prefixes = ("input_hint_block.",)               # `ops.conv3x3_silu`, exact fp32 in every mode

    @staticmethod
    def _layout(cfg):
        return controlnet_layout(cfg)

    @staticmethod
    def _tensors(c):
        return controlnet_tensors(c)

    def _trunk_layers(self) -> List[tuple]:
        return [l for blk in self.layout["input"] for l in blk] + list(self.layout["middle"])

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: dict = SD_V15_CONTROLNET, device="cuda", prefix: str = "control_model.",
                 precision: str = "fp32", attention_precision: str = "fp32", kv_dtype: str = "fp32", weight_dtype: str = "fp32"):
        t32 = self._setup(state_dict, cfg, device, prefix, precision, attention_precision, kv_dtype, weight_dtype)
        self.hint_channels = int(self.cfg["hint_channels"])
        self.hint_pad = (self.hint_channels + 3) // 4 * 4
        self.stem_glue = _torch_glue()
        if self.stem_glue:                                         # the checkpoint's own OIHW weights for F.conv2d
            for name, _, _, _ in self.layout["hint"]:
                self.w[f"{name}.weight.oihw"] = t32[f"{name}.weight"].contiguous().to(self.device)

    # ---- the hint stem ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def hint_stem(self, hint: torch.Tensor) -> torch.Tensor:
        """`input_hint_block` (:164-180, :305): hint f32 [b,hint_channels,8h,8w] on the device -> guided_hint [b,h,w,model_channels]
        NHWC."""
        if not is_f32_cuda(hint, 4) or hint.shape[1] != self.hint_channels:
            raise RuntimeError(f"hint must be a CUDA float32 tensor [b,{self.hint_channels},H,W]")
        if self.stem_glue:
            g = hint
            for i, (name, _, _, stride) in enumerate(self.layout["hint"]):
                g = F.conv2d(g, self.w[f"{name}.weight.oihw"], self.w[f"{name}.bias"], stride=stride, padding=1)
                if i != len(self.layout["hint"]) - 1:
                    g = F.silu(g)
            return g.permute(0, 2, 3, 1).contiguous()
        g = pad_channels4(hint.permute(0, 2, 3, 1), self.hint_channels)
        for i, (name, _, cout, stride) in enumerate(self.layout["hint"]):
            g = ops.conv3x3_silu(g, self.w[f"{name}.weight"], self.w[f"{name}.bias"], cout, stride=stride,
                                 silu=i != len(self.layout["hint"]) - 1)
        return g

    def _check_inputs(self, x, hint, timesteps, context):
        """Every check that needs no launch."""
        if not is_f32_cuda(x, 4) or x.shape[1] != self.in_channels:
            raise RuntimeError(f"x must be a CUDA float32 tensor [B,{self.in_channels},H,W]")
        B, _, H, W = x.shape
        if not is_f32_cuda(hint, 4) or hint.shape[1] != self.hint_channels or hint.shape[0] not in (1, B):
            raise RuntimeError(f"hint must be a CUDA float32 tensor [1 or {B},{self.hint_channels},H,W]")
        if H % self.divisor or W % self.divisor:
            raise ValueError(f"the latent's H and W must be multiples of {self.divisor}, got {H}x{W}")
        if tuple(hint.shape[2:]) != (HINT_SCALE * H, HINT_SCALE * W):
            raise ValueError(f"the hint must be {HINT_SCALE}x the latent: {HINT_SCALE * H}x{HINT_SCALE * W} for a {H}x{W} latent, got "
                             f"{hint.shape[2]}x{hint.shape[3]} (the reference fails in h += guided_hint)")
        self._check_common(B, H, W, timesteps, context)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, hint: torch.Tensor, timesteps: torch.Tensor, context: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """ControlNet.forward (:301-322): x f32 [B,in_channels,H,W] on the device, hint [B or 1,hint_channels,8H,8W], timesteps [B],
        context [B,M,context_dim] -> len(input_blocks) + 1 NCHW fp32 device tensors, the `control` of `UNetModel.forward`.  H and W
        must be multiples of 2 ** (len(channel_mult) - 1) and the hint 8x the latent (ValueError before any launch)."""
        self._check_inputs(x, hint, timesteps, context)
        B = x.shape[0]
        guided = self.hint_stem(hint)
        h = pad_channels4(x.permute(0, 2, 3, 1), self.in_channels)
        emb_all = self.emb_projections(timesteps)
        ref_by_st = route_reference_kv((), self.n_transformers)
        kv_hists: list = []
        outs = []
        zero = self.layout["zero"]
        for i, blk in enumerate(self.layout["input"]):                                 # :310-317
            if i == 0:
                if guided.shape[0] == B:
                    h = self._conv(blk[0][1], h, 3, addend=guided)                     # h += guided_hint in the epilogue
                else:
                    h = self._conv(blk[0][1], h, 3)
                    h += guided                                                        # one hint for the whole batch
            else:
                h = self._block(blk, h, emb_all, context, ref_by_st, kv_hists)
            outs.append(self._conv(zero[i][0], h, 1).permute(0, 3, 1, 2).contiguous())
        h = self._block(self.layout["middle"], h, emb_all, context, ref_by_st, kv_hists)     # :319
        outs.append(self._conv(zero[-1][0], h, 1).permute(0, 3, 1, 2).contiguous())          # :320
        return outs

    __call__ = forward


@dataclass
class SingleControlNet:
    """controlnet.py:326-335, field for field.  `net`: a `ControlNet` the caller built (the reference fills it by model name);
    `result`: the residuals `apply_multi_controlnet` caches on first use."""
    weight: float
    model: str
    args: dict
    condition: np.ndarray
    guidance_start: float = 0
    guidance_end: float = 1
    result: Optional[Any] = None
    net: Optional[Any] = None


def make_hint(model: str, condition, args: Optional[dict] = None, device="cuda") -> torch.Tensor:
    """The tensor half of `extract_control` (:342-370): the hint of one condition image, f32 [1,3,H,W] on `device`.
        'canny' / 'hed'   condition u8 [H,W], an edge map   -> three equal channels of v / 255
        'inpaint'         condition u8 [H,W,3] and args['mask'] u8 [H,W]   -> -1.0 where mask > 127, else v / 255
    Batch 1: `ControlNet.forward` broadcasts it (the reference repeats an edge map to n = 2 and stacks one inpaint map).  The
    edge map of 'canny' comes from `canny_condition` (`cv2.Canny` on the frame with args' thresholds); `apply_hed`, whose module is
    missing from the reference tree, is not built.  Plain torch ops: once per frame."""
    cond = torch.as_tensor(np.ascontiguousarray(condition) if isinstance(condition, np.ndarray) else condition)
    if cond.dtype != torch.uint8:
        raise ValueError(f"make_hint: the condition must be uint8, got {cond.dtype}")
    if model in ("canny", "hed"):
        if cond.dim() != 2:
            raise ValueError(f"make_hint: a {model} condition is an edge map [H,W], got {tuple(cond.shape)}")
        v = cond.to(device).float() / 255.0
        return v[None, None].expand(1, 3, -1, -1).contiguous()
    if model == "inpaint":
        if cond.dim() != 3 or cond.shape[2] != 3:
            raise ValueError(f"make_hint: an inpaint condition is an image [H,W,3], got {tuple(cond.shape)}")
        if not args or "mask" not in args:
            raise KeyError("make_hint: model 'inpaint' needs args['mask']")
        mask = torch.as_tensor(np.ascontiguousarray(args["mask"]) if isinstance(args["mask"], np.ndarray) else args["mask"])
        if tuple(mask.shape) != tuple(cond.shape[:2]):
            raise ValueError(f"make_hint: mask {tuple(mask.shape)} does not match the image {tuple(cond.shape[:2])}")
        v = cond.to(device).float()
        v[mask.to(device) > 127] = -255.0                          # :363: -1 after the division is the inpaint value
        return (v / 255.0).permute(2, 0, 1)[None].contiguous()
    raise NotImplementedError(f"make_hint: model {model!r} is not built (the reference builds 'canny', 'hed' and 'inpaint')")


def canny_condition(frame, low_threshold, high_threshold, device="cuda") -> torch.Tensor:
    """The detector half of `extract_control` for 'canny' (:343-347): `cv2.Canny(frame, low_threshold, high_threshold)` through
    `ops.canny`.  frame u8 [H,W] or [H,W,3] (cv2 channel order), numpy or tensor -> the edge map u8 [H,W] on `device`, 255 or 0:
    what `SingleControlNet.condition` and `make_hint('canny', ...)` take.  A frame already on the device is not copied."""
    f = torch.as_tensor(np.ascontiguousarray(frame) if isinstance(frame, np.ndarray) else frame)
    if f.dtype != torch.uint8 or f.dim() not in (2, 3) or (f.dim() == 3 and f.shape[2] != 3):
        raise ValueError(f"canny_condition: the frame must be uint8 [H,W] or [H,W,3], got {f.dtype} {tuple(f.shape)}")
    return ops.canny(f.to(device).contiguous()[None], low_threshold, high_threshold)[0]


def control_weight(c: SingleControlNet, denoise_percentage: float) -> float:
    """:423-424: the net's weight, 0 outside [guidance_start, guidance_end] (both ends inclusive)."""
    return 0.0 if denoise_percentage < c.guidance_start or denoise_percentage > c.guidance_end else float(c.weight)


def check_control_nets(control_nets: Sequence[SingleControlNet], B: int, C: int, H: int, W: int, timesteps: torch.Tensor, context_dim: int) -> None:
    """What the first `apply_multi_controlnet` of a frame would reject, checked without a launch: every net is set and takes a
    [B,C,H,W] latent with a [B,M,context_dim] context, and every condition is a uint8 image 8x the latent that `make_hint` knows
    how to turn into a hint.  For callers (`GuidedDDIMSampler.decode`) that promise their checks before any GPU work."""
    for c in control_nets:
        what = f"SingleControlNet(model={c.model!r})"
        if c.net is None:
            raise ValueError(f"{what}.net is None: build a ControlNet and set it (checkpoints are not loaded by model name)")
        if c.model not in ("canny", "hed", "inpaint"):
            raise NotImplementedError(f"{what}: make_hint builds 'canny', 'hed' and 'inpaint'")
        shape, dtype = tuple(getattr(c.condition, "shape", ())), str(getattr(c.condition, "dtype", ""))
        want = (HINT_SCALE * H, HINT_SCALE * W) + ((3,) if c.model == "inpaint" else ())
        if shape != want or not dtype.endswith("uint8"):
            raise ValueError(f"{what}: the condition must be uint8 {want} for a {H}x{W} latent, got {dtype or type(c.condition).__name__} {shape}")
        if c.model == "inpaint" and (not c.args or "mask" not in c.args):
            raise KeyError(f"{what} needs args['mask']")
        net = c.net
        if net.in_channels != C or int(net.cfg["context_dim"]) != int(context_dim):
            raise ValueError(f"{what}: the net takes {net.in_channels} latent channels and a context of width {net.cfg['context_dim']}; "
                             f"the sampler has {C} and {context_dim}")
        if H % net.divisor or W % net.divisor:
            raise ValueError(f"{what}: the latent's H and W must be multiples of {net.divisor}, got {H}x{W}")
        net._check_common(B, H, W, timesteps, None)


@torch.no_grad()
def apply_multi_controlnet(x_noisy: torch.Tensor, t: torch.Tensor, cond_txt: Optional[torch.Tensor], denoise_percentage: float,
                           control_nets: Sequence[SingleControlNet]) -> List[torch.Tensor]:
    """controlnet.py:412-432: `sum_n weight_n(p) * result_n[i]` per residual i.  A net's residuals are computed on first use --
    `c.net(x_noisy, make_hint(c.model, c.condition, c.args), t, cond_txt)` -- and cached in `c.result` (when `c.result is None`; the
    reference tests `c.net is None`, module docstring); later calls run no net.  The returned list is fresh: nothing in it aliases a
    cached result, so it can be handed to `UNetModel.forward(control=)` / `GuidedDDIMSampler.decode(control=)` and written to."""
    if not control_nets:
        raise ValueError("apply_multi_controlnet: no control nets")
    for c in control_nets:
        if c.result is None:
            if c.net is None:
                raise ValueError(f"SingleControlNet(model={c.model!r}).net is None: build a ControlNet and set it (checkpoints are "
                                 "not loaded by model name)")
            c.result = list(c.net(x_noisy, make_hint(c.model, c.condition, c.args, device=x_noisy.device), t, cond_txt))
    n = len(control_nets[0].result)
    if any(len(c.result) != n for c in control_nets):
        raise ValueError("apply_multi_controlnet: the nets return different numbers of residuals")
    w0 = control_weight(control_nets[0], denoise_percentage)
    controls = [r * w0 for r in control_nets[0].result]
    for c in control_nets[1:]:
        w = control_weight(c, denoise_percentage)
        for i, r in enumerate(c.result):
            controls[i].add_(r, alpha=w)
    return controls


class ControlSchedule:
    """The guidance windows of `apply_multi_controlnet` inside the sampler's loop: a callable `control(i, p)` for
    `GuidedDDIMSampler.decode(control=)`.  Its value at iteration i is `apply_multi_controlnet`'s mix of the nets' cached `result`s at
    the loop's denoise percentage p, or None when every weight is 0 there.  The mix is recomputed only when the tuple of
    `control_weight(c, p)` changes, so a window that closes costs one mix, not one per step; `mixes` counts them.  Every net must
    hold a `result` (ValueError): the caller runs `apply_multi_controlnet` once per frame, which computes and caches them."""

    def __init__(self, nets: Sequence[SingleControlNet]):
        self.nets = list(nets)
        if not self.nets:
            raise ValueError("ControlSchedule: no control nets")
        for c in self.nets:
            if c.result is None:
                raise ValueError(f"ControlSchedule: SingleControlNet(model={c.model!r}) has no cached result: run "
                                 "apply_multi_controlnet once for this frame first")
        self.mixes = 0
        self._weights: Optional[Tuple[float, ...]] = None
        self._value: Optional[List[torch.Tensor]] = None

    def __call__(self, i: int, p: float) -> Optional[List[torch.Tensor]]:
        weights = tuple(control_weight(c, p) for c in self.nets)
        if weights != self._weights:
            self._weights = weights
            if any(weights):
                self._value = apply_multi_controlnet(None, None, None, p, self.nets)     # every result is cached: no net runs
                self.mixes += 1
            else:
                self._value = None
        return self._value
