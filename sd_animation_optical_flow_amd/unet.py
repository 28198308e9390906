"""The reference's UNet on the device: `UNetModel` / `ControlledUnetModel` with the K/V history of every transformer threaded through.

    UNetModel.__init__ / forward            ldm/modules/diffusionmodules/openaimodel.py:445-739, :757-793
    ControlledUnetModel.forward             controlnet.py:29-62   (`control` residuals, `reference_kv`)
    TimestepEmbedSequential.forward         openaimodel.py:79-90  (entry i of every reference frame goes to transformer i)
    ResBlock._forward                       openaimodel.py:257-277
    Upsample / Downsample                   openaimodel.py:93-162
    timestep_embedding                      ldm/modules/diffusionmodules/util.py:154-174

Everything runs through the C ABI of libofx.so on NHWC fp32; NCHW appears only at the two edges of `forward`.  Nothing is
concatenated or permuted in between:
  * `th.cat([h, hs.pop()], dim=1)` (:786) is never formed.  The GroupNorm behind it reads the two maps through two pointers
    (`ops.groupnorm_cat`; in the v1.5 model the groups straddle the seam, so the maps cannot be normalised separately), and the 1x1
    `skip_connection` reads them as the two channel segments of one convolution (`conv2d_nhwc(x2=)`).
  * `h = h + emb_out` (:275) is never written.  The GroupNorm that follows takes the per-image, per-channel term into its
    statistics and its shift in float64 (`ops.groupnorm_cat(e=)`).
  * The timestep path is one `ops.timestep_embedding`, two `ops.emb_linear` for `time_embed` and ONE `ops.emb_linear` over the
    row-concatenation of every ResBlock's `emb_layers.1` weight, built at load; each ResBlock reads its column slice in place.
  * Every 3x3 / 1x1 / stride-2 convolution is a direct `ofx_conv2d` with bias (and the residual sum) in the epilogue, `Upsample` is
    `ops.upconv2x` (nearest 2x + 3x3 in one launch) with weights folded at load, every transformer is `SpatialTransformer`.

Two deliberate differences from the reference:
  * The caller's `reference_kv` and `control` lists are not consumed (the reference `pop(0)`s / `pop()`s them, :86, controlnet.py
    :50,56) and `control` tensors are not written to.
  * `reference_kv` is honoured when `control is None`.  The reference drops it there: controlnet.py:31-32 forwards to the base
    class, whose `forward` never passes it on.

Not built (NotImplementedError): use_scale_shift_norm, resblock_updown, num_classes, use_linear_in_transformer, AttentionBlock
(use_spatial_transformer=False), conv_resample=False, dims != 2.

`UNetModel(precision=)` ("fp32" default, "fp16", "bf16x3", "bf16x6"; `model.precision`) is the arithmetic of every `ofx_conv2d`
of the model: the 3x3, 1x1 and stride-2 convolutions, `skip_connection`, and through `SpatialTransformer(precision=)` `proj_in` /
`proj_out`, the q / k / v / out projections and the feed-forward GEMMs.  "fp16" is the reference's own mode for this stage (it runs
under torch.autocast): both operands of a contraction rounded to half as the kernel stages them, one product on the fp16 matrix
cores, fp32 accumulation.  These stay fp32 in every precision: `ops.upconv2x` (Upsample), attention and its softmax, GroupNorm,
LayerNorm, GEGLU, the timestep path (`ops.timestep_embedding`, `ops.emb_linear`), every weight and every activation in memory --
so the model is closer to float64 than autocast, which also rounds each layer's output to half and runs attention in half.
"bf16x3" / "bf16x6" are the launcher's split-bf16 kernels on the fly.  The default is bit for bit what the model computed before
the argument existed.

OFX_UNET_TORCH_GLUE=1 in the environment (read once per process; the A/B baseline and a diagnostic): the composition that was
possible before `groupnorm_cat` / `emb_linear` / `timestep_embedding` existed -- `torch.cat` + `ops.groupnorm`, the emb term as a
torch broadcast add, the timestep path through torch.nn.functional.

`UNetTrunk` is the part of the model `controlnet.ControlNet` shares: weight loading, the timestep path, `resblock`, `_block`.
The checkpoint check, the packing of the weights, `_conv` and the seeded stand-in weights are `modelbase`'s, shared with the other
SD-stage models; the `.folded` upsample operands and the side-by-side `emb_layers` are this module's own.

No checkpoint ships with the reference tree: parity is pinned with seeded weights loaded into the reference's own module
(tests/golden/make_golden_unet.py).
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import ops
from .modelbase import DeviceModel, check_activation_bytes, check_weight_dtype, env_flag, is_f32_cuda, load_tensors, pad_channels4, random_tensors, wb
from .transformer import FUSED_HEAD_SIZES, MODEL_PRECISIONS, SpatialTransformer, check_precision, plan_reference_kv, spatial_transformer_tensors

# `unet_config` of guided_ldm_inpaint_v15.yaml (in_channels 9) / guided_ldm_v15.yaml (in_channels 4)
SD_V15_UNET = dict(in_channels=9, out_channels=4, model_channels=320, attention_resolutions=(4, 2, 1), num_res_blocks=2,
                   channel_mult=(1, 2, 4, 4), num_heads=8, transformer_depth=1, context_dim=768, legacy=False)

_UNSUPPORTED = (("use_scale_shift_norm", False), ("resblock_updown", False), ("num_classes", None), ("use_linear_in_transformer", False),
                ("use_spatial_transformer", True), ("conv_resample", True), ("dims", 2))


def _check_cfg(cfg: dict) -> dict:
    for key, want in _UNSUPPORTED:
        if cfg.get(key, want) != want:
            raise NotImplementedError(f"UNetModel: {key}={cfg[key]!r} is not built (only {key}={want!r}, what guided_ldm_*_v15.yaml uses)")
    c = dict(cfg)
    for key in ("in_channels", "out_channels", "model_channels", "attention_resolutions", "num_res_blocks", "channel_mult", "context_dim"):
        if key not in c:
            raise KeyError(f"UNetModel cfg lacks {key}")
    if c.get("num_head_channels", -1) == -1 and c.get("num_heads", -1) == -1:
        raise ValueError("either num_heads or num_head_channels has to be set")          # openaimodel.py:489-493
    if not isinstance(c["num_res_blocks"], int) or not isinstance(c["context_dim"], int):
        raise NotImplementedError("per-level num_res_blocks and a list of context dimensions are not built")
    for key in ("disable_self_attentions", "num_attention_blocks", "n_embed"):
        if c.get(key) is not None:
            raise NotImplementedError(f"UNetModel: {key} is not built")
    if c.get("disable_middle_self_attn", False) or c.get("use_fp16", False):
        raise NotImplementedError("UNetModel: disable_middle_self_attn / use_fp16 are not built")
    c.setdefault("transformer_depth", 1)
    return c


def unet_layout(cfg: dict = SD_V15_UNET) -> Dict[str, object]:
    """The module tree `UNetModel.__init__` builds (openaimodel.py:545-733) as plain data.  "input" / "middle" / "output": blocks
    (`TimestepEmbedSequential`s) as lists of layers, a layer being a tuple
        ("conv", name, cin, cout) | ("res", name, cin, cout) | ("st", name, channels, heads, d_head) | ("down", name, ch) | ("up", name, ch)
    with `name` the state-dict prefix without the trailing dot; "skip": the channels of `hs` in push order."""
    c = _check_cfg(cfg)
    mc, mult, nres = int(c["model_channels"]), tuple(c["channel_mult"]), int(c["num_res_blocks"])
    att = tuple(int(a) for a in c["attention_resolutions"])
    heads0, hch = int(c.get("num_heads", -1)), int(c.get("num_head_channels", -1))

    def st(name, ch):
        heads = heads0 if hch == -1 else ch // hch               # :571-578 (legacy and not: dim_head = ch // num_heads)
        return ("st", name, ch, heads, ch // heads)

    inp: List[List[tuple]] = [[("conv", "input_blocks.0.0", int(c["in_channels"]), mc)]]
    chans, ch, ds = [mc], mc, 1
    for level, m in enumerate(mult):
        for _ in range(nres):
            i = len(inp)
            layers = [("res", f"input_blocks.{i}.0", ch, m * mc)]
            ch = m * mc
            if ds in att:
                layers.append(st(f"input_blocks.{i}.1", ch))
            inp.append(layers)
            chans.append(ch)
        if level != len(mult) - 1:
            inp.append([("down", f"input_blocks.{len(inp)}.0", ch)])
            chans.append(ch)
            ds *= 2
    mid = [("res", "middle_block.0", ch, ch), st("middle_block.1", ch), ("res", "middle_block.2", ch, ch)]
    out: List[List[tuple]] = []
    skips = list(chans)
    for level, m in list(enumerate(mult))[::-1]:
        for i in range(nres + 1):
            ich = skips.pop()
            j = len(out)
            layers = [("res", f"output_blocks.{j}.0", ch + ich, mc * m, ch, ich)]
            ch = mc * m
            if ds in att:
                layers.append(st(f"output_blocks.{j}.{len(layers)}", ch))
            if level and i == nres:
                layers.append(("up", f"output_blocks.{j}.{len(layers)}", ch))
                ds //= 2
            out.append(layers)
    return dict(input=inp, middle=mid, output=out, skip=chans, cfg=c)


def _layers(lay) -> List[tuple]:
    return [l for blk in lay["input"] for l in blk] + list(lay["middle"]) + [l for blk in lay["output"] for l in blk]


def unet_tensors(cfg: dict = SD_V15_UNET) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of every tensor of the reference's `UNetModel(**cfg, use_spatial_transformer=True)` in the module's own order
    (time_embed, input_blocks, middle_block, output_blocks, out), without a prefix."""
    lay = unet_layout(cfg)
    c = lay["cfg"]
    mc, ted = int(c["model_channels"]), 4 * int(c["model_channels"])
    out: List[Tuple[str, Tuple[int, ...]]] = []
    wb(out, "time_embed.0", ted, mc)
    wb(out, "time_embed.2", ted, ted)
    for l in _layers(lay):
        kind, name = l[0], l[1]
        if kind == "conv":
            wb(out, name, l[3], l[2], 3, 3)
        elif kind == "res":
            cin, cout = l[2], l[3]
            wb(out, f"{name}.in_layers.0", cin)
            wb(out, f"{name}.in_layers.2", cout, cin, 3, 3)
            wb(out, f"{name}.emb_layers.1", cout, ted)
            wb(out, f"{name}.out_layers.0", cout)
            wb(out, f"{name}.out_layers.3", cout, cout, 3, 3)
            if cin != cout:
                wb(out, f"{name}.skip_connection", cout, cin, 1, 1)
        elif kind == "st":
            out.extend((f"{name}.{k}", s) for k, s in
                       spatial_transformer_tensors(l[2], l[3], l[4], int(c["context_dim"]), int(c["transformer_depth"])))
        elif kind == "down":
            wb(out, f"{name}.op", l[2], l[2], 3, 3)
        else:
            wb(out, f"{name}.conv", l[2], l[2], 3, 3)
    wb(out, "out.0", mc)
    wb(out, "out.2", int(c["out_channels"]), mc, 3, 3)
    return out


def random_unet_state_dict(seed: int, cfg: dict = SD_V15_UNET) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for the absent checkpoint: fan-in-scaled normal weights, norm scales around 1, small biases.  The
    convolutions the reference wraps in `zero_module` (`out_layers.3`, `out.2`, every `proj_out`) are NOT zeroed: zeroed, every
    ResBlock and transformer would be the identity and the model's output zero (the reason transformer.py gives)."""
    return random_tensors(unet_tensors(cfg), int(seed) + 32452843)


def _torch_glue() -> bool:
    """OFX_UNET_TORCH_GLUE=1 (A/B baseline and diagnostic, read once per process): torch.cat + `ops.groupnorm`, the emb term as a
    torch broadcast add, the timestep path through torch.nn.functional."""
    return env_flag("OFX_UNET_TORCH_GLUE")


def route_reference_kv(reference_kv, n_transformers: int) -> List[list]:
    """`TimestepEmbedSequential.forward` (:85-86) without the pops: reference_kv is a sequence over reference frames, each a
    sequence of one (k, v) per transformer in UNet order (input blocks, middle, output blocks) -> per transformer, the list of that
    transformer's (k, v) of every frame.  A wrong entry count is a ValueError.  Needs no device."""
    frames = [list(f) for f in (reference_kv or ())]
    for i, f in enumerate(frames):
        if len(f) != n_transformers:
            raise ValueError(f"reference_kv[{i}] has {len(f)} entries, the UNet has {n_transformers} transformers")
        for j, e in enumerate(f):
            if not isinstance(e, (tuple, list)) or len(e) not in (2, 3):
                raise ValueError(f"reference_kv[{i}][{j}] must be a (k, v) pair")
    return [[(f[j][0], f[j][1]) for f in frames] for j in range(n_transformers)]


class UNetTrunk(DeviceModel):
    """What `UNetModel` and `controlnet.ControlNet` share: the checkpoint check and the weight loading (`_setup`, through
    `modelbase`), the checks of what both take (`_check_common`), the timestep path (`emb_projections`), `resblock` and `_block`.
    A subclass names its module tree (`_layout`), its tensors (`_tensors`) and the layers it runs (`_trunk_layers`); ControlNet's
    trunk is the `input` and `middle` halves of the same layout, key for key."""
    _what = "UNet"

    @staticmethod
    def _layout(cfg):
        return unet_layout(cfg)

    @staticmethod
    def _tensors(c):
        return unet_tensors(c)

    _fp32_weight_prefixes: Tuple[str, ...] = ()                   # 4-D weights that no `ofx_conv2d` launch reads, by key prefix

    def _trunk_layers(self) -> List[tuple]:
        return _layers(self.layout)

    def _setup(self, state_dict: Dict[str, torch.Tensor], cfg: dict, device, prefix: str, precision: str,
               attention_precision: str, kv_dtype: str = "fp32", weight_dtype: str = "fp32") -> Dict[str, torch.Tensor]:
        """Everything `__init__` does; -> the checked fp32 CPU tensors by key (for what a subclass loads beyond `self.w`)."""
        self.precision = check_precision(precision)                # before the checkpoint is looked at or a device asked for
        self.weight_dtype = check_weight_dtype(weight_dtype, self.precision)   # storage of the conv / GEMM operands (`DeviceModel`)
        self.attention_precision = ops.check_attention_precision(attention_precision, "attention_precision")
        self.kv_dtype = ops.check_kv_dtype(kv_dtype)               # the dtype of the returned kv_hists (`SpatialTransformer(kv_dtype=)`)
        self.layout = self._layout(cfg)
        self.cfg = self.layout["cfg"]
        c = self.cfg
        mc = int(c["model_channels"])
        if mc % 32 or any((int(m) * mc) % 32 for m in c["channel_mult"]):
            raise ValueError("model_channels and every level's channels must be multiples of 32 (GroupNorm(32); the two channel "
                             "segments of a skip convolution)")
        layers = self._trunk_layers()
        for l in layers:
            if l[0] == "res" and len(l) == 6 and l[2] == l[3]:
                raise NotImplementedError(f"{l[1]}: an identity skip over a concatenation is not built")
        t32 = load_tensors(state_dict, self._tensors(c), prefix, self._what)   # the checkpoint is checked before the device is asked for
        self._use_device(device)
        self.in_channels, self.out_channels, self.model_channels = int(c["in_channels"]), int(c["out_channels"]), mc
        self.in_pad = (self.in_channels + 3) // 4 * 4
        self.divisor = 2 ** (len(c["channel_mult"]) - 1)
        self.st: Dict[str, SpatialTransformer] = {}
        emb_w, emb_b, off = [], [], 0
        self.emb_slice: Dict[str, Tuple[int, int]] = {}            # ResBlock name -> (first column, columns) of the emb projections
        for l in layers:
            kind, name = l[0], l[1]
            if kind == "st":
                sub = {k[len(name) + 1:]: v for k, v in t32.items() if k.startswith(name + ".")}
                # the fp16 attention kernel exists for the fused head sizes only (all 16 transformers of SD v1.5: 40 / 80 / 160).  A
                # transformer with another head size keeps fp32 attention, and says so: a warning below, `attention_precision_of`
                ap = self.attention_precision if int(l[4]) in FUSED_HEAD_SIZES else "fp32"
                self.st[name] = SpatialTransformer(sub, l[3], l[4], device=self.device, precision=self.precision, attention_precision=ap,
                                                   kv_dtype=self.kv_dtype, weight_dtype=self.weight_dtype)
            elif kind == "res":
                emb_w.append(t32[f"{name}.emb_layers.1.weight"])
                emb_b.append(t32[f"{name}.emb_layers.1.bias"])
                self.emb_slice[name] = (off, l[3])
                off += l[3]
        self.n_transformers = len(self.st)
        self.st_order = [l for l in layers if l[0] == "st"]
        self.attention_precision_of = {name: st.attention_precision for name, st in self.st.items()}
        kept = [name for name, ap in self.attention_precision_of.items() if ap != self.attention_precision]
        if kept:
            warnings.warn(f"attention_precision={self.attention_precision!r}: the fused kernel does not take the head size of {kept} "
                          f"(fused: {FUSED_HEAD_SIZES}); their attention stays fp32 ({type(self).__name__}.attention_precision_of)", stacklevel=3)
        for key, t in t32.items():
            if any(key.startswith(n + ".") for n in self.st) or ".emb_layers." in key:
                continue
            # not `ofx_conv2d` operands, fp32 in every `weight_dtype`: Upsample (ofx_upconv2x, fp32 in every precision) and what
            # a subclass names (ControlNet's hint stem)
            self._put(key, t, operand=not (key.endswith(".conv.weight") or key.startswith(self._fp32_weight_prefixes)))
            if key.endswith(".conv.weight"):                                   # Upsample: the four parity-folded 2x2 operands
                self.w[key + ".folded"] = ops.upconv2x_weight(t).to(self.device)
        # every ResBlock's emb_layers.1 as one [sum of Cout, 4 * model_channels] Linear
        self._put("emb_layers.weight", torch.cat(emb_w))
        self._put("emb_layers.bias", torch.cat(emb_b))
        self._put("freqs", ops.timestep_freqs(mc))
        self.torch_glue = _torch_glue()
        return t32

    def _check_common(self, B, H, W, timesteps, context) -> None:
        """The checks of timesteps [B], context [B,M,context_dim] and the widest activation of a BxHxW latent; no launch."""
        if not torch.is_tensor(timesteps) or timesteps.dim() != 1 or timesteps.shape[0] != B:
            raise RuntimeError(f"timesteps must be a tensor [{B}]")
        cd = int(self.cfg["context_dim"])
        if context is not None and (not is_f32_cuda(context, 3) or context.shape[0] != B or context.shape[2] != cd):
            raise RuntimeError(f"context must be a CUDA float32 tensor [{B},M,{cd}]")
        widest = 2 * max(int(m) for m in self.cfg["channel_mult"][:1]) * self.model_channels
        check_activation_bytes(B * H * W * widest * 4,
                               "an activation would pass 2 GiB (32-bit byte offsets in the convolution): slice the batch")

    # ---- building blocks ------------------------------------------------------------------------------------------
    def _norm(self, name: str, x: torch.Tensor, x1: Optional[torch.Tensor] = None, e: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """GroupNorm(32, eps 1e-5) + SiLU (`normalization` = GroupNorm32(32, channels), util.py; nn.SiLU)."""
        g, b = self.w[f"{name}.weight"], self.w[f"{name}.bias"]
        if self.torch_glue:
            if x1 is not None:
                x = torch.cat([x, x1], dim=3)
            if e is not None:
                x = x + e[:, None, None, :]
            return ops.groupnorm(x, g, b, 32, 1e-5, True)
        return ops.groupnorm_cat(x, x1, g, b, e=e, groups=32, eps=1e-5, silu=True, out=out)

    def emb_projections(self, timesteps: torch.Tensor) -> torch.Tensor:
        """timesteps [B] on the device -> [B, sum of Cout]: `emb_layers(time_embed(timestep_embedding(t)))` of every ResBlock side
        by side (:770-771, :266); ResBlock `name` owns the columns `emb_slice[name]`."""
        t = timesteps.to(device=self.device, dtype=torch.float32).contiguous()
        w = self.w
        if self.torch_glue:
            args = t[:, None] * w["freqs"][None]
            te = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
            emb = F.linear(F.silu(F.linear(te, w["time_embed.0.weight"], w["time_embed.0.bias"])), w["time_embed.2.weight"],
                           w["time_embed.2.bias"])
            return F.linear(F.silu(emb), w["emb_layers.weight"], w["emb_layers.bias"])
        te = ops.timestep_embedding(t, w["freqs"], self.model_channels)
        emb = ops.emb_linear(ops.emb_linear(te, w["time_embed.0.weight"], w["time_embed.0.bias"]), w["time_embed.2.weight"],
                             w["time_embed.2.bias"], silu_in=True)
        return ops.emb_linear(emb, w["emb_layers.weight"], w["emb_layers.bias"], silu_in=True)

    def resblock(self, name: str, x: torch.Tensor, emb_all: torch.Tensor, skip: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ResBlock._forward (:257-277) on NHWC: x [B,H,W,C] (and `skip` [B,H,W,C1], the second half of the reference's th.cat),
        emb_all from `emb_projections`."""
        off, cout = self.emb_slice[name]
        e = emb_all[:, off:off + cout]
        h = self._conv(f"{name}.in_layers.2", self._norm(f"{name}.in_layers.0", x, skip), 3)
        h = self._norm(f"{name}.out_layers.0", h, e=e, out=h)                          # h + emb_out folded into the statistics
        if f"{name}.skip_connection.weight" in self.w:
            if self.torch_glue and skip is not None:
                sk = self._conv(f"{name}.skip_connection", torch.cat([x, skip], dim=3), 1)
            else:
                sk = self._conv(f"{name}.skip_connection", x, 1, x2=skip)              # the two maps as two channel segments
        else:
            if skip is not None:
                raise NotImplementedError(f"{name}: an identity skip over a concatenation is not built")
            sk = x
        return self._conv(f"{name}.out_layers.3", h, 3, addend=sk)                     # skip_connection(x) + h in the epilogue

    def _block(self, layers, h, emb_all, context, ref_by_st, kv_hists, skip=None):
        """TimestepEmbedSequential.forward (:79-90)."""
        for l in layers:
            kind, name = l[0], l[1]
            if kind == "conv":
                h = self._conv(name, h, 3)
            elif kind == "res":
                h = self.resblock(name, h, emb_all, skip)
                skip = None
            elif kind == "st":
                h, kv = self.st[name].forward_nhwc(h, context, ref_by_st[len(kv_hists)])
                kv_hists.extend(kv)
            elif kind == "down":
                h = self._conv(f"{name}.op", h, 3, stride=2)                           # Downsample (:136-162): 3x3, stride 2, padding 1
            else:
                h = ops.upconv2x(h, self.w[f"{name}.conv.weight.folded"], self.w[f"{name}.conv.bias"])   # Upsample (:93-121)
        return h


class UNetModel(UNetTrunk):
    """`ldm.modules.diffusionmodules.openaimodel.UNetModel` with `ControlledUnetModel.forward` (inference) on a HIP device.
    `precision`: the arithmetic of the convolutions and GEMMs, one of MODEL_PRECISIONS (module docstring); everything else is fp32,
    unless `attention_precision="fp16"` hands the attention of all the transformers to the fp16 matrix-core kernel
    (`SpatialTransformer(attention_precision=)`; the K/V a transformer records is unchanged by it).  That kernel exists for the head
    sizes 40 / 64 / 80 / 128 / 160 -- all 16 transformers of SD v1.5.  In a configuration with another head size (the test
    configuration u0 has a 192-wide middle head) that transformer keeps fp32 attention: a UserWarning names it at construction and
    `attention_precision_of` maps every transformer to the mode it runs.  A SpatialTransformer built directly raises instead.
    `kv_dtype`: "fp32" (default) or "fp16", the dtype of the returned `kv_hists` (`SpatialTransformer(kv_dtype=)`); histories of
    either dtype are accepted as `reference_kv`, and on the fused route they are attended to in place, unwidened.
    `weight_dtype`: "fp32" (default) or "fp16", with precision="fp16" only (ValueError otherwise): every convolution and GEMM
    operand is stored in half and read as such by the same fp16 kernels -- bit-identical outputs, half the weight bytes
    (`modelbase.DeviceModel` lists what stays fp32)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: dict = SD_V15_UNET, device="cuda", prefix: str = "model.diffusion_model.",
                 precision: str = "fp32", attention_precision: str = "fp32", kv_dtype: str = "fp32", weight_dtype: str = "fp32"):
        self._setup(state_dict, cfg, device, prefix, precision, attention_precision, kv_dtype, weight_dtype)

    def _check_inputs(self, B, H, W, timesteps, context, control, reference_kv):
        """Every check that needs no launch; -> (per-transformer reference K/V, control as NHWC views or None)."""
        if H % self.divisor or W % self.divisor:
            raise ValueError(f"the latent's H and W must be multiples of {self.divisor}, got {H}x{W} (the reference fails in th.cat)")
        self._check_common(B, H, W, timesteps, context)
        ref_by_st = route_reference_kv(reference_kv, self.n_transformers)
        if reference_kv:
            # the shapes each transformer will see, checked here so that a bad entry raises before any launch
            ds, sizes = 1, []
            for blk in self.layout["input"] + [self.layout["middle"]] + self.layout["output"]:
                for l in blk:
                    ds = ds * 2 if l[0] == "down" else ds // 2 if l[0] == "up" else ds
                    if l[0] == "st":
                        sizes.append((H // ds) * (W // ds))
            for l, n, ents in zip(self.st_order, sizes, ref_by_st):
                plan_reference_kv([(tuple(k.shape), tuple(v.shape)) for k, v in ents], B, n, l[3], l[4])
        ctl = None
        if control is not None:
            ctl = list(control)
            nin = len(self.layout["input"])
            if len(ctl) != nin + 1:
                raise ValueError(f"control has {len(ctl)} entries, the UNet takes {nin + 1} (one per input block and the middle block)")
            ds, want = 1, []
            for blk, ch in zip(self.layout["input"], self.layout["skip"]):
                ds = ds * 2 if blk[0][0] == "down" else ds
                want.append((B, ch, H // ds, W // ds))
            want.append(want[-1])
            for i, (t, s) in enumerate(zip(ctl, want)):
                if not is_f32_cuda(t, 4) or tuple(t.shape) != s:
                    raise ValueError(f"control[{i}] must be a CUDA float32 tensor {s}")
            ctl = [t.permute(0, 2, 3, 1) for t in ctl]
        return ref_by_st, ctl

    @torch.no_grad()
    def forward_nhwc(self, x: torch.Tensor, timesteps: torch.Tensor, context: Optional[torch.Tensor] = None, control=None,
                     only_mid_control: bool = False, reference_kv=(), *,
                     padded: bool = False) -> Tuple[torch.Tensor, List[Tuple[torch.Tensor, torch.Tensor]]]:
        """`forward` without the two edge permutes: x f32 [B,H,W,in_channels] on the device -> (eps [B,H,W,out_channels], kv_hists).
        padded=True: x is the first convolution's own operand, [B,H,W,in_pad] contiguous with channels in_channels..in_pad-1 zero
        (the caller's duty; they meet zero weights, but a NaN there would spread), and is read in place: no allocation and no copy
        here, which is how `sampler.GuidedDDIMSampler.decode` keeps one input buffer for a whole loop.  x is not written to."""
        cin = self.in_pad if padded else self.in_channels
        if not is_f32_cuda(x, 4) or x.shape[3] != cin:
            raise RuntimeError(f"x must be a CUDA float32 tensor with {cin} channels")
        if padded and not x.is_contiguous():
            raise RuntimeError("padded=True takes a contiguous [B,H,W,in_pad] tensor")
        B, H, W, _ = x.shape
        ref_by_st, ctl = self._check_inputs(B, H, W, timesteps, context, control, reference_kv)
        h = x if padded else pad_channels4(x, self.in_channels)                       # a padded x was checked contiguous above
        emb_all = self.emb_projections(timesteps)
        kv_hists: List[Tuple[torch.Tensor, torch.Tensor]] = []
        hs = []
        for blk in self.layout["input"]:                                               # :779-782
            h = self._block(blk, h, emb_all, context, ref_by_st, kv_hists)
            hs.append(h)
        h = self._block(self.layout["middle"], h, emb_all, context, ref_by_st, kv_hists)     # :783
        if ctl is not None:
            h += ctl[-1]                                                               # controlnet.py:50
        for i, blk in enumerate(self.layout["output"]):                                # :785-788, controlnet.py:52-59
            skip = hs.pop()
            if ctl is not None and not only_mid_control:
                skip += ctl[-2 - i]                # hs.pop() + control.pop(): `skip` is this call's own tensor, read by nothing else
            h = self._block(blk, h, emb_all, context, ref_by_st, kv_hists, skip=skip)
        out = self._conv("out.2", self._norm("out.0", h), 3)                           # self.out (:729-733)
        return out, kv_hists

    @torch.no_grad()
    def forward(self, x: torch.Tensor, timesteps: torch.Tensor, context: Optional[torch.Tensor] = None, control=None,
                only_mid_control: bool = False, reference_kv=()) -> Tuple[torch.Tensor, List[Tuple[torch.Tensor, torch.Tensor]]]:
        """UNetModel.forward (:757-793) with the `control` / `reference_kv` handling of ControlledUnetModel.forward
        (controlnet.py:29-62): x f32 [B,in_channels,H,W] on the device, timesteps [B], context [B,M,context_dim] -> (eps
        [B,out_channels,H,W], kv_hists).  kv_hists: the own self-attention (k, v) of every transformer in the reference's order (input
        blocks, middle, output blocks), device tensors [B, h*w, inner] as `SpatialTransformer.forward_nhwc` returns them.
        control: len(input_blocks) + 1 NCHW device tensors, used from the end as the reference pops them; with only_mid_control only
        the last one is added (after the middle block).  reference_kv: a sequence over reference frames, each a sequence of one
        (k, v) per transformer in that order; transformer i attends to entry i of every frame, in either layout `plan_reference_kv`
        accepts.  Unlike the reference, neither list is consumed, `control` is not written to, and reference_kv is honoured when
        control is None (module docstring).  H and W must be multiples of 2 ** (len(channel_mult) - 1) (ValueError before any launch)."""
        if not torch.is_tensor(x) or x.dim() != 4:
            raise RuntimeError("x must be a CUDA float32 tensor [B,C,H,W]")
        out, kv = self.forward_nhwc(x.permute(0, 2, 3, 1).contiguous(), timesteps, context, control, only_mid_control, reference_kv)
        return out.permute(0, 3, 1, 2).contiguous(), kv

    __call__ = forward
