"""What the five SD-stage models (`unet`, `controlnet`, `vae`, `transformer`, `text_encoder`) share, and nothing else: the home of
checkpoint loading and weight packing.

Plain functions, no device needed: the (key, shape) list helper `wb`, the seeded stand-in weights `random_tensors`, the checkpoint
check `load_tensors`, the once-per-process environment switch `env_flag`, and the input checks `is_f32_cuda`,
`check_activation_bytes`, `pad_channels4`.

`DeviceModel` is the base of every model class: the device check, the placement of a tensor in the kernels' layout in `self.w`
(`_put`, `_put_gemm`) and the two layer calls every model makes, a convolution by state-dict name (`_conv`) and a Linear over token
rows as a 1x1 convolution (`_gemm`), both in `self.precision`; with `weight_dtype="fp16"` (`check_weight_dtype`) the operands of those
two calls are stored in half.  A model checks its configuration, then its checkpoint
(`load_tensors`), then asks for the device (`_use_device`), so that a bad checkpoint is a KeyError / ValueError on any machine.
"""
from __future__ import annotations

import functools
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops

Tensors = List[Tuple[str, Tuple[int, ...]]]


def wb(out: Tensors, name: str, *shape: int) -> None:
    """Appends (name.weight, shape) and (name.bias, (shape[0],)) to a (key, shape) list."""
    out.append((f"{name}.weight", tuple(shape)))
    out.append((f"{name}.bias", (shape[0],)))


def random_tensors(tensors: Sequence[Tuple[str, Tuple[int, ...]]], seed: int) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for an absent checkpoint, drawn in the order of `tensors` from one generator: fan-in-scaled normal matrices
    and convolutions, scales around 1 for every 1-D `.weight` (in these models each one is a norm's), small biases.  The golden
    generators depend on these bits (tests/test_model_weights_host.py)."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for key, shape in tensors:
        if len(shape) >= 2:
            sd[key] = torch.randn(shape, generator=g) * (1.0 / math.sqrt(math.prod(shape[1:])))
        elif key.endswith(".weight"):
            sd[key] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            sd[key] = 0.05 * torch.randn(shape, generator=g)
    return sd


def load_tensors(state_dict: Dict[str, torch.Tensor], want: Sequence[Tuple[str, Tuple[int, ...]]], prefix: str, what: str
                 ) -> Dict[str, torch.Tensor]:
    """The tensors `want` lists, read under `prefix`, as fp32 CPU tensors by un-prefixed key.  KeyError for a missing key,
    ValueError for a wrong shape, in the order of `want`.  Needs no device."""
    t32: Dict[str, torch.Tensor] = {}
    for key, shape in want:
        if prefix + key not in state_dict:
            raise KeyError(f"{what} checkpoint lacks {prefix}{key}")
        t = state_dict[prefix + key].detach().to(torch.float32).cpu()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{prefix}{key}: shape {tuple(t.shape)} != {shape}")
        t32[key] = t
    return t32


@functools.lru_cache(maxsize=None)
def env_flag(name: str) -> bool:
    """An `OFX_*` switch of the environment: set to anything but "" / "0".  Read once per process per name."""
    return os.environ.get(name, "") not in ("", "0")


def is_f32_cuda(t, ndim: int) -> bool:
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == ndim


def check_activation_bytes(nbytes: int, message: str) -> None:
    """The convolution kernel addresses its operands with 32-bit byte offsets: an activation of 2 GiB or more is a RuntimeError."""
    if nbytes >= (1 << 31):
        raise RuntimeError(message)


def pad_channels4(x_nhwc: torch.Tensor, c: int) -> torch.Tensor:
    """x [B,H,W,c] in any strides -> contiguous [B,H,W,c rounded up to a multiple of 4], the tail channels zero (they meet the zero
    weights of `ops.pack_conv_weight`).  c % 4 == 0: `x.contiguous()`, no allocation or copy when x already is."""
    if c % 4 == 0:
        return x_nhwc.contiguous()
    xp = torch.zeros(tuple(x_nhwc.shape[:3]) + ((c + 3) // 4 * 4,), dtype=torch.float32, device=x_nhwc.device)
    xp[..., :c] = x_nhwc
    return xp


WEIGHT_DTYPES = ("fp32", "fp16")       # `weight_dtype=` of UNetModel / ControlNet / SpatialTransformer / VaeEncoder / VaeDecoder


def check_weight_dtype(weight_dtype, precision) -> str:
    """`weight_dtype` as a model's constructor takes it, next to its (already checked) `precision`: ValueError for a value outside
    WEIGHT_DTYPES, and for "fp16" with any arithmetic but precision="fp16" -- half weights feed the fp16 kernels as they are;
    no kernel widens them for another arithmetic.  Needs no checkpoint and no device."""
    if not isinstance(weight_dtype, str) or weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES}, got {weight_dtype!r}")
    if weight_dtype == "fp16" and precision != "fp16":
        raise ValueError(f'weight_dtype="fp16" needs precision="fp16", got precision={precision!r} (half weights are the operand '
                         f"of the fp16 kernels only; there is no widening path)")
    return weight_dtype


class DeviceModel:
    """A model whose weights live in `self.w` on a HIP device in the kernels' layouts.  `self.precision` is the arithmetic of
    `_conv` / `_gemm` (a key of `ops.CONV_PRECISIONS`).

    `self.weight_dtype` ("fp32", the default when a model never sets it, or "fp16"; `check_weight_dtype`) is the storage of the
    `ofx_conv2d` operands, i.e. of what `_conv` / `_gemm` read: with "fp16" `_put` / `_put_gemm` pack in fp32 as always and then
    keep the packed matrix [Cout, Kpad] as IEEE halves (`ops.half_conv_weight`: the rounding the fp16 kernels apply to every weight
    on every launch), and `_conv` / `_gemm` pass precision "fp16_w" -- the same kernels reading halves, bit-identical results, half
    the bytes held and streamed.  `self.half_keys` names those entries.  Everything that is not an `ofx_conv2d` operand stays fp32
    in both settings: biases; norm scales; the `emb_linear` / timestep path (`time_embed.*`, `emb_layers.*`, `freqs`); ControlNet's
    hint stem (`input_hint_block.*`, `ops.conv3x3_silu`); the UNet's own `Upsample` weights (`*.conv.weight` and its `.folded`
    form, which run `ofx_upconv2x` in fp32 in every precision).  The VAE decoder's `Upsample` runs in `self.precision`, so its
    folded operand is stored in half too."""

    weight_dtype = "fp32"

    def _use_device(self, device) -> None:
        """No device is a RuntimeError; otherwise `self.device`, and `self.w` starts empty."""
        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs a HIP device (no CPU fallback)")
        self.device = torch.device(device)
        self.w: Dict[str, torch.Tensor] = {}
        self.half_keys: set = set()                                # entries of `self.w` stored in half (weight_dtype="fp16")

    def _put(self, key: str, t: torch.Tensor, *, operand: bool = True) -> None:
        """A 4-D weight as the packed operand [Cout, Kpad] (Cin padded to a multiple of 4), anything else contiguous.
        weight_dtype="fp16": the packed operand in half, unless `operand` is False (a 4-D weight no `ofx_conv2d` launch reads)."""
        if t.dim() == 4:
            t = ops.pack_conv_weight(t)
            if operand and self.weight_dtype == "fp16":
                t = ops.half_conv_weight(t)
                self.half_keys.add(key)
        self.w[key] = t.contiguous().to(self.device)

    def _put_gemm(self, name: str, t32: Dict[str, torch.Tensor], *parts: str, bias: bool = False) -> None:
        """The Linear (or 1x1 convolution) weights `parts`, concatenated along their outputs, as one packed 1x1 operand
        `name.weight`; with `bias`, their biases as one `name.bias`."""
        self._put(f"{name}.weight", torch.cat([t32[f"{p}.weight"].reshape(t32[f"{p}.weight"].shape[0], -1, 1, 1) for p in parts]))
        if bias:
            self._put(f"{name}.bias", torch.cat([t32[f"{p}.bias"] for p in parts]))

    def _conv(self, name: str, x: torch.Tensor, k: int, *, stride: int = 1, addend: Optional[torch.Tensor] = None,
              x2: Optional[torch.Tensor] = None, pad=None, out_hw=None) -> torch.Tensor:
        w = self.w[f"{name}.weight"]
        return ops.conv2d_nhwc(x, w, k, k, w.shape[0], stride=stride, shift=self.w[f"{name}.bias"], addend=addend, x2=x2, pad=pad,
                               out_hw=out_hw, precision=self._precision_of(w))

    def _gemm(self, name: str, x: torch.Tensor, bias: bool, addend: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B, N, K] -> x W^T (+ bias) (+ addend) [B, N, Cout]: a 1x1 convolution over the token rows."""
        B, N, K = x.shape
        w = self.w[f"{name}.weight"]
        co = w.shape[0]
        out = ops.conv2d_nhwc(x.view(B, 1, N, K), w, 1, 1, co, shift=self.w[f"{name}.bias"] if bias else None,
                              addend=None if addend is None else addend.view(B, 1, N, co), precision=self._precision_of(w))
        return out.view(B, N, co)

    def _precision_of(self, w: torch.Tensor) -> str:
        """The `ops.conv2d_nhwc(precision=)` of a launch on the packed operand `w`: "fp16_w" for one stored in half (it exists
        under precision="fp16" only), else `self.precision`."""
        return "fp16_w" if w.dtype == torch.float16 else self.precision
