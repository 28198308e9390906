"""First-stage (VAE) encoding and decoding of the SD-inpaint hand-off on the device.

`img2img_inpaint` turns the composited frame into `init_latent = get_first_stage_encoding(encode_first_stage(image))`
(guided_ldm_inpainting.py:302) before the first denoising step.  `encode_first_stage` is `AutoencoderKL.encode`
(ldm/models/autoencoder.py:350-354): `Encoder.forward` (ldm/modules/diffusionmodules/model.py:518-543) -> `quant_conv`
-> a diagonal Gaussian whose sample, times `scale_factor` (0.18215, guided_ldm_inpaint4_v15.yaml:16), is the latent
(ldm/models/diffusion/ddpm.py:655-662, ldm/modules/distributions/distributions.py:24-37).

Everything runs through the C ABI of libofx.so on NHWC fp32 tensors: the 3x3 / 1x1 convolutions on the fp32 matrix
cores (`ofx_conv2d`, residual sums as pre-activation addends of the epilogue), GroupNorm(32, eps 1e-6) + x*sigmoid(x)
(`ofx_groupnorm`), the mid-block self-attention (`ofx_attention_f32`; the reference picks xformers there when it is
installed, model.py:282-290).  State-dict keys are the reference's (`encoder.*`, `quant_conv.*`; the `first_stage_model.`
prefix of full SD checkpoints is accepted).  No checkpoint ships with the reference tree: parity is pinned with seeded
weights loaded into the reference's own `Encoder` (tests/golden/make_golden_vae.py).

The way back is `VaeDecoder`: `decode_first_stage` (ldm/models/diffusion/ddpm.py:820-828) = `AutoencoderKL.decode`
(autoencoder.py: `post_quant_conv` -> `Decoder.forward`, model.py:619-652) of `z / scale_factor`, and `decode_latent`
(ofgen_keyframe_inpaint.py:234-235), which ends in the BGR byte frame.  Same kernels, plus the decoder's own: each `Upsample`
(nearest 2x + 3x3 convolution, model.py:43-58) is one `ofx_upconv2x` launch that never forms the upsampled map and contracts 4 taps
per output instead of 9 (OFX_VAE_NO_UPCONV=1 in the environment, read once per process: `ofx_upsample2x_nearest_f32` +
`ofx_conv2d` instead), and `ofx_decode_to_u8` makes the bytes.  Pinned the same way (tests/golden/make_golden_vae_decoder.py).

`precision=` ("fp32", the default and bit for bit what the classes did without the argument, or "fp16") on both classes is the
arithmetic of every contraction but the attention's: the reference runs its whole diffusion stage, first stage included, under
`torch.autocast` (ofgen_keyframe_inpaint.py:212,273, ofgen.py:104).  "fp16" gives every `_conv` the fp16 matrix-core arithmetic of
`ops.conv2d_nhwc(precision="fp16")` and the decoder's `Upsample` that of `ops.upconv2x(precision="fp16")` (the unfused pair:
`upsample2x_nearest` + the same `_conv`): both operands rounded fp32 -> fp16, to nearest even, as the kernel stages them, fp32
accumulation, fp32 bias, addend and result.  GroupNorm, SiLU, the mid-block attention (one head of d = 512, not a fused head size)
and its softmax, the weights and every activation in memory, `sample` and `decode_to_u8` stay fp32 in both modes.  Range: the layers
that read the un-normalised residual stream (`nin_shortcut`, `Upsample`, `Downsample`) round it to half like every other operand, so
a value beyond +-65504 there becomes an infinity, as in the reference's autocast run.  Anything else is a ValueError, raised before
the checkpoint is looked at or a device asked for.

Checkpoint loading, weight packing and the convolution call are `modelbase`'s, shared with the other SD-stage models.  Both classes
check in the order the others do: configuration, then checkpoint, then device.  A checkpoint with a missing key or a wrong shape is
a KeyError / ValueError on a machine without a device too (it used to be the RuntimeError about the device there); the decoder's
4-row padding of `conv_out` and its folded upsample operands are this module's own.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from .modelbase import DeviceModel, check_weight_dtype, env_flag, is_f32_cuda, load_tensors, pad_channels4, random_tensors, wb

SCALE_FACTOR = 0.18215
SD_V1_CONFIG = dict(ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, in_channels=3, z_channels=4, double_z=True, embed_dim=4)


def _resblock_wb(out, name, ci, co):
    """The tensors of a ResnetBlock (model.py:97-127), for the encoder's and the decoder's lists alike."""
    wb(out, f"{name}.norm1", ci)
    wb(out, f"{name}.conv1", co, ci, 3, 3)
    wb(out, f"{name}.norm2", co)
    wb(out, f"{name}.conv2", co, co, 3, 3)
    if ci != co:
        wb(out, f"{name}.nin_shortcut", co, ci, 1, 1)


def _attn_wb(out, name, c):
    wb(out, f"{name}.norm", c)
    for nm in ("q", "k", "v", "proj_out"):
        wb(out, f"{name}.{nm}", c, c, 1, 1)


def encoder_tensors(cfg: dict = SD_V1_CONFIG) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of every tensor of `encoder.*` + `quant_conv.*` for a ddconfig, in module order."""
    ch, mult, nres = cfg["ch"], tuple(cfg["ch_mult"]), cfg["num_res_blocks"]
    out: List[Tuple[str, Tuple[int, ...]]] = []
    wb(out, "encoder.conv_in", ch, cfg["in_channels"], 3, 3)
    block_in = ch
    for lvl, m in enumerate(mult):
        block_out = ch * m
        for j in range(nres):
            _resblock_wb(out, f"encoder.down.{lvl}.block.{j}", block_in, block_out)
            block_in = block_out
        if lvl != len(mult) - 1:
            wb(out, f"encoder.down.{lvl}.downsample.conv", block_in, block_in, 3, 3)
    _resblock_wb(out, "encoder.mid.block_1", block_in, block_in)
    _attn_wb(out, "encoder.mid.attn_1", block_in)
    _resblock_wb(out, "encoder.mid.block_2", block_in, block_in)
    wb(out, "encoder.norm_out", block_in)
    zc = cfg["z_channels"] * (2 if cfg["double_z"] else 1)
    wb(out, "encoder.conv_out", zc, block_in, 3, 3)
    wb(out, "quant_conv", 2 * cfg["embed_dim"], zc, 1, 1)
    return out


def random_vae_state_dict(seed: int = 0, cfg: dict = SD_V1_CONFIG) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for the absent checkpoint: fan-in-scaled normal convolution weights, norm scales around 1."""
    return random_tensors(encoder_tensors(cfg), int(seed) + 7919)


def decoder_tensors(cfg: dict = SD_V1_CONFIG) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of every tensor of `decoder.*` + `post_quant_conv.*` for a ddconfig, in module order (model.py:546-617: the
    levels are built from the coarsest down, `up` is indexed from the finest up)."""
    ch, mult, nres = cfg["ch"], tuple(cfg["ch_mult"]), cfg["num_res_blocks"]
    out: List[Tuple[str, Tuple[int, ...]]] = []
    block_in = ch * mult[-1]
    wb(out, "decoder.conv_in", block_in, cfg["z_channels"], 3, 3)
    _resblock_wb(out, "decoder.mid.block_1", block_in, block_in)
    _attn_wb(out, "decoder.mid.attn_1", block_in)
    _resblock_wb(out, "decoder.mid.block_2", block_in, block_in)
    io = {}
    for lvl in reversed(range(len(mult))):
        io[lvl] = (block_in, ch * mult[lvl])
        block_in = ch * mult[lvl]
    for lvl in range(len(mult)):
        ci, co = io[lvl]
        for j in range(nres + 1):
            _resblock_wb(out, f"decoder.up.{lvl}.block.{j}", ci if j == 0 else co, co)
        if lvl != 0:
            wb(out, f"decoder.up.{lvl}.upsample.conv", co, co, 3, 3)
    wb(out, "decoder.norm_out", block_in)
    wb(out, "decoder.conv_out", cfg.get("out_ch", 3), block_in, 3, 3)
    wb(out, "post_quant_conv", cfg["z_channels"], cfg["embed_dim"], 1, 1)
    return out


def random_vae_decoder_state_dict(seed: int = 0, cfg: dict = SD_V1_CONFIG) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for the decoder half of the absent checkpoint, drawn from a generator of its own (the encoder's tensors of
    `random_vae_state_dict` do not depend on it)."""
    return random_tensors(decoder_tensors(cfg), int(seed) + 104729)


VAE_PRECISIONS = ("fp32", "fp16")      # `precision=` of VaeEncoder / VaeDecoder


def check_precision(precision) -> str:
    if not isinstance(precision, str) or precision not in VAE_PRECISIONS:
        raise ValueError(f"precision must be one of {VAE_PRECISIONS}, got {precision!r}")
    return precision


def _no_upconv() -> bool:
    """OFX_VAE_NO_UPCONV=1 (diagnostic, read once per process): the decoder's Upsample layers run unfused."""
    return env_flag("OFX_VAE_NO_UPCONV")


class _VaeBlocks(DeviceModel):
    """What `Encoder` and `Decoder` share (model.py): weights on the device in the kernels' layouts (`modelbase.DeviceModel`), and
    the GroupNorm, ResnetBlock and AttnBlock calls."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], tensors, device, cfg: dict, scale_factor: float, precision: str,
                 weight_dtype: str = "fp32"):
        self.cfg, self.scale_factor = dict(cfg), float(scale_factor)
        self.precision = check_precision(precision)                # the arithmetic of every `_conv`; before the checkpoint or a device
        self.weight_dtype = check_weight_dtype(weight_dtype, self.precision)   # storage of the convolution operands (`DeviceModel`)
        strip = len("first_stage_model.")                          # the prefix of full SD checkpoints, where a key has it
        sd = {k[strip:] if k.startswith("first_stage_model.") else k: v for k, v in state_dict.items()}
        t32 = load_tensors(sd, tensors, "", "VAE")                 # the checkpoint is checked before the device is asked for
        self._use_device(device)
        for key, t in t32.items():
            self._put(key, t)

    # ---- building blocks (model.py line numbers) -----------------------------------------------------------
    def _norm(self, name: str, x: torch.Tensor, silu: bool) -> torch.Tensor:
        return ops.groupnorm(x, self.w[f"{name}.weight"], self.w[f"{name}.bias"], 32, 1e-6, silu)

    def _resblock(self, name: str, x: torch.Tensor) -> torch.Tensor:
        """ResnetBlock.forward (:129-149), temb = None, dropout 0."""
        h = self._conv(f"{name}.conv1", self._norm(f"{name}.norm1", x, True), 3)
        h = self._norm(f"{name}.norm2", h, True)
        skip = self._conv(f"{name}.nin_shortcut", x, 1) if f"{name}.nin_shortcut.weight" in self.w else x
        return self._conv(f"{name}.conv2", h, 3, addend=skip)                 # x + h in the epilogue

    def _attn(self, name: str, x: torch.Tensor) -> torch.Tensor:
        """AttnBlock.forward (:179-203): one head over all H*W positions, d = channels."""
        B, H, W, Cn = x.shape
        hn = self._norm(f"{name}.norm", x, False)
        q = self._conv(f"{name}.q", hn, 1).reshape(B, H * W, Cn)
        k = self._conv(f"{name}.k", hn, 1).reshape(B, H * W, Cn)
        v = self._conv(f"{name}.v", hn, 1).reshape(B, H * W, Cn)
        a = ops.attention(q, k, v, None, float(Cn) ** -0.5).reshape(B, H, W, Cn)
        return self._conv(f"{name}.proj_out", a, 1, addend=x)


class VaeEncoder(_VaeBlocks):
    """`AutoencoderKL.encode` + `get_first_stage_encoding` on a HIP device.  `weight_dtype`: "fp32" (default) or "fp16" (with
    precision="fp16" only): the convolution operands stored in half, bit-identical results (`modelbase.DeviceModel`)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", cfg: dict = SD_V1_CONFIG, scale_factor: float = SCALE_FACTOR,
                 precision: str = "fp32", weight_dtype: str = "fp32"):
        super().__init__(state_dict, encoder_tensors(cfg), device, cfg, scale_factor, precision, weight_dtype)

    def max_batch(self, H: int, W: int) -> int:
        """Images one pass of the encoder can take at this size: the convolution kernel addresses its operands with 32-bit byte
        offsets, so the widest activation -- the full-resolution `ch * ch_mult[0]`-channel maps of level 0 -- must stay under
        2 GiB (10 frames at 512x768, 4 at 1024x1024).  `encode_moments` slices larger batches (images are independent)."""
        widest = H * W * self.cfg["ch"] * max(1, self.cfg["ch_mult"][0]) * 4
        return max(1, ((1 << 31) - 4096) // widest)

    @torch.no_grad()
    def encode_moments(self, image: torch.Tensor) -> torch.Tensor:
        """image f32 [B,3,H,W] in [-1,1] (what img2img_inpaint builds, guided_ldm_inpainting.py:299-301), H and W
        multiples of 8 -> moments f32 [B, 2*z, H/8, W/8] = quant_conv(encoder(image)) (autoencoder.py:350-352)."""
        if not image.is_cuda or image.dtype != torch.float32 or image.dim() != 4 or image.shape[1] != self.cfg["in_channels"]:
            raise RuntimeError("image must be a CUDA float32 tensor [B,3,H,W]")
        B, _, H, W = image.shape
        n_down = len(self.cfg["ch_mult"]) - 1
        if H % (1 << n_down) or W % (1 << n_down):
            raise RuntimeError(f"H and W must be multiples of {1 << n_down}")
        mb = self.max_batch(H, W)
        if B > mb:
            return torch.cat([self.encode_moments(image[b0:b0 + mb]) for b0 in range(0, B, mb)])
        x = pad_channels4(image.permute(0, 2, 3, 1), self.cfg["in_channels"])          # NHWC, channel 3 = 0 (Cin padded to 4)
        h = self._conv("encoder.conv_in", x, 3)
        for lvl in range(len(self.cfg["ch_mult"])):
            for j in range(self.cfg["num_res_blocks"]):
                h = self._resblock(f"encoder.down.{lvl}.block.{j}", h)
            if lvl != n_down:
                # Downsample (:80-84): F.pad(x, (0,1,0,1)) + 3x3 stride-2 conv without padding = taps past the bottom /
                # right edge read zeros
                h = self._conv(f"encoder.down.{lvl}.downsample.conv", h, 3, stride=2, pad=(0, 0), out_hw=(h.shape[1] // 2, h.shape[2] // 2))
        h = self._resblock("encoder.mid.block_1", h)
        h = self._attn("encoder.mid.attn_1", h)
        h = self._resblock("encoder.mid.block_2", h)
        h = self._conv("encoder.conv_out", self._norm("encoder.norm_out", h, True), 3)
        m = self._conv("quant_conv", h, 1)
        return m.permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def sample(moments: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """DiagonalGaussianDistribution(moments).sample() (distributions.py:24-37); noise defaults to torch.randn."""
        mean, logvar = torch.chunk(moments, 2, dim=1)
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        if noise is None:
            noise = torch.randn(mean.shape, device=moments.device)
        return mean + std * noise

    @torch.no_grad()
    def get_first_stage_encoding(self, image: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`self.get_first_stage_encoding(self.encode_first_stage(image))` (guided_ldm_inpainting.py:302)."""
        return self.scale_factor * self.sample(self.encode_moments(image), noise)


class VaeDecoder(_VaeBlocks):
    """`AutoencoderKL.decode` / `decode_first_stage` / `decode_latent` on a HIP device.  `weight_dtype`: "fp32" (default) or "fp16"
    (with precision="fp16" only): the convolution operands and the folded `Upsample` operands stored in half, bit-identical
    results (`modelbase.DeviceModel`)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", cfg: dict = SD_V1_CONFIG, scale_factor: float = SCALE_FACTOR,
                 precision: str = "fp32", weight_dtype: str = "fp32"):
        super().__init__(state_dict, decoder_tensors(cfg), device, cfg, scale_factor, precision, weight_dtype)
        # Upsample layers that run fused (level -> bool); OFX_VAE_NO_UPCONV=1 turns every one to the unfused pair
        self.fused_upsample = {lvl: not _no_upconv() for lvl in range(1, len(self.cfg["ch_mult"]))}

    def _put(self, key: str, t: torch.Tensor) -> None:
        if key == "decoder.conv_out.weight" and t.shape[0] % 4:
            # rows of 4 floats for the RGB map (the byte exit reads 16-byte pixels): output channels padded with zero weights
            t = torch.cat([t, t.new_zeros((4 - t.shape[0] % 4,) + tuple(t.shape[1:]))])
        elif key == "decoder.conv_out.bias" and t.shape[0] % 4:
            t = torch.cat([t, t.new_zeros((4 - t.shape[0] % 4,))])
        super()._put(key, t)
        if key.endswith(".upsample.conv.weight"):
            folded = ops.upconv2x_weight(t)                                    # [4 parities, Cout, 4 taps, Cin]
            if self.weight_dtype == "fp16":                                    # `ops.upconv2x(precision="fp16")` reads halves as they are
                folded = ops.half_conv_weight(folded)
                self.half_keys.add(key + ".folded")
            self.w[key + ".folded"] = folded.to(self.device)

    def _upsample(self, lvl: int, x: torch.Tensor) -> torch.Tensor:
        """Upsample.forward (:52-58): interpolate(scale_factor=2.0, mode="nearest") + 3x3 convolution."""
        name = f"decoder.up.{lvl}.upsample.conv"
        if self.fused_upsample[lvl]:
            return ops.upconv2x(x, self.w[f"{name}.weight.folded"], self.w[f"{name}.bias"], precision=self.precision)
        return self._conv(name, ops.upsample2x_nearest(x), 3)                  # the unfused pair, the convolution in `self.precision`

    def max_batch(self, H: int, W: int) -> int:
        """Frames of HxW pixels one pass of the decoder can take: the convolution kernel addresses its operands with 32-bit byte
        offsets, so the widest activation must stay under 2 GiB.  That is what the last Upsample writes: the full-resolution map
        with the `ch * ch_mult[1]` channels of level 1 (256: 5 frames at 512x768, 1 at 1024x1024).  `decode` slices larger batches."""
        mult = tuple(self.cfg["ch_mult"])
        widest = 0
        for lvl in range(len(mult)):
            c = self.cfg["ch"] * max(mult[lvl], mult[min(lvl + 1, len(mult) - 1)])
            widest = max(widest, (H >> lvl) * (W >> lvl) * c * 4)
        return max(1, ((1 << 31) - 4096) // widest)

    @torch.no_grad()
    def _decode_nhwc(self, z: torch.Tensor) -> torch.Tensor:
        """z f32 [B,z,h,w] -> the RGB map f32 NHWC [B,8h,8w,4] (channel 3 = 0), one pass."""
        n_lvl = len(self.cfg["ch_mult"])
        h = self._conv("post_quant_conv", z.permute(0, 2, 3, 1).contiguous(), 1)          # autoencoder.py decode
        h = self._conv("decoder.conv_in", h, 3)
        h = self._resblock("decoder.mid.block_1", h)
        h = self._attn("decoder.mid.attn_1", h)
        h = self._resblock("decoder.mid.block_2", h)
        for lvl in reversed(range(n_lvl)):
            for j in range(self.cfg["num_res_blocks"] + 1):
                h = self._resblock(f"decoder.up.{lvl}.block.{j}", h)
            if lvl != 0:
                h = self._upsample(lvl, h)
        return self._conv("decoder.conv_out", self._norm("decoder.norm_out", h, True), 3)

    def _check(self, z: torch.Tensor) -> None:
        if not is_f32_cuda(z, 4) or z.shape[1] != self.cfg["z_channels"]:
            raise RuntimeError(f"z must be a CUDA float32 tensor [B,{self.cfg['z_channels']},h,w]")
        if self.cfg["embed_dim"] % 4 or self.cfg["z_channels"] % 4:
            raise RuntimeError("embed_dim and z_channels must be multiples of 4")

    def _slices(self, z: torch.Tensor, max_batch: Optional[int]):
        up = 1 << (len(self.cfg["ch_mult"]) - 1)
        mb = self.max_batch(z.shape[2] * up, z.shape[3] * up)
        mb = mb if max_batch is None else max(1, min(mb, int(max_batch)))
        return [z[b0:b0 + mb] for b0 in range(0, z.shape[0], mb)]

    @torch.no_grad()
    def decode(self, z: torch.Tensor, max_batch: Optional[int] = None) -> torch.Tensor:
        """z f32 [B,4,h,w] -> image f32 [B,3,8h,8w] = decoder(post_quant_conv(z)) (AutoencoderKL.decode).  Batches beyond
        `max_batch` (default: what `max_batch()` allows at this size) are decoded in slices (latents are independent)."""
        self._check(z)
        nout = self.cfg.get("out_ch", 3)
        return torch.cat([self._decode_nhwc(p)[..., :nout].permute(0, 3, 1, 2).contiguous() for p in self._slices(z, max_batch)])

    @torch.no_grad()
    def decode_first_stage(self, z: torch.Tensor, max_batch: Optional[int] = None) -> torch.Tensor:
        """`decode_first_stage(z)` (ddpm.py:820-828): z = 1. / scale_factor * z, then decode."""
        self._check(z)
        return self.decode(1.0 / self.scale_factor * z, max_batch)

    @torch.no_grad()
    def decode_latent(self, z: torch.Tensor, max_batch: Optional[int] = None) -> torch.Tensor:
        """`decode_latent(model, latent)` (ofgen_keyframe_inpaint.py:234-235) for a batch: u8 BGR [B,8h,8w,3] on the device =
        (decode_first_stage(z).clip(-1, 1) * 127.5 + 127.5).astype(uint8), channels reversed."""
        self._check(z)
        return torch.cat([ops.decode_to_u8(self._decode_nhwc(p)) for p in self._slices(1.0 / self.scale_factor * z, max_batch)])
