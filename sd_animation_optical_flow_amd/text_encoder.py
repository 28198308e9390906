"""The reference's CLIP text encoder on the device: from prompt tokens to the UNet's context.

    get_learned_conditioning([c_text]) / ([uc_text])     guided_ldm_inpainting.py:200-203, 276-279, 362-365
    FrozenCLIPEmbedder                                   ldm/modules/encoders/modules.py
    hack_everything / _hacked_clip_forward               hack.py:23-70

`_hacked_clip_forward` cuts a prompt's raw token ids into three pieces of 75, wraps each as [bos] + piece + [eos] padded to 77
(`chunk_tokens`, host code), runs the three 77-token sequences through transformers' CLIPTextModel (with `clip_skip`, hack.py:42-47)
and lays the results side by side: [B, 231, 768], the `context` / `unconditional_context` of `sampler.img2img_inpaint` and the M
the UNet's cross-attention takes.  The prompt is per frame in the reference (its tagger feeds it), so this runs once per frame.

A CLIP layer is pre-LN: x += out_proj(attention(q|k|v(LN1(x)))), x += fc2(quick_gelu(fc1(LN2(x)))), with a causal mask.  On the
device that is 8 launches per layer, nothing permuted or concatenated between them:
    1 `ops.layernorm`   2 the q|k|v GEMM with bias (one [3*width, width] operand, 1x1 `ops.conv2d_nhwc`)
    3 `ops.attention_bnhd` on the thirds in place (scale d_head^-0.5, the shared [T,T] causal bias: 0 on and below the diagonal,
      -inf above)       4 the out_proj GEMM with bias and addend = x
    5 `ops.layernorm`   6 the fc1 GEMM with bias       7 `ops.quick_gelu` in place       8 the fc2 GEMM with bias and addend = x
`ops.clip_embed` (token gather + position embedding) runs before the first layer and one `ops.layernorm` (final_layer_norm) after
the last one used.  All LayerNorm eps are 1e-5.  The two kernels this module adds are csrc/text_encoder.hip; the causal mask is a
bias tensor of the existing attention kernel.

`dedupe=True`: identical rows of the host ids are encoded once and scattered back.  Every sequence is independent of the others
(the attention is per sequence, every other operation per row), so this is the same function; for a prompt under 75 tokens chunks 2
and 3 are the constant [bos, eos, pad...], and a (prompt, negative prompt) pair is three distinct sequences instead of six.  Not
bit-identical to `dedupe=False`: the GEMM's tile and split-K choice may depend on the row count.

Only what guided_ldm_*_v15.yaml's FrozenCLIPEmbedder loads is built: quick_gelu, causal, pre-LN.  Not built: the BPE tokenizer
(`encode` takes any object with the transformers tokenizer's call interface), the tagger, FrozenOpenCLIPEmbedder / T5.

The checkpoint check (`load_clip_text_tensors` over `modelbase.load_tensors`), the packing of the weights and the GEMM call are
`modelbase`'s, shared with the other SD-stage models; the two embedding tables are this module's own.

OFX_CLIP_TORCH_GLUE=1 in the environment (read once per process; the A/B baseline and a diagnostic): the embedding and quick_gelu
through torch ops instead of the two kernels.

No checkpoint ships with the reference tree: parity is pinned with seeded weights loaded into the reference's own embedder
(tests/golden/make_golden_text_encoder.py).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import ops
from .modelbase import DeviceModel, check_activation_bytes, env_flag, load_tensors, random_tensors, wb

# CLIPTextConfig of openai/clip-vit-large-patch14, the `version` FrozenCLIPEmbedder defaults to
SD_V15_CLIP_TEXT = dict(vocab=49408, width=768, heads=12, layers=12, intermediate=3072, positions=77)
CHUNKS, CHUNK_LEN = 3, 75                      # hack.py:49-50
LN_EPS = 1e-5
_CFG_KEYS = ("vocab", "width", "heads", "layers", "intermediate", "positions")
# what a config may also say, and the one value that is built
_CFG_FIXED = dict(hidden_act="quick_gelu", layer_norm_eps=LN_EPS, causal=True, pre_ln=True)


def _check_cfg(cfg: dict) -> Dict[str, int]:
    """The six sizes as ints.  Anything but quick_gelu / causal / pre-LN CLIP raises (NotImplementedError), as does an unknown key."""
    for k in _CFG_KEYS:
        if k not in cfg:
            raise KeyError(f"CLIP text cfg lacks {k}")
    for k, v in cfg.items():
        if k in _CFG_KEYS:
            continue
        if k not in _CFG_FIXED or v != _CFG_FIXED[k]:
            raise NotImplementedError(f"CLIP text cfg {k}={v!r} is not built (only quick_gelu, causal, pre-LN CLIP with eps {LN_EPS})")
    c = {k: int(cfg[k]) for k in _CFG_KEYS}
    if min(c.values()) <= 0:
        raise ValueError(f"CLIP text cfg sizes must be positive, got {c}")
    if c["width"] % c["heads"]:
        raise ValueError(f"width {c['width']} is not a multiple of heads {c['heads']}")
    d = c["width"] // c["heads"]
    if d not in ops.ATTENTION_FUSED_HEAD_SIZES:
        raise ValueError(f"head size {d} is outside the fused attention's {ops.ATTENTION_FUSED_HEAD_SIZES}")
    if c["width"] % 4 or c["intermediate"] % 4:
        raise ValueError("width and intermediate must be multiples of 4")
    return c


def clip_text_tensors(cfg: dict = SD_V15_CLIP_TEXT) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of every tensor of the text tower of transformers' `CLIPTextModel` in the module's own order, without a prefix.
    `embeddings.position_ids` is a buffer, not a weight, and is not listed.  Needs no device."""
    c = _check_cfg(cfg)
    W, I = c["width"], c["intermediate"]
    out: List[Tuple[str, Tuple[int, ...]]] = [("embeddings.token_embedding.weight", (c["vocab"], W)),
                                              ("embeddings.position_embedding.weight", (c["positions"], W))]
    for i in range(c["layers"]):
        l = f"encoder.layers.{i}"
        for p in ("k_proj", "v_proj", "q_proj", "out_proj"):
            wb(out, f"{l}.self_attn.{p}", W, W)
        wb(out, f"{l}.layer_norm1", W)
        wb(out, f"{l}.mlp.fc1", I, W)
        wb(out, f"{l}.mlp.fc2", W, I)
        wb(out, f"{l}.layer_norm2", W)
    wb(out, "final_layer_norm", W)
    return out


def random_clip_text_state_dict(seed: int, cfg: dict = SD_V15_CLIP_TEXT) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for the absent checkpoint, built like `random_controlnet_state_dict`: fan-in-scaled normal matrices (the two
    embedding tables among them), norm scales around 1, small biases."""
    return random_tensors(clip_text_tensors(cfg), int(seed) + 86028121)


def load_clip_text_tensors(state_dict: Dict[str, torch.Tensor], cfg: dict = SD_V15_CLIP_TEXT,
                           prefix: str = "cond_stage_model.transformer.") -> Dict[str, torch.Tensor]:
    """The tower's tensors as fp32 CPU tensors under the keys of `clip_text_tensors`, read under `prefix` with or without a
    following `text_model.` (SD checkpoints carry it; the CLIPTextModel of transformers 5 does not).  `embeddings.position_ids` is
    ignored.  KeyError for a missing key, ValueError for a wrong shape.  Needs no device."""
    want = clip_text_tensors(cfg)
    if any(k.startswith(prefix + "text_model.") for k in state_dict):
        prefix += "text_model."
    return load_tensors(state_dict, want, prefix, "CLIP text")


def chunk_tokens(raw: Sequence[Sequence[int]], bos: int, eos: int, pad: int, chunks: int = CHUNKS, chunk_len: int = CHUNK_LEN
                 ) -> torch.Tensor:
    """hack.py:49-62 on the host: per prompt, the first chunks * chunk_len raw ids are cut into `chunks` pieces (later ids are dropped,
    as the reference drops them), each piece -- the empty ones too -- becomes [bos] + piece + [eos] padded with `pad` to
    chunk_len + 2.  raw: one id list per prompt -> int32 [B, chunks, chunk_len + 2] on the CPU."""
    out = torch.full((len(raw), chunks, chunk_len + 2), int(pad), dtype=torch.int32)
    for b, ids in enumerate(raw):
        ids = [int(v) for v in ids]
        for f in range(chunks):
            piece = [int(bos)] + ids[f * chunk_len:(f + 1) * chunk_len] + [int(eos)]
            out[b, f, :len(piece)] = torch.tensor(piece, dtype=torch.int32)
    return out


def tokenize_prompts(texts: Sequence[str], tokenizer) -> torch.Tensor:
    """hack.py:33-40, :55-62: '_' becomes a space, `tokenizer(texts, truncation=False, add_special_tokens=False)["input_ids"]`, the
    special ids from the tokenizer's `bos_token_id / eos_token_id / pad_token_id` -> `chunk_tokens` of them, int32 [B,3,77]."""
    if isinstance(texts, str):
        raise TypeError("texts is a list of prompts (the reference passes [c_text])")
    raw = tokenizer([t.replace("_", " ") for t in texts], truncation=False, add_special_tokens=False)["input_ids"]
    return chunk_tokens(raw, tokenizer.bos_token_id, tokenizer.eos_token_id, tokenizer.pad_token_id)


def _torch_glue() -> bool:
    """OFX_CLIP_TORCH_GLUE=1 (A/B baseline and diagnostic, read once per process): the embedding and quick_gelu through torch ops."""
    return env_flag("OFX_CLIP_TORCH_GLUE")


class ClipTextEncoder(DeviceModel):
    """`FrozenCLIPEmbedder` under `hack.hack_everything(clip_skip)` (inference) on a HIP device."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: dict = SD_V15_CLIP_TEXT, device="cuda",
                 prefix: str = "cond_stage_model.transformer.", clip_skip: int = 0, dedupe: bool = True):
        c = _check_cfg(cfg)                                        # everything up to the device check needs no device
        self.cfg = c
        self.width, self.heads, self.layers, self.positions, self.vocab = c["width"], c["heads"], c["layers"], c["positions"], c["vocab"]
        self.d_head = self.width // self.heads
        self.clip_skip = int(clip_skip)
        if self.clip_skip < 0 or self.clip_skip > self.layers + 1:
            raise ValueError(f"clip_skip must be in [0, {self.layers + 1}] (hidden_states has layers + 1 entries), got {clip_skip}")
        # hack.py:42-47: final_layer_norm of hidden_states[-clip_skip] (the embedding output and every layer output) when
        # clip_skip > 1, of the last layer's output otherwise; layers past the one used are not run
        self.layers_run = self.layers if self.clip_skip <= 1 else self.layers + 1 - self.clip_skip
        self.dedupe = bool(dedupe)
        self.precision = "fp32"                                    # the arithmetic of every `_gemm`
        t32 = load_clip_text_tensors(state_dict, c, prefix)
        self._use_device(device)
        # weights are laid out once: every Linear a packed 1x1 convolution operand [Cout, Kpad]; q_proj | k_proj | v_proj one
        # [3*width, width] operand with one concatenated bias; the two embedding tables stay the checkpoint's row-major tensors
        self.tok = t32["embeddings.token_embedding.weight"].contiguous().to(self.device)
        self.pos = t32["embeddings.position_embedding.weight"].contiguous().to(self.device)
        for i in range(self.layers):
            l = f"encoder.layers.{i}"
            self._put_gemm(f"{l}.self_attn.qkv", t32, f"{l}.self_attn.q_proj", f"{l}.self_attn.k_proj", f"{l}.self_attn.v_proj", bias=True)
            for n in ("self_attn.out_proj", "mlp.fc1", "mlp.fc2"):
                self._put_gemm(f"{l}.{n}", t32, f"{l}.{n}", bias=True)
        for key, t in t32.items():
            if t.dim() == 1 and ("layer_norm" in key):
                self._put(key, t)
        self.torch_glue = _torch_glue()
        self._causal: Dict[int, torch.Tensor] = {}
        self.embed_calls = 0           # how often the embedding ran, and the rows (sequences * T) of its last run: what `dedupe` saves
        self.embed_rows = 0

    # ---- building blocks ------------------------------------------------------------------------------------------
    def causal_bias(self, T: int) -> torch.Tensor:
        """[T,T] fp32 on the device: 0 on and below the diagonal, -inf above (keys after the query are masked).  Built once per T."""
        if T not in self._causal:
            self._causal[T] = torch.full((T, T), float("-inf"), dtype=torch.float32).triu(1).to(self.device)
        return self._causal[T]

    def _layernorm(self, name: str, x: torch.Tensor) -> torch.Tensor:
        return ops.layernorm(x, self.w[f"{name}.weight"], self.w[f"{name}.bias"], LN_EPS)

    def _embed(self, ids: torch.Tensor) -> torch.Tensor:
        S, T = ids.shape
        self.embed_calls += 1
        self.embed_rows = S * T
        if self.torch_glue:
            return (F.embedding(ids.long(), self.tok) + self.pos[:T]).contiguous()
        return ops.clip_embed(ids, self.tok, self.pos, T)

    def _quick_gelu_(self, m: torch.Tensor) -> torch.Tensor:
        if self.torch_glue:
            return m.mul_(torch.sigmoid(1.702 * m))
        return ops.quick_gelu(m, out=m)

    def _layer(self, i: int, x: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
        """CLIPEncoderLayer.forward on x [S, T, width]: the 8 launches of the module docstring."""
        l = f"encoder.layers.{i}"
        W = self.width
        qkv = self._gemm(f"{l}.self_attn.qkv", self._layernorm(f"{l}.layer_norm1", x), True)
        a = ops.attention_bnhd(qkv[..., :W], qkv[..., W:2 * W], qkv[..., 2 * W:], self.heads, bias=bias, scale=self.d_head ** -0.5)
        x = self._gemm(f"{l}.self_attn.out_proj", a, True, addend=x)
        m = self._gemm(f"{l}.mlp.fc1", self._layernorm(f"{l}.layer_norm2", x), True)
        return self._gemm(f"{l}.mlp.fc2", self._quick_gelu_(m), True, addend=x)

    # ---- forward --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_ids(self, ids, hidden_states: bool = False):
        """The transformer proper (hack.py:42-47): ids [S,T] integers, T <= positions -> final_layer_norm(h) fp32 [S,T,width] on the
        device, h the last layer's output (clip_skip <= 1) or hidden_states[-clip_skip].  With `hidden_states`, (that, the list of
        the embedding output and every layer output that was run).  ids as a list or a CPU tensor are checked against [0, vocab)
        (ValueError) and, with `dedupe`, identical rows are encoded once; ids already on the device are used as they are (an id
        out of range gives a NaN row, `ops.clip_embed`)."""
        inverse = None
        if torch.is_tensor(ids) and ids.is_cuda:
            if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64):
                raise RuntimeError("ids must be an integer tensor [S,T]")
            dev_ids = ids.to(torch.int32).contiguous()
        else:
            host = torch.as_tensor(ids)
            if host.dim() != 2 or host.dtype.is_floating_point or host.dtype == torch.bool or host.numel() == 0:
                raise RuntimeError("ids must be a non-empty integer tensor or list [S,T]")
            host = host.to(torch.int64)
            if host.shape[1] > self.positions:
                raise ValueError(f"ids [S,T] need T <= {self.positions}, got T = {host.shape[1]}")
            if int(host.min()) < 0 or int(host.max()) >= self.vocab:
                raise ValueError(f"token ids must be in [0, {self.vocab}), got [{int(host.min())}, {int(host.max())}]")
            if self.dedupe:
                uniq, inv = torch.unique(host, dim=0, return_inverse=True)
                if uniq.shape[0] < host.shape[0]:
                    host, inverse = uniq, inv.to(self.device)
            dev_ids = host.to(torch.int32).contiguous().to(self.device)
        S, T = dev_ids.shape
        if S == 0 or T == 0 or T > self.positions:
            raise ValueError(f"ids [S,T] need S >= 1 and 1 <= T <= {self.positions}, got {(S, T)}")
        check_activation_bytes(S * T * max(self.cfg["intermediate"], 3 * self.width) * 4,
                               "an activation would pass 2 GiB (32-bit byte offsets in the GEMM): slice the sequences")
        bias = self.causal_bias(T)
        x = self._embed(dev_ids)
        hs = [x]
        for i in range(self.layers_run):
            x = self._layer(i, x, bias)
            if hidden_states:
                hs.append(x)
        out = self._layernorm("final_layer_norm", x)
        if inverse is not None:
            out = out.index_select(0, inverse)
            hs = [h.index_select(0, inverse) for h in hs] if hidden_states else hs
        return (out, hs) if hidden_states else out

    @torch.no_grad()
    def forward_tokens(self, tokens) -> torch.Tensor:
        """hack.py:64-70: tokens [B,F,T] integers (`chunk_tokens`: F = 3, T = 77) -> [B, F*T, width]; the `(b f) i` and
        `b (f i) c` rearrangements are views."""
        tokens = torch.as_tensor(tokens)
        if tokens.dim() != 3:
            raise RuntimeError("tokens must be [B,F,T]")
        B, Fn, T = tokens.shape
        return self.encode_ids(tokens.reshape(B * Fn, T)).view(B, Fn * T, self.width)

    def encode(self, texts: Sequence[str], tokenizer) -> torch.Tensor:
        """`FrozenCLIPEmbedder.forward(texts)` as hack.py replaces it: prompts -> [B,231,width].  `tokenizer`: any object with the
        transformers tokenizer's call interface and `bos_token_id / eos_token_id / pad_token_id` (`tokenize_prompts`)."""
        return self.forward_tokens(tokenize_prompts(texts, tokenizer))

    @torch.no_grad()
    def conditioning(self, tokens_c, tokens_uc) -> Tuple[torch.Tensor, torch.Tensor]:
        """Both `get_learned_conditioning` calls of an `img2img*` (guided_ldm_inpainting.py:200-203) in one pass: tokens_c, tokens_uc
        [B,3,77] on the host -> (context, unconditional_context), two contiguous fp32 [B,231,width] device tensors: the operands of
        `sampler.img2img_inpaint` and `GuidedDDIMSampler.decode`."""
        tc, tu = torch.as_tensor(tokens_c), torch.as_tensor(tokens_uc)
        if tc.dim() != 3 or tuple(tc.shape) != tuple(tu.shape):
            raise RuntimeError(f"tokens_c and tokens_uc must be [B,F,T] of one shape, got {tuple(tc.shape)} and {tuple(tu.shape)}")
        B = tc.shape[0]
        both = self.forward_tokens(torch.cat([tc, tu.to(tc.device)]))
        return both[:B], both[B:]
