"""`SpatialTransformer` of the reference's UNet on the device, with the K/V history of reference frames.

ldm/modules/attention.py is the one UNet file the reference rewrote: `SpatialTransformer.forward` (:515-537) ->
`BasicTransformerBlock._forward` (:464-469) -> `MemoryEfficientCrossAttention.forward` (:326-436).  Its self-attention hands back
its own K/V (`kv_hist`, :353) and can attend to the K/V of reference frames instead (`ref_kv_hists`, :358-369): the mechanism behind
`generate_ai_frame_with_ref_self_attn` and `VideoData.put_kv / get_kv`.

Everything runs through the C ABI of libofx.so on NHWC fp32: GroupNorm(32, eps 1e-6) (`ofx_groupnorm`), `proj_in` / `proj_out` and
every Linear as 1x1 `ofx_conv2d` GEMMs on the fp32 matrix cores (biases and the residual sums in the epilogue), LayerNorm
(`ofx_layernorm`), GEGLU (`ofx_geglu`) and the fused attention kernel on token rows (`ofx_attention_bnhd_f32`), which reads q / k / v
where the projection GEMM left them: the NHWC output of `proj_in` already is the token matrix [B, h*w, inner], `to_q | to_k | to_v`
of the self-attention are one GEMM into one [B, N, 3*inner] buffer whose thirds are the attention's operands, and no activation is
permuted or copied between layouts anywhere but at the NCHW edges of `forward`.  The K/V history stays on the device, as
[B, N, inner] tensors (`to_reference_layout` gives the reference's [(b h), n, d]).

`precision=` ("fp32" default, "fp16", "bf16x3", "bf16x6") chooses the arithmetic of the GEMMs alone: `proj_in` / `proj_out`, the
q / k / v / out projections and the two feed-forward GEMMs.  "fp16" rounds both operands of each to half as the kernel stages them
and accumulates in fp32 (what torch.autocast gives the reference's Linears); the split-bf16 modes are the launcher's existing ones.
GroupNorm, LayerNorm, GEGLU, the attention (softmax included) and every activation in memory stay fp32 in every precision -- closer
to float64 than autocast, which also rounds each layer's output and runs attention in half.

`attention_precision=` ("fp32" default, "fp16") is separate and chooses the arithmetic of the fused attention kernel alone
(`ofx_attention_bnhd_prec`): "fp16" rounds q, k, v and the probabilities to half as the kernel stages them and runs both products
on the fp16 matrix cores with fp32 accumulation; the softmax, the scale and the tensors in memory stay fp32, and `kv_hists` -- taken
before the attention -- are exactly what they are without it.  It exists on the fused route only: with OFX_ST_TORCH_GLUE=1, or a head
size outside `FUSED_HEAD_SIZES`, "fp16" is a ValueError at construction (no silent fallback).

Reference K/V are read in place: on the fused route the entries of `reference_kv` reach the kernel as a per-image segment table
(`ops.attention_bnhd_segments`, `ofx_attention_bnhd_segs`), float32 or float16 as they are stored, bit for bit what attending to
their float32 concatenation gives; nothing is widened or joined with torch.cat, and the "positive" mode is one launch (image 0's
segment is its own k / v thirds of the qkv buffer) unless the history is float16, where it stays two (one element type per launch).
`plan_kv_route` decides from shapes and dtypes alone; entries in the reference's [(b h), n, d] layout, mixed dtypes, tables beyond
8 segments per image / 64 per launch and the unfused routes keep the concatenation path, which widens float16 entries.
`kv_dtype=` ("fp32" default, "fp16") is the dtype of the returned `kv_hists`: "fp16" rounds the block's own K/V to half (nearest
even, beyond +-65504 to infinity, as under torch.autocast, whose `kv_hist` is half too) -- half the memory and half the pickle.  The
block's own attention still reads the float32 K/V.  Histories of either dtype are accepted as `reference_kv`.  A float16 history
pairs with `attention_precision="fp16"`, where a launch on half entries is about 14 % faster than the concatenation path; with
fp32 attention it trades time for memory: the fp32 kernel widens half rows as it stages them and a launch is about 15 % slower
than widening and concatenating first (2.60 against 2.26 ms at 6144 queries x 12288 keys, profiles/r38_kv_history_rate.txt).

OFX_ST_KV_CONCAT=1 in the environment (read once per process; the A/B baseline and a diagnostic): reference K/V always take the
concatenation path.

OFX_ST_TORCH_GLUE=1 in the environment (read once per process; the A/B baseline and a diagnostic): LayerNorm and GEGLU through
torch.nn.functional, attention through permute + `ops.attention`, i.e. the glue this module replaces.  Head sizes the fused kernel
does not take (`FUSED_HEAD_SIZES`) go the permute + `ops.attention` way on their own.

State-dict keys are the reference's (`use_linear=False`, the conv `proj_in` / `proj_out` that guided_ldm_*_v15.yaml builds); a
full-checkpoint prefix such as `model.diffusion_model.input_blocks.1.1.` goes through `prefix`.  The checkpoint check, the packing
of the weights (several Linears side by side as one 1x1 operand) and the GEMM call are `modelbase`'s.  No checkpoint ships with the
reference tree: parity is pinned with seeded weights loaded into the reference's own module
(tests/golden/make_golden_transformer.py).
"""
from __future__ import annotations

import ctypes
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import ops
from .modelbase import DeviceModel, check_activation_bytes, check_weight_dtype, env_flag, is_f32_cuda, load_tensors, random_tensors, wb

FUSED_HEAD_SIZES = (40, 64, 80, 128, 160)      # ofx_attention_flash_ok (csrc/attn_flash.hip)
# `precision=` of SpatialTransformer / UNetModel: the arithmetic of every `ops.conv2d_nhwc` contraction (weights stay plain fp32)
MODEL_PRECISIONS = ("fp32", "fp16", "bf16x3", "bf16x6")


def check_precision(precision) -> str:
    if precision not in MODEL_PRECISIONS:
        raise ValueError(f"precision must be one of {MODEL_PRECISIONS}, got {precision!r}")
    return precision


def spatial_transformer_tensors(in_channels: int, n_heads: int, d_head: int, context_dim: Optional[int], depth: int = 1
                                ) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of every tensor of a `SpatialTransformer(in_channels, n_heads, d_head, depth, context_dim=context_dim)` with
    use_linear=False, in the module's own order (26 per depth-1 module).  context_dim None: the cross-attention's K / V read the
    tokens themselves (attention.py:208)."""
    inner = n_heads * d_head
    ctx = inner if context_dim is None else int(context_dim)
    out: List[Tuple[str, Tuple[int, ...]]] = []

    def attn(name, kv_dim):
        out.append((f"{name}.to_q.weight", (inner, inner)))
        out.append((f"{name}.to_k.weight", (inner, kv_dim)))
        out.append((f"{name}.to_v.weight", (inner, kv_dim)))
        wb(out, f"{name}.to_out.0", inner, inner)

    wb(out, "norm", in_channels)
    wb(out, "proj_in", inner, in_channels, 1, 1)
    for i in range(depth):
        blk = f"transformer_blocks.{i}"
        attn(f"{blk}.attn1", inner)
        wb(out, f"{blk}.ff.net.0.proj", 8 * inner, inner)       # FeedForward(mult=4, glu=True): values and gates
        wb(out, f"{blk}.ff.net.2", inner, 4 * inner)
        attn(f"{blk}.attn2", ctx)
        for n in ("norm1", "norm2", "norm3"):
            wb(out, f"{blk}.{n}", inner)
    wb(out, "proj_out", in_channels, inner, 1, 1)
    return out


def random_spatial_transformer_state_dict(seed: int, in_channels: int, n_heads: int, d_head: int, context_dim: Optional[int],
                                          depth: int = 1) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for the absent checkpoint: fan-in-scaled normal weights, norm scales around 1, small biases.  `proj_out` is
    NOT zeroed (the reference zero-initialises it before training, :506; zeroed, the module would be the identity)."""
    return random_tensors(spatial_transformer_tensors(in_channels, n_heads, d_head, context_dim, depth), int(seed) + 15485863)


def _torch_glue() -> bool:
    """OFX_ST_TORCH_GLUE=1 (A/B baseline and diagnostic, read once per process): LayerNorm / GEGLU through torch.nn.functional and
    attention through permute + `ops.attention`."""
    return env_flag("OFX_ST_TORCH_GLUE")


_torch_glue.cache_clear = env_flag.cache_clear                     # the switch stays clearable where a test changes the environment


def to_reference_layout(t: torch.Tensor, heads: int) -> torch.Tensor:
    """[B, N, heads*d] -> the reference's [(b h), n, d] (attention.py:338-345)."""
    B, N, inner = t.shape
    return t.reshape(B, N, heads, inner // heads).permute(0, 2, 1, 3).reshape(B * heads, N, inner // heads).contiguous()


def from_reference_layout(t: torch.Tensor, heads: int) -> torch.Tensor:
    """The reference's [(b h), n, d] -> [B, N, heads*d]."""
    BH, N, d = t.shape
    return t.reshape(BH // heads, heads, N, d).permute(0, 2, 1, 3).reshape(BH // heads, N, heads * d).contiguous()


def plan_reference_kv(shapes: Sequence[Tuple[Tuple[int, ...], Tuple[int, ...]]], B: int, N: int, heads: int, d_head: int
                      ) -> Tuple[str, int, List[bool]]:
    """What attention.py:358-369 does with reference K/V of these (k shape, v shape) pairs for a batch of B images of N tokens,
    decided from the shapes alone (no device): ("all", tokens, ...) -- every image attends to the references' `tokens` keys and not
    to its own; ("positive", N, ...) -- references of batch B - 1 with exactly N tokens in total replace the K/V of images 1..B-1,
    image 0 (the unconditional half) keeps its own (`k[nhead:] = k2`).  The third item says per entry whether it is in the
    reference's [(b h), n, d] layout (last dimension d_head) rather than [b, n, heads*d_head].  Any other combination is a
    ValueError (the reference fails there with a shape error)."""
    inner = heads * d_head
    if not shapes:
        raise ValueError("reference_kv is empty")
    batches, tokens, ref_layout = [], 0, []
    for i, (ks, vs) in enumerate(shapes):
        ks, vs = tuple(int(s) for s in ks), tuple(int(s) for s in vs)
        if ks != vs or len(ks) != 3 or min(ks) <= 0:
            raise ValueError(f"reference_kv[{i}]: k and v must be 3-D tensors of one shape, got {ks} and {vs}")
        if ks[2] == inner:
            ref_layout.append(False)
            batches.append(ks[0])
        elif ks[2] == d_head and ks[0] % heads == 0:
            ref_layout.append(True)
            batches.append(ks[0] // heads)
        else:
            raise ValueError(f"reference_kv[{i}]: last dimension {ks[2]} is neither heads * d_head = {inner} ([b, n, h*d]) nor "
                             f"d_head = {d_head} ([(b h), n, d])")
        tokens += ks[1]
    if len(set(batches)) != 1:
        raise ValueError(f"reference_kv entries have different batch sizes {batches}")
    b = batches[0]
    if b == B:
        return "all", tokens, ref_layout
    if b == B - 1 and tokens == N:
        return "positive", tokens, ref_layout
    raise ValueError(f"reference_kv of batch {b} with {tokens} tokens does not fit {B} images of {N} tokens: batch {B} (any token "
                     f"count), or batch {B - 1} with exactly {N} tokens")


def _kv_concat() -> bool:
    """OFX_ST_KV_CONCAT=1 (A/B baseline and diagnostic, read once per process): reference K/V always go the concatenation way --
    every entry widened to float32, several joined with torch.cat -- and never through the segment table."""
    return env_flag("OFX_ST_KV_CONCAT")


_kv_concat.cache_clear = env_flag.cache_clear                      # clearable like _torch_glue, where a test changes the environment


KV_MAX_SEGMENTS, KV_MAX_ENTRIES = 8, 64        # OFX_KV_MAX_SEGMENTS / OFX_KV_MAX_ENTRIES (include/ofx.h)


def plan_kv_route(mode: str, dtypes: Sequence, ref_layout: Sequence[bool], B: int, d_head: int, *, torch_glue: bool = False,
                  force_concat: bool = False) -> str:
    """How the self-attention reads reference K/V entries of these dtypes (torch dtypes or their names) for a batch of B images,
    decided from metadata alone (no device): "segments" -- the fused kernel reads every entry in place through a segment table
    (`ops.attention_bnhd_segments`), nothing is widened or concatenated; "segments+own" -- `mode` "positive" with a float16 history:
    image 0 on its own float32 K/V in one launch, images 1.. on the segments in a second (one element type per launch); "concat"
    -- today's path, entries widened to float32 and joined with torch.cat.  "concat" is what remains for entries in the reference's
    [(b h), n, d] layout, head sizes outside FUSED_HEAD_SIZES, OFX_ST_TORCH_GLUE=1 (`torch_glue`), OFX_ST_KV_CONCAT=1
    (`force_concat`), entries of mixed or other dtypes, and tables beyond 8 segments per image or 64 entries per launch.
    The arithmetic of the attention is not asked: a float16 history under fp32 attention stays on the segment route, which keeps
    its memory saving (nothing is widened in memory) at the cost of a slower launch -- the trade stated in the module docstring."""
    if mode not in ("all", "positive"):
        raise ValueError(f"mode must be 'all' or 'positive', got {mode!r}")
    names = {str(d).replace("torch.", "") for d in dtypes}
    if force_concat or torch_glue or int(d_head) not in FUSED_HEAD_SIZES or any(ref_layout) or len(names) != 1:
        return "concat"
    dt = next(iter(names))
    if dt not in ("float32", "float16"):
        return "concat"
    E = len(ref_layout)                                            # entries; `dtypes` may name every k and v tensor, or one per entry
    if E < 1 or E > KV_MAX_SEGMENTS:
        return "concat"
    if mode == "all":
        return "segments" if B * E <= KV_MAX_ENTRIES else "concat"
    if dt == "float32":                                            # image 0's own k / v is one more segment of the same launch
        return "segments" if 1 + (B - 1) * E <= KV_MAX_ENTRIES else "concat"
    return "segments+own" if (B - 1) * E <= KV_MAX_ENTRIES else "concat"


class SpatialTransformer(DeviceModel):
    """`ldm.modules.attention.SpatialTransformer` (use_linear=False, inference) on a HIP device.  `weight_dtype`: "fp32" (default)
    or "fp16" (with precision="fp16" only): `proj_in` / `proj_out` and every Linear are stored in half and read by the same fp16
    kernels, bit-identical results; norm scales and biases stay fp32 (`modelbase.DeviceModel`)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], n_heads: int, d_head: int, device="cuda", prefix: str = "",
                 use_linear: bool = False, precision: str = "fp32", attention_precision: str = "fp32", kv_dtype: str = "fp32",
                 weight_dtype: str = "fp32"):
        self.precision = check_precision(precision)                # before the checkpoint is looked at or a device asked for
        self.weight_dtype = check_weight_dtype(weight_dtype, self.precision)   # storage of the GEMM operands (`DeviceModel`)
        self.attention_precision = ops.check_attention_precision(attention_precision, "attention_precision")
        self.kv_dtype = ops.check_kv_dtype(kv_dtype)
        self.kv_concat = _kv_concat()
        self._kv_memo = None                                       # `_reference_kv`: the plan of the previous call's reference tensors
        if self.attention_precision != "fp32":                     # the fused kernel only: no unfused fp16 path, no silent fallback
            if _torch_glue():
                raise ValueError(f"attention_precision={attention_precision!r} does not combine with OFX_ST_TORCH_GLUE=1")
            if int(d_head) not in FUSED_HEAD_SIZES:
                raise ValueError(f"attention_precision={attention_precision!r} needs d_head in {FUSED_HEAD_SIZES}, got {d_head}")
        if use_linear:
            raise NotImplementedError("use_linear=True (Linear proj_in / proj_out) is not what guided_ldm_*_v15.yaml builds")
        self._use_device(device)                                   # this class asks for the device before it reads the checkpoint
        self.heads, self.d_head, self.inner = int(n_heads), int(d_head), int(n_heads) * int(d_head)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        if "norm.weight" not in sd or "proj_in.weight" not in sd:
            raise KeyError(f"SpatialTransformer checkpoint lacks {prefix}norm.weight / {prefix}proj_in.weight")
        self.in_channels = int(sd["norm.weight"].shape[0])
        self.depth = 1 + max([int(k.split(".")[1]) for k in sd if k.startswith("transformer_blocks.")], default=-1)
        kkey = "transformer_blocks.0.attn2.to_k.weight"
        if self.depth < 1 or kkey not in sd:
            raise KeyError(f"SpatialTransformer checkpoint lacks {prefix}{kkey}")
        self.context_dim = int(sd[kkey].shape[1]) if sd[kkey].dim() == 2 else -1
        if self.in_channels % 32 or self.inner % 4 or self.context_dim % 4:
            raise ValueError("in_channels must be a multiple of 32 (GroupNorm), n_heads * d_head and context_dim multiples of 4")
        t32 = load_tensors(state_dict, spatial_transformer_tensors(self.in_channels, self.heads, self.d_head, self.context_dim, self.depth),
                           prefix, "SpatialTransformer")
        # weights are laid out once: every Linear a 1x1 convolution operand [Cout, Kpad]; to_q | to_k | to_v of the self-attention
        # (no bias, one input) one [3*inner, inner] operand, to_k | to_v of the cross-attention one [2*inner, context_dim] operand
        for key, t in t32.items():
            if t.dim() == 1:
                self._put(key, t)
        self._put_gemm("proj_in", t32, "proj_in")
        self._put_gemm("proj_out", t32, "proj_out")
        for i in range(self.depth):
            b = f"transformer_blocks.{i}"
            self._put_gemm(f"{b}.attn1.to_qkv", t32, f"{b}.attn1.to_q", f"{b}.attn1.to_k", f"{b}.attn1.to_v")
            self._put_gemm(f"{b}.attn2.to_q", t32, f"{b}.attn2.to_q")
            self._put_gemm(f"{b}.attn2.to_kv", t32, f"{b}.attn2.to_k", f"{b}.attn2.to_v")
            for n in ("attn1.to_out.0", "attn2.to_out.0", "ff.net.0.proj", "ff.net.2"):
                self._put_gemm(f"{b}.{n}", t32, f"{b}.{n}")
        self.torch_glue = _torch_glue()
        self.fused_attention = (not self.torch_glue) and self.d_head in FUSED_HEAD_SIZES

    # ---- building blocks ------------------------------------------------------------------------------------------
    def _layernorm(self, name: str, x: torch.Tensor) -> torch.Tensor:
        if self.torch_glue:
            return F.layer_norm(x, (x.shape[-1],), self.w[f"{name}.weight"], self.w[f"{name}.bias"], 1e-5)
        return ops.layernorm(x, self.w[f"{name}.weight"], self.w[f"{name}.bias"], 1e-5)

    def _geglu(self, a: torch.Tensor) -> torch.Tensor:
        if self.torch_glue:
            v, gate = a.chunk(2, dim=-1)
            return (v * F.gelu(gate)).contiguous()
        return ops.geglu(a)

    def _attention(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """q [B,Nq,inner], k / v [B,Nk,inner] (possibly slices of wider GEMM outputs) -> [B,Nq,inner], written to `out` when given."""
        if self.fused_attention:
            return ops.attention_bnhd(q, k, v, self.heads, out=out, precision=self.attention_precision)
        # the glue this module replaces (attention.py:338-345, :430-435): [(b h), n, d] copies in, one copy out
        B, Nq, _ = q.shape
        o = ops.attention(*(to_reference_layout(t, self.heads) for t in (q, k, v)))
        o = o.view(B, self.heads, Nq, self.d_head).permute(0, 2, 1, 3).reshape(B, Nq, self.inner)
        if out is None:
            return o.contiguous()
        out.copy_(o)
        return out

    def _attention_segments(self, q: torch.Tensor, table, nk: int, half: bool, out: Optional[torch.Tensor] = None, ctab=None) -> torch.Tensor:
        """`ops.attention_bnhd_segments` on table rows per image (`_reference_kv`): one launch, K / V read where they lie.  ctab: the
        (`ofx_kv_segment` array, counts) of exactly these rows, where `_reference_kv` has built them already."""
        if ctab is None:
            ctab = (ops._kv_segment_table([r for t in table for r in t]), (ctypes.c_int * len(table))(*[len(t) for t in table]))
        return ops._attention_bnhd_segment_table(q, ctab[0], ctab[1], half, nk, self.heads, out=out, precision=self.attention_precision)

    def _reference_kv(self, reference_kv, B: int, N: int):
        """-> None, or (mode, route, payload) with `route` of `plan_kv_route`.  "concat": payload = (k, v) on the device in our
        layout, float32, entries concatenated along tokens (attention.py:361-362).  "segments" / "segments+own": payload = (table, tokens, half,
        tensors, ctab): table[b] holds the `ofx_kv_segment` rows of every entry for reference image b, in the entries' own dtype and
        memory (`tensors` keeps them alive) -- nothing widened, nothing concatenated."""
        if not reference_kv:
            return None
        entries = [tuple(e) for e in reference_kv]
        if any(len(e) not in (2, 3) for e in entries):
            raise ValueError("reference_kv entries are (k, v) or (k, v, layer) tuples")
        # A sampler hands every UNet call of a frame the SAME tensors: the plan and the table of the previous call are kept (by weak
        # reference: no history is kept alive here) and reused while every entry is that very tensor at that very address
        ts = [t for e in entries for t in e[:2]]
        m = self._kv_memo
        if m is not None and m[0] == (B, N, len(ts)) and all(r() is t and p == t.data_ptr() and sh == t.shape
                                                             for (r, p, sh), t in zip(m[1], ts)):
            return m[2]
        self._kv_memo = None
        mode, _, ref_layout = plan_reference_kv([(e[0].shape, e[1].shape) for e in entries], B, N, self.heads, self.d_head)
        route = plan_kv_route(mode, [t.dtype for e in entries for t in e[:2]], ref_layout, B, self.d_head, torch_glue=self.torch_glue,
                              force_concat=self.kv_concat)
        if route != "concat":
            # rows the kernel can load 4 elements at a time where they are; anything else (never a recorded history) is copied once
            rows = lambda t: t if (t.stride(2) == 1 and t.stride(1) >= t.shape[2] and t.stride(1) % 4 == 0 and t.stride(0) % 4 == 0
                                   and t.data_ptr() % (4 * t.element_size()) == 0) else t.contiguous()
            dev = [(rows(e[0].to(self.device)), rows(e[1].to(self.device))) for e in entries]
            # the table rows (k pointer, v pointer, tokens, row strides) of every reference image, by pointer arithmetic: this
            # forward is host-enqueue bound, and a tensor view per image and entry costs more than the launch it feeds
            es = dev[0][0].element_size()
            table = [[(k.data_ptr() + b * k.stride(0) * es, v.data_ptr() + b * v.stride(0) * es, int(k.shape[1]), int(k.stride(1)),
                       int(v.stride(1))) for k, v in dev] for b in range(dev[0][0].shape[0])]
            # "all": the table is the launch's own, built once; "positive" prepends image 0's k / v of each call
            ctab = (ops._kv_segment_table([r for t in table for r in t]), (ctypes.c_int * len(table))(*[len(t) for t in table])) \
                if mode == "all" else None
            ref = (mode, route, (table, sum(int(k.shape[1]) for k, _ in dev), dev[0][0].dtype == torch.float16, dev, ctab))
            if all(d is t for d, t in zip((d for pair in dev for d in pair), ts)):      # read where the caller's tensors lie: no copy of ours
                self._kv_memo = ((B, N, len(ts)), [(weakref.ref(t), t.data_ptr(), t.shape) for t in ts], ref[:2] + (ref[2][:3] + (None, ctab),))
            return ref
        ks, vs = [], []
        for e, rl in zip(entries, ref_layout):
            for t, dst in ((e[0], ks), (e[1], vs)):
                t = t.to(device=self.device, dtype=torch.float32)
                dst.append(from_reference_layout(t, self.heads) if rl else t.contiguous())
        k = ks[0] if len(ks) == 1 else torch.cat(ks, dim=1)
        v = vs[0] if len(vs) == 1 else torch.cat(vs, dim=1)
        return mode, "concat", (k, v)

    def _block(self, i: int, x: torch.Tensor, context: Optional[torch.Tensor], ref) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """BasicTransformerBlock._forward (:464-469) on tokens x [B, N, inner]."""
        b = f"transformer_blocks.{i}"
        inner = self.inner
        B, N, _ = x.shape
        # self-attention: one GEMM for q | k | v, the attention reads its thirds in place
        qkv = self._gemm(f"{b}.attn1.to_qkv", self._layernorm(f"{b}.norm1", x), False)
        q, k, v = qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:]
        # the block's own K/V, recorded before any replacement (:353); kv_dtype="fp16": one rounding copy (nearest even, beyond
        # +-65504 to infinity, as under autocast) in place of the plain one
        kv_hist = (k.contiguous(), v.contiguous()) if self.kv_dtype == "fp32" else tuple(
            torch.empty((B, N, inner), dtype=torch.float16, device=x.device).copy_(t) for t in (k, v))
        if ref is None:
            a = self._attention(q, k, v)
        elif ref[1] == "segments":
            # the fused kernel reads every entry where it lies; "positive" (:365-366): image 0's segment is its own k / v thirds
            table, nk, half, _, ctab = ref[2]
            if ref[0] != "all":
                table = [[(k.data_ptr(), v.data_ptr(), N, int(k.stride(1)), int(v.stride(1)))]] + table
            a = self._attention_segments(q, table, nk, half, ctab=ctab)
        elif ref[1] == "segments+own":
            # "positive" with a float16 history: one element type per launch, so image 0 on its own float32 K/V stays a launch
            a = torch.empty((B, N, inner), dtype=torch.float32, device=x.device)
            self._attention(q[:1], k[:1], v[:1], out=a[:1])
            table, nk, half, _, _ = ref[2]
            self._attention_segments(q[1:], table, nk, half, out=a[1:])
        elif ref[0] == "all":
            a = self._attention(q, *ref[2])                        # k = k2, v = v2 (:368-369)
        else:
            # k[nhead:] = k2 (:365-366): image 0 on its own K/V, images 1.. on the references'; two launches into one buffer
            a = torch.empty((B, N, inner), dtype=torch.float32, device=x.device)
            self._attention(q[:1], k[:1], v[:1], out=a[:1])
            self._attention(q[1:], *ref[2], out=a[1:])
        x = self._gemm(f"{b}.attn1.to_out.0", a, True, addend=x)
        # cross-attention (a second self-attention without context, :467)
        hn = self._layernorm(f"{b}.norm2", x)
        src = hn if context is None else context
        kv = self._gemm(f"{b}.attn2.to_kv", src, False)
        a = self._attention(self._gemm(f"{b}.attn2.to_q", hn, False), kv[..., :inner], kv[..., inner:])
        x = self._gemm(f"{b}.attn2.to_out.0", a, True, addend=x)
        # feed-forward: Linear -> GEGLU -> Linear (:59-76)
        g = self._geglu(self._gemm(f"{b}.ff.net.0.proj", self._layernorm(f"{b}.norm3", x), True))
        x = self._gemm(f"{b}.ff.net.2", g, True, addend=x)
        return x, kv_hist

    def _contexts(self, context, B: int) -> List[Optional[torch.Tensor]]:
        """One context per block: a tensor serves every block (the reference indexes a list, :517-518, :530)."""
        ctxs = list(context) if isinstance(context, (list, tuple)) else [context] * self.depth
        if len(ctxs) != self.depth:
            raise ValueError(f"{len(ctxs)} contexts for {self.depth} blocks")
        out = []
        for c in ctxs:
            if c is None:
                if self.context_dim != self.inner:
                    raise ValueError(f"context=None needs context_dim == n_heads * d_head, this module has {self.context_dim}")
                out.append(None)
                continue
            if not is_f32_cuda(c, 3) or c.shape[0] != B or c.shape[2] != self.context_dim:
                raise RuntimeError(f"context must be a CUDA float32 tensor [{B},M,{self.context_dim}]")
            out.append(c.contiguous())
        return out

    @torch.no_grad()
    def forward_nhwc(self, x: torch.Tensor, context=None, reference_kv=()) -> Tuple[torch.Tensor, List[Tuple[torch.Tensor, torch.Tensor]]]:
        """`forward` on NHWC: x f32 [B,h,w,C] on the device -> (out [B,h,w,C], kv_hists)."""
        if not is_f32_cuda(x, 4) or x.shape[3] != self.in_channels:
            raise RuntimeError(f"x must be a CUDA float32 tensor with {self.in_channels} channels")
        x = x.contiguous()
        B, h, w, _ = x.shape
        N = h * w
        check_activation_bytes(B * N * 8 * self.inner * 4,
                               "the feed-forward activation would pass 2 GiB (32-bit byte offsets in the GEMM): slice the batch")
        ctxs = self._contexts(context, B)
        ref = self._reference_kv(reference_kv, B, N)               # raises before any launch
        t = ops.groupnorm(x, self.w["norm.weight"], self.w["norm.bias"], 32, 1e-6, False)
        # proj_in / proj_out stay direct calls with constant keys: this forward is host-enqueue bound at the UNet's sizes, and
        # `_conv` would add two name lookups to each (profiles/r30_model_base_rate.txt was measured with these lines)
        t = ops.conv2d_nhwc(t, self.w["proj_in.weight"], 1, 1, self.inner, shift=self.w["proj_in.bias"],
                            precision=self._precision_of(self.w["proj_in.weight"])).view(B, N, self.inner)
        kv_hists = []
        for i in range(self.depth):
            t, kv = self._block(i, t, ctxs[i], ref)
            kv_hists.append(kv)
        out = ops.conv2d_nhwc(t.view(B, h, w, self.inner), self.w["proj_out.weight"], 1, 1, self.in_channels,
                              shift=self.w["proj_out.bias"], addend=x, precision=self._precision_of(self.w["proj_out.weight"]))
        return out, kv_hists

    @torch.no_grad()
    def forward(self, x: torch.Tensor, context=None, reference_kv=()) -> Tuple[torch.Tensor, List[Tuple[torch.Tensor, torch.Tensor]]]:
        """SpatialTransformer.forward (:515-537): x f32 [B,C,h,w] on the device, context [B,M,context_dim] or None, reference_kv a
        sequence of (k, v) or (k, v, layer) -> (x + proj_out(blocks(proj_in(norm(x)))), kv_hists); kv_hists[i] = the own
        self-attention (k, v) of block i, contiguous device tensors [B, h*w, inner]."""
        if not torch.is_tensor(x) or x.dim() != 4:
            raise RuntimeError("x must be a CUDA float32 tensor [B,C,h,w]")
        out, kv = self.forward_nhwc(x.permute(0, 2, 3, 1).contiguous(), context, reference_kv)
        return out.permute(0, 3, 1, 2).contiguous(), kv

    __call__ = forward
