"""Device operators: thin torch-tensor wrappers over the C ABI of libofx.so.

PyTorch is plumbing here (device memory + the current HIP stream); every byte of arithmetic happens
in the hand-written HIP kernels.  Preconditions mirror the reference's extension
(`RAFT/alt_cuda_corr/correlation.cpp:19-21`): tensors must be on the GPU and contiguous, otherwise a
RuntimeError is raised -- nothing silently falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import json
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ConvDesc, check

WARP_MODES = {"bilinear": 0, "bicubic": 1, "cv2_cubic": 2}
ACTS = {None: 0, "none": 0, "relu": 1, "sigmoid": 2, "tanh": 3}
EPI_PLAIN, EPI_GRU_ZR, EPI_GRU_Q, EPI_FLOW = 0, 1, 2, 3
TILE_WINOGRAD = 1      # conv2d_nhwc(tile=): force the fused Winograd kernel, F(2x2,3x3) or F(4,5) (OFX_CONV_TILE_WINOGRAD)
TILE_WINOGRAD4 = 2     # conv2d_nhwc(tile=): force the fused Winograd F(4x4,3x3) kernel (OFX_CONV_TILE_WINOGRAD4)


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: torch.Tensor, name: str, dtype=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")       # correlation.cpp:19
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")          # correlation.cpp:20
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    return t


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


# --------------------------------------------------------------------------------------
# profiling
# --------------------------------------------------------------------------------------
def prof_enable(on) -> None:
    """False/0: off; True/1: per kernel family; 2: per layer of the RAFT executor ("family:layer")."""
    check(_lib.lib().ofx_prof_enable(int(on)), "ofx_prof_enable")


def prof_collect() -> dict:
    buf = C.create_string_buffer(1 << 18)
    check(_lib.lib().ofx_prof_collect(buf, len(buf)), "ofx_prof_collect")
    return json.loads(buf.value.decode())


# --------------------------------------------------------------------------------------
# warp
# --------------------------------------------------------------------------------------
def warp(frame: torch.Tensor, flow: torch.Tensor, mode: str = "bilinear", sign: float = 1.0) -> torch.Tensor:
    """frame [H,W,C] (one frame shared by all flows) or [B,H,W,C], uint8 or float32;
    flow f32 [B,H,W,2] or [H,W,2].  Returns the warped frames, [B,H,W,C] (or [H,W,C])."""
    squeeze = flow.dim() == 3
    fl = _chk(flow if not squeeze else flow[None], "flow", torch.float32)
    B, H, W, _ = fl.shape
    if frame.dim() == 2:
        raise RuntimeError("frame must be HWC; add a channel axis")
    shared = frame.dim() == 3
    fr = _chk(frame, "frame")
    Cn = fr.shape[-1]
    if tuple(fr.shape[-3:-1]) != (H, W) or (not shared and fr.shape[0] != B):
        raise RuntimeError(f"frame {tuple(fr.shape)} does not match flow {tuple(fl.shape)}")
    out = torch.empty((B, H, W, Cn), dtype=fr.dtype, device=fr.device)
    stride = 0 if shared else H * W * Cn
    L = _lib.lib()
    if fr.dtype == torch.uint8:
        fn, nm = L.ofx_warp_u8, "ofx_warp_u8"
    elif fr.dtype == torch.float32:
        fn, nm = L.ofx_warp_f32, "ofx_warp_f32"
    else:
        raise RuntimeError(f"warp: unsupported dtype {fr.dtype}")
    check(fn(_ptr(fr), stride, _ptr(fl), _ptr(out), B, H, W, Cn, WARP_MODES[mode], float(sign), _stream()), nm)
    return out[0] if (squeeze and shared) else out


def resize_cubic(img: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """f32 [B,H,W,C] -> [B,out_h,out_w,C], cv2.resize(INTER_CUBIC) semantics."""
    x = _chk(img, "img", torch.float32)
    B, H, W, Cn = x.shape
    out = torch.empty((B, out_h, out_w, Cn), dtype=torch.float32, device=x.device)
    check(_lib.lib().ofx_resize_cubic_f32(_ptr(x), _ptr(out), B, H, W, out_h, out_w, Cn, _stream()), "ofx_resize_cubic_f32")
    return out


# --------------------------------------------------------------------------------------
# masks
# --------------------------------------------------------------------------------------
def generate_mask(conf: torch.Tensor, log_conf: Optional[torch.Tensor] = None, thres: float = 0.8,
                  ksize: int = 7, cmp_gt: bool = False) -> torch.Tensor:
    """conf f32 [B,H,W]; log_conf (optional, modified IN PLACE like the reference). -> uint8 [B,H,W]."""
    c = _chk(conf, "confidence", torch.float32)
    B, H, W = c.shape
    if log_conf is not None:
        _chk(log_conf, "log_confidence", torch.float32)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=c.device)
    check(_lib.lib().ofx_generate_mask(_ptr(c), _ptr(log_conf), _ptr(out), B, H, W, float(thres), int(ksize),
                                       1 if cmp_gt else 0, _stream()), "ofx_generate_mask")
    return out


def dilate(mask: torch.Tensor, ksize: int) -> torch.Tensor:
    m = _chk(mask, "mask", torch.uint8)
    B, H, W = m.shape
    out = torch.empty_like(m)
    check(_lib.lib().ofx_dilate_u8(_ptr(m), _ptr(out), B, H, W, int(ksize), _stream()), "ofx_dilate_u8")
    return out


def expand_mask(mask: torch.Tensor, image_bgr: torch.Tensor, edge_thres: int = 20, ksize: int = 7) -> torch.Tensor:
    m = _chk(mask, "mask", torch.uint8)
    img = _chk(image_bgr, "image", torch.uint8)
    B, H, W = m.shape
    if tuple(img.shape) != (B, H, W, 3):
        raise RuntimeError("image must be uint8 [B,H,W,3]")
    out = torch.empty_like(m)
    check(_lib.lib().ofx_expand_mask(_ptr(m), _ptr(img), _ptr(out), None, B, H, W, int(edge_thres), int(ksize), _stream()),
          "ofx_expand_mask")
    return out


def travel_distance(flow: torch.Tensor, conf: torch.Tensor, conf_floor: float = 0.9) -> torch.Tensor:
    fl = _chk(flow, "flow", torch.float32)
    c = _chk(conf, "confidence", torch.float32)
    B, H, W, _ = fl.shape
    out = torch.empty((B, H, W), dtype=torch.float32, device=fl.device)
    check(_lib.lib().ofx_travel_distance(_ptr(fl), _ptr(c), _ptr(out), B, H, W, float(conf_floor), _stream()),
          "ofx_travel_distance")
    return out


def flow_magnitude(flow: torch.Tensor) -> torch.Tensor:
    """|flow| per pixel: f32 [...,2] -> f32 [...] (the RAFT-variant of_calc's `v`, reference ofgen.py:45-49)."""
    fl = _chk(flow, "flow", torch.float32)
    if fl.shape[-1] != 2:
        raise RuntimeError("flow must be [...,2]")
    out = torch.empty(tuple(fl.shape[:-1]), dtype=torch.float32, device=fl.device)
    check(_lib.lib().ofx_flow_magnitude(_ptr(fl), _ptr(out), out.numel(), _stream()), "ofx_flow_magnitude")
    return out


def travel_mask(conf, flow, dist, travel, thres: float, warp_mode: str = "cv2_cubic") -> Tuple[torch.Tensor, torch.Tensor]:
    """confidence_to_mask core (before the 15x15 dilation): returns (raw mask, new travel)."""
    c = _chk(conf, "confidence", torch.float32)
    fl = _chk(flow, "flow", torch.float32)
    d = _chk(dist, "dist", torch.float32)
    t = _chk(travel, "travel", torch.float32)
    B, H, W = c.shape
    tout = torch.empty_like(t)
    raw = torch.empty((B, H, W), dtype=torch.uint8, device=c.device)
    check(_lib.lib().ofx_travel_mask(_ptr(c), _ptr(fl), _ptr(d), _ptr(t), _ptr(tout), _ptr(raw), B, H, W, float(thres),
                                     WARP_MODES[warp_mode], _stream()), "ofx_travel_mask")
    return raw, tout


def merge_images(base, second, mask) -> torch.Tensor:
    b = _chk(base, "base", torch.uint8)
    s = _chk(second, "second", torch.uint8)
    m = _chk(mask, "mask", torch.uint8)
    B, H, W, Cn = b.shape
    out = torch.empty_like(b)
    check(_lib.lib().ofx_merge_images(_ptr(b), _ptr(s), _ptr(m), _ptr(out), B, H, W, Cn, _stream()), "ofx_merge_images")
    return out


def mix_frames(raw, warped, mask, ppw: float) -> torch.Tensor:
    r = _chk(raw, "raw", torch.uint8)
    w = _chk(warped, "warped", torch.uint8)
    m = _chk(mask, "mask", torch.uint8)
    B, H, W, Cn = r.shape
    out = torch.empty_like(r)
    check(_lib.lib().ofx_mix_frames(_ptr(r), _ptr(w), _ptr(m), _ptr(out), B, H, W, Cn, float(ppw), _stream()), "ofx_mix_frames")
    return out


def conf_sum(x: torch.Tensor, chan: int) -> torch.Tensor:
    """x f32 [N,H,W,nchan] -> f64 [N] sums of channel `chan` over H,W."""
    t = _chk(x, "x", torch.float32)
    N, H, W, nc = t.shape
    out = torch.empty((N,), dtype=torch.float64, device=t.device)
    check(_lib.lib().ofx_conf_sum(_ptr(t), _ptr(out), N, H * W, nc, int(chan), _stream()), "ofx_conf_sum")
    return out


COMPOSE_MAX_REFS = 8


def compose_refs(flow: torch.Tensor, conf: torch.Tensor, frames: torch.Tensor, thres: float, mode: str = "cv2_cubic",
                 first_only: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The greedy multi-reference composition of generate_ai_frame_with_ref (ofgen_keyframe_inpaint.py:995-1024) in two launches
    (`ofx_compose_refs`): flow f32 [N,H,W,2], conf f32 [N,H,W] (raw confidence), frames u8 [N,H,W,3] ->
        (ret u8 [H,W,3], mask u8 [H,W], select u8 [H,W], order i32 [N], counts i32 [N]), all on the device.
    mask is 255 where some reference is confident (the caller forms 255 - mask); select names the reference each pixel was sampled
    from; order / counts are the draws of the reference's rounds and their winning pixel counts.  first_only: sample order[0]
    everywhere (the `both` mode).  1 <= N <= 8 and H*W < 2^31, a ValueError before anything else is looked at.  No host
    synchronisation."""
    shp = tuple(getattr(flow, "shape", ()))
    if len(shp) != 4 or shp[3] != 2:
        raise ValueError(f"compose_refs: flow must be [N,H,W,2], got {shp}")
    N, H, W, _ = shp
    if not 1 <= N <= COMPOSE_MAX_REFS:
        raise ValueError(f"compose_refs: 1 to {COMPOSE_MAX_REFS} references, got {N}")
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError(f"compose_refs: H*W must be in 1..2^31-1, got {H}x{W}")
    if tuple(getattr(conf, "shape", ())) != (N, H, W) or tuple(getattr(frames, "shape", ())) != (N, H, W, 3):
        raise ValueError(f"compose_refs: conf must be [{N},{H},{W}] and frames [{N},{H},{W},3]")
    if mode not in WARP_MODES:
        raise ValueError(f"compose_refs: mode must be one of {sorted(WARP_MODES)}, got {mode!r}")
    fl = _chk(flow, "flow", torch.float32)
    cf = _chk(conf, "conf", torch.float32)
    fr = _chk(frames, "frames", torch.uint8)
    dev = fl.device
    L = _lib.lib()
    nbytes = int(L.ofx_compose_scratch_bytes(N, H, W))
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    ret = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    select = torch.empty((H, W), dtype=torch.uint8, device=dev)
    oc = torch.empty((2, N), dtype=torch.int32, device=dev)
    check(L.ofx_compose_refs(_ptr(fl), _ptr(cf), _ptr(fr), _ptr(ret), _ptr(mask), _ptr(select), _ptr(oc[0]), _ptr(oc[1]),
                             _ptr(scratch), nbytes, N, H, W, float(thres), WARP_MODES[mode], 1 if first_only else 0, _stream()),
          "ofx_compose_refs")
    return ret, mask, select, oc[0], oc[1]


def fb_confidence(flow_fw: torch.Tensor, flow_bw: torch.Tensor, sigma: float = 3.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Extension: forward-backward consistency (confidence, log_confidence), each f32 [B,H,W]."""
    a = _chk(flow_fw, "flow_fw", torch.float32)
    b = _chk(flow_bw, "flow_bw", torch.float32)
    B, H, W, _ = a.shape
    conf = torch.empty((B, H, W), dtype=torch.float32, device=a.device)
    logc = torch.empty_like(conf)
    check(_lib.lib().ofx_fb_confidence(_ptr(a), _ptr(b), _ptr(conf), _ptr(logc), B, H, W, float(sigma), _stream()),
          "ofx_fb_confidence")
    return conf, logc


def warp_and_mask(frame, flow, conf, warp_mode="bilinear", sign=1.0, thres=0.95, ksize=7, cmp_gt=False):
    """Fused tail of the hot path for a batch: (warped uint8 [B,H,W,C], mask uint8 [B,H,W])."""
    fl = _chk(flow, "flow", torch.float32)
    c = _chk(conf, "confidence", torch.float32)
    fr = _chk(frame, "frame", torch.uint8)
    B, H, W, _ = fl.shape
    shared = fr.dim() == 3
    Cn = fr.shape[-1]
    warped = torch.empty((B, H, W, Cn), dtype=torch.uint8, device=fr.device)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=fr.device)
    check(_lib.lib().ofx_warp_and_mask(_ptr(fr), 0 if shared else H * W * Cn, _ptr(fl), _ptr(c), _ptr(warped), _ptr(mask),
                                       B, H, W, Cn, WARP_MODES[warp_mode], float(sign), float(thres), int(ksize),
                                       1 if cmp_gt else 0, _stream()), "ofx_warp_and_mask")
    return warped, mask


# --------------------------------------------------------------------------------------
# network building blocks (exposed for stage-level parity tests and custom pipelines)
# --------------------------------------------------------------------------------------
def pack_conv_weight(w_oihw: torch.Tensor, cin_pad: Optional[int] = None) -> torch.Tensor:
    """OIHW fp32 (CPU) -> packed [Cout, Kpad] fp32 (CPU)."""
    w = w_oihw.detach().to(torch.float32).contiguous().cpu()
    co, ci, kh, kw = w.shape
    cp = cin_pad if cin_pad else ((ci + 3) // 4) * 4
    L = _lib.lib()
    kpad = L.ofx_pack_conv_weight(None, co, ci, kh, kw, cp, None)
    if kpad < 0:
        raise _lib.OfxError(int(kpad), "ofx_pack_conv_weight")
    out = torch.empty((co, kpad), dtype=torch.float32)
    L.ofx_pack_conv_weight(C.c_void_p(w.data_ptr()), co, ci, kh, kw, cp, C.c_void_p(out.data_ptr()))
    return out


def _wino_weight(fn: str, w: torch.Tensor, *shape) -> torch.Tensor:
    """The Winograd operand of `w` (fp32 OIHW, CPU) from the C entry point `fn`(w, *shape, out) as a flat fp32 CPU tensor."""
    f = getattr(_lib.lib(), fn)
    n = f(None, *shape, None)
    if n < 0:
        raise _lib.OfxError(int(n), fn)
    out = torch.empty((n,), dtype=torch.float32)
    st = f(C.c_void_p(w.data_ptr()), *shape, C.c_void_p(out.data_ptr()))
    if st < 0:
        raise _lib.OfxError(int(st), fn)
    return out


def wino_conv_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 3x3 (CPU) -> the Winograd F(2x2,3x3) operand U = G g G^T (float64, one rounding) as a flat fp32 CPU tensor
    in the fused kernel's order (ofx_wino_conv_weight); pass it to conv2d_nhwc(..., wino_w=)."""
    w = w_oihw.detach().to(torch.float32).contiguous().cpu()
    co, ci, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise RuntimeError("wino_conv_weight: 3x3 weights only")
    return _wino_weight("ofx_wino_conv_weight", w, co, ci)


def wino44_conv_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 3x3 (CPU) -> the Winograd F(4x4,3x3) operand U = G g G^T over the points {0, 1, -1, 2, -2, inf} (float64, one
    rounding) as a flat fp32 CPU tensor in the fused kernel's order (ofx_wino44_conv_weight); pass it to
    conv2d_nhwc(..., wino4_w=)."""
    w = w_oihw.detach().to(torch.float32).contiguous().cpu()
    co, ci, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise RuntimeError("wino44_conv_weight: 3x3 weights only")
    return _wino_weight("ofx_wino44_conv_weight", w, co, ci)


def wino15_conv_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 1x5 or 5x1 (CPU) -> the 1D Winograd F(4,5) operand U = G g (float64, one rounding) as a flat fp32 CPU tensor
    in the fused kernel's order (ofx_wino15_conv_weight); pass it to conv2d_nhwc(..., wino_w=)."""
    w = w_oihw.detach().to(torch.float32).contiguous().cpu()
    co, ci, kh, kw = w.shape
    return _wino_weight("ofx_wino15_conv_weight", w, co, ci, kh, kw)


def split_conv_weight(w_packed: torch.Tensor) -> torch.Tensor:
    """Packed fp32 weights (CPU) -> the pre-split bf16x3 operand format (same shape, fp32 container); feed it to
    conv2d_nhwc(..., precision="bf16x3_w")."""
    w = w_packed.detach().to(torch.float32).contiguous().cpu()
    out = torch.empty_like(w)
    check(_lib.lib().ofx_split_conv_weight(C.c_void_p(w.data_ptr()), w.numel(), C.c_void_p(out.data_ptr())), "ofx_split_conv_weight")
    return out


def split_conv_weight3(w_packed: torch.Tensor) -> torch.Tensor:
    """Packed fp32 weights (CPU, the whole [Cout, Kpad] matrix) -> the pre-split bf16x6 operand format: a flat fp32 container of
    1.5 x the size ([hi x4 | mid x4] groups, then the [lo x4] groups); feed it to conv2d_nhwc(..., precision="bf16x6_w")."""
    w = w_packed.detach().to(torch.float32).contiguous().cpu()
    out = torch.empty((w.numel() * 3 // 2,), dtype=torch.float32)
    check(_lib.lib().ofx_split_conv_weight3(C.c_void_p(w.data_ptr()), w.numel(), C.c_void_p(out.data_ptr())), "ofx_split_conv_weight3")
    return out


def half_conv_weight(w_packed: torch.Tensor) -> torch.Tensor:
    """Packed fp32 weights (CPU; `pack_conv_weight`, or the folded operand of `upconv2x_weight`) -> the same shape in float16,
    rounded to nearest even exactly as the fp16 kernels round a weight when they stage it (ofx_half_conv_weight: subnormals kept,
    beyond +-65504 an infinity).  Feed it to conv2d_nhwc(..., precision="fp16_w") / upconv2x(..., precision="fp16")."""
    w = w_packed.detach().to(torch.float32).contiguous().cpu()
    out = torch.empty(w.shape, dtype=torch.float16)
    check(_lib.lib().ofx_half_conv_weight(C.c_void_p(w.data_ptr()), w.numel(), C.c_void_p(out.data_ptr())), "ofx_half_conv_weight")
    return out


# conv2d_nhwc(precision=) -> OFX_PREC_*.  *_w: the weight comes from split_conv_weight / split_conv_weight3.  "fp16": both operands
# rounded to half as they are staged, fp32 accumulate (OFX_PREC_F16; plain fp32 [Cout, Kpad] weights, fp32 activations and epilogue;
# no nmean / stats_part / splitk_ws).  "fp16_epi": the same arithmetic with nmean and stats_part served (OFX_PREC_F16_EPI, the flow
# network's encoder layers under `RaftEngine(precision="fp16")`).  "fp16_w": "fp16" on weights already stored in half
# (OFX_PREC_F16_W; a float16 [Cout, Kpad] from half_conv_weight, staged as it is: bit-identical to "fp16" on the fp32 weights)
CONV_PRECISIONS = {"fp32": 0, "bf16x3": 1, "bf16x3_w": 2, "bf16x6": 3, "bf16x6_w": 4, "fp16": 5, "fp16_epi": 5 | 256, "fp16_w": 7}


def conv2d_nhwc(x: torch.Tensor, w_packed: torch.Tensor, kh: int, kw: int, cout: int, *, stride: int = 1,
                shift: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, act: Optional[str] = None,
                x2: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
                nmean: Optional[torch.Tensor] = None, nrstd: Optional[torch.Tensor] = None, tile: int = 0,
                precision: str = "fp32", splitk_ws: Optional[torch.Tensor] = None, pad: Optional[Tuple[int, int]] = None,
                out_hw: Optional[Tuple[int, int]] = None, addend: Optional[torch.Tensor] = None,
                wino_w: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_off: int = 0,
                stats_part: Optional[torch.Tensor] = None, wino4_w: Optional[torch.Tensor] = None):
    """Plain-epilogue convolution: x [B,H,W,C0] (+ optional second channel segment x2 [B,H,W,C1]),
    'same' padding (k//2) unless `pad` = (top, left) is given; `out_hw` overrides the output size (taps beyond the
    input read zeros: pad (0, 0) with out_hw = (H/2, W/2) is the VAE's F.pad(x, (0,1,0,1)) + stride-2 convolution).
    `addend` [B,Hout,Wout,cout] is added before the activation (`res` adds after it and applies ReLU).
    `wino_w` (wino_conv_weight / wino15_conv_weight, on the device) lets a qualifying 3x3 / 1x5 / 5x1 layer run the fused
    Winograd kernel (tile = TILE_WINOGRAD forces it); `wino4_w` (wino44_conv_weight) lets a qualifying 3x3 layer run the
    F(4x4,3x3) kernel where its grid pays (tile = TILE_WINOGRAD4 forces it), `res`, `nmean` / `nrstd` and `stats_part` included.  `out` [B,Hout,Wout,C >= out_off + cout]: write channels
    [out_off, out_off + cout) of it.  `stats_part` (f32 on the device): run ofx_conv2d_stats, which leaves the per-channel
    (sum, sum of squares) partials of the outputs there when the launch can produce them ([B][rows][cout][2]; see inorm_finalize).
    `precision`: a key of CONV_PRECISIONS (default exact fp32).  "fp16_w" takes a float16 `w_packed` (half_conv_weight) and every
    other precision a float32 one: a mismatch either way is a RuntimeError before any launch.
    Returns [B,Hout,Wout,cout], or `out`; with `stats_part`, (that, rows per image), rows = 0 when none were produced."""
    ph, pw = (kh // 2, kw // 2) if pad is None else pad
    if ph < 0 or pw < 0:            # (ofx_conv2d: OFX_EINVAL) padding is rows / columns of zeros above and left of the image, never a crop
        raise RuntimeError(f"pad must be >= 0, got {(ph, pw)}")
    x = _chk(x, "x", torch.float32)
    B, H, W, c0 = x.shape
    d = ConvDesc()
    d.in0, d.ld0, d.c0 = x.data_ptr(), c0, c0
    if x2 is not None:
        x2 = _chk(x2, "x2", torch.float32)
        d.in1, d.ld1, d.c1 = x2.data_ptr(), x2.shape[-1], x2.shape[-1]
    wp = _chk(w_packed, "w_packed", torch.float16 if precision == "fp16_w" else torch.float32)
    d.w = wp.data_ptr()
    d.scale = 0 if scale is None else _chk(scale, "scale", torch.float32).data_ptr()
    d.shift = 0 if shift is None else _chk(shift, "shift", torch.float32).data_ptr()
    Ho, Wo = ((H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1) if out_hw is None else out_hw
    if out is None:
        out = torch.empty((B, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    out = _chk(out, "out", torch.float32)
    if tuple(out.shape[:3]) != (B, Ho, Wo) or out.shape[3] < out_off + cout or out_off < 0:
        raise RuntimeError(f"out must be [{B},{Ho},{Wo},>= {out_off + cout}], got {tuple(out.shape)}")
    d.out, d.ldo = out.data_ptr() + 4 * out_off, out.shape[3]
    if wino_w is not None:
        d.wino_w = _chk(wino_w, "wino_w", torch.float32).data_ptr()
    if wino4_w is not None:
        d.wino4_w = _chk(wino4_w, "wino4_w", torch.float32).data_ptr()
    if addend is not None:
        addend = _chk(addend, "addend", torch.float32)
        if tuple(addend.shape) != (B, Ho, Wo, cout):
            raise RuntimeError(f"addend must be {(B, Ho, Wo, cout)}, got {tuple(addend.shape)}")
        d.addend, d.ldadd = addend.data_ptr(), cout
    if res is not None:
        res = _chk(res, "res", torch.float32)
        d.res, d.ldres = res.data_ptr(), res.shape[-1]
    if nmean is not None:
        d.nmean = _chk(nmean, "nmean", torch.float32).data_ptr()
        d.nrstd = _chk(nrstd, "nrstd", torch.float32).data_ptr()
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, H, W, Ho, Wo, cout
    d.KH, d.KW, d.stride, d.padH, d.padW = kh, kw, stride, ph, pw
    d.act, d.epi, d.tile = ACTS[act], EPI_PLAIN, tile
    d.precision = CONV_PRECISIONS[precision]
    if splitk_ws is not None:       # uint8 scratch whose first 64 KiB are zero (see ofx_conv_desc.splitk_ws): allows split-K
        ws = _chk(splitk_ws, "splitk_ws", torch.uint8)
        d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel()
    if stats_part is not None:
        part = _chk(stats_part, "stats_part", torch.float32)
        rows = C.c_int(0)
        check(_lib.lib().ofx_conv2d_stats(C.byref(d), C.c_void_p(part.data_ptr()), part.numel(), C.byref(rows), _stream()),
              "ofx_conv2d_stats")
        return out, rows.value
    check(_lib.lib().ofx_conv2d(C.byref(d), _stream()), "ofx_conv2d")
    return out


def inorm_finalize(part: torch.Tensor, B: int, rows: int, HW: int, C_: int, eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """mean and 1/sqrt(var + eps) [B, C_] from the partials conv2d_nhwc(..., stats_part=part) left (rows per image, HW pixels per
    image), reduced in a fixed order (ofx_inorm_finalize)."""
    part = _chk(part, "part", torch.float32)
    mean = torch.empty((B, C_), dtype=torch.float32, device=part.device)
    rstd = torch.empty_like(mean)
    check(_lib.lib().ofx_inorm_finalize(_ptr(part), _ptr(mean), _ptr(rstd), B, rows, HW, C_, float(eps), _stream()), "ofx_inorm_finalize")
    return mean, rstd


def flow_head(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, coords1: torch.Tensor, hx: torch.Tensor,
              frows: torch.Tensor, flow_off: int = 0) -> None:
    """The flow head's 3x3 256 -> 2 convolution fused with coords1 += delta (`ofx_flow_head`, update.py:6-14 + raft.py:131).
    x f32 [B,h,w,ldx] (the first 256 channels are read); w_packed [2, kpad] = pack_conv_weight of the OIHW [2,256,3,3] weight, on
    the device; bias [2].  Written in place: coords1 f32 [B,h,w,2]; channels flow_off, flow_off + 1 of hx f32 [B,h,w,ldh] get
    coords1 - grid; frows f32 [B,h,w,16] gets, in slot s = 0..6 of a pixel's row, the flow of the pixel s - 3 columns away where
    that pixel is inside the image (nothing else of hx or frows is touched)."""
    x = _chk(x, "x", torch.float32)
    wp = _chk(w_packed, "w_packed", torch.float32)
    b = _chk(bias, "bias", torch.float32)
    c = _chk(coords1, "coords1", torch.float32)
    hx = _chk(hx, "hx", torch.float32)
    fr = _chk(frows, "frows", torch.float32)
    B, h, w, ldx = x.shape
    if (tuple(c.shape) != (B, h, w, 2) or tuple(hx.shape[:3]) != (B, h, w) or tuple(fr.shape) != (B, h, w, 16)
            or wp.dim() != 2 or wp.shape[0] != 2 or b.numel() != 2 or not 0 <= flow_off <= hx.shape[3] - 2):
        raise RuntimeError("shapes: x [B,h,w,ldx], w_packed [2,kpad], bias [2], coords1 [B,h,w,2], hx [B,h,w,ldh] with "
                           "flow_off + 2 <= ldh, frows [B,h,w,16]")
    check(_lib.lib().ofx_flow_head(_ptr(x), ldx, _ptr(wp), wp.shape[1], _ptr(b), _ptr(c), C.c_void_p(hx.data_ptr() + 4 * flow_off),
                                   hx.shape[3], _ptr(fr), B, h, w, _stream()), "ofx_flow_head")


def forward_interpolate(flow: torch.Tensor) -> torch.Tensor:
    """forward_interpolate of RAFT/core/utils/utils.py:26-53 on the device (`ofx_forward_interpolate`): the warm start of a video
    chain.  flow f32 [B,h,w,2] or [h,w,2] (the engine's flow_low layout) -> the same shape: every output pixel takes the flow of the
    valid source (x0 + dx, y0 + dy; 0 < x1 < w, 0 < y1 < h) nearest to it in float64, ties to the lowest source index; a field
    without a valid source gives NaN.  Fields are independent; runs on the current stream."""
    fl = _chk(flow, "flow", torch.float32)
    one = fl.dim() == 3
    if one:
        fl = fl[None]
    if fl.dim() != 4 or fl.shape[3] != 2 or fl.numel() == 0:
        raise RuntimeError("flow must be f32 [B,h,w,2] or [h,w,2]")
    B, h, w, _ = fl.shape
    L = _lib.lib()
    need = L.ofx_forward_interpolate_scratch_bytes(B, h, w)
    if need == 0:
        raise RuntimeError(f"unsupported size B={B} h={h} w={w}")
    scratch = torch.empty((need,), dtype=torch.uint8, device=fl.device)
    out = torch.empty_like(fl)
    check(L.ofx_forward_interpolate(_ptr(fl), _ptr(out), _ptr(scratch), need, B, h, w, _stream()), "ofx_forward_interpolate")
    return out[0] if one else out


def conv2d_desc(d: ConvDesc) -> None:
    check(_lib.lib().ofx_conv2d(C.byref(d), _stream()), "ofx_conv2d")


def inorm_stats(x: torch.Tensor, eps: float = 1e-5, c_off: int = 0, c: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """mean and 1/sqrt(var + eps) [B, c] of x [B,H,W,ld] per image and channel (`ofx_inorm_stats`); `c_off` / `c` select the channel
    slice [c_off, c_off + c) of the rows (c_off % 4 == 0; default: all ld channels)."""
    x = _chk(x, "x", torch.float32)
    B, H, W, ld = x.shape
    Cn = ld - c_off if c is None else c
    if c_off < 0 or Cn <= 0 or c_off + Cn > ld:
        raise RuntimeError(f"channel slice [{c_off}, {c_off + Cn}) outside the {ld} channels of x")
    mean = torch.empty((B, Cn), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    scratch = torch.empty((max(B * 64, min(B, 7) * 256) * Cn * 2,), dtype=torch.float64, device=x.device)
    check(_lib.lib().ofx_inorm_stats(C.c_void_p(x.data_ptr() + 4 * c_off), ld, _ptr(mean), _ptr(rstd), _ptr(scratch), B, H * W, Cn,
                                     float(eps), _stream()), "ofx_inorm_stats")
    return mean, rstd


def inorm_apply(x, mean, rstd, res=None, res_mean=None, res_rstd=None, relu=True) -> torch.Tensor:
    """`ofx_inorm_apply`.  relu: True / False (ReLU or not; a residual merge always applies it), or the integer mode of the C entry
    point -- bit 0 the ReLU, bit 1 (relu = 3) a ReLU on the normalised residual as well."""
    x = _chk(x, "x", torch.float32)
    B, H, W, Cn = x.shape
    out = torch.empty_like(x)
    mode = (1 if relu else 0) if isinstance(relu, bool) else int(relu)
    check(_lib.lib().ofx_inorm_apply(_ptr(x), _ptr(mean), _ptr(rstd), _ptr(res), _ptr(res_mean), _ptr(res_rstd), _ptr(out),
                                     B, H * W, Cn, mode, _stream()), "ofx_inorm_apply")
    return out


def preprocess_u8(img: torch.Tensor, bgr: bool = False) -> torch.Tensor:
    x = _chk(img, "img", torch.uint8)
    if x.shape[-1] != 3:
        raise RuntimeError("img must be [...,3]")
    out = torch.empty(tuple(x.shape[:-1]) + (4,), dtype=torch.float32, device=x.device)
    check(_lib.lib().ofx_preprocess_u8(_ptr(x), _ptr(out), x.numel() // 3, 1 if bgr else 0, _stream()), "ofx_preprocess_u8")
    return out


def corr_slice_floats(hl: int, wl: int) -> int:
    """Floats per pixel slice of an hl x wl pyramid level in the blocked layout (4 x 8 blocks, see include/ofx.h)."""
    return ((hl + 3) // 4) * ((wl + 7) // 8) * 32


def corr_volume(f1: torch.Tensor, f2: torch.Tensor, levels: int = 4) -> List[torch.Tensor]:
    """f1, f2 f32 [B,h,w,D] (NHWC) -> pyramid list, level l: [B*h*w, corr_slice_floats(h>>l, w>>l)] in the blocked
    layout `corr_lookup` reads; `corr_unblock` gives the [B*h*w, h>>l, w>>l] view of CorrBlock.corr_pyramid."""
    a = _chk(f1, "fmap1", torch.float32)
    b = _chk(f2, "fmap2", torch.float32)
    B, h, w, D = a.shape
    pyr = [torch.empty((B * h * w, corr_slice_floats(h >> l, w >> l)), dtype=torch.float32, device=a.device) for l in range(levels)]
    arr = (C.c_void_p * levels)(*[p.data_ptr() for p in pyr])
    check(_lib.lib().ofx_corr_volume(_ptr(a), _ptr(b), arr, B, h, w, D, levels, _stream()), "ofx_corr_volume")
    return pyr


_VOLUME_PLANES = {"fp32": 1, "bf16x3": 2, "bf16x6": 3}


def corr_volume_split(f1: torch.Tensor, f2: torch.Tensor, levels: int = 4, precision: str = "bf16x6") -> List[torch.Tensor]:
    """`corr_volume` with the GEMM in split-bf16 arithmetic (`ofx_corr_volume_split`; opt-in, RAFT/core/corr.py:52-60 is fp32).
    f1 f32 [B,h,w,256]; f2 f32 [B,h,w,256] or [1,h,w,256] (one key frame shared by the B pairs).  precision 'bf16x3' | 'bf16x6', or
    'fp32': the same A-stationary kernel on the fp32 matrix cores -- bit-identical to `corr_volume`."""
    a = _chk(f1, "fmap1", torch.float32)
    b = _chk(f2, "fmap2", torch.float32)
    if precision not in _VOLUME_PLANES:
        raise ValueError("precision: 'fp32', 'bf16x3' or 'bf16x6'")
    B, h, w, D = a.shape
    if b.shape[0] not in (1, B) or tuple(b.shape[1:]) != (h, w, D):
        raise RuntimeError("fmap2: [B,h,w,D] or [1,h,w,D]")
    pyr = [torch.empty((B * h * w, corr_slice_floats(h >> l, w >> l)), dtype=torch.float32, device=a.device) for l in range(levels)]
    arr = (C.c_void_p * levels)(*[p.data_ptr() for p in pyr])
    check(_lib.lib().ofx_corr_volume_split(_ptr(a), _ptr(b), arr, B, h, w, D, levels, _VOLUME_PLANES[precision],
                                           1 if (b.shape[0] == 1 and B > 1) else 0, _stream()), "ofx_corr_volume_split")
    return pyr


def corr_unblock(p: torch.Tensor, hl: int, wl: int) -> torch.Tensor:
    """Blocked slices [M, corr_slice_floats(hl, wl)] (or a flat buffer) -> row-major [M, hl, wl] (pure indexing: for
    tests and inspection, not on any hot path)."""
    hb, wb = (hl + 3) // 4, (wl + 7) // 8
    q = p.reshape(-1, hb, wb, 4, 8).permute(0, 1, 3, 2, 4).reshape(-1, hb * 4, wb * 8)
    return q[:, :hl, :wl].contiguous()


def upsample_flow_warp(coords1: torch.Tensor, mask: torch.Tensor, frame: torch.Tensor, sign: float = 1.0, want_flow: bool = True):
    """RAFT.upsample_flow (raft.py:72-83) + the bilinear backward warp of one shared uint8 frame [8h,8w,3] in ONE kernel.
    coords1 f32 [B,h,w,2], mask f32 [B,h,w,576] -> (flow_up f32 [B,8h,8w,2] or None, warped u8 [B,8h,8w,3])."""
    c = _chk(coords1, "coords1", torch.float32)
    m = _chk(mask, "mask", torch.float32)
    fr = _chk(frame, "frame", torch.uint8)
    B, h, w, _ = c.shape
    if tuple(fr.shape) != (8 * h, 8 * w, 3) or tuple(m.shape) != (B, h, w, 576):
        raise RuntimeError("shapes: coords1 [B,h,w,2], mask [B,h,w,576], frame [8h,8w,3]")
    flow = torch.empty((B, 8 * h, 8 * w, 2), dtype=torch.float32, device=c.device) if want_flow else None
    warped = torch.empty((B, 8 * h, 8 * w, 3), dtype=torch.uint8, device=c.device)
    check(_lib.lib().ofx_upsample_flow_warp(_ptr(c), _ptr(m), _ptr(flow) if want_flow else C.c_void_p(0), _ptr(fr), _ptr(warped), B, h, w,
                                            float(sign), _stream()), "ofx_upsample_flow_warp")
    return flow, warped


def upflow8(coords1: torch.Tensor) -> torch.Tensor:
    """The small network's upsample (upflow8, RAFT/core/utils/utils.py:80-82): coords1 f32 [B,h,w,2] -> flow_up f32 [B,8h,8w,2] =
    8 * F.interpolate(coords1 - coords0, (8h, 8w), mode='bilinear', align_corners=True), channels-last."""
    c = _chk(coords1, "coords1", torch.float32)
    B, h, w, _ = c.shape
    out = torch.empty((B, 8 * h, 8 * w, 2), dtype=torch.float32, device=c.device)
    check(_lib.lib().ofx_upflow8(_ptr(c), _ptr(out), B, h, w, _stream()), "ofx_upflow8")
    return out


def upflow8_warp(coords1: torch.Tensor, frame: torch.Tensor, sign: float = 1.0, want_flow: bool = True):
    """upflow8 + the bilinear backward warp of one shared uint8 frame [8h,8w,3] in ONE kernel.
    coords1 f32 [B,h,w,2] -> (flow_up f32 [B,8h,8w,2] or None, warped u8 [B,8h,8w,3])."""
    c = _chk(coords1, "coords1", torch.float32)
    fr = _chk(frame, "frame", torch.uint8)
    B, h, w, _ = c.shape
    if tuple(fr.shape) != (8 * h, 8 * w, 3):
        raise RuntimeError("shapes: coords1 [B,h,w,2], frame [8h,8w,3]")
    flow = torch.empty((B, 8 * h, 8 * w, 2), dtype=torch.float32, device=c.device) if want_flow else None
    warped = torch.empty((B, 8 * h, 8 * w, 3), dtype=torch.uint8, device=c.device)
    check(_lib.lib().ofx_upflow8_warp(_ptr(c), _ptr(flow) if want_flow else C.c_void_p(0), _ptr(fr), _ptr(warped), B, h, w, float(sign),
                                      _stream()), "ofx_upflow8_warp")
    return flow, warped


def corr_lookup(pyr: Sequence[torch.Tensor], coords: torch.Tensor, B: int, h: int, w: int, radius: int = 4) -> torch.Tensor:
    """coords f32 [B,h,w,2] (x,y) -> [B,h,w,L*(2r+1)^2] (channels-last version of CorrBlock.__call__)."""
    c = _chk(coords, "coords", torch.float32)
    for i, p in enumerate(pyr):
        _chk(p, f"pyr[{i}]", torch.float32)
    levels = len(pyr)
    nch = levels * (2 * radius + 1) ** 2
    out = torch.empty((B, h, w, nch), dtype=torch.float32, device=c.device)
    arr = (C.c_void_p * levels)(*[p.data_ptr() for p in pyr])
    check(_lib.lib().ofx_corr_lookup(arr, _ptr(c), _ptr(out), nch, B, h, w, levels, radius, _stream()), "ofx_corr_lookup")
    return out


def local_corr(fmap1: torch.Tensor, fmap2: torch.Tensor, coords: torch.Tensor, radius: int) -> torch.Tensor:
    """`alt_cuda_corr.forward` semantics; see alt_cuda_corr.py."""
    a = _chk(fmap1, "fmap1", torch.float32)
    b = _chk(fmap2, "fmap2", torch.float32)
    c = _chk(coords, "coords", torch.float32)
    B, H1, W1, Cn = a.shape
    _, H2, W2, _ = b.shape
    N = c.shape[1]
    rd = 2 * radius + 1
    out = torch.empty((B, N, rd * rd, H1, W1), dtype=torch.float32, device=a.device)
    check(_lib.lib().ofx_local_corr_fwd(_ptr(a), _ptr(b), _ptr(c), _ptr(out), B, H1, W1, H2, W2, Cn, N, radius, _stream()),
          "ofx_local_corr_fwd")
    return out


def local_corr_rows(fmap1: torch.Tensor, fmap2_levels, coords: torch.Tensor, radius: int, rows: torch.Tensor = None, idx1=None, idx2=None,
                    tiled: bool = True) -> torch.Tensor:
    """The engine's volume-free lookup, all pyramid levels at once (`ofx_local_corr_rows`): fmap1 f32[n1,H,W,C]; fmap2_levels: list of
    f32[n2,H>>l,W>>l,C]; coords f32[B,H,W,2] on the level-0 grid; idx1 / idx2: int32 CUDA tensors [B] (image of fmap1 / fmap2 per pair)
    or None (pair b uses image b).  Writes columns [0, levels * (2r+1)^2) of `rows` f32[B*H*W, ld] (allocated with exactly that many
    columns when not given) and returns it; the other columns keep their content.  tiled=False: the per-pixel kernel (no indices)."""
    a = _chk(fmap1, "fmap1", torch.float32)
    lv = [_chk(f, f"fmap2_levels[{l}]", torch.float32) for l, f in enumerate(fmap2_levels)]
    c = _chk(coords, "coords", torch.float32)
    _n1, H, W, Cn = a.shape
    B = c.shape[0]
    if tuple(c.shape) != (B, H, W, 2):
        raise RuntimeError(f"coords must be [B,{H},{W},2], got {tuple(c.shape)}")
    for l, f in enumerate(lv):
        if tuple(f.shape[1:]) != (H >> l, W >> l, Cn) or f.shape[0] != lv[0].shape[0]:
            raise RuntimeError(f"fmap2_levels[{l}] must be [n2,{H >> l},{W >> l},{Cn}], got {tuple(f.shape)}")
    n_out = len(lv) * (2 * radius + 1) ** 2
    if rows is None:
        rows = torch.empty((B * H * W, n_out), dtype=torch.float32, device=a.device)
    if not rows.is_cuda or rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous() or rows.shape[0] != B * H * W or rows.shape[1] < n_out:
        raise RuntimeError(f"rows must be a contiguous CUDA float32 tensor [{B * H * W}, >= {n_out}]")
    ix = []
    for nm, t, n in (("idx1", idx1, a.shape[0]), ("idx2", idx2, lv[0].shape[0])):
        if t is None:
            if n < B:
                raise RuntimeError(f"{nm} is None (pair b uses image b) but there are only {n} images for {B} pairs")
            ix.append(None)
            continue
        t = t.to(device=a.device, dtype=torch.int32).contiguous()
        if t.numel() != B or int(t.min()) < 0 or int(t.max()) >= n:
            raise RuntimeError(f"{nm} must hold {B} indices in [0, {n})")
        ix.append(t)
    ptrs = (C.c_void_p * len(lv))(*[f.data_ptr() for f in lv])
    check(_lib.lib().ofx_local_corr_rows(_ptr(a), ptrs, C.c_void_p(ix[0].data_ptr() if ix[0] is not None else 0),
                                         C.c_void_p(ix[1].data_ptr() if ix[1] is not None else 0), _ptr(c), _ptr(rows), rows.shape[1], B, H, W, Cn,
                                         len(lv), int(radius), 1 if tiled else 0, _stream()), "ofx_local_corr_rows")
    return rows


def local_corr_backward(fmap1: torch.Tensor, fmap2: torch.Tensor, coords: torch.Tensor, corr_grad: torch.Tensor, radius: int):
    """`alt_cuda_corr.backward` semantics: (fmap1_grad, fmap2_grad) for corr_grad f32[B,N,(2r+1)^2,H1,W1]."""
    a = _chk(fmap1, "fmap1", torch.float32)
    b = _chk(fmap2, "fmap2", torch.float32)
    c = _chk(coords, "coords", torch.float32)
    g = _chk(corr_grad, "corr_grad", torch.float32)
    B, H1, W1, Cn = a.shape
    _, H2, W2, _ = b.shape
    N = c.shape[1]
    rd = 2 * radius + 1
    if tuple(g.shape) != (B, N, rd * rd, H1, W1):
        raise RuntimeError(f"corr_grad must be {(B, N, rd * rd, H1, W1)}, got {tuple(g.shape)}")
    g1 = torch.empty_like(a)
    g2 = torch.empty_like(b)
    check(_lib.lib().ofx_local_corr_bwd(_ptr(a), _ptr(b), _ptr(c), _ptr(g), _ptr(g1), _ptr(g2), B, H1, W1, H2, W2, Cn, N, radius,
                                        _stream()), "ofx_local_corr_bwd")
    return g1, g2


def avgpool2_nhwc(x: torch.Tensor) -> torch.Tensor:
    x = _chk(x, "x", torch.float32)
    B, H, W, Cn = x.shape
    out = torch.empty((B, H // 2, W // 2, Cn), dtype=torch.float32, device=x.device)
    check(_lib.lib().ofx_avgpool2_nhwc(_ptr(x), _ptr(out), B, H, W, Cn, _stream()), "ofx_avgpool2_nhwc")
    return out


def upsample_flow(coords1: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """coords1 f32 [B,h,w,2], mask f32 [B,h,w,576] -> flow_up f32 [B,8h,8w,2]."""
    c = _chk(coords1, "coords1", torch.float32)
    m = _chk(mask, "mask", torch.float32)
    B, h, w, _ = c.shape
    out = torch.empty((B, 8 * h, 8 * w, 2), dtype=torch.float32, device=c.device)
    check(_lib.lib().ofx_upsample_flow(_ptr(c), _ptr(m), _ptr(out), B, h, w, _stream()), "ofx_upsample_flow")
    return out


# --------------------------------------------------------------------------------------
# SD-inpaint hand-off: Pillow-exact mask blur / resize, composite + conditioning tensors
# --------------------------------------------------------------------------------------
def gaussian_blur_u8(mask: torch.Tensor, radius: float) -> torch.Tensor:
    """uint8 [B,H,W] -> PIL.ImageFilter.GaussianBlur(radius) of every [H,W] plane."""
    m = _chk(mask, "mask", torch.uint8)
    B, H, W = m.shape
    out = torch.empty_like(m)
    scratch = torch.empty_like(m)
    check(_lib.lib().ofx_gaussian_blur_u8(_ptr(m), _ptr(out), _ptr(scratch), B, H, W, float(radius), _stream()), "ofx_gaussian_blur_u8")
    return out


def resize_bicubic_u8(img: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """uint8 [B,H,W] -> PIL Image.resize((out_w, out_h)) (default BICUBIC resample) of every plane."""
    m = _chk(img, "img", torch.uint8)
    B, H, W = m.shape
    out = torch.empty((B, out_h, out_w), dtype=torch.uint8, device=m.device)
    scratch = torch.empty((B, H, out_w), dtype=torch.uint8, device=m.device)
    check(_lib.lib().ofx_resize_bicubic_u8(_ptr(m), _ptr(out), _ptr(scratch), B, H, W, int(out_h), int(out_w), _stream()),
          "ofx_resize_bicubic_u8")
    return out


def sd_handoff(image_bgr: torch.Tensor, reference_bgr: torch.Tensor, image_mask: torch.Tensor, mask_latent: torch.Tensor):
    """See ofx_sd_handoff in include/ofx.h.  Returns (image, cond_image, cond_mask, latmask, cond_mask_latent)."""
    a = _chk(image_bgr, "image_bgr", torch.uint8)
    r = _chk(reference_bgr, "reference_bgr", torch.uint8)
    m = _chk(image_mask, "image_mask", torch.uint8)
    ml = _chk(mask_latent, "mask_latent", torch.uint8)
    B, H, W, c3 = a.shape
    if c3 != 3 or tuple(r.shape) != tuple(a.shape) or tuple(m.shape) != (B, H, W) or ml.dim() != 3 or ml.shape[0] != B:
        raise RuntimeError("sd_handoff: shapes must be image/reference [B,H,W,3], image_mask [B,H,W], mask_latent [B,h,w]")
    h, w = ml.shape[1:]
    dev = a.device
    image = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    cond_image = torch.empty_like(image)
    cond_mask = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    latmask = torch.empty((B, 4, h, w), dtype=torch.float32, device=dev)
    cml = torch.empty((B, h, w), dtype=torch.float32, device=dev)
    check(_lib.lib().ofx_sd_handoff(_ptr(a), _ptr(r), _ptr(m), _ptr(ml), _ptr(image), _ptr(cond_image), _ptr(cond_mask), _ptr(latmask),
                                    _ptr(cml), B, H, W, h, w, _stream()), "ofx_sd_handoff")
    return image, cond_image, cond_mask, latmask, cml


def gaussian_blur_rgba_u8(img: torch.Tensor, radius: float) -> torch.Tensor:
    """uint8 [B,H,W,4] -> PIL.ImageFilter.GaussianBlur(radius) of every 4-channel image, the channels alike (what Pillow does to
    'RGBa' / 'RGBA'); the cost does not depend on the radius.  See ofx_gaussian_blur_rgba_u8 in include/ofx.h for the limits."""
    m = _chk(img, "img", torch.uint8)
    if m.dim() != 4 or m.shape[3] != 4:
        raise RuntimeError("gaussian_blur_rgba_u8: img must be [B,H,W,4]")
    B, H, W, _ = m.shape
    out = torch.empty_like(m)
    scratch = torch.empty_like(m)
    check(_lib.lib().ofx_gaussian_blur_rgba_u8(_ptr(m), _ptr(out), _ptr(scratch), B, H, W, float(radius), _stream()),
          "ofx_gaussian_blur_rgba_u8")
    return out


def fill_mask_input(image_bgr: torch.Tensor, image_mask: torch.Tensor) -> torch.Tensor:
    """See ofx_fill_mask_input in include/ofx.h: image_bgr uint8 [B,H,W,3], image_mask uint8 [B,H,W] (the blurred mask, 255 =
    repaint) -> the filled frame uint8 [B,H,W,3]."""
    a = _chk(image_bgr, "image_bgr", torch.uint8)
    m = _chk(image_mask, "image_mask", torch.uint8)
    if a.dim() != 4 or a.shape[3] != 3 or tuple(m.shape) != tuple(a.shape[:3]):
        raise RuntimeError("fill_mask_input: shapes must be image_bgr [B,H,W,3], image_mask [B,H,W]")
    B, H, W, _ = a.shape
    L = _lib.lib()
    out = torch.empty_like(a)
    scratch = torch.empty((L.ofx_fill_mask_input_scratch_bytes(B, H, W),), dtype=torch.uint8, device=a.device)
    check(L.ofx_fill_mask_input(_ptr(a), _ptr(m), _ptr(out), _ptr(scratch), B, H, W, _stream()), "ofx_fill_mask_input")
    return out


def groupnorm(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], groups: int = 32, eps: float = 1e-6,
              silu: bool = False, out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm(groups, C, eps, affine) of an NHWC tensor [B,H,W,C] (+ x * sigmoid(x) when silu): `Normalize` /
    `nonlinearity` of ldm/modules/diffusionmodules/model.py:35-41.  `out`: a float32 tensor of at least x.numel() elements to
    write (x itself: in place); `scratch`: a uint8 tensor whose whole length is offered as the scratch
    (ofx_groupnorm_scratch_bytes(B, C) bytes are needed).  Returns a [B,H,W,C] tensor either way: a new one, or a view of
    the first x.numel() elements of `out`."""
    t = _chk(x, "x", torch.float32)
    B, H, W, Cn = t.shape
    L = _lib.lib()
    if scratch is None:
        scratch = torch.empty((L.ofx_groupnorm_scratch_bytes(B, Cn),), dtype=torch.uint8, device=t.device)
    scratch = _chk(scratch, "scratch", torch.uint8)
    if out is None:
        out = torch.empty_like(t)
    out = _chk(out, "out", torch.float32)
    if out.numel() < t.numel():
        raise RuntimeError(f"out must hold {t.numel()} floats, got {out.numel()}")
    g = None if gamma is None else _chk(gamma, "gamma", torch.float32)
    b = None if beta is None else _chk(beta, "beta", torch.float32)
    check(L.ofx_groupnorm(_ptr(t), _ptr(g), _ptr(b), _ptr(out), _ptr(scratch), scratch.numel(), B, H * W, Cn, int(groups), float(eps),
                          1 if silu else 0, _stream()), "ofx_groupnorm")
    return out.view(-1)[:t.numel()].view_as(t)


def softmax_rows(x: torch.Tensor, rows: int, ld: int, n: int, scale: float = 1.0, bias: Optional[torch.Tensor] = None,
                 ld_bias: int = 0, bias_rows: int = 1) -> torch.Tensor:
    """In place on the float32 buffer `x` (at least rows * ld floats): x[r][0..n) = softmax(x[r][0..n) * scale +
    bias[r % bias_rows][0..n)), columns n..ld-1 set to 0 (ofx_softmax_rows).  bias: rows of ld_bias floats."""
    x = _chk(x, "x", torch.float32)
    if x.numel() < rows * ld:
        raise RuntimeError(f"x must hold rows * ld = {rows * ld} floats, got {x.numel()}")
    b = None if bias is None else _chk(bias, "bias", torch.float32)
    if b is not None and b.numel() < (bias_rows - 1) * ld_bias + n:
        raise RuntimeError("bias must hold bias_rows rows of ld_bias floats")
    check(_lib.lib().ofx_softmax_rows(_ptr(x), int(rows), int(ld), int(n), float(scale), _ptr(b), int(ld_bias), int(bias_rows), _stream()),
          "ofx_softmax_rows")
    return x


def upconv2x_weight(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW fp32 3x3 (CPU) -> the four parity-folded 2x2 operands of `upconv2x` (float64 sums, one rounding) as an fp32 CPU tensor
    [4, Cout, 4, Cin]: parity 2*py + px of the output pixel, tap 2*ty + tx over the low-resolution pixel
    (y - 1 + py + ty, x - 1 + px + tx) (ofx_upconv2x_weight)."""
    w = w_oihw.detach().to(torch.float32).contiguous().cpu()
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError("upconv2x_weight: OIHW 3x3 weights only")
    co, ci = int(w.shape[0]), int(w.shape[1])
    return _wino_weight("ofx_upconv2x_weight", w, co, ci).reshape(4, co, 4, ci)


# upconv2x(precision=) -> OFX_PREC_* of ofx_upconv2x_prec.  "fp16": x and the folded weights rounded to half (nearest even) as the
# kernel stages them, the contraction on the fp16 matrix cores with fp32 accumulation, bias and result fp32 (include/ofx.h).
UPCONV_PRECISIONS = {"fp32": 0, "fp16": 5}


def check_upconv_precision(precision, name: str = "precision") -> str:
    if not isinstance(precision, str) or precision not in UPCONV_PRECISIONS:
        raise ValueError(f"{name} must be one of {tuple(UPCONV_PRECISIONS)}, got {precision!r}")
    return precision


def upconv2x_bn(cout: int, precision: str = "fp32") -> int:
    """The column-tile width (64 or 128) of the 128 x BN tile `upconv2x` launches for `cout` output channels (ofx_upconv2x_bn; no
    device needed)."""
    bn = _lib.lib().ofx_upconv2x_bn(int(cout), UPCONV_PRECISIONS[check_upconv_precision(precision)])
    if bn < 0:
        raise _lib.OfxError(bn, "ofx_upconv2x_bn")
    return bn


def upconv2x(x: torch.Tensor, w_folded: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             out_off: int = 0, precision: str = "fp32") -> torch.Tensor:
    """conv3x3(pad 1)(nearest 2x upsample of x) + bias in one kernel that never forms the upsampled map: x [B,H,W,Cin],
    w_folded [4,Cout,4,Cin] from `upconv2x_weight` (on the device) -> [B,2H,2W,Cout].  `out` [B,2H,2W,C >= out_off + Cout]: write
    channels [out_off, out_off + Cout) of it (a strided row).  precision: "fp32" (default, `ofx_upconv2x`) or "fp16"
    (`ofx_upconv2x_prec`: both operands rounded to half as they are staged, fp32 accumulation); anything else is a ValueError.
    Under "fp16" a float16 `w_folded` (`half_conv_weight` of the folded operand) is read as it is (OFX_PREC_F16_W), bit-identical
    to the float32 operand it was rounded from; a float16 `w_folded` under "fp32" is a RuntimeError before any launch."""
    check_upconv_precision(precision)                              # before a device is touched
    x = _chk(x, "x", torch.float32)
    half_w = precision == "fp16" and isinstance(w_folded, torch.Tensor) and w_folded.dtype == torch.float16
    w = _chk(w_folded, "w_folded", torch.float16 if half_w else torch.float32)
    if x.dim() != 4 or w.dim() != 4 or w.shape[0] != 4 or w.shape[2] != 4 or w.shape[3] != x.shape[3]:
        raise RuntimeError(f"upconv2x: x [B,H,W,Cin] and w_folded [4,Cout,4,Cin] expected, got {tuple(x.shape)} and {tuple(w.shape)}")
    B, H, W, ci = x.shape
    co = int(w.shape[1])
    b = None if bias is None else _chk(bias, "bias", torch.float32)
    if b is not None and tuple(b.shape) != (co,):
        raise RuntimeError(f"upconv2x: bias must be [{co}]")
    if out is None:
        out = torch.empty((B, 2 * H, 2 * W, co), dtype=torch.float32, device=x.device)
    out = _chk(out, "out", torch.float32)
    if tuple(out.shape[:3]) != (B, 2 * H, 2 * W) or out_off < 0 or out.shape[3] < out_off + co:
        raise RuntimeError(f"out must be [{B},{2 * H},{2 * W},>= {out_off + co}], got {tuple(out.shape)}")
    po = C.c_void_p(out.data_ptr() + 4 * out_off)
    if precision == "fp32":
        check(_lib.lib().ofx_upconv2x(_ptr(x), _ptr(w), _ptr(b), po, out.shape[3], B, H, W, ci, co, _stream()), "ofx_upconv2x")
    else:
        check(_lib.lib().ofx_upconv2x_prec(_ptr(x), _ptr(w), _ptr(b), po, out.shape[3], B, H, W, ci, co,
                                           CONV_PRECISIONS["fp16_w"] if half_w else UPCONV_PRECISIONS[precision], _stream()), "ofx_upconv2x_prec")
    return out


def conv3x3_silu(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], cout: int, stride: int = 1, silu: bool = True,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """silu(conv3x3(x, padding 1, stride 1 | 2) + bias) in one kernel (ofx_conv3x3_silu; a layer of ControlNet's hint stem):
    x [B,H,W,C] NHWC fp32 on the device -- C >= Cin, the channels beyond Cin are skipped (a strided row) -- and w
    `pack_conv_weight`'s [cout, Kpad] of a [cout, Cin', 3, 3] weight on the device, Cin = Cin' rounded up to a multiple of 4 (the
    padding meets zero weights) = the one multiple of 4 whose Kpad this is (Kpad grows by 32, 9 Cin by 36).  silu=False: no activation.
    -> [B,Hout,Wout,cout], Hout = (H - 1) // stride + 1; `out` [B,Hout,Wout,C' >= cout]: columns [0, cout) of it are written."""
    x = _chk(x, "x", torch.float32)
    w = _chk(w, "w", torch.float32)
    if x.dim() != 4 or w.dim() != 2 or w.shape[0] != cout:
        raise RuntimeError(f"conv3x3_silu: x [B,H,W,C] and w [{cout},Kpad] expected, got {tuple(x.shape)} and {tuple(w.shape)}")
    B, H, W, ldx = x.shape
    cin = int(w.shape[1]) // 9 // 4 * 4
    if cin <= 0 or -(-9 * cin // 32) * 32 != w.shape[1] or ldx < cin:
        raise RuntimeError(f"conv3x3_silu: w {tuple(w.shape)} is not a packed 3x3 weight over at most the {ldx} channels of x")
    b = None if bias is None else _chk(bias, "bias", torch.float32)
    if b is not None and tuple(b.shape) != (cout,):
        raise RuntimeError(f"conv3x3_silu: bias must be [{cout}]")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((B, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    out = _chk(out, "out", torch.float32)
    if out.dim() != 4 or tuple(out.shape[:3]) != (B, Ho, Wo) or out.shape[3] < cout:
        raise RuntimeError(f"out must be [{B},{Ho},{Wo},>= {cout}], got {tuple(out.shape)}")
    check(_lib.lib().ofx_conv3x3_silu(_ptr(x), int(ldx), cin, _ptr(w), int(w.shape[1]), _ptr(b), _ptr(out), int(out.shape[3]), int(cout),
                                      B, H, W, int(stride), int(bool(silu)), _stream()), "ofx_conv3x3_silu")
    return out


def upsample2x_nearest(x: torch.Tensor) -> torch.Tensor:
    """F.interpolate(scale_factor=2.0, mode="nearest") of an NHWC fp32 tensor [B,H,W,C] -> [B,2H,2W,C] (C % 4 == 0)."""
    x = _chk(x, "x", torch.float32)
    if x.dim() != 4:
        raise RuntimeError("upsample2x_nearest: x must be [B,H,W,C]")
    B, H, W, Cn = x.shape
    out = torch.empty((B, 2 * H, 2 * W, Cn), dtype=torch.float32, device=x.device)
    check(_lib.lib().ofx_upsample2x_nearest_f32(_ptr(x), _ptr(out), B, H, W, Cn, _stream()), "ofx_upsample2x_nearest_f32")
    return out


def decode_to_u8(x: torch.Tensor) -> torch.Tensor:
    """f32 NHWC RGB [B,H,W,C >= 3] (the first three channels are read) -> u8 BGR [B,H,W,3] =
    (clip(x, -1, 1) * 127.5 + 127.5).astype(uint8), the bits of decode_latent's numpy expression."""
    x = _chk(x, "x", torch.float32)
    if x.dim() != 4 or x.shape[3] < 3:
        raise RuntimeError("decode_to_u8: x must be [B,H,W,C >= 3]")
    B, H, W, ld = x.shape
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device)
    check(_lib.lib().ofx_decode_to_u8(_ptr(x), ld, _ptr(out), B, H, W, _stream()), "ofx_decode_to_u8")
    return out


# attention(precision=) / attention_bnhd(precision=) -> OFX_PREC_* of ofx_attention_prec / ofx_attention_bnhd_prec.  "fp16": q, k, v and
# the probabilities rounded to half (nearest even) as the kernel stages them, both products on the fp16 matrix cores with fp32
# accumulation, softmax, scale and bias in fp32 (include/ofx.h); the fused head sizes only, tensors stay fp32 in memory.
ATTENTION_PRECISIONS = {"fp32": 0, "fp16": 5}
ATTENTION_FUSED_HEAD_SIZES = (40, 64, 80, 128, 160)


def check_attention_precision(precision, name: str = "precision") -> str:
    if not isinstance(precision, str) or precision not in ATTENTION_PRECISIONS:
        raise ValueError(f"{name} must be one of {tuple(ATTENTION_PRECISIONS)}, got {precision!r}")
    return precision


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, bias: Optional[torch.Tensor] = None,
              scale: Optional[float] = None, max_workspace_bytes: int = 8 << 30, precision: str = "fp32") -> torch.Tensor:
    """softmax(q k^T * scale + bias) v for fp32 [BH,Nq,D] / [BH,Nk,D] tensors; bias [Nq,Nk] (shared) or [BH,Nq,Nk].
    scale defaults to D^-0.5.  Batch-heads are processed in slices that keep the score matrix under
    `max_workspace_bytes`.  precision: "fp32" (default, `ofx_attention_f32`) or "fp16" (`ofx_attention_prec`, the fused head sizes
    40 / 64 / 80 / 128 / 160 only: any other D is a ValueError, there is no unfused fp16 path)."""
    check_attention_precision(precision)                           # before a device is touched
    if precision == "fp16":
        if not isinstance(q, torch.Tensor) or q.dim() != 3 or int(q.shape[-1]) not in ATTENTION_FUSED_HEAD_SIZES:
            raise ValueError(f'attention: precision="fp16" needs q [BH,Nq,D] with D in {ATTENTION_FUSED_HEAD_SIZES}')
    q = _chk(q, "q", torch.float32)
    k = _chk(k, "k", torch.float32)
    v = _chk(v, "v", torch.float32)
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    if tuple(k.shape) != (BH, Nk, D) or tuple(v.shape) != (BH, Nk, D):
        raise RuntimeError("attention: q [BH,Nq,D], k / v [BH,Nk,D] expected")
    per_bh = bias is not None and bias.dim() == 3
    if bias is not None:
        bias = _chk(bias, "bias", torch.float32)
        if tuple(bias.shape) not in ((Nq, Nk), (BH, Nq, Nk)):
            raise RuntimeError("attention: bias must be [Nq,Nk] or [BH,Nq,Nk]")
    scale = float(D) ** -0.5 if scale is None else float(scale)
    L = _lib.lib()
    one = L.ofx_attention_workspace_bytes(1, Nq, Nk, D)          # 0: the fused kernel takes this head size, no scores in HBM
    step = BH if one == 0 else max(1, min(BH, int(max_workspace_bytes // one)))
    ws = torch.empty((max(16, L.ofx_attention_workspace_bytes(step, Nq, Nk, D)),), dtype=torch.uint8, device=q.device)
    out = torch.empty_like(q)
    for z0 in range(0, BH, step):
        n = min(step, BH - z0)
        bz = None if bias is None else (bias[z0:z0 + n] if per_bh else bias)
        if precision == "fp32":
            check(L.ofx_attention_f32(_ptr(q[z0:z0 + n]), _ptr(k[z0:z0 + n]), _ptr(v[z0:z0 + n]), _ptr(bz), Nq * Nk if per_bh else 0,
                                      _ptr(out[z0:z0 + n]), n, Nq, Nk, D, scale, _ptr(ws), ws.numel(), _stream()), "ofx_attention_f32")
        else:
            check(L.ofx_attention_prec(_ptr(q[z0:z0 + n]), _ptr(k[z0:z0 + n]), _ptr(v[z0:z0 + n]), _ptr(bz), Nq * Nk if per_bh else 0,
                                       _ptr(out[z0:z0 + n]), n, Nq, Nk, D, scale, ATTENTION_PRECISIONS[precision], _ptr(ws), ws.numel(),
                                       _stream()), "ofx_attention_prec")
    return out


# --------------------------------------------------------------------------------------
# SpatialTransformer pieces (ldm/modules/attention.py:438-537): LayerNorm, GEGLU, attention on token rows
# --------------------------------------------------------------------------------------
def _rows_view(t: torch.Tensor, name: str) -> Tuple[int, int, int]:
    """(rows, C, ld) of a float32 CUDA tensor [..., C] whose leading dimensions flatten to rows `ld` floats apart: a contiguous
    tensor, or a last-axis slice of a wider contiguous one."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() < 1 or t.numel() == 0:
        raise RuntimeError(f"{name} must be a non-empty CUDA float32 tensor")
    Cn = int(t.shape[-1])
    ld, span = Cn, None
    for i in range(t.dim() - 2, -1, -1):
        if t.shape[i] == 1:
            continue
        if span is None:
            ld = int(t.stride(i))
        elif t.stride(i) != span:
            raise RuntimeError(f"{name} must be contiguous, or a last-axis slice of a contiguous tensor")
        span = int(t.stride(i)) * int(t.shape[i])
    if (Cn > 1 and t.stride(-1) != 1) or ld < Cn:
        raise RuntimeError(f"{name} must be contiguous, or a last-axis slice of a contiguous tensor")
    return t.numel() // Cn, Cn, ld


def layernorm(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float = 1e-5,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.LayerNorm(C) over the last axis (biased variance; `ofx_layernorm`, one wave per row).  x: [..., C] float32, contiguous or a
    last-axis slice of a wider contiguous tensor (rows `stride(-2)` floats apart); C % 4 == 0, C <= 4096.  `out`: the same shape
    (x itself: in place), also possibly a slice; a new contiguous tensor otherwise."""
    rows, Cn, ldx = _rows_view(x, "x")
    if out is None:
        out = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    _, _, ldo = _rows_view(out, "out")
    if tuple(out.shape) != tuple(x.shape):
        raise RuntimeError(f"out must be {tuple(x.shape)}, got {tuple(out.shape)}")
    g = None if gamma is None else _chk(gamma, "gamma", torch.float32)
    b = None if beta is None else _chk(beta, "beta", torch.float32)
    for nm, t in (("gamma", g), ("beta", b)):
        if t is not None and tuple(t.shape) != (Cn,):
            raise RuntimeError(f"{nm} must be [{Cn}]")
    check(_lib.lib().ofx_layernorm(_ptr(x), ldx, _ptr(g), _ptr(b), _ptr(out), ldo, rows, Cn, float(eps), _stream()), "ofx_layernorm")
    return out


def geglu(a: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GEGLU.forward after its Linear (attention.py:54-56): a [..., 2 * inner] -> a[..., :inner] * gelu(a[..., inner:]), gelu in the
    exact erf form (`ofx_geglu`).  a and `out` [..., inner]: contiguous or last-axis slices of wider tensors; inner % 4 == 0."""
    rows, two, lda = _rows_view(a, "a")
    if two % 2:
        raise RuntimeError("geglu: the last axis holds the values and the gates, an even count")
    inner = two // 2
    shape = tuple(a.shape[:-1]) + (inner,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=a.device)
    _, _, ldo = _rows_view(out, "out")
    if tuple(out.shape) != shape:
        raise RuntimeError(f"out must be {shape}, got {tuple(out.shape)}")
    check(_lib.lib().ofx_geglu(_ptr(a), lda, _ptr(out), ldo, rows, inner, _stream()), "ofx_geglu")
    return out


def _bnhd(t: torch.Tensor, name: str) -> int:
    """The row stride of a [B,N,H*D] operand of `attention_bnhd`: dense along the last axis, rows stride(1) floats apart, images
    N rows apart."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3:
        raise RuntimeError(f"{name} must be a CUDA float32 tensor [B,N,H*D]")
    B, N, W = t.shape
    ld = int(t.stride(1)) if N > 1 else (int(t.stride(0)) if B > 1 else W)
    if (W > 1 and t.stride(2) != 1) or ld < W or (B > 1 and t.stride(0) != N * ld):
        raise RuntimeError(f"{name} must be contiguous, or a last-axis slice of a contiguous [B,N,wider] tensor")
    return ld


def attention_bnhd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, bias: Optional[torch.Tensor] = None,
                   scale: Optional[float] = None, out: Optional[torch.Tensor] = None, precision: str = "fp32") -> torch.Tensor:
    """`attention` on token rows: q [B,Nq,H*D], k / v [B,Nk,H*D] with the heads side by side in a row, as a projection GEMM leaves
    them -- contiguous tensors, or last-axis slices of wider ones (the three thirds of one fused q|k|v buffer); the row stride is
    read from stride(1).  bias [Nq,Nk] or [B*H,Nq,Nk]; scale defaults to D^-0.5.  Returns `out` [B,Nq,H*D] (new and contiguous when
    not given), bit for bit what `attention` gives on the permuted contiguous copies.  Head sizes the fused kernel takes only
    (`ofx_attention_bnhd_f32`: D in 40 / 64 / 80 / 128 / 160, OFX_EINVAL otherwise).  precision: "fp32" (default) or "fp16"
    (`ofx_attention_bnhd_prec`, as in `attention`); anything else is a ValueError before a device is touched."""
    check_attention_precision(precision)
    ldq, ldk, ldv = _bnhd(q, "q"), _bnhd(k, "k"), _bnhd(v, "v")
    B, Nq, W = q.shape
    Nk = k.shape[1]
    H = int(heads)
    if H <= 0 or W % H or tuple(k.shape) != (B, Nk, W) or tuple(v.shape) != (B, Nk, W):
        raise RuntimeError("attention_bnhd: q [B,Nq,H*D], k / v [B,Nk,H*D] expected")
    D = W // H
    per_bh = bias is not None and bias.dim() == 3
    if bias is not None:
        bias = _chk(bias, "bias", torch.float32)
        if tuple(bias.shape) not in ((Nq, Nk), (B * H, Nq, Nk)):
            raise RuntimeError("attention_bnhd: bias must be [Nq,Nk] or [B*H,Nq,Nk]")
    if out is None:
        out = torch.empty((B, Nq, W), dtype=torch.float32, device=q.device)
    ldo = _bnhd(out, "out")
    if tuple(out.shape) != (B, Nq, W):
        raise RuntimeError(f"out must be {(B, Nq, W)}, got {tuple(out.shape)}")
    scale = float(D) ** -0.5 if scale is None else float(scale)
    if precision == "fp32":
        check(_lib.lib().ofx_attention_bnhd_f32(_ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, _ptr(bias), Nq * Nk if per_bh else 0, _ptr(out), ldo,
                                                B, H, Nq, Nk, D, scale, _stream()), "ofx_attention_bnhd_f32")
    else:
        check(_lib.lib().ofx_attention_bnhd_prec(_ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, _ptr(bias), Nq * Nk if per_bh else 0, _ptr(out),
                                                 ldo, B, H, Nq, Nk, D, scale, ATTENTION_PRECISIONS[precision], _stream()),
              "ofx_attention_bnhd_prec")
    return out


KV_DTYPES = {"fp32": torch.float32, "fp16": torch.float16}       # `kv_dtype=` of the models: the dtype of a recorded K/V history


def check_kv_dtype(kv_dtype, name: str = "kv_dtype") -> str:
    if not isinstance(kv_dtype, str) or kv_dtype not in KV_DTYPES:
        raise ValueError(f"{name} must be one of {tuple(KV_DTYPES)}, got {kv_dtype!r}")
    return kv_dtype


def _kv_segment_lists(segments, B: int) -> list:
    """`segments` of `attention_bnhd_segments` -> B lists of (k, v), checked as far as metadata goes (no device): the list
    structure, one dtype throughout, the table limits.  ValueError otherwise."""
    if not isinstance(segments, (list, tuple)) or len(segments) == 0:
        raise ValueError("segments must be a non-empty list of (k, v) pairs, or one such list per image")
    is_pair = lambda e: isinstance(e, (list, tuple)) and len(e) == 2 and all(isinstance(t, torch.Tensor) for t in e)
    if all(is_pair(e) for e in segments):
        per_image = [list(segments)] * B                          # one list shared by all images
    else:
        if len(segments) != B:
            raise ValueError(f"segments holds {len(segments)} per-image lists, q has {B} images")
        per_image = [list(s) if isinstance(s, (list, tuple)) else [s] for s in segments]
        for b, segs in enumerate(per_image):
            if not segs or not all(is_pair(e) for e in segs):
                raise ValueError(f"segments[{b}] must be a non-empty list of (k, v) tensor pairs")
    dtypes = {t.dtype for segs in per_image for e in segs for t in e}
    if len(dtypes) != 1 or next(iter(dtypes)) not in (torch.float32, torch.float16):
        raise ValueError(f"segments must be all float32 or all float16 (one element type per launch), got {sorted(str(d) for d in dtypes)}")
    if max(len(s) for s in per_image) > _lib.KV_MAX_SEGMENTS or sum(len(s) for s in per_image) > _lib.KV_MAX_ENTRIES:
        raise ValueError(f"at most {_lib.KV_MAX_SEGMENTS} segments per image and {_lib.KV_MAX_ENTRIES} in all, got "
                         f"{[len(s) for s in per_image]}")
    return per_image


def attention_bnhd_segments(q: torch.Tensor, segments, heads: int, bias: Optional[torch.Tensor] = None, scale: Optional[float] = None,
                            out: Optional[torch.Tensor] = None, precision: str = "fp32") -> torch.Tensor:
    """`attention_bnhd` with K and V read in place through a segment table (`ofx_attention_bnhd_segs`): image b attends to the
    logical concatenation of its segments, nothing is copied, widened or concatenated.  segments: one list of (k, v) per image, or
    one list shared by all images; each k / v is [n_i, H*D], contiguous or a last-axis slice of a wider tensor (a third of a q|k|v
    buffer), all float32 or all float16; every image's n_i sum to the same Nk.  At most 8 segments per image, 64 in all.  q, bias
    ([Nq,Nk] or [B*H,Nq,Nk]) and out are float32 as in `attention_bnhd`.  Bit for bit `attention_bnhd` on the concatenated float32
    tensors; float16 segments feed the "fp16" kernel without a second rounding and are widened exactly in the "fp32" kernel.
    Every check runs before a device is touched; a bad structure, mixed dtypes or a table beyond the limits is a ValueError."""
    check_attention_precision(precision)
    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        raise RuntimeError("q must be a CUDA float32 tensor [B,Nq,H*D]")
    B, Nq, W = (int(s) for s in q.shape)
    H = int(heads)
    if H <= 0 or W % H:
        raise RuntimeError("attention_bnhd_segments: q [B,Nq,H*D] expected")
    D = W // H
    per_image = _kv_segment_lists(segments, B)
    half = per_image[0][0][0].dtype == torch.float16
    table = (_lib.KvSegment * sum(len(s) for s in per_image))()
    counts = (C.c_int * B)(*[len(s) for s in per_image])
    for b, segs in enumerate(per_image):                          # shapes and totals first: metadata, as the checks above
        for i, (k, v) in enumerate(segs):
            for t in (k, v):
                if t.dim() != 2 or t.shape[1] != W or t.shape[0] != k.shape[0] or t.shape[0] == 0:
                    raise ValueError(f"segments[{b}][{i}]: k and v must be [n, {W}] with one n > 0, got {tuple(k.shape)} and {tuple(v.shape)}")
    totals = [sum(int(k.shape[0]) for k, _ in segs) for segs in per_image]
    if len(set(totals)) != 1:
        raise ValueError(f"every image's segments must sum to one token count, got {totals}")
    at = 0
    for b, segs in enumerate(per_image):
        for i, (k, v) in enumerate(segs):
            lds = []
            for nm, t in (("k", k), ("v", v)):
                ld = int(t.stride(0)) if t.shape[0] > 1 else W
                if (W > 1 and t.stride(1) != 1) or ld < W or ld % 4 or not t.is_cuda or t.device != q.device:
                    raise RuntimeError(f"segments[{b}][{i}].{nm} must be on q's device, dense along the last axis, rows a multiple of 4 "
                                       f"elements apart")
                lds.append(ld)
            table[at].k, table[at].v, table[at].n, table[at].ldk, table[at].ldv = k.data_ptr(), v.data_ptr(), int(k.shape[0]), lds[0], lds[1]
            at += 1
    return _attention_bnhd_segment_table(q, table, counts, half, totals[0], H, bias, scale, out, precision)


def _kv_segment_table(rows):
    """(kptr, vptr, n, ldk, ldv) rows -> the `ofx_kv_segment` array `ofx_attention_bnhd_segs` takes."""
    return (_lib.KvSegment * len(rows))(*rows)


def _attention_bnhd_segment_table(q: torch.Tensor, table, counts, half: bool, Nk: int, heads: int, bias: Optional[torch.Tensor] = None,
                                 scale: Optional[float] = None, out: Optional[torch.Tensor] = None, precision: str = "fp32") -> torch.Tensor:
    """Internal.  The launch of `attention_bnhd_segments` for a caller that holds the table already (`_kv_segment_table`; image b owns the next
    counts[b] entries, a ctypes int array) and keeps the segments' tensors alive: `SpatialTransformer` builds one table per forward
    from entries it has planned, without a tensor view per image and entry.  q, bias and out are checked here; the table is
    checked by the C entry, before any launch."""
    check_attention_precision(precision)
    B, Nq, W = (int(s) for s in q.shape)
    H = int(heads)
    D = W // H
    ldq = _bnhd(q, "q")
    per_bh = bias is not None and bias.dim() == 3
    if bias is not None:
        bias = _chk(bias, "bias", torch.float32)
        if tuple(bias.shape) not in ((Nq, Nk), (B * H, Nq, Nk)):
            raise RuntimeError("attention_bnhd_segments: bias must be [Nq,Nk] or [B*H,Nq,Nk]")
    if out is None:
        out = torch.empty((B, Nq, W), dtype=torch.float32, device=q.device)
    ldo = _bnhd(out, "out")
    if tuple(out.shape) != (B, Nq, W):
        raise RuntimeError(f"out must be {(B, Nq, W)}, got {tuple(out.shape)}")
    scale = float(D) ** -0.5 if scale is None else float(scale)
    check(_lib.lib().ofx_attention_bnhd_segs(_ptr(q), ldq, table, counts, _lib.KV_TYPES["fp16" if half else "fp32"], _ptr(bias),
                                             Nq * Nk if per_bh else 0, _ptr(out), ldo, B, H, Nq, D, scale, ATTENTION_PRECISIONS[precision],
                                             _stream()), "ofx_attention_bnhd_segs")
    return out


# --------------------------------------------------------------------------------------
# CLIP text encoder pieces (hack.py:32-70): the token + position embedding and quick_gelu
# --------------------------------------------------------------------------------------
def clip_embed(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor, T: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """CLIPTextEmbeddings.forward (`ofx_clip_embed`): ids int32 [...] on the device, flattened to rows in sequence-major order; tok
    [vocab,C] and pos [>=T,C] float32, contiguous -> out[r] = tok[ids[r]] + pos[r % T], float32 [..., C] (new and contiguous when not
    given; `out` may be a last-axis slice of a wider tensor).  C % 4 == 0.  A row whose id is outside [0, vocab) comes out all NaN."""
    ids = _chk(ids, "ids", torch.int32)
    tok = _chk(tok, "tok", torch.float32)
    pos = _chk(pos, "pos", torch.float32)
    T = int(T)
    if tok.dim() != 2 or pos.dim() != 2 or pos.shape[1] != tok.shape[1] or T <= 0 or pos.shape[0] < T:
        raise RuntimeError("clip_embed: tok [vocab,C] and pos [>=T,C] expected")
    vocab, Cn = (int(s) for s in tok.shape)
    rows = ids.numel()
    shape = tuple(ids.shape) + (Cn,)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=ids.device)
    if tuple(out.shape) != shape:
        raise RuntimeError(f"out must be {shape}, got {tuple(out.shape)}")
    if rows == 0:
        return out
    _, _, ldo = _rows_view(out, "out")
    check(_lib.lib().ofx_clip_embed(_ptr(ids), _ptr(tok), _ptr(pos), _ptr(out), ldo, rows, T, Cn, vocab, _stream()), "ofx_clip_embed")
    return out


def quick_gelu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x * sigmoid(1.702 x) over the last axis' rows (`ofx_quick_gelu`).  x and `out` [..., n] float32: contiguous or last-axis slices
    of wider tensors; n % 4 == 0.  `out`: the same shape (x itself: in place); a new contiguous tensor otherwise."""
    rows, n, ldx = _rows_view(x, "x")
    if out is None:
        out = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    _, _, ldo = _rows_view(out, "out")
    if tuple(out.shape) != tuple(x.shape):
        raise RuntimeError(f"out must be {tuple(x.shape)}, got {tuple(out.shape)}")
    check(_lib.lib().ofx_quick_gelu(_ptr(x), ldx, _ptr(out), ldo, rows, n, _stream()), "ofx_quick_gelu")
    return out


# --------------------------------------------------------------------------------------
# UNet pieces (ldm/modules/diffusionmodules/openaimodel.py:257-277, :530-534, :757-793; util.py:154-174)
# --------------------------------------------------------------------------------------
def _nhwc_seg(t: torch.Tensor, name: str) -> Tuple[int, int, int, int, int]:
    """(B, H, W, C, ld) of a float32 CUDA tensor [B,H,W,C]: contiguous, or a channel slice of a wider contiguous tensor."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise RuntimeError(f"{name} must be a CUDA float32 tensor [B,H,W,C]")
    _, Cn, ld = _rows_view(t, name)
    return int(t.shape[0]), int(t.shape[1]), int(t.shape[2]), Cn, ld


def groupnorm_cat(x0: torch.Tensor, x1: Optional[torch.Tensor], gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor],
                  e: Optional[torch.Tensor] = None, groups: int = 32, eps: float = 1e-6, silu: bool = False,
                  out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm(groups, C0 + C1, eps, affine) of th.cat([x0, x1], channels) + e[b, c] (+ x * sigmoid(x) when silu) without forming
    the concatenation or the shifted map: `in_layers` / `out_layers` of `ResBlock._forward` (openaimodel.py:257-277) behind
    `th.cat([h, hs.pop()], dim=1)` (:786) and `h + emb_out` (:275).  x0 [B,H,W,C0], x1 [B,H,W,C1] or None: float32 NHWC, contiguous
    or channel slices of wider contiguous tensors; e [B, C0 + C1] or None, contiguous or a column slice of a wider [B, n] tensor;
    gamma / beta [C0 + C1] or None.  C0, C1 and the row strides are multiples of 4.  `out`: a contiguous [B,H,W,C0 + C1] tensor (x0
    itself, in place, only when x1 is None and x0 is contiguous); `scratch`: a uint8 tensor of at least
    ofx_groupnorm_cat_scratch_bytes(B, C0 + C1) bytes.  With x1 = e = None the bits are `groupnorm`'s (`ofx_groupnorm_cat`)."""
    B, H, W, C0, ld0 = _nhwc_seg(x0, "x0")
    C1, ld1 = 0, 0
    if x1 is not None:
        B1, H1, W1, C1, ld1 = _nhwc_seg(x1, "x1")
        if (B1, H1, W1) != (B, H, W):
            raise RuntimeError(f"x1 must be [{B},{H},{W},C1], got {tuple(x1.shape)}")
    Cn = C0 + C1
    lde = 0
    if e is not None:
        if not isinstance(e, torch.Tensor) or e.dim() != 2 or tuple(e.shape) != (B, Cn):
            raise RuntimeError(f"e must be a CUDA float32 tensor [{B},{Cn}]")
        _, _, lde = _rows_view(e, "e")
    L = _lib.lib()
    if scratch is None:
        scratch = torch.empty((L.ofx_groupnorm_cat_scratch_bytes(B, Cn),), dtype=torch.uint8, device=x0.device)
    scratch = _chk(scratch, "scratch", torch.uint8)
    if out is None:
        out = torch.empty((B, H, W, Cn), dtype=torch.float32, device=x0.device)
    out = _chk(out, "out", torch.float32)
    if tuple(out.shape) != (B, H, W, Cn):
        raise RuntimeError(f"out must be {(B, H, W, Cn)}, got {tuple(out.shape)}")
    g = None if gamma is None else _chk(gamma, "gamma", torch.float32)
    b = None if beta is None else _chk(beta, "beta", torch.float32)
    for nm, t in (("gamma", g), ("beta", b)):
        if t is not None and tuple(t.shape) != (Cn,):
            raise RuntimeError(f"{nm} must be [{Cn}]")
    check(L.ofx_groupnorm_cat(_ptr(x0), ld0, C0, _ptr(x1), ld1, C1, _ptr(e), lde, _ptr(g), _ptr(b), _ptr(out), _ptr(scratch),
                              scratch.numel(), B, H * W, int(groups), float(eps), 1 if silu else 0, _stream()), "ofx_groupnorm_cat")
    return out


EMB_LINEAR_ROWS = 16      # rows per launch of ofx_emb_linear


def emb_linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, silu_in: bool = False,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`nn.Linear` on a handful of rows, behind `nn.SiLU` when silu_in: `time_embed` and the `emb_layers` of the UNet
    (openaimodel.py:530-534, :220-226).  x [B, K] float32 (contiguous or a column slice), w [N, K] as the checkpoint holds it, bias
    [N] or None -> out [B, N]: a new contiguous tensor, or `out` (possibly a column slice of a wider tensor, whose other columns are
    left alone).  K % 4 == 0.  `ofx_emb_linear` takes 16 rows a launch; more rows are sliced here."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise RuntimeError("x must be a CUDA float32 tensor [B, K]")
    B, K, ldx = _rows_view(x, "x")
    w = _chk(w, "w", torch.float32)
    if w.dim() != 2 or w.shape[1] != K:
        raise RuntimeError(f"w must be [N, {K}], got {tuple(w.shape)}")
    N = int(w.shape[0])
    bb = None if bias is None else _chk(bias, "bias", torch.float32)
    if bb is not None and tuple(bb.shape) != (N,):
        raise RuntimeError(f"bias must be [{N}]")
    if out is None:
        out = torch.empty((B, N), dtype=torch.float32, device=x.device)
    if not isinstance(out, torch.Tensor) or out.dim() != 2 or tuple(out.shape) != (B, N):
        raise RuntimeError(f"out must be a CUDA float32 tensor [{B}, {N}]")
    _, _, ldo = _rows_view(out, "out")
    fn = _lib.lib().ofx_emb_linear
    for r0 in range(0, B, EMB_LINEAR_ROWS):
        nb = min(EMB_LINEAR_ROWS, B - r0)
        check(fn(C.c_void_p(x.data_ptr() + 4 * r0 * ldx), ldx, _ptr(w), _ptr(bb), C.c_void_p(out.data_ptr() + 4 * r0 * ldo), ldo, nb, K, N,
                 1 if silu_in else 0, _stream()), "ofx_emb_linear")
    return out


def timestep_freqs(dim: int, max_period: float = 10000.0) -> torch.Tensor:
    """The frequency table of `timestep_embedding` in the reference's own arithmetic (util.py:165-167): fp32 on the CPU,
    exp(-log(max_period) * arange(half) / half), half = dim // 2.  Move it to the device once."""
    half = int(dim) // 2
    return torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half) if half else torch.zeros((0,))


def timestep_embedding(t: torch.Tensor, freqs: torch.Tensor, dim: int) -> torch.Tensor:
    """`timestep_embedding(timesteps, dim)` (util.py:154-174): t float32 [B] on the device (fractional values are legal), freqs
    [dim // 2] from `timestep_freqs` on the device -> [B, dim] = cos(t f) | sin(t f) (| a zero column when dim is odd)."""
    t = _chk(t, "t", torch.float32)
    f = _chk(freqs, "freqs", torch.float32)
    dim = int(dim)
    if t.dim() != 1 or t.numel() == 0 or dim <= 0 or tuple(f.shape) != (dim // 2,):
        raise RuntimeError(f"timestep_embedding: t [B] and freqs [{dim // 2}] expected, got {tuple(t.shape)} and {tuple(f.shape)}")
    out = torch.empty((t.shape[0], dim), dtype=torch.float32, device=t.device)
    check(_lib.lib().ofx_timestep_embedding(_ptr(t), _ptr(f) if dim >= 2 else None, _ptr(out), int(t.shape[0]), dim, _stream()),
          "ofx_timestep_embedding")
    return out


# --------------------------------------------------------------------------------------
# sampler (guided_ldm_inpainting.py:28-137, guided_ldm.py:30-158)
# --------------------------------------------------------------------------------------
DDIM_COEF_FIELDS = ("cfg", "sqrt_at", "sqrt_1m_at", "sqrt_aprev", "dir_coef", "sigma_t", "g", "sa", "s1")


def ddim_step(x: torch.Tensor, coef: Dict[str, float], eps_c: Optional[torch.Tensor] = None, eps_u: Optional[torch.Tensor] = None,
              guidance: Optional[torch.Tensor] = None, gmap: Optional[torch.Tensor] = None, step_noise: Optional[torch.Tensor] = None,
              init: Optional[torch.Tensor] = None, nmask: Optional[torch.Tensor] = None, blend_noise: Optional[torch.Tensor] = None,
              out0: Optional[torch.Tensor] = None, out1: Optional[torch.Tensor] = None, pred_out: Optional[torch.Tensor] = None,
              blend_only: bool = False) -> torch.Tensor:
    """One guided DDIM step and the mask blend that opens the next one in one launch (`ofx_ddim_step`, whose header comment gives the
    chain).  Every tensor is float32 on the device, [..., C] with C % 4 == 0 and the same leading shape, contiguous or a channel slice
    of a wider contiguous tensor (channels 0..3 of the UNet's 12-wide NHWC input, say); gmap is a contiguous per-pixel map of the
    leading shape.  coef: the fields of `ofx_ddim_coef` (DDIM_COEF_FIELDS); a field left out is 0.  blend_only: skip the DDIM part
    (xp = x); eps_c is required otherwise.  out0 defaults to a new contiguous tensor; out0 / out1 may each be x itself.  -> out0."""
    rows, Cn, ldx = _rows_view(x, "x")
    lead = tuple(x.shape[:-1])
    unknown = set(coef) - set(DDIM_COEF_FIELDS)
    if unknown:
        raise RuntimeError(f"coef has unknown fields {sorted(unknown)}")
    if not blend_only and eps_c is None:
        raise RuntimeError("eps_c is required unless blend_only")

    def view(t, name):
        if t is None:
            return 0
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != lead + (Cn,):
            raise RuntimeError(f"{name} must be a CUDA float32 tensor {lead + (Cn,)}")
        return _rows_view(t, name)[2]

    lde = view(eps_c, "eps_c")
    if eps_u is not None and view(eps_u, "eps_u") != lde:
        raise RuntimeError("eps_u must have the row stride of eps_c")
    if gmap is not None:
        gmap = _chk(gmap, "gmap", torch.float32)
        if tuple(gmap.shape) != lead:
            raise RuntimeError(f"gmap must be {lead}, got {tuple(gmap.shape)}")
    if out0 is None:
        out0 = torch.empty(lead + (Cn,), dtype=torch.float32, device=x.device)
    k = _lib.DdimCoef(**{f: float(v) for f, v in coef.items()})
    check(_lib.lib().ofx_ddim_step(_ptr(x), ldx, _ptr(eps_c), _ptr(eps_u), lde, _ptr(guidance), view(guidance, "guidance"), _ptr(gmap),
                                   _ptr(step_noise), view(step_noise, "step_noise"), _ptr(init), view(init, "init"), _ptr(nmask),
                                   view(nmask, "nmask"), _ptr(blend_noise), view(blend_noise, "blend_noise"), _ptr(out0),
                                   view(out0, "out0"), _ptr(out1), view(out1, "out1"), _ptr(pred_out), view(pred_out, "pred_out"),
                                   C.byref(k), 1 if blend_only else 0, rows, Cn, _stream()), "ofx_ddim_step")
    return out0


# --------------------------------------------------------------------------------------
# key-frame detector
# --------------------------------------------------------------------------------------
def detect_edges(frames_bgr: torch.Tensor, ksize: int) -> torch.Tensor:
    """uint8 [B,H,W,3] (cv2 channel order) -> uint8 [B,H,W] dilated Canny edge maps (_detect_edges of the reference)."""
    f = _chk(frames_bgr, "frames_bgr", torch.uint8)
    B, H, W, c3 = f.shape
    if c3 != 3:
        raise RuntimeError("frames_bgr must be [B,H,W,3]")
    L = _lib.lib()
    need = L.ofx_detect_edges_scratch_bytes(B, H, W)
    scratch = torch.empty((need,), dtype=torch.uint8, device=f.device)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=f.device)
    check(L.ofx_detect_edges(_ptr(f), _ptr(out), _ptr(scratch), need, B, H, W, int(ksize), _stream()), "ofx_detect_edges")
    return out


def canny(images: torch.Tensor, low, high) -> torch.Tensor:
    """`cv2.Canny(image, low, high)` (aperture 3, L1 gradient) per image: uint8 [B,H,W] or [B,H,W,3] (any channel order: the
    strongest channel wins per pixel) -> uint8 [B,H,W], 255 or 0.  The thresholds are numbers and are floored (cvFloor), and
    swapped when low > high, as cv::Canny does."""
    f = _chk(images, "images", torch.uint8)
    if f.dim() not in (3, 4) or (f.dim() == 4 and f.shape[3] != 3):
        raise RuntimeError(f"images must be uint8 [B,H,W] or [B,H,W,3], got {tuple(f.shape)}")
    B, H, W = f.shape[:3]
    lo, hi = int(math.floor(low)), int(math.floor(high))
    L = _lib.lib()
    need = L.ofx_canny_u8_scratch_bytes(B, H, W)
    scratch = torch.empty((need,), dtype=torch.uint8, device=f.device)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=f.device)
    check(L.ofx_canny_u8(_ptr(f), 3 if f.dim() == 4 else 1, _ptr(out), _ptr(scratch), need, B, H, W, lo, hi, _stream()), "ofx_canny_u8")
    return out


def abs_diff_sum_u8(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a: uint8 [B,...]; b: same shape or one image [...] shared by the batch -> int64 [B] sums of |a - b|."""
    x = _chk(a, "a", torch.uint8)
    y = _chk(b, "b", torch.uint8)
    B = x.shape[0]
    n = x[0].numel()
    shared = y.dim() == x.dim() - 1
    if (shared and y.numel() != n) or (not shared and tuple(y.shape) != tuple(x.shape)):
        raise RuntimeError("abs_diff_sum_u8: shape mismatch")
    sums = torch.empty((B,), dtype=torch.int64, device=x.device)
    check(_lib.lib().ofx_abs_diff_sum_u8(_ptr(x), n, _ptr(y), 0 if shared else n, _ptr(sums), B, n, _stream()), "ofx_abs_diff_sum_u8")
    return sums
