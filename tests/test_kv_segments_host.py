"""CPU: the host side of the in-place reference K/V -- `transformer.plan_kv_route`, the ValueErrors of `kv_dtype=` and of
`ops.attention_bnhd_segments` before any device call, and the new symbol and struct in include/ofx.h and `_lib`.  No GPU is used."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16 = torch.float32, torch.float16


def test_plan_kv_route_segments_and_every_fallback():
    from sd_animation_optical_flow_amd import transformer as T
    plan = T.plan_kv_route
    two = [False, False]
    # the fused route: every entry in place, either dtype
    assert plan("all", [F32] * 4, two, 2, 40) == "segments"
    assert plan("all", [F16] * 4, two, 2, 40) == "segments"
    assert plan("all", ["float16", "torch.float16"], [False], 2, 160) == "segments"          # dtype names count as the dtypes
    # "positive": one launch with a float32 history (image 0's own k / v is a segment), two with a half one
    assert plan("positive", [F32] * 4, two, 2, 80) == "segments"
    assert plan("positive", [F16] * 4, two, 2, 80) == "segments+own"
    # the concatenation path remains for ...
    assert plan("all", [F32] * 4, [False, True], 2, 40) == "concat"                           # an entry in the [(b h), n, d] layout
    assert plan("all", [F32] * 4, two, 2, 32) == "concat" and plan("all", [F16] * 4, two, 2, 192) == "concat"     # unfused head sizes
    assert plan("all", [F32] * 4, two, 2, 40, torch_glue=True) == "concat"                    # OFX_ST_TORCH_GLUE=1
    assert plan("all", [F32] * 4, two, 2, 40, force_concat=True) == "concat"                  # OFX_ST_KV_CONCAT=1
    assert plan("all", [F32, F32, F16, F16], two, 2, 40) == "concat"                          # mixed dtypes
    assert plan("all", [F32, F16], [False], 2, 40) == "concat"                                # k and v of one entry differ
    assert plan("all", [torch.float64] * 2, [False], 2, 40) == "concat" and plan("all", [torch.bfloat16] * 2, [False], 2, 40) == "concat"
    # ... and for tables beyond 8 segments per image or 64 entries per launch
    assert plan("all", [F32] * 16, [False] * 8, 8, 40) == "segments" and plan("all", [F32] * 18, [False] * 9, 2, 40) == "concat"
    assert plan("all", [F32] * 16, [False] * 8, 9, 40) == "concat"                            # 72 entries
    assert plan("positive", [F32] * 14, [False] * 7, 10, 40) == "segments"                    # 1 + 9 * 7 = 64
    assert plan("positive", [F32] * 16, [False] * 8, 9, 40) == "concat"                       # 1 + 8 * 8 = 65
    assert plan("positive", [F16] * 16, [False] * 8, 9, 40) == "segments+own"                 # 8 * 8 = 64 in the second launch
    assert (T.KV_MAX_SEGMENTS, T.KV_MAX_ENTRIES) == (8, 64)
    with pytest.raises(ValueError, match="mode"):
        plan("some", [F32] * 2, [False], 2, 40)


def test_kv_dtype_is_checked_at_construction_before_anything_else():
    from sd_animation_optical_flow_amd import controlnet, ops, render, transformer, unet
    assert ops.check_kv_dtype("fp32") == "fp32" and ops.check_kv_dtype("fp16") == "fp16"
    assert ops.KV_DTYPES == {"fp32": torch.float32, "fp16": torch.float16}
    for bad in ("bf16", "float16", None, 16, torch.float16):
        with pytest.raises(ValueError, match="kv_dtype"):
            ops.check_kv_dtype(bad)
        # no checkpoint is looked at and no device asked for: an empty state dict and a device that does not exist
        with pytest.raises(ValueError, match="kv_dtype"):
            transformer.SpatialTransformer({}, 2, 40, device="cuda:99", kv_dtype=bad)
        with pytest.raises(ValueError, match="kv_dtype"):
            unet.UNetModel({}, device="cuda:99", kv_dtype=bad)
        with pytest.raises(ValueError, match="kv_dtype"):
            controlnet.ControlNet({}, device="cuda:99", kv_dtype=bad)
        with pytest.raises(ValueError, match="kv_dtype"):
            render.SdRenderer(None, None, None, (None, None), kv_dtype=bad)
        if bad is not None:                                       # run_exp(kv_dtype=None) is the renderer's own kv_dtype
            with pytest.raises(ValueError, match="kv_dtype"):
                render.run_exp(None, None, render.SdRenderer(None, None, None, (None, None)), kv_dtype=bad)
    r = render.SdRenderer(None, None, None, (None, None))
    assert r.kv_dtype == "fp32" and render.SdRenderer(None, None, None, (None, None), kv_dtype="fp16").kv_dtype == "fp16"


def test_as_kv_dtype_rounds_once_and_copies_nothing_it_need_not():
    from sd_animation_optical_flow_amd import render
    k = torch.tensor([[[1.0, 65504.0, 65520.0, -1.0e5, 3.0e-6, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]]])
    hist = [(k, -k)]
    assert render.as_kv_dtype(hist, "fp32") is hist                                          # already there: the list itself
    h16 = render.as_kv_dtype(hist, "fp16")
    assert h16[0][0].dtype == torch.float16 and torch.equal(h16[0][0], k.half()) and torch.equal(h16[0][1], (-k).half())
    got = h16[0][0].float().flatten().tolist()
    assert got[1] == 65504.0 and got[2] == float("inf") and got[3] == float("-inf")          # beyond +-65504: infinities, as under autocast
    assert got[5] == 1.0 and got[6] == 1.0 + 2.0 ** -9 and 0.0 < got[4] < 6.2e-5              # ties to even; a subnormal is kept
    assert render.as_kv_dtype(h16, "fp16") is h16
    assert render.as_kv_dtype(h16, "fp32")[0][0].dtype == torch.float32


def test_attention_bnhd_segments_raises_before_any_device_call():
    """CPU tensors throughout: a check that came after a device call could not raise these."""
    from sd_animation_optical_flow_amd import ops
    q = torch.zeros((2, 5, 80))
    seg = lambda n, dt=F32: (torch.zeros((n, 80), dtype=dt), torch.zeros((n, 80), dtype=dt))
    with pytest.raises(ValueError, match="precision"):
        ops.attention_bnhd_segments(q, [seg(3)], 2, precision="bf16")
    with pytest.raises(ValueError, match="all float32 or all float16"):
        ops.attention_bnhd_segments(q, [seg(3), seg(4, F16)], 2)                              # mixed dtypes across segments
    with pytest.raises(ValueError, match="all float32 or all float16"):
        ops.attention_bnhd_segments(q, [(torch.zeros((3, 80)), torch.zeros((3, 80), dtype=F16))], 2)      # k and v of one segment
    with pytest.raises(ValueError, match="all float32 or all float16"):
        ops.attention_bnhd_segments(q, [seg(3, torch.float64)], 2)
    with pytest.raises(ValueError, match="per-image lists"):
        ops.attention_bnhd_segments(q, [[seg(3)], [seg(3)], [seg(3)]], 2)                     # three lists for two images
    with pytest.raises(ValueError, match="per-image lists"):
        ops.attention_bnhd_segments(q, [[seg(3)]], 2)
    with pytest.raises(ValueError, match="non-empty"):
        ops.attention_bnhd_segments(q, [], 2)
    with pytest.raises(ValueError, match="non-empty"):
        ops.attention_bnhd_segments(q, [[seg(3)], []], 2)
    with pytest.raises(ValueError, match="at most 8 segments per image"):
        ops.attention_bnhd_segments(q, [seg(1)] * 9, 2)
    with pytest.raises(ValueError, match="at most 8 segments per image"):
        ops.attention_bnhd_segments(torch.zeros((9, 5, 80)), [seg(1)] * 8, 2)                 # shared by 9 images: 72 entries
    with pytest.raises(ValueError, match="one token count"):
        ops.attention_bnhd_segments(q, [[seg(3), seg(2)], [seg(4)]], 2)                       # per-image totals 5 and 4
    with pytest.raises(ValueError, match=r"must be \[n, 80\]"):
        ops.attention_bnhd_segments(q, [(torch.zeros((3, 40)), torch.zeros((3, 40)))], 2)


def test_the_new_symbol_and_struct_are_declared_and_bound():
    from sd_animation_optical_flow_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofx.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", header)
    m = re.search(r"typedef struct ofx_kv_segment \{(.*?)\} ofx_kv_segment;", flat)
    assert m, "ofx_kv_segment is not declared"
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["const void* k", "const void* v", "int n", "int ldk", "int ldv"]
    assert [(n, t) for n, t in _lib.KvSegment._fields_] == [("k", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int), ("ldk", C.c_int), ("ldv", C.c_int)]
    assert C.sizeof(_lib.KvSegment) == 32
    for name, value in (("OFX_KV_F32", 0), ("OFX_KV_F16", 1), ("OFX_KV_MAX_SEGMENTS", 8), ("OFX_KV_MAX_ENTRIES", 64)):
        assert f"#define {name} {value} " in flat + " ", name
    assert _lib.KV_TYPES == {"fp32": 0, "fp16": 1} and (_lib.KV_MAX_SEGMENTS, _lib.KV_MAX_ENTRIES) == (8, 64)
    proto = re.search(r"\bint ofx_attention_bnhd_segs ?\(([^;]*?)\) ?;", flat)
    assert proto, "ofx_attention_bnhd_segs is not declared"
    args = [a.strip() for a in proto.group(1).split(",")]
    assert args == ["const float* q", "int ldq", "const ofx_kv_segment* segs", "const int* seg_counts", "int kv_type", "const float* bias",
                    "long bias_bstride", "float* out", "int ldo", "int B", "int H", "int Nq", "int D", "float scale", "int precision", "void* stream"]
    res, table = _lib.SIGNATURES["ofx_attention_bnhd_segs"]
    kind = {C.c_void_p: "p", C.c_int: "i", C.c_long: "l", C.c_float: "f", C.POINTER(_lib.KvSegment): "p", C.POINTER(C.c_int): "p"}
    want = ["p" if "*" in a else {"int": "i", "long": "l", "float": "f"}[a.split(" ")[0]] for a in args]
    assert res is C.c_int and [kind[t] for t in table] == want
    lib = _lib.lib()
    assert hasattr(lib, "ofx_attention_bnhd_segs")
    # argument validation precedes every HIP call: testable without a device
    buf = (C.c_float * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    tab = (_lib.KvSegment * 2)()
    for t in tab:
        t.k, t.v, t.n, t.ldk, t.ldv = p, p, 3, 80, 80
    one = (C.c_int * 2)(1, 1)
    call = lambda D=40, kv_type=0, precision=0, counts=one: lib.ofx_attention_bnhd_segs(C.c_void_p(p), 80, tab, counts, kv_type, None, 0, C.c_void_p(p), 80,
                                                                                      2, 2, 4, D, 1.0, precision, None)
    assert call(D=48) == -1 and call(kv_type=2) == -1 and call(precision=1) == -1 and call(counts=(C.c_int * 2)(9, 1)) == -1
    tab[1].n = 4
    assert call() == -1                                                                       # per-image totals differ
    tab[1].n, tab[0].n = 3, 0
    assert call() == -1                                                                       # a non-positive token count
    tab[0].n, tab[0].k = 3, p + 4
    assert call() == -1                                                                       # a misaligned pointer
    tab[0].k, tab[0].ldv = p, 82
    assert call() == -1                                                                       # a stride that is no multiple of 4
    assert lib.ofx_attention_bnhd_segs(None, 80, tab, one, 0, None, 0, None, 80, 2, 2, 4, 40, 1.0, 0, None) == -1
