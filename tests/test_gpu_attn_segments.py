"""`ops.attention_bnhd_segments` (ofx_attention_bnhd_segs, csrc/attn_flash_segs.hip) on the device: K and V read in place through a
per-image segment table, float32 or float16.

The kernel walks tiles of BK logical keys (`fa_bk`: 64 at D = 40, 32 otherwise) exactly as the strided kernel walks the concatenated
tensor, so every comparison here is BITWISE against `ops.attention_bnhd` on the float32 concatenation, for both arithmetic modes and
every fused head size.  The shapes are the smallest that reach every way the table can go wrong: the degenerate one-segment table, a
seam inside tile 0, a seam on a tile boundary, a ragged tail, a segment shorter than a tile between two seams, one query, two query
tiles with a ragged second, two images with different seams and pointers, segments that are last-axis slices of wider buffers (the
columns beside them hold NaN), and a shared bias whose columns all differ with one fully masked row.  One case per head size is
also held against the float64 reference of flash_attn_check under that module's bound.
"""
import pytest
import torch

import flash_attn_check as fc

pytestmark = pytest.mark.gpu
HEADS = 2


def _bits(t):
    return t.contiguous().view(torch.int32)


def _seed(*key):
    s = 12345
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _cases(D):
    bk = fc.fa_bk(D)
    s3 = [1, bk - 1, bk + 2]
    return {
        "s1-degenerate": dict(counts=[[bk + 6]], Nq=33),
        "s3-seams": dict(counts=[s3], Nq=33),
        "s4-short-middle": dict(counts=[[bk + 5, 3, bk, 7]], Nq=33),
        "nq1": dict(counts=[s3], Nq=1),
        "nq129": dict(counts=[s3], Nq=129),
        "b2-different-seams": dict(counts=[s3, [bk + 5, 3, bk - 6]], Nq=33),
        "shared-list": dict(counts=[s3], Nq=33, B=2, shared=True),
        "bias-masked-row": dict(counts=[s3, [bk + 5, 3, bk - 6]], Nq=33, bias=True),
    }


CASE_NAMES = list(_cases(64))


def _build(D, case, name):
    """q [B,Nq,W] and per image the (k, v) float32 segments on the CPU; every second segment is a last-axis slice (at column 4 / 8)
    of a wider buffer whose other columns are NaN, k and v with different row strides."""
    g = _seed(D, name)
    W = HEADS * D
    counts = case["counts"]
    B = case.get("B", len(counts))
    q = torch.randn((B, case["Nq"], W), generator=g)
    lists = []
    for b, cnt in enumerate(counts):
        segs = []
        for i, n in enumerate(cnt):
            k, v = torch.randn((n, W), generator=g), torch.randn((n, W), generator=g) * 1.5 + 0.25
            segs.append((k, v, (i + b) % 2 == 1))
        lists.append(segs)
    Nk = sum(counts[0])
    bias = None
    if case.get("bias"):
        bias = torch.randn((case["Nq"], Nk), generator=g) * 2.0 + torch.arange(Nk).float() * 0.01      # every column differs
        bias[5] = float("-inf")                                                                          # a fully masked row: NaN
    return q, lists, bias


def _place(t, sliced, off):
    """A CPU [n, W] tensor on the device: dense, or columns off .. off+W of a buffer 12 wider filled with NaN."""
    if not sliced:
        return t.cuda()
    wide = torch.full((t.shape[0], t.shape[1] + 12), float("nan"), dtype=t.dtype)
    wide[:, off:off + t.shape[1]] = t
    return wide.cuda()[:, off:off + t.shape[1]]


def _device_segments(lists, dtype=torch.float32):
    return [[(_place(k.to(dtype), sl, 4), _place(v.to(dtype), sl, 8)) for k, v, sl in segs] for segs in lists]


def _concat(lists, B):
    per = [(torch.cat([k for k, _, _ in segs]), torch.cat([v for _, v, _ in segs])) for segs in lists]
    if len(per) == 1 and B > 1:
        per = per * B
    return torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("D", fc.FLASH_D)
def test_segments_are_bitwise_the_concatenation(cuda, D, name, precision):
    from sd_animation_optical_flow_amd import ops
    case = _cases(D)[name]
    q, lists, bias = _build(D, case, name)
    B = q.shape[0]
    K, V = _concat(lists, B)
    assert K.shape[0] == B and len({sum(c) for c in case["counts"]}) == 1
    qd, bd = q.cuda(), None if bias is None else bias.cuda()
    want = ops.attention_bnhd(qd, K.cuda(), V.cuda(), HEADS, bias=bd, precision=precision)
    segs = _device_segments(lists)
    got = ops.attention_bnhd_segments(qd, segs[0] if case.get("shared") else segs, HEADS, bias=bd, precision=precision)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want)), f"D {D} {name} {precision}: segments differ from the concatenation"
    nan_rows = torch.isnan(got).all(-1)
    if bias is not None:
        assert bool(nan_rows[:, 5].all()) and int(nan_rows.sum()) == B, "the fully masked row, and only it, is NaN"
    else:
        assert not bool(torch.isnan(got).any()), "a NaN beside a sliced segment was read"
    # into a slice of a wider buffer: the columns beside it keep their sentinel
    wide = torch.full((B, q.shape[1], HEADS * D + 8), 7.0, device="cuda")
    ops.attention_bnhd_segments(qd, segs[0] if case.get("shared") else segs, HEADS, bias=bd, out=wide[..., 4:4 + HEADS * D], precision=precision)
    assert torch.equal(_bits(wide[..., 4:4 + HEADS * D]), _bits(want)) and bool((wide[..., :4] == 7.0).all()) and bool((wide[..., -4:] == 7.0).all())


@pytest.mark.parametrize("D", fc.FLASH_D)
def test_segments_against_float64(cuda, D):
    """The two-image case with the shared bias, in float32 arithmetic, inside flash_attn_check's bound for this kernel; NaN exactly
    where the float64 reference has it."""
    from sd_animation_optical_flow_amd import ops
    name = "bias-masked-row"
    case = _cases(D)[name]
    q, lists, bias = _build(D, case, name)
    B, Nq, W = q.shape
    K, V = _concat(lists, B)
    heads_first = lambda t: t.view(B, t.shape[1], HEADS, D).permute(0, 2, 1, 3).reshape(B * HEADS, t.shape[1], D)
    ref, bound = fc.fa_reference(heads_first(q), heads_first(K), heads_first(V), bias, float(D) ** -0.5)
    got = ops.attention_bnhd_segments(q.cuda(), _device_segments(lists), HEADS, bias=bias.cuda()).cpu()
    rep = fc.fa_compare(heads_first(got), ref, bound)
    print(f"ratio segments-f64 d{D} {rep['ratio']:.4g}")
    assert rep["ok"], rep


def _half_data(D, B=2):
    """Float32 K / V for two images with seams, carrying magnitudes beyond 65504 (infinite as halves) and values that are subnormal
    as halves; the large K element sits in image 1, head 1 only (its scores are infinite there), the large V element and the
    subnormals are everywhere else too."""
    name = "b2-different-seams"
    case = _cases(D)[name]
    q, lists, _ = _build(D, case, "half-" + name)
    out = []
    for b, segs in enumerate(lists):
        new = []
        for i, (k, v, sl) in enumerate(segs):
            k, v = k.clone(), v.clone()
            k[0, 3] = 3.0e-6                  # subnormal as a half (below 2^-14), kept by the matrix core
            v[0, 5] = -4.0e-7
            k[-1, D + 1] = 5.9e-8             # the smallest half subnormal's neighbourhood
            if i == 1:
                v[0, 2] = 1.0e5               # beyond 65504: infinity as a half
                if b == 1:
                    k[0, D + 7] = -7.0e4
            new.append((k, v, sl))
        out.append(new)
    return q, out


@pytest.mark.parametrize("D", fc.FLASH_D)
def test_half_segments_feed_the_fp16_kernel_without_a_second_rounding(cuda, D):
    """precision="fp16": segments of k.half() give bitwise what `attention_bnhd(precision="fp16")` gives on the float32 originals --
    the rounding happens once either way."""
    from sd_animation_optical_flow_amd import ops
    q, lists = _half_data(D)
    K, V = _concat(lists, 2)
    assert float(K.abs().max()) > 65504 and float(V.abs().max()) > 65504 and float(K.abs()[K != 0].min()) < 6.0e-8 * 1.01
    want = ops.attention_bnhd(q.cuda(), K.cuda(), V.cuda(), HEADS, precision="fp16")
    got = ops.attention_bnhd_segments(q.cuda(), _device_segments(lists, torch.float16), HEADS, precision="fp16")
    assert torch.equal(_bits(got), _bits(want))
    assert bool(torch.isfinite(got[0, :, D:]).all()) and not bool(torch.isfinite(got[0, :, 2]).any())   # the overflowed V column alone


@pytest.mark.parametrize("D", fc.FLASH_D)
def test_half_segments_are_widened_exactly_in_the_fp32_kernel(cuda, D):
    """precision="fp32": segments of k.half() give bitwise `attention_bnhd` on k.half().float()."""
    from sd_animation_optical_flow_amd import ops
    q, lists = _half_data(D)
    K, V = _concat(lists, 2)
    want = ops.attention_bnhd(q.cuda(), K.half().float().cuda(), V.half().float().cuda(), HEADS)
    got = ops.attention_bnhd_segments(q.cuda(), _device_segments(lists, torch.float16), HEADS)
    assert torch.equal(_bits(got), _bits(want))
    assert bool((K.half().float() != K).any())


def test_the_c_entry_rejects_bad_tables_before_any_launch(cuda):
    """OFX_EINVAL for an unsupported D, too many segments or entries, a non-positive token count, per-image totals that differ, a
    misaligned pointer or stride and an unknown element type -- with valid device pointers, so nothing but the check refuses."""
    import ctypes as C
    from sd_animation_optical_flow_amd import _lib
    L = _lib.lib()
    D, W = 40, 80
    q = torch.zeros((2, 4, W), device="cuda")
    out = torch.full((2, 4, W), 5.0, device="cuda")
    kv = torch.zeros((64, W + 4), device="cuda")
    kh = torch.zeros((64, W + 4), dtype=torch.float16, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(segs, counts, kv_type=0, d=D, B=2):
        tab = (_lib.KvSegment * len(segs))()
        for i, (kp, vp, n, ldk, ldv) in enumerate(segs):
            tab[i].k, tab[i].v, tab[i].n, tab[i].ldk, tab[i].ldv = kp, vp, n, ldk, ldv
        return L.ofx_attention_bnhd_segs(p(q), W, tab, (C.c_int * len(counts))(*counts), kv_type, None, 0, p(out), W, B, 2, 4, d, 1.0, 0, None)

    a, ld = kv.data_ptr(), W + 4
    ok = (a, a, 3, ld, ld)
    assert call([ok, ok], [1, 1]) == 0                                                    # the table itself is fine
    torch.cuda.synchronize()
    out.fill_(5.0)
    bad = [
        ("D", dict(segs=[ok, ok], counts=[1, 1], d=48)),
        ("segments per image", dict(segs=[(a, a, 1, ld, ld)] * 9 + [(a, a, 9, ld, ld)], counts=[9, 1])),
        ("entries", dict(segs=[(a, a, 1, ld, ld)] * 66, counts=[8] * 8 + [2], B=9)),
        ("n = 0", dict(segs=[(a, a, 0, ld, ld), ok], counts=[1, 1])),
        ("totals", dict(segs=[ok, (a, a, 4, ld, ld)], counts=[1, 1])),
        ("pointer", dict(segs=[(a + 4, a, 3, ld, ld), ok], counts=[1, 1])),
        ("half pointer", dict(segs=[(kh.data_ptr() + 4, kh.data_ptr(), 3, ld, ld), (kh.data_ptr(),) * 2 + (3, ld, ld)], counts=[1, 1], kv_type=1)),
        ("stride", dict(segs=[(a, a, 3, ld + 2, ld), ok], counts=[1, 1])),
        ("stride < H * D", dict(segs=[(a, a, 3, W - 4, ld), ok], counts=[1, 1])),
        ("element type", dict(segs=[ok, ok], counts=[1, 1], kv_type=2)),
        ("count 0", dict(segs=[ok, ok], counts=[0, 2])),
    ]
    for label, kw in bad:
        assert call(**kw) == -1, label
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()), "a refused call launched"
