"""The fp16 form of the fused attention kernel (csrc/attn_flash.hip, flash_attn_f16_kernel) on the device: ofx_attention_prec and
ofx_attention_bnhd_prec with OFX_PREC_F16 and `ops.attention(precision="fp16")` at every case of flash_attn_check.FA_CASES against the
float64 reference of the rounded operands (flash_attn_f16_check.py: bound, emulation, simulated bugs), the exactness tests a bound
cannot replace, OFX_PREC_FP32 through the new entries bit for bit the old entries, and the rejections.  The kernel keeps the fp32
kernel's BK, so the table's 2 BK + 1 cases reuse both of its LDS buffers.  Every test prints its ratios (-s)."""
import ctypes as C_

import pytest
import torch

import flash_attn_check as fc
import flash_attn_f16_check as f16
import sd_ops_check as sc

pytestmark = pytest.mark.gpu
GUARD = fc.FA_GUARD
IDS = [c["name"] for c in fc.FA_CASES]
F16, FP32 = f16.PREC_F16, f16.PREC_FP32


def _L():
    from sd_animation_optical_flow_amd import _lib
    return _lib.lib()


def _p(t):
    return C_.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return None if t is None else t.cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _bstride(bias, Nq, Nk):
    return Nq * Nk if (bias is not None and bias.dim() == 3) else 0


def _raw(q, k, v, bias, scale, precision, entry="prec", expect=0, fill=float("nan")):
    """ofx_attention_prec (or ofx_attention_f32 for entry="f32") called directly with no workspace; `out` starts as `fill` and is
    followed by GUARD sentinel floats.  Returns out [BH, Nq, D] on the CPU."""
    L = _L()
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    qd, kd, vd, bd = q.cuda(), k.cuda(), v.cuda(), _dev(bias)
    obuf = torch.cat([torch.full((q.numel(),), fill), torch.full((GUARD,), 12345.0)]).cuda()
    if entry == "f32":
        st = L.ofx_attention_f32(_p(qd), _p(kd), _p(vd), _p(bd), _bstride(bias, Nq, Nk), _p(obuf), BH, Nq, Nk, D, scale, None, 0, _stream())
    else:
        st = L.ofx_attention_prec(_p(qd), _p(kd), _p(vd), _p(bd), _bstride(bias, Nq, Nk), _p(obuf), BH, Nq, Nk, D, scale, precision, None, 0,
                                  _stream())
    torch.cuda.synchronize()
    assert st == expect, st
    assert bool((obuf[q.numel():] == 12345.0).all()), "written past out"
    return obuf[:q.numel()].view(BH, Nq, D).cpu()


def _check(label, out, ref, bound):
    rep = fc.fa_compare(out, ref, bound)
    print(f"ratio {label} {rep['ratio']:.4g}")                              # printed before it is judged
    assert rep["ratio"] <= 1.0, (label, rep)
    assert rep["nan_missing"] == 0 and rep["nan_extra"] == 0, (label, rep)
    return rep


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2: every case against float64, both entries

@pytest.mark.parametrize("c", fc.FA_CASES, ids=IDS)
def test_flash_attention_f16_against_float64(cuda, c):
    """`ops.attention(precision="fp16")` and ofx_attention_prec called directly: every element inside the bound, NaN exactly where
    the reference has it, nothing written behind `out`; the wrapper gives the direct call's bits."""
    from sd_animation_optical_flow_amd import ops
    q, k, v, bias, ref, bound = f16.fa16_case_data(c)
    out = ops.attention(q.cuda(), k.cuda(), v.cuda(), _dev(bias), scale=c["scale"], precision="fp16").cpu()
    _check(f"ops.attention fp16 {c['name']}", out, ref, bound)
    raw = _raw(q, k, v, bias, fc.fa_scale(c), F16)
    assert torch.equal(_bits(raw), _bits(out)), "ops.attention differs from ofx_attention_prec"


def _heads(BH):
    return {1: (2, 1, 2), 3: (1, 1, 3), 8: (1, 2, 4), 16: (1, 2, 8)}[BH]


@pytest.mark.parametrize("c", fc.FA_CASES, ids=IDS)
def test_flash_attention_bnhd_f16_on_slices_of_one_qkv_buffer(cuda, c):
    """`ops.attention_bnhd(precision="fp16")` on last-axis slices of one fused buffer with NaN columns on both sides: q|k|v of one
    [B, N, 3 W + 8] buffer where Nq == Nk (self-attention), and where they differ q in a buffer of its own and k|v in one
    [B, Nk, 2 W + 8] buffer (cross-attention: an image's rows must be N * ld apart).  `out` is a slice of a wider buffer that keeps its
    sentinel.  Bit for bit the contiguous entry, and inside the bound."""
    from sd_animation_optical_flow_amd import ops
    q, k, v, bias, ref, bound = f16.fa16_case_data(c)
    copies, B, H = _heads(c["BH"])
    if copies == 2:
        q, k, v, ref, bound = (torch.cat([t, t]) for t in (q, k, v, ref, bound))
        if bias is not None and bias.dim() == 3:
            bias = torch.cat([bias, bias])
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    W = H * D
    rows = lambda t: t.view(B, H, t.shape[1], D).permute(0, 2, 1, 3).reshape(B, t.shape[1], W)
    if Nq == Nk:
        fused = torch.full((B, Nq, 3 * W + 8), float("nan"))
        fused[..., 4:4 + W], fused[..., 4 + W:4 + 2 * W], fused[..., 4 + 2 * W:4 + 3 * W] = rows(q), rows(k), rows(v)
        fused = fused.cuda()
        qs, ks, vs = fused[..., 4:4 + W], fused[..., 4 + W:4 + 2 * W], fused[..., 4 + 2 * W:4 + 3 * W]
    else:
        qb, kv = torch.full((B, Nq, W + 12), float("nan")), torch.full((B, Nk, 2 * W + 8), float("nan"))
        qb[..., 8:8 + W], kv[..., 4:4 + W], kv[..., 4 + W:4 + 2 * W] = rows(q), rows(k), rows(v)
        qb, kv = qb.cuda(), kv.cuda()
        qs, ks, vs = qb[..., 8:8 + W], kv[..., 4:4 + W], kv[..., 4 + W:4 + 2 * W]
    ldo = W + 20
    obuf = torch.cat([torch.full((B * Nq * ldo,), 7.0), torch.full((GUARD,), 12345.0)]).cuda()
    wide = obuf[:B * Nq * ldo].view(B, Nq, ldo)
    os_ = wide[..., 4:4 + W]
    got = ops.attention_bnhd(qs, ks, vs, H, bias=_dev(bias), scale=fc.fa_scale(c), out=os_, precision="fp16")
    torch.cuda.synchronize()
    assert got.data_ptr() == os_.data_ptr()
    assert bool((obuf[B * Nq * ldo:] == 12345.0).all()), "written past out"
    assert bool((wide[..., :4] == 7.0).all()) and bool((wide[..., 4 + W:] == 7.0).all()), "written beside the out slice"
    out = os_.cpu().view(B, Nq, H, D).permute(0, 2, 1, 3).reshape(BH, Nq, D)
    assert torch.equal(_bits(out), _bits(_raw(q, k, v, bias, fc.fa_scale(c), F16))), "the strided entry differs from the contiguous one"
    _check(f"attention_bnhd fp16 {c['name']}", out, ref, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: exactness

@pytest.mark.parametrize("D", fc.FLASH_D)
def test_scale_zero_gives_the_mean_of_v_bit_for_bit(cuda, D):
    """scale = 0, no bias, integer V with |v| <= 8, Nk a power of two <= 32: every p is exactly 1 (and exactly 1 in fp16), every
    partial sum an integer, l = Nk: out == mean(v), through both entries."""
    from sd_animation_optical_flow_amd import ops
    for Nk in (1, 2, 4, 8, 16, 32):
        q, k, v, want = f16.fa16_mean_case(D, Nk)
        out = ops.attention(q.cuda(), k.cuda(), v.cuda(), scale=0.0, precision="fp16").cpu()
        assert torch.equal(_bits(out), _bits(want)), (D, Nk, float((out - want).abs().max()))
        BH, Nq, _ = q.shape
        tok = lambda t: t.permute(1, 0, 2).reshape(1, t.shape[1], BH * D).contiguous().cuda()
        o2 = ops.attention_bnhd(tok(q), tok(k), tok(v), BH, scale=0.0, precision="fp16").cpu().view(Nq, BH, D).permute(1, 0, 2)
        assert torch.equal(_bits(o2), _bits(want)), (D, Nk)


@pytest.mark.parametrize("D", fc.FLASH_D)
def test_one_hot_selection_returns_the_selected_row_bit_for_bit(cuda, D):
    """Nq = Nk = 2 BK + 1 (three K / V tiles: both LDS buffers reused), a per-batch-head bias that is 0 at key pi(q) and -inf
    elsewhere: p is exactly 1 at one key and 0 elsewhere, l = 1, so the output EQUALS v.half().float()[pi(q)].  A wrong key order in
    the V fragment, a slip of the transposed read, a stale LDS buffer or a pad column leaking into d < D return another value."""
    from sd_animation_optical_flow_amd import ops
    q, k, v, bias, want = f16.fa16_onehot_case(D)
    assert q.shape[1] == 2 * fc.fa_bk(D) + 1 and fc.fa_geometry(dict(BH=3, Nq=q.shape[1], Nk=k.shape[1], D=D))["nt"] == 3
    out = ops.attention(q.cuda(), k.cuda(), v.cuda(), bias.cuda(), precision="fp16").cpu()
    wrong = (_bits(out) != _bits(want))
    assert not bool(wrong.any()), (D, int(wrong.sum()), wrong.nonzero()[:4].tolist())
    BH, N, _ = q.shape
    tok = lambda t: t.permute(1, 0, 2).reshape(1, N, BH * D).contiguous().cuda()
    o2 = ops.attention_bnhd(tok(q), tok(k), tok(v), BH, bias=bias.cuda(), precision="fp16").cpu().view(N, BH, D).permute(1, 0, 2)
    assert torch.equal(_bits(o2), _bits(want)), D


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: fp32 through the new entries is the old entries, bit for bit

def _three_cases(D):
    want = ("nk77-shared-lead32", "nk3tiles-per-leadBK-grouped", "nk33-nan-query")
    cs = [c for c in fc.FA_CASES if c["D"] == D and c["name"].endswith(want)]
    assert len(cs) == 3
    return cs


@pytest.mark.parametrize("D", fc.FLASH_D)
def test_fp32_through_the_new_entries_is_bit_identical_to_the_old_entries(cuda, D):
    from sd_animation_optical_flow_amd import ops
    L = _L()
    for c in _three_cases(D):
        q, k, v, bias, _, _ = fc.fa_case_data(c)
        scale = fc.fa_scale(c)
        old = _raw(q, k, v, bias, scale, None, entry="f32")
        assert torch.equal(_bits(_raw(q, k, v, bias, scale, FP32)), _bits(old)), c["name"]
        qd, kd, vd, bd = q.cuda(), k.cuda(), v.cuda(), _dev(bias)
        assert torch.equal(_bits(ops.attention(qd, kd, vd, bd, scale=scale, precision="fp32").cpu()), _bits(old)), c["name"]
        assert torch.equal(_bits(ops.attention(qd, kd, vd, bd, scale=scale).cpu()), _bits(old)), c["name"]
        half = _raw(q, k, v, bias, scale, F16)
        assert not torch.equal(_bits(half), _bits(old)), c["name"]                      # the other kernel ran
        # the strided pair: one head per image, rows of D floats
        BH, Nq, _ = q.shape
        Nk = k.shape[1]
        o_old, o_new = torch.full_like(qd, 3.0), torch.full_like(qd, 3.0)
        args = lambda o: (_p(qd), D, _p(kd), D, _p(vd), D, _p(bd), _bstride(bias, Nq, Nk), _p(o), D, BH, 1, Nq, Nk, D, scale)
        assert L.ofx_attention_bnhd_f32(*args(o_old), _stream()) == 0
        assert L.ofx_attention_bnhd_prec(*args(o_new), FP32, _stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(o_new.cpu()), _bits(o_old.cpu())) and torch.equal(_bits(o_old.cpu()), _bits(old)), c["name"]
        assert torch.equal(_bits(ops.attention_bnhd(qd, kd, vd, 1, bias=bd, scale=scale, precision="fp32").cpu()), _bits(old)), c["name"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: rejections leave `out` untouched

def test_unfused_head_size_and_unknown_precisions_are_einval_and_launch_nothing(cuda):
    L = _L()
    g = torch.Generator().manual_seed(5)
    # the VAE's head: D = 512 has no fp16 path (fp32 through the same entry still runs it, given its workspace)
    q = torch.randn((1, 8, 512), generator=g)
    out = _raw(q, q, q, None, 512 ** -0.5, F16, expect=sc.EINVAL, fill=777.0)
    assert bool((out == 777.0).all())
    qd = q.cuda()
    o = torch.full((1, 8, 512), 777.0).cuda()
    assert L.ofx_attention_bnhd_prec(_p(qd), 512, _p(qd), 512, _p(qd), 512, None, 0, _p(o), 512, 1, 1, 8, 8, 512, 1.0, F16, _stream()) == sc.EINVAL
    torch.cuda.synchronize()
    assert bool((o == 777.0).all())
    # any precision other than 0 / 5, at a fused head size
    q = torch.randn((2, 33, 40), generator=g)
    qd = q.cuda()
    for prec in (1, 2, 3, 4, 6, -1, 50):
        out = _raw(q, q, q, None, 40 ** -0.5, prec, expect=sc.EINVAL, fill=777.0)
        assert bool((out == 777.0).all()), prec
        o = torch.full((2, 33, 40), 777.0).cuda()
        assert L.ofx_attention_bnhd_prec(_p(qd), 40, _p(qd), 40, _p(qd), 40, None, 0, _p(o), 40, 2, 1, 33, 33, 40, 1.0, prec, _stream()) == sc.EINVAL
        torch.cuda.synchronize()
        assert bool((o == 777.0).all()), prec
    # the existing argument checks apply unchanged to the fp16 mode: a row stride below H * D, a misaligned pointer
    o = torch.full((2, 33, 40), 777.0).cuda()
    assert L.ofx_attention_bnhd_prec(_p(qd), 36, _p(qd), 40, _p(qd), 40, None, 0, _p(o), 40, 2, 1, 33, 33, 40, 1.0, F16, _stream()) == sc.EINVAL
    assert L.ofx_attention_bnhd_prec(C_.c_void_p(qd.data_ptr() + 4), 40, _p(qd), 40, _p(qd), 40, None, 0, _p(o), 40, 2, 1, 32, 33, 40, 1.0, F16,
                                     _stream()) == sc.EALIGN
    assert L.ofx_attention_prec(C_.c_void_p(qd.data_ptr() + 4), _p(qd), _p(qd), None, 0, _p(o), 2, 32, 33, 40, 1.0, F16, None, 0, _stream()) == sc.EALIGN
    torch.cuda.synchronize()
    assert bool((o == 777.0).all())
