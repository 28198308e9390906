"""-m gpu: `SpatialTransformer` on the HIP kernels -- ofx_layernorm and ofx_geglu against float64 within derived bounds, the
head-strided attention entry bit for bit against `ops.attention` on permuted copies, and the module against the vectors of the real
reference module and against the float64 restatement (tests/transformer_check.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flash_attn_check as FC    # noqa: E402
import sd_ops_check as SC        # noqa: E402
import transformer_check as TC   # noqa: E402

TAGS = ("c0", "c1")


def gold_path(tag):
    return os.path.join(HERE, "golden", f"spatial_transformer_ref_{tag}.npz")


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 3) * int(v) for i, v in enumerate(key)) % (2 ** 31))


def _affine(Cn, g):
    """gamma of both signs around +-1, beta of both signs."""
    gamma = torch.randn((Cn,), generator=g) * 0.5 + torch.where(torch.arange(Cn) % 2 == 0, 1.0, -1.0)
    return gamma, torch.randn((Cn,), generator=g)


# ------------------------------------------------------------------------------------------------------------- LayerNorm
def _check_ln(out, x, gamma, beta, label, eps=TC.LN_EPS_DEFAULT):
    ref, bound = TC.ln_reference(x, gamma, beta, eps)
    ratio = SC._worst((out.double().cpu() - ref).abs(), bound)
    print(f"layernorm {label}: max |err| {float((out.double().cpu() - ref).abs().max()):.3e}, worst err / bound {ratio:.4f}")
    assert ratio <= 1.0, (label, ratio)
    return ref


LN_SHAPES = [(1, 4), (3, 40), (65, 320), (130, 1280), (5, 260), (2, 4096)]


@pytest.mark.parametrize("rows,Cn", LN_SHAPES, ids=lambda v: str(v))
def test_layernorm_against_float64(cuda, rows, Cn):
    """Every instantiation (1, 2, 3, 5, 8, 16 float4 per lane; 260 and 40 leave lanes idle), more rows than one block of 4 waves
    takes, gamma and beta of both signs."""
    from sd_animation_optical_flow_amd import ops
    g = _gen(rows, Cn)
    x = torch.randn((rows, Cn), generator=g) * 2.0 + 0.5
    gamma, beta = _affine(Cn, g)
    out = ops.layernorm(x.cuda(), gamma.cuda(), beta.cuda())
    assert tuple(out.shape) == (rows, Cn) and out.is_contiguous()
    _check_ln(out, x, gamma, beta, f"{rows}x{Cn}")
    # leading dimensions flatten to rows; no affine parameters at all
    x3 = x.reshape(1, rows, Cn) if rows % 5 else x.reshape(5, rows // 5, Cn)
    _check_ln(ops.layernorm(x3.cuda(), None, None).reshape(rows, Cn), x, None, None, f"{rows}x{Cn}, no affine")


def test_layernorm_strided_rows_leave_the_rest_untouched(cuda):
    """ld > C on both sides (last-axis slices of wider tensors): the columns outside the slice and the rows behind the last one
    keep their content."""
    from sd_animation_optical_flow_amd import ops
    rows, Cn = 9, 320
    g = _gen(rows, Cn, 1)
    gamma, beta = _affine(Cn, g)
    wide_x = torch.randn((rows, Cn + 24), generator=g)
    wide_o = torch.full((rows + 3, Cn + 12), 7.0)
    xd, od = wide_x.cuda(), wide_o.cuda()
    out = ops.layernorm(xd[:, 8:8 + Cn], gamma.cuda(), beta.cuda(), out=od[:rows, 4:4 + Cn])
    assert out.data_ptr() == od.data_ptr() + 16
    _check_ln(od[:rows, 4:4 + Cn], wide_x[:, 8:8 + Cn], gamma, beta, "strided")
    oc = od.cpu()
    assert bool((oc[:, :4] == 7.0).all()) and bool((oc[:, 4 + Cn:] == 7.0).all()) and bool((oc[rows:] == 7.0).all())
    assert torch.equal(xd.cpu(), wide_x)


def test_layernorm_in_place(cuda):
    from sd_animation_optical_flow_amd import ops
    rows, Cn = 37, 640
    g = _gen(rows, Cn, 2)
    x = torch.randn((2, rows, Cn), generator=g) * 3.0 - 1.0
    gamma, beta = _affine(Cn, g)
    xd = x.cuda()
    out = ops.layernorm(xd, gamma.cuda(), beta.cuda(), out=xd)
    assert out.data_ptr() == xd.data_ptr()
    _check_ln(xd.reshape(-1, Cn), x.reshape(-1, Cn), gamma, beta, "in place")


def test_layernorm_large_mean_and_constant_rows(cuda):
    """Rows of mean 1e3 and unit spread: a variance formed as E[x^2] - mean^2 loses all of it (~C u 1e6 against var = 1) and
    lands far outside the bound.  A constant row: rstd = eps^-1/2 and the output is beta, up to the bound's mean term."""
    from sd_animation_optical_flow_amd import ops
    rows, Cn = 6, 1280
    g = _gen(rows, Cn, 3)
    gamma, beta = _affine(Cn, g)
    x = torch.randn((rows, Cn), generator=g) + 1000.0
    ref = _check_ln(ops.layernorm(x.cuda(), gamma.cuda(), beta.cuda()), x, gamma, beta, "mean 1e3")
    assert 2.0 < float(ref.abs().max()) < 12.0                                    # the rows are normalised, not flattened
    # what the one-pass variance would give, in float32 on the host: outside the bound (the test can tell the two apart)
    xf = x.float()
    var1 = (xf * xf).mean(1, keepdim=True) - xf.mean(1, keepdim=True) ** 2
    one_pass = (xf - xf.mean(1, keepdim=True)) / torch.sqrt(var1.clamp_min(0) + 1e-5) * gamma + beta
    _, bound = TC.ln_reference(x, gamma, beta)
    assert SC._worst((one_pass.double() - ref).abs(), bound) > 1.0
    for value in (0.75, -3.1, 1000.0, 0.0):
        xc = torch.full((3, Cn), value)
        out = ops.layernorm(xc.cuda(), gamma.cuda(), beta.cuda())
        _check_ln(out, xc, gamma, beta, f"constant {value}")
    assert torch.equal(ops.layernorm(torch.zeros((2, 8), device="cuda"), None, beta[:8].cuda()).cpu(), beta[:8].expand(2, 8))


def test_layernorm_and_geglu_reject_bad_arguments_without_launching(cuda):
    from sd_animation_optical_flow_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros((4, 16), device="cuda")
    o = torch.full((4, 16), 5.0, device="cuda")
    s = ops._stream()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert L.ofx_layernorm(p(x), 16, None, None, p(o), 16, 1, 16, 1e-5, s) == 0
    torch.cuda.synchronize()
    assert bool((o[0] == 0).all()) and bool((o[1:] == 5.0).all())
    o.fill_(5.0)
    assert L.ofx_layernorm(None, 16, None, None, p(o), 16, 4, 16, 1e-5, s) == SC.EINVAL
    assert L.ofx_layernorm(p(x), 16, None, None, p(o), 16, 0, 16, 1e-5, s) == SC.EINVAL              # no rows
    assert L.ofx_layernorm(p(x), 12, None, None, p(o), 16, 4, 16, 1e-5, s) == SC.EINVAL              # ldx < C
    assert L.ofx_layernorm(p(x), 4100, None, None, p(o), 4100, 1, 4100, 1e-5, s) == SC.EINVAL        # C > 4096
    assert L.ofx_layernorm(p(x), 16, None, None, p(o), 16, 4, 14, 1e-5, s) == SC.EALIGN              # C % 4
    assert L.ofx_layernorm(p(x), 18, None, None, p(o), 16, 1, 16, 1e-5, s) == SC.EALIGN              # ld % 4
    assert L.ofx_layernorm(p(x, 4), 16, None, None, p(o), 16, 1, 8, 1e-5, s) == SC.EALIGN            # x not 16-byte aligned
    assert L.ofx_layernorm(p(x), 16, p(x, 8), None, p(o), 16, 1, 8, 1e-5, s) == SC.EALIGN            # gamma not aligned
    assert L.ofx_geglu(None, 16, p(o), 16, 4, 8, s) == SC.EINVAL
    assert L.ofx_geglu(p(x), 12, p(o), 16, 4, 8, s) == SC.EINVAL                                     # lda < 2 * inner
    assert L.ofx_geglu(p(x), 16, p(o), 4, 4, 8, s) == SC.EINVAL                                      # ldo < inner
    assert L.ofx_geglu(p(x), 16, p(o), 16, 4, 6, s) == SC.EALIGN                                     # inner % 4
    assert L.ofx_geglu(p(x), 18, p(o), 16, 1, 8, s) == SC.EALIGN                                     # lda % 4
    assert L.ofx_geglu(p(x), 16, p(o, 4), 16, 1, 8, s) == SC.EALIGN                                  # out not aligned
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())
    with pytest.raises(RuntimeError):
        ops.layernorm(x.cpu(), None, None)
    with pytest.raises(RuntimeError):
        ops.layernorm(x.t(), None, None)                                                             # last axis not dense
    with pytest.raises(RuntimeError):
        ops.layernorm(x, torch.zeros((8,), device="cuda"), None)                                     # gamma of the wrong length
    with pytest.raises(RuntimeError):
        ops.geglu(torch.zeros((4, 15), device="cuda"))


# ------------------------------------------------------------------------------------------------------------- GEGLU
@pytest.mark.parametrize("rows,inner,pad", [(1, 4, 0), (5, 1280, 0), (33, 2560, 8)], ids=["1x4", "5x1280", "33x2560-wide"])
def test_geglu_against_float64(cuda, rows, inner, pad):
    """Gates: random, +-20 (the negative one must give +-0, not NaN), +-0.0, around +-1e-4, and -6..-3 where 1 + erf cancels.  The
    wide case has lda > 2 * inner and ldo > inner: the pad columns and the rows behind keep their content."""
    from sd_animation_optical_flow_amd import ops
    g = _gen(rows, inner, 5)
    a = torch.full((rows, 2 * inner + pad), 3.0)
    a[:, :inner] = torch.randn((rows, inner), generator=g) * 2.0
    a[:, inner:2 * inner] = TC.geglu_gates(rows * inner, g).reshape(rows, inner)
    ref, bound = TC.geglu_reference(a, inner)
    ad = a.cuda()
    if pad:
        wide = torch.full((rows + 2, inner + pad), 7.0, device="cuda")
        out = ops.geglu(ad[:, :2 * inner], out=wide[:rows, :inner])
        wc = wide.cpu()
        assert bool((wc[:, inner:] == 7.0).all()) and bool((wc[rows:] == 7.0).all())
    else:
        out = ops.geglu(ad)
        assert out.is_contiguous()
    assert tuple(out.shape) == (rows, inner)
    oc = out.cpu()
    assert not bool(torch.isnan(oc).any())
    gates = a[:, inner:2 * inner]
    if rows * inner >= 17:
        assert bool((oc[gates == -20.0] == 0).all()) and bool((oc[gates == 0.0] == 0).all())      # (-0.0 == 0.0 takes both zeros)
        assert int((gates == -20.0).sum()) == 1 and int((gates == 0.0).sum()) == 2
    ratio = SC._worst((oc.double() - ref).abs(), bound)
    print(f"geglu {rows}x{inner}: max |err| {float((oc.double() - ref).abs().max()):.3e}, worst err / bound {ratio:.4f}")
    assert ratio <= 1.0, ratio
    assert torch.equal(ad.cpu(), a)


# ------------------------------------------------------------------------------------------------------------- attention on token rows
def _permuted(t, H):
    """[B, N, H*D] (any strides) -> contiguous [(b h), n, d]."""
    B, N, W = t.shape
    return t.reshape(B, N, H, W // H).permute(0, 2, 1, 3).reshape(B * H, N, W // H).contiguous()


def _bnhd_case(B, H, D, Nq, Nk, layout, g):
    """q, k, v as slices of GEMM-shaped buffers on the device: "q+kv" -- q from an inner-wide buffer, k | v from one 2*inner-wide
    buffer; "qkv" -- all three from one 3*inner-wide buffer (Nq == Nk); "separate" -- three contiguous tensors."""
    inner = H * D
    if layout == "qkv":
        assert Nq == Nk
        buf = torch.randn((B, Nq, 3 * inner), generator=g).cuda()
        return buf[..., :inner], buf[..., inner:2 * inner], buf[..., 2 * inner:]
    q = torch.randn((B, Nq, inner), generator=g).cuda()
    if layout == "q+kv":
        kv = torch.randn((B, Nk, 2 * inner), generator=g).cuda()
        return q, kv[..., :inner], kv[..., inner:]
    return q, torch.randn((B, Nk, inner), generator=g).cuda(), torch.randn((B, Nk, inner), generator=g).cuda()


BNHD_CASES = [
    (2, 8, 40, 30, 30, "q+kv", None), (2, 8, 40, 132, 77, "q+kv", "shared"), (1, 2, 64, 132, 132, "qkv", "per"),
    (1, 1, 80, 70, 70, "separate", None), (1, 3, 128, 70, 33, "separate", None), (1, 2, 160, 129, 65, "separate", None),
]


@pytest.mark.parametrize("B,H,D,Nq,Nk,layout,bias", BNHD_CASES, ids=lambda v: str(v))
def test_attention_bnhd_is_bit_identical_to_attention_on_permuted_copies(cuda, B, H, D, Nq, Nk, layout, bias):
    """The same kernel with other addresses: torch.equal, not a tolerance.  More than one 128-query tile, ragged last key blocks
    (Nk % 32 != 0), batch-heads that are and are not a multiple of the 8 XCDs, a shared and a per-batch-head bias."""
    from sd_animation_optical_flow_amd import ops
    g = _gen(B, H, D, Nq, Nk)
    q, k, v = _bnhd_case(B, H, D, Nq, Nk, layout, g)
    bz = None
    if bias:
        bz = (torch.randn((Nq, Nk) if bias == "shared" else (B * H, Nq, Nk), generator=g) * 2.0)
        bz[..., 1::7] = float("-inf")                                   # masked keys; key 0 stays open in every row
        bz = bz.cuda()
    out = ops.attention_bnhd(q, k, v, H, bias=bz)
    assert tuple(out.shape) == (B, Nq, H * D) and out.is_contiguous()
    ref = ops.attention(_permuted(q, H), _permuted(k, H), _permuted(v, H), bz)
    assert torch.equal(_permuted(out, H), ref)
    # written into a slice of a wider buffer, with an explicit scale: the other columns keep their content
    wide = torch.full((B, Nq, H * D + 8), 7.0, device="cuda")
    ops.attention_bnhd(q, k, v, H, bias=bz, scale=0.2, out=wide[..., 4:4 + H * D])
    assert torch.equal(_permuted(wide[..., 4:4 + H * D], H), ops.attention(_permuted(q, H), _permuted(k, H), _permuted(v, H), bz, 0.2))
    assert bool((wide[..., :4] == 7.0).all()) and bool((wide[..., 4 + H * D:] == 7.0).all())
    if (D, bias) == (40, "shared"):
        # and against float64 within the bound derived for the fused kernel (flash_attn_check.fa_reference), capped by the bound of
        # the unfused kernel this check used before, so that it asks no less than it did
        operands = (_permuted(q, H).cpu(), _permuted(k, H).cpu(), _permuted(v, H).cpu(), bz.cpu(), float(D) ** -0.5)
        ref64, bound = FC.fa_reference(*operands)
        bound = torch.minimum(bound, SC.at_reference(*operands)[1])
        ratio = SC._worst((_permuted(out, H).cpu().double() - ref64).abs(), bound)
        print(f"attention_bnhd vs float64: worst err / bound {ratio:.4f}")
        assert ratio <= 1.0


def test_attention_bnhd_rejects_bad_arguments_without_launching(cuda):
    from sd_animation_optical_flow_amd import _lib, ops
    L = _lib.lib()
    B, H, D, N = 1, 2, 40, 8
    q = torch.zeros((B, N, 3 * H * D + 4), device="cuda")
    o = torch.full((B, N, H * D), 5.0, device="cuda")
    s = ops._stream()
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    call = lambda qp, ld, d, h=H, op=None: L.ofx_attention_bnhd_f32(qp, ld, p(q, 4 * H * D), ld, p(q, 8 * H * D), ld, None, 0, op or p(o), H * D,
                                                                    B, h, N, N, d, 1.0, s)
    assert call(p(q), 3 * H * D + 4, D) == 0
    torch.cuda.synchronize()
    assert not bool((o == 5.0).any())
    o.fill_(5.0)
    assert call(p(q), 3 * H * D + 4, 48) == SC.EINVAL                      # a head size the fused kernel does not take
    assert call(p(q), 3 * H * D + 4, 20, h=4) == SC.EINVAL
    assert call(None, 3 * H * D + 4, D) == SC.EINVAL
    assert call(p(q), H * D - 4, D) == SC.EINVAL                           # rows shorter than H * D
    assert call(p(q, 4), 3 * H * D + 4, D) == SC.EALIGN                    # q not 16-byte aligned
    assert call(p(q), 3 * H * D + 4, D, op=p(o, 8)) == SC.EALIGN           # out not 16-byte aligned
    assert call(p(q), 3 * H * D + 2, D) == SC.EALIGN                       # ld % 4 != 0
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())
    with pytest.raises(_lib.OfxError):
        ops.attention_bnhd(q[..., :96], q[..., 96:192], q[..., 96:192], 2)                     # D = 48 through the wrapper
    with pytest.raises(RuntimeError):
        ops.attention_bnhd(q[..., :80], q[..., 80:160], q[:, :4, 80:160], 2, out=o[:, :4])     # k and v of different lengths
    with pytest.raises(RuntimeError):
        ops.attention_bnhd(q[..., :80].cpu(), q[..., :80], q[..., :80], 2)


# ------------------------------------------------------------------------------------------------------------- the module
@pytest.fixture(scope="module")
def gold():
    """Per configuration: the stored vectors, the module on the device (built once) and the reference K/V of the stored runs."""
    from sd_animation_optical_flow_amd import transformer as T
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for tag in TAGS:
        g = np.load(gold_path(tag))
        Cn, heads, d, ctx = (int(v) for v in g["cfg"][:4])
        sd = T.random_spatial_transformer_state_dict(0, Cn, heads, d, ctx)
        prefix = "model.diffusion_model.input_blocks.1.1."                # the prefix of a full checkpoint
        mod = T.SpatialTransformer({prefix + k: v for k, v in sd.items()}, heads, d, prefix=prefix)
        k, v = torch.from_numpy(g["k"]), torch.from_numpy(g["v"])
        out[tag] = dict(g=g, mod=mod, heads=heads, x=torch.from_numpy(g["x"]).cuda(), context=torch.from_numpy(g["context"]).cuda(),
                        ref_all=TC.reference_all(k, v, heads), ref_pos=TC.reference_positive(k, v, heads))
    return out


def _within_bar(mine, ref, label):
    err = float((mine.cpu() - ref).abs().max())
    print(f"{label}: max |err| {err:.3e}, bar {TC.bar_of(ref):.3e}")
    assert tuple(mine.shape) == tuple(ref.shape)
    assert err <= TC.bar_of(ref), (label, err)


@pytest.mark.parametrize("tag", TAGS)
def test_module_against_the_reference_vectors(cuda, gold, tag):
    """The HIP module on the stored inputs against what the REAL reference module produced: the output, both halves of kv_hist, the
    run on reference K/V of batch B (given in the reference's layout, on the host, with a layer index) and of batch B - 1 (given in
    our layout, on the device), whose image 0 equals the plain run bit for bit."""
    from sd_animation_optical_flow_amd import transformer as T
    c = gold[tag]
    g, mod, heads = c["g"], c["mod"], c["heads"]
    assert mod.fused_attention and not mod.torch_glue and mod.depth == 1 and mod.context_dim == int(g["cfg"][3])
    out, hist = mod(c["x"], c["context"])
    _within_bar(out, torch.from_numpy(g["out"]), f"{tag} out")
    assert len(hist) == 1 and all(t.is_cuda and t.is_contiguous() and tuple(t.shape) == (c["x"].shape[0], c["x"].shape[2] * c["x"].shape[3], mod.inner)
                                  for t in hist[0])
    _within_bar(T.to_reference_layout(hist[0][0], heads), torch.from_numpy(g["k"]), f"{tag} kv_hist k")
    _within_bar(T.to_reference_layout(hist[0][1], heads), torch.from_numpy(g["v"]), f"{tag} kv_hist v")
    out_all, hist_all = mod(c["x"], c["context"], reference_kv=[(c["ref_all"][0], c["ref_all"][1], 0)])
    _within_bar(out_all, torch.from_numpy(g["out_refall"]), f"{tag} reference_kv of batch B")
    assert torch.equal(hist_all[0][0], hist[0][0]) and torch.equal(hist_all[0][1], hist[0][1])        # the own K/V, not the references'
    kp, vp = (T.from_reference_layout(t, heads).cuda() for t in c["ref_pos"])
    out_pos, hist_pos = mod(c["x"], c["context"], reference_kv=[(kp, vp)])
    _within_bar(out_pos, torch.from_numpy(g["out_refpos"]), f"{tag} reference_kv of batch B - 1")
    assert torch.equal(out_pos[0], out[0]) and not torch.equal(out_pos[1], out[1])
    assert torch.equal(hist_pos[0][0], hist[0][0])


@pytest.mark.parametrize("tag", TAGS)
def test_forward_nhwc_and_forward_agree_bit_for_bit(cuda, gold, tag):
    c = gold[tag]
    out, hist = c["mod"](c["x"], c["context"])
    out2, hist2 = c["mod"].forward_nhwc(c["x"].permute(0, 2, 3, 1).contiguous(), c["context"])
    assert tuple(out2.shape) == tuple(c["x"].permute(0, 2, 3, 1).shape)
    assert torch.equal(out2.permute(0, 3, 1, 2), out) and torch.equal(hist2[0][0], hist[0][0]) and torch.equal(hist2[0][1], hist[0][1])


def test_module_rejects_bad_reference_kv_and_inputs_before_any_launch(cuda, gold):
    from sd_animation_optical_flow_amd import transformer as T
    c = gold["c0"]
    mod, x, ctx = c["mod"], c["x"], c["context"]
    B, N = x.shape[0], x.shape[2] * x.shape[3]
    z = lambda b, n: torch.zeros((b, n, mod.inner))
    for bad in ([(z(1, N - 1), z(1, N - 1))], [(z(3, N), z(3, N))], [(z(1, N), z(1, N)), (z(1, N), z(1, N))], [(z(2, N),)],
                [(z(2, N), z(2, N + 1))], [(torch.zeros((B, N, 24)), torch.zeros((B, N, 24)))]):
        with pytest.raises(ValueError):
            mod(x, ctx, reference_kv=bad)
    with pytest.raises(ValueError):
        mod(x, None)                                                          # context_dim 768 != inner: no context is no option
    with pytest.raises(RuntimeError):
        mod(x.cpu(), ctx)
    with pytest.raises(RuntimeError):
        mod(x[:, :64], ctx)                                                   # wrong channel count
    with pytest.raises(RuntimeError):
        mod(x, ctx[:, :, :64])
    sd = T.random_spatial_transformer_state_dict(0, 64, 2, 40, 32)
    with pytest.raises(KeyError):
        T.SpatialTransformer({k: v for k, v in sd.items() if "norm2" not in k}, 2, 40)
    with pytest.raises(ValueError):
        T.SpatialTransformer(dict(sd, **{"transformer_blocks.0.ff.net.2.bias": torch.zeros(81)}), 2, 40)
    with pytest.raises(NotImplementedError):
        T.SpatialTransformer(sd, 2, 40, use_linear=True)


# small configurations for the float64 comparisons: (in_channels, heads, d_head, context_dim, depth)
SMALL = {"ctx": (64, 2, 40, 32, 1), "noctx": (64, 2, 40, None, 1), "depth2": (64, 2, 40, 32, 2), "unfused-d32": (64, 2, 32, 32, 1)}


@pytest.fixture(scope="module")
def small():
    from sd_animation_optical_flow_amd import transformer as T
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for name, (Cn, heads, d, ctx, depth) in SMALL.items():
        sd = T.random_spatial_transformer_state_dict(3, Cn, heads, d, ctx, depth)
        out[name] = dict(mod=T.SpatialTransformer(sd, heads, d), sd64=TC.to64(sd), heads=heads, depth=depth, C=Cn, ctx=ctx)
    return out


def _small_inputs(s, B, h, w, M=7):
    g = _gen(B, h, w, s["depth"], s["heads"])
    x = torch.randn((B, s["C"], h, w), generator=g)
    context = None if s["ctx"] is None else torch.randn((B, M, s["ctx"]), generator=g)
    return x, context


@pytest.mark.parametrize("name,B,h,w", [("ctx", 1, 1, 1), ("ctx", 2, 6, 5), ("ctx", 1, 12, 11), ("noctx", 2, 6, 5), ("depth2", 2, 6, 5),
                                        ("unfused-d32", 2, 6, 5)], ids=lambda v: str(v))
def test_module_against_the_float64_restatement(cuda, small, name, B, h, w):
    """Shapes that are not in the golden files (a single token; one and two 128-query tiles), context=None (the cross-attention
    is a second self-attention), two blocks, and a head size the fused kernel does not take (permute + `ops.attention`)."""
    s = small[name]
    mod = s["mod"]
    assert mod.depth == s["depth"] and mod.fused_attention == (name != "unfused-d32")
    x, context = _small_inputs(s, B, h, w)
    ref, hist64 = TC.spatial_transformer64(s["sd64"], x, s["heads"], context, depth=s["depth"])
    out, hist = mod(x.cuda(), None if context is None else context.cuda())
    _within_bar(out.double(), ref, f"{name} {B}x{h}x{w} out")
    assert len(hist) == s["depth"]
    for i in range(s["depth"]):
        _within_bar(hist[i][0].double(), hist64[i][0], f"{name} block {i} k")
        _within_bar(hist[i][1].double(), hist64[i][1], f"{name} block {i} v")


def test_two_concatenated_references_against_the_float64_restatement(cuda, small):
    """Two references of different token counts at batch B, one in each layout: Nk = 13 + 30 keys, none of them the image's own."""
    from sd_animation_optical_flow_amd import transformer as T
    s = small["ctx"]
    B, h, w = 2, 6, 5
    x, context = _small_inputs(s, B, h, w)
    g = _gen(13, 30)
    inner = s["mod"].inner
    refs = [(torch.randn((B, n, inner), generator=g), torch.randn((B, n, inner), generator=g)) for n in (13, 30)]
    ref, _ = TC.spatial_transformer64(s["sd64"], x, s["heads"], context, refs)
    given = [(T.to_reference_layout(refs[0][0], s["heads"]), T.to_reference_layout(refs[0][1], s["heads"]), 4), (refs[1][0].cuda(), refs[1][1].cuda())]
    out, _ = s["mod"](x.cuda(), context.cuda(), reference_kv=given)
    _within_bar(out.double(), ref, "two references")
    plain, _ = TC.spatial_transformer64(s["sd64"], x, s["heads"], context)
    assert float((plain - ref).abs().max()) > 100 * TC.bar_of(ref)                # the references matter


_CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import transformer_check as TC
from sd_animation_optical_flow_amd import transformer as T
for path in sys.argv[2:]:
    g = np.load(path)
    Cn, heads, d, ctx = (int(v) for v in g["cfg"][:4])
    mod = T.SpatialTransformer(T.random_spatial_transformer_state_dict(0, Cn, heads, d, ctx), heads, d)
    assert mod.torch_glue and not mod.fused_attention
    x, context = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["context"]).cuda()
    k, v = torch.from_numpy(g["k"]), torch.from_numpy(g["v"])
    out, hist = mod(x, context)
    out_all, _ = mod(x, context, reference_kv=[TC.reference_all(k, v, heads)])
    out_pos, _ = mod(x, context, reference_kv=[TC.reference_positive(k, v, heads)])
    for mine, name in ((out, "out"), (T.to_reference_layout(hist[0][0], heads), "k"), (T.to_reference_layout(hist[0][1], heads), "v"),
                       (out_all, "out_refall"), (out_pos, "out_refpos")):
        ref = torch.from_numpy(g[name])
        print("ERR %s %.9e %.9e" % (name, float((mine.cpu() - ref).abs().max()), float(ref.abs().max())))
"""


def test_torch_glue_path_in_a_fresh_process(cuda):
    """OFX_ST_TORCH_GLUE=1 is read once per process, so the glue path (torch LayerNorm / GEGLU, permute + `ops.attention`) runs in a
    child: same stored vectors, same bar."""
    env = dict(os.environ, OFX_ST_TORCH_GLUE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(HERE)] + [gold_path(t) for t in TAGS], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("ERR ")]
    assert len(lines) == 5 * len(TAGS)
    for _, name, err, mx in lines:
        print(f"glue path {name}: max |err| {float(err):.3e}")
        assert float(err) <= 2e-4 * max(1.0, float(mx)), name
