"""The fp16 arithmetic (OFX_PREC_F16) and the `precision=` of the UNet, as far as the host can tell: the launcher's plan and its
rejections (ofx_conv2d_plan: the launcher's own validation and rule, no operand read, no device), every convolution / GEMM shape of
the v1.5 UNet, the constructors' argument check, the oracle of tests/f16_check.py against an independent fp32 evaluation, and the
stored autocast yardstick.  No GPU: the descriptors carry dummy, aligned, never-dereferenced pointers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import f16_check as FC   # noqa: E402
import unet_check as UC   # noqa: E402

PTR = 0x10000                       # non-null, 16-byte aligned, never dereferenced
EINVAL = -1
TILES = {(128, 128), (128, 64), (64, 64)}
GOLD = os.path.join(HERE, "golden", "unet_ref_u0_autocast.npz")


def _lib():
    from sd_animation_optical_flow_amd import _lib
    return _lib


def _desc(B, H, W, c0, cout, k, stride=1, tile=0, c1=0, precision=FC.PREC_F16, **kw):
    d = _lib().ConvDesc()
    d.in0, d.ld0, d.c0, d.w = PTR, c0, c0, PTR
    if c1:
        d.in1, d.ld1, d.c1 = PTR, c1, c1
    d.out, d.ldo = PTR, cout
    d.B, d.Hin, d.Win = B, H, W
    d.Hout, d.Wout = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    d.Cout, d.KH, d.KW, d.stride, d.padH, d.padW = cout, k, k, stride, k // 2, k // 2
    d.tile, d.precision = tile, precision
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def _query(d, stats_cap=0, pool=0):
    p = _lib().ConvPlan()
    return _lib().lib().ofx_conv2d_plan(C.byref(d), stats_cap, pool, C.byref(p)), p


@pytest.mark.parametrize("c", FC.CASES, ids=FC.IDS)
def test_every_case_plans_onto_the_path_it_is_there_for(c):
    st, p = _query(_desc(c["B"], c["H"], c["W"], c["c0"], c["cout"], c["k"], c["stride"], c["tile"], c["c1"]))
    assert st == 0
    assert p.path == 0 and p.prec == FC.PREC_F16 and p.ks == 1 and p.ksplit == 1
    assert (p.bm, p.bn, p.bk, p.mode) == c["plan"], (c["name"], (p.bm, p.bn, p.bk, p.mode))


def test_plan_of_a_patchable_layer():
    for B, H, W, cin, cout in ((2, 64, 96, 320, 320), (2, 32, 48, 640, 640), (16, 64, 96, 128, 128), (4, 16, 24, 1280, 1280)):
        st, p = _query(_desc(B, H, W, cin, cout, 3))
        assert st == 0 and p.prec == FC.PREC_F16 and (p.bm, p.bn) in TILES and p.mode == 2 and p.bk == 16 and p.ks == p.ksplit == 1, (B, H, W, p.mode)
    # wino_w / wino4_w are ignored, as under the split-bf16 modes
    st, p = _query(_desc(16, 64, 96, 128, 128, 3, wino_w=PTR, wino4_w=PTR))
    assert st == 0 and p.path == 0 and p.prec == FC.PREC_F16 and p.mode == 2


def test_plan_rejections():
    base = dict(B=2, H=8, W=16, c0=64, cout=64, k=3)
    ok = lambda **kw: _query(_desc(**dict(base, **kw)))[0]
    assert ok() == 0
    gru = dict(aux_z=PTR, aux_rh=PTR, aux_h=PTR, ldh=64)
    flow = dict(aux_coords=PTR, aux_h=PTR, aux_flow4=PTR, cout=2)
    assert ok(precision=0, epi=1, **gru) == 0 and ok(precision=0, epi=3, **flow) == 0       # fp32 takes them: the precision rejects
    assert ok(epi=1, **gru) == EINVAL                       # OFX_EPI_GRU_ZR
    assert ok(epi=2, **gru) == EINVAL                       # OFX_EPI_GRU_Q
    assert ok(epi=3, **flow) == EINVAL                      # OFX_EPI_FLOW
    assert ok(nmean=PTR, nrstd=PTR) == EINVAL               # fused instance norm
    assert _query(_desc(**base), stats_cap=1 << 40)[0] == EINVAL      # ofx_conv2d_stats
    assert ok(splitk_ws=PTR, splitk_ws_bytes=1 << 40) == EINVAL       # split-K
    assert _query(_desc(**dict(base, precision=0, splitk_ws=PTR, splitk_ws_bytes=1 << 40)))[1].ksplit > 1
    assert ok(tile=2032064064) == EINVAL                    # paired pipelines
    assert ok(nz=2) == EINVAL                               # batched GEMM
    assert _query(_desc(1, 16, 16, 256, 256, 1), pool=1)[0] == EINVAL                      # pooled correlation volume
    assert _query(_desc(1, 16, 16, 256, 256, 1, precision=0), pool=1)[0] == 0
    assert ok(precision=6) == EINVAL and ok(precision=-1) == EINVAL
    # (a forced tile this arithmetic lacks, 128x192 say, is mapped onto one of its three like under the split-bf16 modes)
    st, p = _query(_desc(**dict(base, tile=16128192)))
    assert st == 0 and (p.bm, p.bn) == (128, 128)


def v15_conv_layers(B=2, H=64, W=96, tokens=77):
    """Every `ofx_conv2d` launch of `UNetModel(SD_V15_UNET)` on a B x H x W latent as (name, B, H, W, c0, c1, cout, k, stride),
    walked from `unet_layout` as `UNetModel._block` / `SpatialTransformer._block` issue them."""
    from sd_animation_optical_flow_amd.unet import SD_V15_UNET, unet_layout
    lay = unet_layout(SD_V15_UNET)
    ctx = int(lay["cfg"]["context_dim"])
    out = []
    h, w = H, W
    for blk in lay["input"] + [lay["middle"]] + lay["output"]:
        for l in blk:
            kind, name = l[0], l[1]
            if kind == "conv":
                out.append((name, B, h, w, (l[2] + 3) // 4 * 4, 0, l[3], 3, 1))
            elif kind == "res":
                cin, cout = l[2], l[3]
                out.append((f"{name}.in_layers.2", B, h, w, cin, 0, cout, 3, 1))
                out.append((f"{name}.out_layers.3", B, h, w, cout, 0, cout, 3, 1))
                if cin != cout:
                    c0, c1 = (l[4], l[5]) if len(l) == 6 else (cin, 0)
                    out.append((f"{name}.skip_connection", B, h, w, c0, c1, cout, 1, 1))
            elif kind == "st":
                ch, inner, n = l[2], l[3] * l[4], h * w
                out.append((f"{name}.proj_in", B, h, w, ch, 0, inner, 1, 1))
                for gname, rows, k, co in (("attn1.to_qkv", n, inner, 3 * inner), ("attn1.to_out.0", n, inner, inner),
                                           ("attn2.to_kv", tokens, ctx, 2 * inner), ("attn2.to_q", n, inner, inner),
                                           ("attn2.to_out.0", n, inner, inner), ("ff.net.0.proj", n, inner, 8 * inner),
                                           ("ff.net.2", n, 4 * inner, inner)):
                    out.append((f"{name}.{gname}", B, 1, rows, k, 0, co, 1, 1))
                out.append((f"{name}.proj_out", B, h, w, inner, 0, ch, 1, 1))
            elif kind == "down":
                out.append((f"{name}.op", B, h, w, l[2], 0, l[2], 3, 2))
                h, w = h // 2, w // 2
            else:
                h, w = 2 * h, 2 * w                                   # Upsample is ofx_upconv2x: fp32 in every precision
    mc = int(lay["cfg"]["model_channels"])
    out.append(("out.2", B, H, W, mc, 0, int(lay["cfg"]["out_channels"]), 3, 1))
    return out


def test_every_layer_of_the_v15_unet_plans():
    layers = v15_conv_layers()
    assert len(layers) == 1 + 22 * 2 + 14 + 16 * 9 + 3 + 1, len(layers)    # conv_in, 22 ResBlocks (14 with a skip conv), 16 transformers, 3 Downsamples, out
    total = patch = 0.0
    modes = {0: 0, 1: 0, 2: 0}
    for name, B, h, w, c0, c1, cout, k, stride in layers:
        d = _desc(B, h, w, c0, cout, k, stride, c1=c1, shift=PTR)
        st, p = _query(d)
        assert st == 0, name
        assert p.path == 0 and p.prec == FC.PREC_F16 and (p.bm, p.bn) in TILES and p.bk in (16, 32) and p.ks == 1 and p.ksplit == 1, name
        flops = 2.0 * B * d.Hout * d.Wout * cout * k * k * (c0 + c1)
        total += flops
        patch += flops if p.mode == 2 else 0.0
        modes[p.mode] += 1
    print(f"v1.5 UNet, batch 2, 64x96 latent: {len(layers)} ofx_conv2d launches, {total / 1e9:.1f} GFLOP; on the halo patch {100 * patch / total:.1f} % "
          f"of the FLOPs; launches by schedule: general {modes[0]}, scalar {modes[1]}, patch {modes[2]}")
    assert patch > 0.0


def test_precision_argument_is_checked_first():
    from sd_animation_optical_flow_amd.transformer import MODEL_PRECISIONS, SpatialTransformer
    from sd_animation_optical_flow_amd.unet import UNetModel
    assert MODEL_PRECISIONS == ("fp32", "fp16", "bf16x3", "bf16x6")
    # an empty checkpoint would be a KeyError and a missing device a RuntimeError: the precision is looked at before either
    with pytest.raises(ValueError, match="precision"):
        UNetModel({}, UC.U0, precision="fp17")
    with pytest.raises(ValueError, match="precision"):
        SpatialTransformer({}, 1, 64, precision="bf16x6_w")
    with pytest.raises(ValueError, match="precision"):
        UNetModel({}, UC.U0, precision=None)


def test_ops_precision_table():
    from sd_animation_optical_flow_amd import ops
    assert ops.CONV_PRECISIONS["fp16"] == FC.PREC_F16 == 5
    assert [ops.CONV_PRECISIONS[k] for k in ("fp32", "bf16x3", "bf16x3_w", "bf16x6", "bf16x6_w")] == [0, 1, 2, 3, 4]
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ofx.h")).read()
    assert "#define OFX_PREC_F16 5" in hdr


@pytest.mark.parametrize("c", FC.CASES[:12], ids=FC.IDS[:12])
def test_oracle_against_an_fp32_evaluation(c):
    """F.conv2d in float32 over the rounded operands is one admissible summation order of exact products: inside the bound."""
    t = FC.inputs(c)
    ref, bound = FC.reference(c, t)
    x = t["x"] if t["x2"] is None else torch.cat([t["x"], t["x2"]], dim=3)
    v = F.conv2d(x.half().float().permute(0, 3, 1, 2), t["w"].half().float(), stride=c["stride"], padding=c["k"] // 2).permute(0, 2, 3, 1)
    if t["scale"] is not None:
        v = v * t["scale"]
    for name in ("shift", "addend"):
        if t[name] is not None:
            v = v + t[name]
    if c["extra"].get("act") == "relu":
        v = v.clamp_min(0.0)
    if t["res"] is not None:
        v = (v + t["res"]).clamp_min(0.0)
    worst = FC.worst_ratio(v, ref, bound)
    # and the bound notices the arithmetic it is not for: unrounded operands are ~2^-11 relative away per product, 2^-11.5 sqrt(K) of
    # an rms product in the sum, against a bound of K u times the sum of magnitudes -- above it up to K of a few hundred
    raw = F.conv2d(x.permute(0, 3, 1, 2).double(), t["w"].double(), stride=c["stride"], padding=c["k"] // 2).permute(0, 2, 3, 1)
    plain = c["extra"].get("act") is None and all(t[n] is None for n in ("scale", "shift", "addend", "res")) and t["w"][0].numel() <= 320
    print(f"{c['name']}: fp32 evaluation |error| / bound {worst:.3f}")
    assert worst <= 1.0
    if plain:
        away = FC.worst_ratio(raw, ref, bound)
        print(f"{c['name']}: the unrounded float64 convolution |difference| / bound {away:.1f}")
        assert away > 1.0


def test_small_case_reaches_fp16_subnormals():
    c = next(c for c in FC.CASES if c["name"] == "small")
    t = FC.inputs(c)
    xh = t["x"].half()
    sub = (xh != 0) & (xh.abs().float() < 2.0 ** -14)
    print(f"small: {int(sub.sum())} of {xh.numel()} activations are fp16 subnormals")
    assert int(sub.sum()) >= 32
    m = next(c for c in FC.CASES if c["name"] == "max")
    tm = FC.inputs(m)
    assert float(tm["x"].abs().max()) == 65504.0 and float(tm["w"].abs().max()) == 65504.0
    assert bool(torch.isfinite(tm["x"].half()).all())


def test_autocast_yardstick_is_stored_for_every_output():
    g = np.load(GOLD)
    keys = [str(k) for k in g["dist_keys"]]
    want = ["out", "out_refall", "out_refpos", "out_ctl", "out_ctl_mid"] + [f"{kv}{i}" for i in range(7) for kv in "kv"]
    assert sorted(keys) == sorted(want)
    d = dict(zip(keys, g["autocast_vs_f64"].tolist()))
    fp32 = np.load(os.path.join(HERE, "golden", "unet_ref_u0.npz"))
    d32 = dict(zip([str(k) for k in fp32["dist_keys"]], fp32["ref_vs_f64"].tolist()))
    for k in want:
        assert g[k].dtype == np.float32 and g[k].shape == fp32[k].shape, k
        assert 1e-4 < d[k] < 5e-2, (k, d[k])                         # half-precision level on values of order 1 ...
        assert d[k] > 50 * d32[k], (k, d[k], d32[k])                 # ... far above the fp32 module's distance
        assert abs(float(np.abs(g[k].astype(np.float64) - fp32[k]).max()) - d[k]) < 0.5 * d[k] + 1e-4, k   # the stored arrays are that run
    print("autocast vs float64: " + ", ".join(f"{k} {d[k]:.2e}" for k in want[:5]))
