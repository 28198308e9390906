"""The fp16 form of the fused attention kernel (OFX_PREC_F16: ofx_attention_prec / ofx_attention_bnhd_prec, `ops.attention(precision=)`,
`attention_precision=` of SpatialTransformer / UNetModel) as far as the host can tell: the checker of flash_attn_f16_check.py against
its own emulation and simulated bugs, the arithmetic alone against the model-level bars of attn_f16_model_check.py, the argument
checks that need no device, the prototypes, and the compiler's resource remarks.  No test here needs a GPU."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import attn_f16_model_check as MC   # noqa: E402
import flash_attn_f16_check as f16  # noqa: E402
import transformer_check as TC      # noqa: E402
import unet_check as UC             # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1 - 3: the checker

@pytest.fixture(scope="module")
def sweep():
    """Every case of the table through the unmodified emulation and through every simulated bug, once."""
    good, bad = {}, {}
    for c in f16.FA_CASES:
        q, k, v, bias, ref, bound = f16.fa16_case_data(c)
        scale = f16.fa_scale(c)
        good[c["name"]] = f16.fa_compare(f16.fa16_emulate(q, k, v, bias, scale), ref, bound)
        for bug in f16.FA16_BUGS:
            if f16.fa16_applies(bug, c["D"]):
                bad[(bug, c["name"])] = f16.fa_compare(f16.fa16_emulate(q, k, v, bias, scale, bug=bug), ref, bound)
    return good, bad


def test_the_reference_of_the_rounded_operands_is_nan_where_the_fp32_one_is():
    """Rounding to half moves no NaN and makes no new one at the table's magnitudes: the planted rows stay the planted rows."""
    for c in f16.FA_CASES:
        q, k, v, bias, ref, bound = f16.fa16_case_data(c)
        flat = torch.isnan(ref.reshape(-1, c["D"]))
        assert flat.all(1).nonzero().flatten().tolist() == f16.fa_planted(c) and not bool((flat.any(1) & ~flat.all(1)).any()), c["name"]
        ok = ~torch.isnan(ref)
        assert bool(torch.isfinite(bound[ok]).all()) and bool((bound[ok] > 0).all()), c["name"]
        assert bool(torch.isfinite(q[~torch.isnan(q)].half().float()).all()) and bool(torch.isfinite(k.half().float()).all())


def test_the_emulation_is_inside_the_bound_at_every_case(sweep):
    good, _ = sweep
    worst = max((rep["ratio"], name) for name, rep in good.items())
    print(f"ratio emulation, worst case {worst[1]} {worst[0]:.4g}")
    for name, rep in good.items():
        assert rep["ok"], (name, rep)


def test_the_checker_catches_each_simulated_bug_at_every_head_size(sweep):
    _, bad = sweep
    for bug in f16.FA16_CATCHABLE:
        total, closest = 0, float("inf")
        for D in f16.FLASH_D:
            if not f16.fa16_applies(bug, D):
                continue
            hits = [rep["ratio"] for (b, name), rep in bad.items() if b == bug and name.startswith(f"d{D}-") and not rep["ok"]]
            assert hits, f"{bug} goes unnoticed at every case of head size {D}"
            total, closest = total + len(hits), min(closest, max(hits))
        print(f"bug {bug}: caught at {total} cases; the smallest over the head sizes of its largest ratio {closest:.4g}")
    # the uncatchable ones: listed with their measured ratios, not asserted (header of flash_attn_f16_check.py)
    for bug in f16.FA16_UNCATCHABLE:
        reps = [(rep["ratio"], name) for (b, name), rep in bad.items() if b == bug]
        print(f"bug {bug}: NOT catchable by a bound; largest ratio {max(reps)[0]:.4g} ({max(reps)[1]}), outside at "
              f"{sum(1 for (b, _), rep in bad.items() if b == bug and not rep['ok'])} cases")


def test_the_d40_cases_catch_a_nan_in_the_pad_columns(sweep):
    _, bad = sweep
    cases = [c for c in f16.FA_CASES if c["D"] == 40]
    assert f16.fa16_dp(40) == 48 and all(f16.fa16_dp(D) == D for D in f16.FLASH_D if D != 40)
    for c in cases:
        rep = bad[("pad_columns_nan", c["name"])]
        assert not rep["ok"] and rep["nan_extra"] > 0, (c["name"], rep)
    assert not any(b == "pad_columns_nan" and not name.startswith("d40-") for (b, name) in bad)


def test_the_key_permutation_of_the_p_fragment():
    """Element j of lane half h in k-step s is key 16 s + 8 (j >> 2) + 4 h + (j & 3): a permutation of the block, its own inverse,
    and what the transposed V read must supply (read a = j >> 2 takes keys 16 s + 8 a + 4 h + 0..3)."""
    perm = f16.fa16_key_perm()
    assert sorted(perm.tolist()) == list(range(32)) and torch.equal(perm[perm], torch.arange(32))
    assert perm[:16].tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]


def test_the_exactness_cases_are_exact_in_the_emulation():
    for D in f16.FLASH_D:
        q, k, v, bias, want = f16.fa16_onehot_case(D)
        assert q.shape[1] == k.shape[1] == 2 * f16.fa_bk(D) + 1
        assert torch.equal(f16.fa16_emulate(q, k, v, bias, D ** -0.5), want)
        for bug in ("v_natural_key_order", "kv_buffer_reused_early"):
            assert not torch.equal(f16.fa16_emulate(q, k, v, bias, D ** -0.5, bug=bug), want), (D, bug)
        for Nk in (1, 2, 16, 32):
            q, k, v, want = f16.fa16_mean_case(D, Nk)
            assert torch.equal(f16.fa16_emulate(q, k, v, None, 0.0), want), (D, Nk)


# ---------------------------------------------------------------------------------------------------------------------------------
# the arithmetic alone against the model-level bars

@pytest.mark.parametrize("tag", ["c0", "c1"])
def test_the_arithmetic_alone_stays_inside_the_transformer_bar(tag):
    from sd_animation_optical_flow_amd import transformer as T
    g = np.load(os.path.join(HERE, "golden", f"spatial_transformer_ref_{tag}.npz"))
    Cn, heads, d, ctx = (int(v) for v in g["cfg"][:4])
    sd64 = TC.to64(T.random_spatial_transformer_state_dict(0, Cn, heads, d, ctx))
    x, c = torch.from_numpy(g["x"]), torch.from_numpy(g["context"])
    ref, hist = MC.spatial_transformer64_r(sd64, x, heads, c, attn="half")
    ker, hist_k = MC.spatial_transformer64_r(sd64, x, heads, c, attn="kernel")
    exact, hist_e = TC.spatial_transformer64(sd64, x, heads, c)
    err = float((ker - ref).abs().max())
    print(f"{tag}: kernel arithmetic vs the half restatement {err:.3e}; bar {MC.bar_st(ref):.3e}; the mode vs exact {float((ref - exact).abs().max()):.3e}")
    assert err <= MC.bar_st(ref)
    assert float((ref - exact).abs().max()) > 0                            # the roundings are really made
    for a, b in zip(hist + hist_k, hist_e + hist_e):                       # the K/V history is taken before the attention
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_arithmetic_alone_stays_inside_the_unet_bar():
    """unet64 with the contraction operands, the attention operands and P rounded to half, against unet64: inside 2 x the autocast
    yardstick at all five scenarios, before any device is asked (header of attn_f16_model_check.py)."""
    from sd_animation_optical_flow_amd import unet as UN
    gold = np.load(os.path.join(HERE, "golden", "unet_ref_u0.npz"))
    ga = np.load(os.path.join(HERE, "golden", "unet_ref_u0_autocast.npz"))
    yard = {str(k): float(v) for k, v in zip(ga["dist_keys"], ga["autocast_vs_f64"])}
    sd64 = TC.to64(UN.random_unet_state_dict(0, UC.U0))
    lay = UN.unet_layout(UC.U0)
    heads = UC.transformer_heads(lay)
    hist0 = [(torch.from_numpy(gold[f"k{i}"]), torch.from_numpy(gold[f"v{i}"])) for i in range(len(heads))]
    x, t, ctx = (torch.from_numpy(gold[n]) for n in ("x", "timesteps", "context"))
    ctl = UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)
    f64 = lambda mode: [[(TC.heads_last(k, h).double(), TC.heads_last(v, h).double())
                         for (k, v), h in zip(UC.reference_frames(hist0, heads, mode)[0], heads)]]
    scen = {"out": {}, "out_refall": dict(reference_kv=f64("all")), "out_refpos": dict(reference_kv=f64("positive")),
            "out_ctl": dict(control=ctl), "out_ctl_mid": dict(control=ctl, only_mid_control=True)}
    keep = (UC._conv, UC.upsample64, TC.spatial_transformer64)
    dist = {}
    for name, kw in scen.items():
        exact, hist_e = UC.unet64(sd64, lay, x, t, ctx, **kw)
        both, hist_b = MC.unet64_r(sd64, lay, x, t, ctx, gemm=True, attn="kernel", **kw)
        attn_only, hist_a = MC.unet64_r(sd64, lay, x, t, ctx, gemm=False, attn="kernel", **kw)
        dist[name] = (float((both - exact).abs().max()), float((attn_only - exact).abs().max()))
        # fp32 contractions: what the first transformer records precedes every attention and does not see the attention's mode
        assert torch.equal(hist_a[0][0], hist_e[0][0]) and torch.equal(hist_a[0][1], hist_e[0][1]) and len(hist_a) == len(hist_e) == len(heads)
    assert (UC._conv, UC.upsample64, TC.spatial_transformer64) == keep     # the restatements are back in place
    for name, (d_both, d_attn) in dist.items():
        print(f"{name}: contractions + attention in half vs float64 {d_both:.3e}; attention alone {d_attn:.3e}; bar {2.0 * yard[name]:.3e}")
    for name, (d_both, d_attn) in dist.items():
        assert 0.0 < d_attn <= 2.0 * yard[name] and 0.0 < d_both <= 2.0 * yard[name], name


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: the surface, without a device

def test_bad_precisions_are_value_errors_before_a_device_is_touched(monkeypatch):
    from sd_animation_optical_flow_amd import ops, transformer as T, unet as UN
    q = torch.zeros((1, 4, 40))                                            # CPU tensors: a device check would be a RuntimeError
    for bad in ("fp64", "bf16x3", "FP16", None, 5):
        with pytest.raises(ValueError, match="precision"):
            ops.attention(q, q, q, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ops.attention_bnhd(q, q, q, 1, precision=bad)
        with pytest.raises(ValueError, match="attention_precision"):
            T.SpatialTransformer({}, 8, 40, attention_precision=bad)       # before the (empty) checkpoint is read
        with pytest.raises(ValueError, match="attention_precision"):
            UN.UNetModel({}, UC.U0, attention_precision=bad)
    # fp16 with a head size the fused kernel does not take: no unfused fp16 path
    for D in (512, 32, 48):
        z = torch.zeros((1, 4, D))
        with pytest.raises(ValueError, match="fp16"):
            ops.attention(z, z, z, precision="fp16")
        with pytest.raises(ValueError, match="d_head"):
            T.SpatialTransformer({}, 1, D, attention_precision="fp16")
    assert T.FUSED_HEAD_SIZES == ops.ATTENTION_FUSED_HEAD_SIZES == f16.FLASH_D
    assert ops.ATTENTION_PRECISIONS == {"fp32": f16.PREC_FP32, "fp16": f16.PREC_F16}
    # fp16 with the torch glue: a ValueError at construction, no silent fallback (the switch is cached per process)
    T._torch_glue.cache_clear() if hasattr(T._torch_glue, "cache_clear") else None
    monkeypatch.setenv("OFX_ST_TORCH_GLUE", "1")
    try:
        with pytest.raises(ValueError, match="OFX_ST_TORCH_GLUE"):
            T.SpatialTransformer({}, 8, 40, attention_precision="fp16")
    finally:
        monkeypatch.delenv("OFX_ST_TORCH_GLUE")
        T._torch_glue.cache_clear() if hasattr(T._torch_glue, "cache_clear") else None
    # the default arguments reach the old checks: an empty checkpoint, not a precision, is what is wrong
    with pytest.raises((KeyError, RuntimeError)):
        T.SpatialTransformer({}, 8, 40, attention_precision="fp32")


def test_every_transformer_of_sd_v15_takes_the_fp16_kernel_and_u0_has_one_that_does_not():
    """UNetModel hands attention_precision to every transformer whose head size the fused kernel takes: all 16 of SD v1.5; at the
    test configuration u0 the middle transformer (192) is the one exception, which the model keeps at fp32 and warns about."""
    from sd_animation_optical_flow_amd import unet as UN
    d_heads = lambda cfg: [(l[1], int(l[4])) for l in UN._layers(UN.unet_layout(cfg)) if l[0] == "st"]
    sd15 = d_heads(UN.SD_V15_UNET)
    assert len(sd15) == 16 and {d for _, d in sd15} == {40, 80, 160} and all(d in f16.FLASH_D for _, d in sd15)
    assert [(n, d) for n, d in d_heads(UC.U0) if d not in f16.FLASH_D] == [("middle_block.1", 192)]


def _proto(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_ctypes_table_and_the_header_agree_on_the_new_prototypes():
    import ctypes as C
    from sd_animation_optical_flow_amd import _lib
    header = open(os.path.join(ROOT, "include", "ofx.h")).read()
    kind = lambda a: ("p" if "*" in a else {"int": "i", "long": "l", "float": "f", "size_t": "z"}[a.rsplit(" ", 1)[0].replace("const ", "")])
    ctype = {C.c_void_p: "p", C.c_int: "i", C.c_long: "l", C.c_float: "f", C.c_size_t: "z"}
    for new, old in (("ofx_attention_prec", "ofx_attention_f32"), ("ofx_attention_bnhd_prec", "ofx_attention_bnhd_f32")):
        args, base = _proto(header, new), _proto(header, old)
        res, table = _lib.SIGNATURES[new]
        assert res is C.c_int and [ctype[t] for t in table] == [kind(a) for a in args], new
        i = next(n for n, a in enumerate(args) if a == "int precision")
        assert args[:i] + args[i + 1:] == base and args[i - 1] == "float scale", new      # the old prototype with `precision` after `scale`
    assert "#define OFX_PREC_FP32 0" in re.sub(r" +", " ", header) and "#define OFX_PREC_F16 5" in re.sub(r" +", " ", header)
    lib = _lib.lib()
    # argument validation precedes every HIP call: testable without a device
    assert lib.ofx_attention_prec(None, None, None, None, 0, None, 1, 1, 1, 40, 1.0, 5, None, 0, None) == TC.SC.EINVAL
    assert lib.ofx_attention_bnhd_prec(None, 40, None, 40, None, 40, None, 0, None, 40, 1, 1, 1, 1, 40, 1.0, 5, None) == TC.SC.EINVAL
    buf = (C.c_float * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)
    for prec in (1, 2, 3, 4, 6, -1):
        assert lib.ofx_attention_prec(p, p, p, None, 0, p, 1, 1, 1, 40, 1.0, prec, None, 0, None) == TC.SC.EINVAL
        assert lib.ofx_attention_bnhd_prec(p, 40, p, 40, p, 40, None, 0, p, 40, 1, 1, 1, 1, 40, 1.0, prec, None) == TC.SC.EINVAL
    assert lib.ofx_attention_prec(p, p, p, None, 0, p, 1, 1, 1, 512, 1.0, 5, None, 0, None) == TC.SC.EINVAL
    assert lib.ofx_attention_bnhd_prec(p, 512, p, 512, p, 512, None, 0, p, 512, 1, 1, 1, 1, 512, 1.0, 5, None) == TC.SC.EINVAL
    assert lib.ofx_attention_bnhd_prec(p, 36, p, 40, p, 40, None, 0, p, 40, 1, 1, 1, 1, 40, 1.0, 5, None) == TC.SC.EINVAL      # ld < H * D


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: resources

# flash_attn_kernel<D, BK, STRIDED> on the commit before the fp16 kernel was added, read from a build of that commit:
# (D, STRIDED) -> (VGPRs, AGPRs, LDS [static bytes: the tiles are dynamic], Occupancy)
FP32_ROWS = {
    (40, True): (166, 32, 0, 2), (64, True): (134, 32, 0, 3), (80, True): (186, 64, 0, 2), (128, True): (240, 80, 0, 1), (160, True): (256, 128, 0, 1),
    (40, False): (127, 32, 0, 3), (64, False): (128, 32, 0, 3), (80, False): (160, 64, 0, 2), (128, False): (226, 80, 0, 1), (160, False): (254, 112, 0, 1),
}
F16_OCCUPANCY = 2                  # __launch_bounds__(256, 2)


@pytest.mark.skipif(not HIPCC, reason="no hipcc")
def test_resources_of_both_kernel_families():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kres
    finally:
        sys.path.pop(0)
    src = os.path.join(ROOT, "sd_animation_optical_flow_amd", "csrc", "attn_flash.hip")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
           os.devnull, kres.REMARKS]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = kres.parse_remarks(out.stderr)
    key = lambda r: tuple(int(v) if v.isdigit() else v == "1" for v in re.search(r"ILi(\d+)ELi\d+ELb([01])E", r["name"]).groups())
    fp32 = {key(r): r for r in rows if "flash_attn_kernel" in r["name"]}
    half = {key(r): r for r in rows if "flash_attn_f16_kernel" in r["name"]}
    assert sorted(fp32) == sorted(half) == sorted(FP32_ROWS) and len(rows) == 20
    for k, r in sorted(half.items()):
        print(f"fp16 D {k[0]} strided {k[1]}: vgpr {r['VGPRs']} agpr {r['AGPRs']} lds {r['LDS']} scratch {r['ScratchSize']} occupancy {r['Occupancy']}")
        assert r["ScratchSize"] == 0 and r["Occupancy"] >= F16_OCCUPANCY and r["VGPRs"] + r["AGPRs"] <= 512 // F16_OCCUPANCY, (k, r)
    for k, r in sorted(fp32.items()):
        assert (r["VGPRs"], r["AGPRs"], r["LDS"], r["Occupancy"]) == FP32_ROWS[k] and r["ScratchSize"] == 0, (k, r)
