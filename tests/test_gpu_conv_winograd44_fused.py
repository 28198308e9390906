"""The fused variants of the Winograd F(4x4,3x3) kernel (conv_wino.hip, wino44_fused_kernel<NORM, RES, STATS>; plan path 4): the
encoders' instance norm + ReLU on the operand, the residual merge and the epilogue statistics, at the smallest shapes at which
they can go wrong.

Shapes: 1x16x32, one patch, where every halo pixel of the border ring is padding, and 2x32x64, four patches per image: seams, and
the second image's mean / rstd and statistics rows.  Channels (Cin = Cout): 16, one trip of the two-slab loop with the prologue's
clamps; 48, three trips; 64; 96, a Cout tail whose second 64-block has an empty half.

Every case is forced with TILE_WINOGRAD4 and checked elementwise against float64 F.conv2d with the operand-scaled bound of
wino_check and K_F43 of wino44_check (the fused norm's operand in float64 from the fp32 mean / rstd the kernel is given; the
residual adds |res| to the magnitude).  It must differ from the F(2x2,3x3) result: the new kernel ran.  Largest ratio measured
on MI355X over this file's cases: 69.1 (norm, 64 channels, one patch), below the 72.5 K_F43 was set from, so K_F43 holds here
unchanged.  GPU tests are marked -m gpu.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino_check as wc  # noqa: E402
from wino44_check import K_F43, nchw, nhwc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 16, 32), (2, 32, 64)]
CHANNELS = [16, 48, 64, 96]
VARIANTS = ["norm", "res", "stats", "norm_stats", "norm_res"]


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


_CACHE = {}


def _case(shape, c, variant):
    """The case's CPU tensors, float64 reference and magnitude (computed once per case, never modified)."""
    key = (shape, c, variant)
    if key in _CACHE:
        return _CACHE[key]
    B, H, W = shape
    g = torch.Generator().manual_seed(1000 * c + 10 * H + VARIANTS.index(variant))
    w = torch.randn((c, c, 3, 3), generator=g) / np.sqrt(9 * c)
    norm, res, stats = "norm" in variant, "res" in variant, "stats" in variant
    d = dict(w=w, c=c, shape=shape, norm=norm, res=None, stats=stats, scale=None, relu=False)
    if norm:
        # channel means of either sign: where the mean is negative, normalising the padding instead of zeroing it would feed
        # relu(-mean * rstd) ~ 0.75 into every border tap
        off = torch.where(torch.arange(c) % 2 == 0, 1.5, -1.5).view(1, c, 1, 1)
        x = torch.randn((B, c, H, W), generator=g) * 2.0 + off
        mean = x.double().mean(dim=(2, 3)).float()
        rstd = (1.0 / torch.sqrt(x.double().var(dim=(2, 3), unbiased=False) + 1e-5)).float()
        xin = torch.relu((x.double() - mean.double().view(B, c, 1, 1)) * rstd.double().view(B, c, 1, 1))
        d.update(mean=mean, rstd=rstd)
    else:
        x = torch.randn((B, c, H, W), generator=g) + (0.5 if stats else 0.0)
        xin = x.double()
    d["x"] = x
    d["shift"] = torch.randn((c,), generator=g) * 0.1
    if res:   # cnet's conv2: folded scale / shift with ReLU, then relu(y + res)
        d["scale"] = 0.5 + torch.rand((c,), generator=g)
        d["relu"] = True
        d["res"] = torch.randn((B, c, H, W), generator=g)
    ref, mag = wc.reference(xin, w, 3, 3, scale=d["scale"], shift=d["shift"], relu=d["relu"])
    if res:
        ref, mag = torch.relu(ref + d["res"].double()), mag + d["res"].double().abs()
    d.update(ref=ref, mag=mag)
    _CACHE[key] = d
    return d


def _kw(ops, d):
    kw = dict(shift=d["shift"].cuda(), act="relu" if d["relu"] else None)
    if d["scale"] is not None:
        kw["scale"] = d["scale"].cuda()
    if d["norm"]:
        kw.update(nmean=d["mean"].cuda(), nrstd=d["rstd"].cuda())
    if d["res"] is not None:
        kw["res"] = nhwc(d["res"])
    return kw


def _run(ops, d, tile, part=None):
    w = d["w"]
    kw = _kw(ops, d)
    if part is not None:
        kw["stats_part"] = part
    return ops.conv2d_nhwc(nhwc(d["x"]), ops.pack_conv_weight(w).cuda(), 3, 3, d["c"], wino_w=ops.wino_conv_weight(w).cuda(),
                           wino4_w=ops.wino44_conv_weight(w).cuda(), tile=tile, **kw)


BORDERS = (("all", np.s_[:]), ("top", np.s_[:, :, 0]), ("bottom", np.s_[:, :, -1]), ("left", np.s_[:, :, :, 0]),
           ("right", np.s_[:, :, :, -1]))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=["one_patch", "four_patches"])
def test_forced_route_against_float64(cuda, shape, c, variant):
    ops = _ops()
    d = _case(shape, c, variant)
    B, H, W = shape
    rows = (H // 16) * (W // 32)
    need = B * rows * c * 2
    part = torch.full((need + 256,), float("nan"), device="cuda") if d["stats"] else None
    out = _run(ops, d, ops.TILE_WINOGRAD4, part)
    if d["stats"]:
        out, got_rows = out
        assert got_rows == rows
    got = nchw(out)
    for name, sl in BORDERS:   # (the four borders separately: a normalised padding shows there)
        ratio = wc.worst_ratio(got[sl], d["ref"][sl], d["mag"][sl])
        print(f"{variant} c={c} {shape} {name}: worst ratio {ratio:.3g} (K_F43 = {K_F43})")
    for name, sl in BORDERS:
        wc.check(got[sl], d["ref"][sl], d["mag"][sl], K_F43, f"{variant} {name}")
    # the F(2x2,3x3) kernel on the same descriptor: within its own bound, and another result
    f22 = _run(ops, d, ops.TILE_WINOGRAD, torch.empty((4 * need,), device="cuda") if d["stats"] else None)
    f22 = nchw(f22[0] if d["stats"] else f22)
    wc.check(f22, d["ref"], d["mag"], wc.K_F23, variant + " F(2x2)")
    assert not torch.equal(got, f22), "the F(4x4) kernel did not run"
    again_part = torch.full((need + 256,), float("nan"), device="cuda") if d["stats"] else None
    again = _run(ops, d, ops.TILE_WINOGRAD4, again_part)
    assert torch.equal(got, nchw(again[0] if d["stats"] else again)), "not bit-identical on a second call"
    if not d["stats"]:
        return
    # nothing behind [B][rows][Cout][2] (the 96-channel layers' second block computes 32 channels that do not exist)
    assert torch.isfinite(part[:need]).all() and torch.isnan(part[need:]).all()
    assert torch.equal(part[:need], again_part[:need]) and torch.isnan(again_part[need:]).all(), "partials differ on a repeat"
    # each row is its patch's own sums: against float64 sums of the kernel's output over that 16x32 patch
    o = got.double().view(B, c, H // 16, 16, W // 32, 32)
    ps = part[:need].double().cpu().view(B, H // 16, W // 32, c, 2)
    assert torch.allclose(ps[..., 0], o.sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3)
    assert torch.allclose(ps[..., 1], (o * o).sum(dim=(3, 5)).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-3)
    # Finalised mean / rstd against float64 of the reference.  The bounds follow from the elementwise one: an output is within
    # e = K_F43 2^-24 M of the reference, so the mean is within mean(e), and E[v^2] within mean(2 |ref| e + e^2); the fp32 sums
    # (chains of at most 48 values per lane, 24 half-waves, `rows` rows) add (72 + rows) 2^-24 of the summed magnitudes.  The
    # variance's error, relative to the variance, is twice rstd's.
    mean, rstd = ops.inorm_finalize(part[:need].clone(), B, rows, H * W, c)
    ref = d["ref"]
    e = K_F43 * wc.EPS * d["mag"]
    chain = (72 + rows) * wc.EPS
    rmean, rvar = ref.mean(dim=(2, 3)), ref.var(dim=(2, 3), unbiased=False)
    rrstd = 1.0 / torch.sqrt(rvar + 1e-5)
    tol_mean = e.mean(dim=(2, 3)) + chain * ref.abs().mean(dim=(2, 3))
    tol_sq = (2 * ref.abs() * e + e * e).mean(dim=(2, 3)) + chain * (ref * ref).mean(dim=(2, 3))
    tol_var = tol_sq + 2 * rmean.abs() * tol_mean + tol_mean * tol_mean
    err_mean = (mean.double().cpu() - rmean).abs()
    err_rstd = ((rstd.double().cpu() - rrstd) / rrstd).abs()
    print(f"mean error {err_mean.max().item():.3g} (bound {tol_mean.min().item():.3g}), rstd error {err_rstd.max().item():.3g} "
          f"(bound {(0.5 * tol_var / (rvar + 1e-5)).min().item():.3g})")
    assert bool((err_mean <= tol_mean).all())
    assert bool((err_rstd <= 0.5 * tol_var / (rvar + 1e-5) * 1.01).all())   # (1.01: the first-order term of 1 / sqrt)
    with pytest.raises(RuntimeError):   # statistics are of raw outputs only: with a residual merge the forced route is refused
        ops.conv2d_nhwc(nhwc(d["x"]), ops.pack_conv_weight(d["w"]).cuda(), 3, 3, c, wino4_w=ops.wino44_conv_weight(d["w"]).cuda(),
                        tile=ops.TILE_WINOGRAD4, stats_part=part, res=out, **_kw(ops, d))


_ENGINE_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd.raft import RaftEngine
from sd_animation_optical_flow_amd.weights import random_state_dict
B, H, W = 4, 512, 768
g = torch.Generator().manual_seed(5)
base = torch.rand((1, 3, H + 32, W + 32), generator=g)
base = torch.nn.functional.conv2d(base, torch.ones((3, 1, 5, 5)) / 25.0, padding=2, groups=3)
base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)[0].permute(1, 2, 0)
key = base[16:16 + H, 16:16 + W].contiguous().cuda()
frames = torch.stack([base[16 + (b % 5) - 2:16 + (b % 5) - 2 + H, 16 + (3 * b % 7) - 3:16 + (3 * b % 7) - 3 + W] for b in range(B)])
frames = frames.contiguous().cuda()
out = []
for norm in ("eval", "batch"):
    eng = RaftEngine(random_state_dict(0), "cuda", cnet_norm=norm)
    a = eng.forward(frames, key, iters=2).cpu().numpy()
    b = eng.forward(frames, key, iters=2).cpu().numpy()
    assert np.array_equal(a, b), norm   # the epilogue statistics are deterministic: a repeat is bit-identical
    out.append(a)
    if norm == "eval":   # the feature encoder's output for the frames: fnet has no plain 3x3 layer, every one of its routed layers is fused
        np.save(sys.argv[3], eng.buffer("fmap1").cpu().numpy())
np.save(sys.argv[2], np.stack(out))
"""


@pytest.mark.gpu
def test_engine_flow_with_and_without_the_fused_route(cuda, tmp_path):
    """Four 512x768 pairs, 2 iterations: the encoders' layer1 (768 + 192 workgroups of a 16x32 patch) takes the fused F(4x4,3x3)
    kernels, the update block's layers stay below their gate.  OFX_CONV_NO_WINOGRAD4 (read once per process, hence child
    processes) keeps F(2x2,3x3); the flows differ by less than the project's bar for a route, in both cnet_norm modes.  The
    flow alone would also move through cnet's plain conv1 layers, which take the plain kernel (path 3) under the same switch; the
    feature maps of fnet, whose routed layers all carry a fused norm or statistics, move only if the fused variants ran."""
    def run(tag, extra):
        env = {k: v for k, v in os.environ.items() if not k.startswith("OFX_CONV_NO_WINOGRAD")}
        env.update(extra)
        path = str(tmp_path / f"{tag}.npy")
        fmap = str(tmp_path / f"{tag}_fmap1.npy")
        out = subprocess.run([sys.executable, "-c", _ENGINE_SCRIPT, ROOT, path, fmap], env=env, capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return np.load(path), np.load(fmap)

    f44, fm44 = run("f44", {})
    f22, fm22 = run("f22", {"OFX_CONV_NO_WINOGRAD4": "1"})
    assert np.isfinite(f44).all() and np.isfinite(fm44).all()
    dfm = np.abs(fm44 - fm22).max()
    print(f"fnet: max |fmap1(F(4x4)) - fmap1(F(2x2))| = {dfm:.3g} (max |fmap1| {np.abs(fm22).max():.3g})")
    assert dfm > 0, "fnet's layers did not take the fused F(4x4) kernels"
    for k, norm in enumerate(("eval", "batch")):
        d = np.abs(f44[k] - f22[k]).max()
        print(f"cnet_norm={norm}: max |flow(F(4x4)) - flow(F(2x2))| = {d:.3g} px")
    for k, norm in enumerate(("eval", "batch")):
        d = np.abs(f44[k] - f22[k]).max()
        assert 0 < d < 1e-4, (norm, d)
