"""The UNet on the device: `ofx_groupnorm_cat`, `ofx_emb_linear` and `ofx_timestep_embedding` against float64 with the bounds of
tests/unet_check.py (every element), ResBlocks alone and the whole model on configuration u0 against the float64 restatement with
the bar of four times the reference's own distance (tests/golden/unet_ref_u0.npz).  Every test prints its figures (-s)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sd_ops_check as SC   # noqa: E402
import transformer_check as TC   # noqa: E402
import unet_check as UC   # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "unet_ref_u0.npz")


@pytest.fixture(scope="module")
def ops(cuda):
    from sd_animation_optical_flow_amd import ops as O
    return O


# ---------------------------------------------------------------------------------------------------------------------------------
# groupnorm_cat

def _wide(t, pad=4):
    """t [B,HW,C] -> the same values as a channel slice of a wider device tensor whose other columns hold NaN."""
    B, HW, Cn = t.shape
    w = torch.full((B, 1, HW, Cn + 2 * pad), float("nan"), device="cuda")
    w[..., pad:pad + Cn] = t.cuda().view(B, 1, HW, Cn)
    return w[..., pad:pad + Cn]


@pytest.mark.parametrize("c", UC.GNC_CASES, ids=[c["name"] for c in UC.GNC_CASES])
def test_groupnorm_cat_against_float64(ops, c):
    x0, x1, e, gamma, beta = UC.gnc_input(c)
    x, ref = UC.gnc_reference(x0, x1, e, gamma, beta, c["groups"])
    B, HW, C0 = x0.shape
    if c["kind"] == "nan_slices":
        d0, d1 = _wide(x0), _wide(x1, 8)
        de = torch.full((B, x.shape[2] + 12), float("nan"), device="cuda")
        de[:, 8:8 + x.shape[2]] = e.cuda()
        de = de[:, 8:8 + x.shape[2]]
        assert not d0.is_contiguous() and not de.is_contiguous()
    else:
        d0 = x0.cuda().view(B, 1, HW, C0)
        d1 = None if x1 is None else x1.cuda().view(B, 1, HW, -1)
        de = None if e is None else e.cuda()
    out = ops.groupnorm_cat(d0, d1, gamma.cuda(), beta.cuda(), e=de, groups=c["groups"], eps=UC.GN_EPS, silu=c["silu"],
                            out=d0 if c["kind"] == "alias" else None)
    if c["kind"] == "alias":
        assert out.data_ptr() == d0.data_ptr()
    got = out.cpu().view(B, HW, -1)
    assert bool(torch.isfinite(got).all())
    worst, used = SC.gn_ratios(got, x, ref, c["silu"])
    print(f"{c['name']}: |error| / bound {worst:.3f}, measured-term use {used:.3f}")
    assert worst <= 1.0
    if x1 is None and e is None:                                   # one dense segment, no e: the bits of ofx_groupnorm
        same = ops.groupnorm(x0.cuda().view(B, 1, HW, C0), gamma.cuda(), beta.cuda(), c["groups"], UC.GN_EPS, c["silu"])
        assert torch.equal(same, out)


def test_groupnorm_cat_rejects_before_any_launch(ops):
    from sd_animation_optical_flow_amd import _lib
    L = _lib.lib()
    B, HW, C0, C1 = 2, 8, 64, 32
    POISON = 7.25
    x0 = torch.randn((B, HW, C0 + 4), device="cuda")
    x1 = torch.randn((B, HW, C1), device="cuda")
    e = torch.randn((B, C0 + C1), device="cuda")
    out = torch.full((B, HW, C0 + C1 + 4), POISON, device="cuda")
    need = L.ofx_groupnorm_cat_scratch_bytes(B, C0 + C1)
    scratch = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(x0p=None, ld0=C0, c0=C0, x1p="x1", ld1=C1, c1=C1, ep="e", lde=C0 + C1, outp=None, sp=None, sbytes=need, b=B, groups=32):
        return L.ofx_groupnorm_cat(p(x0) if x0p is None else x0p, ld0, c0, p(x1) if x1p == "x1" else x1p, ld1, c1, p(e) if ep == "e" else ep,
                                   lde, None, None, p(out) if outp is None else outp, p(scratch) if sp is None else sp, sbytes, b, HW,
                                   groups, 1e-5, 1, None)

    cases = [
        ("groups do not divide C0 + C1", call(groups=5), SC.EINVAL),
        ("C0 % 4", call(c0=62, c1=34, ld1=36), SC.EALIGN),
        ("C1 % 4", call(c0=66, c1=30, ld0=68), SC.EALIGN),
        ("ld0 % 4", call(ld0=C0 + 2), SC.EALIGN),
        ("ld1 % 4", call(ld1=C1 + 2), SC.EALIGN),
        ("ld0 < C0", call(ld0=C0 - 4), SC.EINVAL),
        ("ld1 < C1", call(ld1=C1 - 4), SC.EINVAL),
        ("lde < C0 + C1", call(lde=C0), SC.EINVAL),
        ("x0 not 16-byte aligned", call(x0p=p(x0, 4)), SC.EALIGN),
        ("x1 not 16-byte aligned", call(x1p=p(x1, 8)), SC.EALIGN),
        ("e not 16-byte aligned", call(ep=p(e, 4)), SC.EALIGN),
        ("out not 16-byte aligned", call(outp=p(out, 4)), SC.EALIGN),
        ("scratch not 16-byte aligned", call(sp=p(scratch, 8)), SC.EALIGN),
        ("x1 NULL with C1 > 0", call(x1p=None), SC.EINVAL),
        ("x1 given with C1 = 0", call(c1=0, c0=C0 + C1, ld0=C0 + C1, groups=32), SC.EINVAL),
        ("x0 NULL", call(x0p=C.c_void_p(0)), SC.EINVAL),
        ("B > 65535", call(b=65536), SC.EINVAL),
        ("scratch too small", call(sbytes=need - 1), SC.ENOMEM),
        ("out aliases x0 with C1 > 0", call(outp=p(x0)), SC.EINVAL),
        ("out aliases x0 with ld0 != C0", call(x1p=None, c1=0, ld0=C0 + 4, lde=C0, outp=p(x0)), SC.EINVAL),
        ("out overlaps x1", call(outp=p(x1)), SC.EINVAL),
    ]
    torch.cuda.synchronize()
    for what, got, want in cases:
        assert got == want, (what, got, want)
    assert bool((out == POISON).all()) and bool((scratch == 0x5A).all())          # nothing was launched
    # the valid call on the same buffers runs
    assert call(ld0=C0 + 4) == 0
    torch.cuda.synchronize()
    assert not bool((out.view(-1)[:B * HW * (C0 + C1)] == POISON).any())
    with pytest.raises(RuntimeError):
        ops.groupnorm_cat(x0[..., :C0].reshape(B, 1, HW, C0), x1.view(B, 2, HW // 2, C1), None, None)


# ---------------------------------------------------------------------------------------------------------------------------------
# emb_linear, timestep_embedding

@pytest.mark.parametrize("K,N", [(320, 1280), (1280, 100), (36, 7)])
@pytest.mark.parametrize("B", [1, 2, 3, 16])
def test_emb_linear_against_float64(ops, B, K, N):
    g = SC._gen(f"emb-{B}-{K}-{N}")
    x = torch.randn((B, K), generator=g) * 1.5
    w = torch.randn((N, K), generator=g) / K ** 0.5
    bias = torch.randn((N,), generator=g) * 0.05
    for silu in (False, True):
        ref, bound = UC.emb_linear_reference(x, w, bias, silu)
        ldo = N + 5
        wide = torch.full((B, ldo), -3.5, device="cuda")
        out = ops.emb_linear(x.cuda(), w.cuda(), bias.cuda(), silu_in=silu, out=wide[:, :N])
        assert out.data_ptr() == wide.data_ptr()
        assert bool((wide[:, N:] == -3.5).all())                   # the gap is left alone
        r = SC._worst((wide[:, :N].cpu().double() - ref).abs(), bound)
        again = ops.emb_linear(x.cuda(), w.cuda(), bias.cuda(), silu_in=silu)
        assert torch.equal(again, wide[:, :N])
        print(f"emb_linear B {B} K {K} N {N} silu {silu}: |error| / bound {r:.4f}")
        assert r <= 1.0
    nb, _ = UC.emb_linear_reference(x, w, None, False)
    assert SC._worst((ops.emb_linear(x.cuda(), w.cuda()).cpu().double() - nb).abs(), UC.emb_linear_reference(x, w, None, False)[1]) <= 1.0


def test_emb_linear_row_limit(ops):
    from sd_animation_optical_flow_amd import _lib
    g = SC._gen("emb-17")
    x, w = torch.randn((17, 36), generator=g).cuda(), torch.randn((7, 36), generator=g).cuda()
    out = torch.full((17, 7), 9.0, device="cuda")
    fn = _lib.lib().ofx_emb_linear
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert fn(p(x), 36, p(w), None, p(out), 7, 17, 36, 7, 0, None) == SC.EINVAL
    assert fn(p(x), 36, p(w), None, p(out), 6, 2, 36, 7, 0, None) == SC.EINVAL          # ldo < N
    assert fn(p(x), 36, p(w), None, p(out), 7, 2, 34, 7, 0, None) == SC.EALIGN          # K % 4
    assert fn(p(x, 4), 36, p(w), None, p(out), 7, 2, 36, 7, 0, None) == SC.EALIGN
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())
    ref, bound = UC.emb_linear_reference(x.cpu(), w.cpu(), None, True)
    assert SC._worst((ops.emb_linear(x, w, silu_in=True).cpu().double() - ref).abs(), bound) <= 1.0     # the wrapper slices the rows


@pytest.mark.parametrize("dim", UC.TS_DIMS)
def test_timestep_embedding_against_float64(ops, dim):
    t = torch.tensor(UC.TS_T)
    ref, bound = UC.timestep_embedding_reference(t, dim)
    out = ops.timestep_embedding(t.cuda(), ops.timestep_freqs(dim).cuda(), dim).cpu()
    assert tuple(out.shape) == (len(UC.TS_T), dim)
    err = (out.double() - ref).abs()
    r = SC._worst(err[:, :2 * (dim // 2)], bound[:, :2 * (dim // 2)])
    print(f"timestep_embedding dim {dim}: |error| / bound {r:.3f}, worst |error| {float(err.max()) / UC.U:.2f} u")
    assert r <= 1.0
    if dim % 2:
        assert bool((out[:, -1] == 0).all())
    assert bool((out[0, :dim // 2] == 1).all()) and bool((out[0, dim // 2:] == 0).all())          # t = 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the model

@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def yard(gold):
    return {str(k): float(v) for k, v in zip(gold["dist_keys"], gold["ref_vs_f64"])}


@pytest.fixture(scope="module")
def u0(cuda):
    from sd_animation_optical_flow_amd import unet as UN
    sd = UN.random_unet_state_dict(0, UC.U0)
    model = UN.UNetModel(sd, UC.U0, prefix="")
    assert not model.torch_glue
    return UN, model, TC.to64(sd), model.layout


def _frames(gold, heads, mode):
    hist = [(torch.from_numpy(gold[f"k{i}"]), torch.from_numpy(gold[f"v{i}"])) for i in range(len(heads))]
    return UC.reference_frames(hist, heads, mode)


def _f64(frames, heads):
    return [[(TC.heads_last(k, h).double(), TC.heads_last(v, h).double()) for (k, v), h in zip(frames[0], heads)]]


@pytest.fixture(scope="module")
def refs64(gold, u0):
    """The float64 restatement of the five stored runs, computed once and left unchanged."""
    _, _, sd64, lay = u0
    heads = UC.transformer_heads(lay)
    x, t, ctx = (torch.from_numpy(gold[n]) for n in ("x", "timesteps", "context"))
    ctl = UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)
    out, hist = UC.unet64(sd64, lay, x, t, ctx)
    r = {"out": out}
    for i, ((k, v), h) in enumerate(zip(hist, heads)):
        r[f"k{i}"], r[f"v{i}"] = TC.heads_first(k, h), TC.heads_first(v, h)
    r["out_refall"] = UC.unet64(sd64, lay, x, t, ctx, reference_kv=_f64(_frames(gold, heads, "all"), heads))[0]
    r["out_refpos"] = UC.unet64(sd64, lay, x, t, ctx, reference_kv=_f64(_frames(gold, heads, "positive"), heads))[0]
    r["out_ctl"] = UC.unet64(sd64, lay, x, t, ctx, control=ctl)[0]
    r["out_ctl_mid"] = UC.unet64(sd64, lay, x, t, ctx, control=ctl, only_mid_control=True)[0]
    return r


def _hold(name, mine, ref64, yardstick):
    dist = float((mine.detach().cpu().double() - ref64).abs().max())
    print(f"{name}: device vs float64 {dist:.3e}; the reference's own fp32 module {yardstick:.3e}; bar {UC.bar4(yardstick):.3e}")
    assert dist <= UC.bar4(yardstick), (name, dist, UC.bar4(yardstick))


@pytest.mark.parametrize("ci", range(len(UC.RESBLOCK_CASES)), ids=[c[0] for c in UC.RESBLOCK_CASES])
def test_resblock_alone(u0, gold, yard, ci):
    _, model, sd64, _ = u0
    _, name, _, up = UC.RESBLOCK_CASES[ci]
    t = torch.from_numpy(gold["timesteps"])
    xb, skip = UC.resblock_inputs(ci)
    r = UC.resblock64(sd64, name, (xb if skip is None else torch.cat([xb, skip], 1)).double(), UC.time_embed64(sd64, t, UC.U0["model_channels"]))
    nhwc = lambda a: None if a is None else a.permute(0, 2, 3, 1).contiguous().cuda()
    emb_all = model.emb_projections(t.cuda())
    h = model.resblock(name, nhwc(xb), emb_all, nhwc(skip))
    if up is not None:
        r = UC.upsample64(sd64, up, r)
        h = model._block([("up", up, h.shape[3])], h, emb_all, None, None, [])
    _hold(f"rb{ci} {name}", h.permute(0, 3, 1, 2), r, yard[f"rb{ci}"])


def test_emb_projections_against_float64(u0, gold):
    """The timestep path on its own: timestep_embedding -> time_embed -> every emb_layers.1, held to the bounds' own composition: the
    last Linear's bound with the error of its input carried through |w|."""
    _, model, sd64, _ = u0
    t = torch.from_numpy(gold["timesteps"])
    emb = UC.time_embed64(sd64, t, UC.U0["model_channels"])
    got = model.emb_projections(t.cuda()).cpu().double()
    assert got.shape[1] == sum(n for _, n in model.emb_slice.values())
    worst = 0.0
    for name, (off, n) in model.emb_slice.items():
        ref = UC.silu64(emb) @ sd64[f"{name}.emb_layers.1.weight"].T + sd64[f"{name}.emb_layers.1.bias"]
        worst = max(worst, float((got[:, off:off + n] - ref).abs().max()))
    print(f"emb projections: device vs float64 {worst:.3e}")
    assert worst <= 2e-5              # three chained Linears of K <= 256 on values of order 1: u K |terms| ~ 1e-5 at the outside


def test_unet_plain_run_and_history(u0, gold, yard, refs64):
    UN, model, _, lay = u0
    heads = UC.transformer_heads(lay)
    x, t, ctx = (torch.from_numpy(gold[n]).cuda() for n in ("x", "timesteps", "context"))
    out, hist = model(x, t, ctx)
    assert tuple(out.shape) == (UC.U0_B, 4, UC.U0_H, UC.U0_W) and len(hist) == 7
    _hold("out", out, refs64["out"], yard["out"])
    from sd_animation_optical_flow_amd.transformer import to_reference_layout
    for i, ((k, v), h) in enumerate(zip(hist, heads)):
        assert k.is_cuda and k.dim() == 3 and k.shape[0] == UC.U0_B
        _hold(f"k{i}", to_reference_layout(k, h), refs64[f"k{i}"], yard[f"k{i}"])
        _hold(f"v{i}", to_reference_layout(v, h), refs64[f"v{i}"], yard[f"v{i}"])
    out2, hist2 = model(x, t, ctx)
    assert torch.equal(out, out2) and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(hist, hist2))
    nh, _ = model.forward_nhwc(x.permute(0, 2, 3, 1).contiguous(), t, ctx)
    assert torch.equal(nh.permute(0, 3, 1, 2), out)


def test_unet_reference_kv(u0, gold, yard, refs64):
    UN, model, _, lay = u0
    heads = UC.transformer_heads(lay)
    x, t, ctx = (torch.from_numpy(gold[n]).cuda() for n in ("x", "timesteps", "context"))
    plain, _ = model(x, t, ctx)
    fa, fp = _frames(gold, heads, "all"), _frames(gold, heads, "positive")
    n_before = [len(f) for f in fa]
    out_all, hist_all = model(x, t, ctx, reference_kv=fa)
    out_pos, _ = model(x, t, ctx, reference_kv=fp)
    assert [len(f) for f in fa] == n_before                          # not consumed
    _hold("out_refall", out_all, refs64["out_refall"], yard["out_refall"])
    _hold("out_refpos", out_pos, refs64["out_refpos"], yard["out_refpos"])
    assert not torch.equal(out_all, plain) and torch.equal(out_pos[0], plain[0]) and not torch.equal(out_pos[1], plain[1])
    # the other layout plan_reference_kv accepts, [b, n, heads * d] on the device: the same bits
    fb = [[(TC.heads_last(k, h).cuda(), TC.heads_last(v, h).cuda()) for (k, v), h in zip(fa[0], heads)]]
    assert torch.equal(model(x, t, ctx, reference_kv=fb)[0], out_all)
    # two reference frames: every transformer sees entry i of both
    two, _ = model(x, t, ctx, reference_kv=[fa[0], fa[0]])
    assert bool(torch.isfinite(two).all())
    with pytest.raises(ValueError, match="6 entries"):
        model(x, t, ctx, reference_kv=[fa[0][:6]])
    with pytest.raises(ValueError):
        model(x, t, ctx, reference_kv=[fa[0][:6] + [(fa[0][6][0][:, :5], fa[0][6][1][:, :5])], fp[0]])       # mixed batches


def test_unet_control(u0, gold, yard, refs64):
    _, model, _, lay = u0
    x, t, ctx = (torch.from_numpy(gold[n]).cuda() for n in ("x", "timesteps", "context"))
    ctl = [c.cuda() for c in UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)]
    keep = [c.clone() for c in ctl]
    out, _ = model(x, t, ctx, control=ctl)
    mid, _ = model(x, t, ctx, control=ctl, only_mid_control=True)
    assert len(ctl) == len(keep) and all(torch.equal(a, b) for a, b in zip(ctl, keep))      # neither consumed nor written to
    _hold("out_ctl", out, refs64["out_ctl"], yard["out_ctl"])
    _hold("out_ctl_mid", mid, refs64["out_ctl_mid"], yard["out_ctl_mid"])
    with pytest.raises(ValueError, match="control has"):
        model(x, t, ctx, control=ctl[:-1])
    with pytest.raises(ValueError, match=r"control\[2\]"):
        model(x, t, ctx, control=ctl[:2] + [ctl[2][:, :, :2]] + ctl[3:])


def test_unet_batch_one_and_input_rules(u0, gold, yard):
    _, model, sd64, lay = u0
    x, t, ctx = (torch.from_numpy(gold[n]) for n in ("x", "timesteps", "context"))
    ref, _ = UC.unet64(sd64, lay, x[:1], t[:1], ctx[:1])
    out, hist = model(x[:1].cuda(), t[:1].cuda(), ctx[:1].cuda())
    assert all(k.shape[0] == 1 for k, _ in hist)
    _hold("out, B = 1", out, ref, yard["out"])
    with pytest.raises(ValueError, match="multiples of 4"):
        model(torch.zeros((1, 9, 8, 10), device="cuda"), t[:1].cuda(), ctx[:1].cuda())
    with pytest.raises(RuntimeError):
        model(torch.zeros((1, 4, 8, 12), device="cuda"), t[:1].cuda(), ctx[:1].cuda())
    with pytest.raises(RuntimeError):
        model(x[:1].cuda(), t.cuda(), ctx[:1].cuda())


_CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import transformer_check as TC, unet_check as UC
from sd_animation_optical_flow_amd import unet as UN
from sd_animation_optical_flow_amd.transformer import to_reference_layout
g, refs = np.load(sys.argv[2]), np.load(sys.argv[3])
model = UN.UNetModel(UN.random_unet_state_dict(0, UC.U0), UC.U0, prefix="")
assert model.torch_glue
heads = UC.transformer_heads(model.layout)
x, t, ctx = (torch.from_numpy(g[n]).cuda() for n in ("x", "timesteps", "context"))
hist0 = [(torch.from_numpy(g[f"k{i}"]), torch.from_numpy(g[f"v{i}"])) for i in range(len(heads))]
ctl = [c.cuda() for c in UC.control_residuals(model.layout, UC.U0_B, UC.U0_H, UC.U0_W)]
out, hist = model(x, t, ctx)
res = {"out": out}
for i, ((k, v), h) in enumerate(zip(hist, heads)):
    res[f"k{i}"], res[f"v{i}"] = to_reference_layout(k, h), to_reference_layout(v, h)
res["out_refall"] = model(x, t, ctx, reference_kv=UC.reference_frames(hist0, heads, "all"))[0]
res["out_refpos"] = model(x, t, ctx, reference_kv=UC.reference_frames(hist0, heads, "positive"))[0]
res["out_ctl"] = model(x, t, ctx, control=ctl)[0]
res["out_ctl_mid"] = model(x, t, ctx, control=ctl, only_mid_control=True)[0]
for name, mine in res.items():
    print("ERR %s %.9e" % (name, float((mine.cpu().double() - torch.from_numpy(refs[name])).abs().max())))
"""


def test_torch_glue_path_in_a_fresh_process(cuda, yard, refs64):
    """OFX_UNET_TORCH_GLUE=1 is read once per process, so the glue path (torch.cat + `ops.groupnorm`, the emb term as a torch add, the
    timestep path through torch.nn.functional) runs in a child: same float64 references, same bar."""
    env = dict(os.environ, OFX_UNET_TORCH_GLUE="1")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "refs64.npz")
        np.savez(path, **{k: v.numpy() for k, v in refs64.items()})
        r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(HERE), GOLD, path], env=env, capture_output=True, text=True,
                           timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("ERR ")]
    assert sorted(ln[1] for ln in lines) == sorted(refs64)
    for _, name, err in lines:
        print(f"glue path {name}: device vs float64 {float(err):.3e}; bar {UC.bar4(yard[name]):.3e}")
        assert float(err) <= UC.bar4(yard[name]), name
