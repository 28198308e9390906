"""Reference K/V read in place by `SpatialTransformer` and `UNetModel`, and `kv_dtype=`, on the device.

`runs()` executes one fixed set of calls on the small transformer of tests/test_gpu_transformer.py ("ctx": 64 channels, 2 heads of
40) and on the UNet configuration u0 of unet_check (head sizes 64, 128 and an unfused 192): a plain call, a two-entry
`reference_kv` in "all" mode and one in "positive" mode.  The test process runs it on the segment route; a fresh child process runs
it with OFX_ST_KV_CONCAT=1 (the switch is read once per process), and every output and every K/V history of the two arms must be
BITWISE equal.  The `kv_dtype="fp16"` tests then hold the recorded history against the fp32 history rounded, and the outputs of
feeding a half history against those of feeding its fp32 original (fp16 attention: the same rounding, once) or its widened copy
(fp32 attention: an exact conversion)."""
import os
import subprocess
import sys

import pytest
import torch

import unet_check as UC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ST_CFG = (64, 2, 40, 32)            # channels, heads, d_head, context_dim: SMALL["ctx"] of test_gpu_transformer.py
ST_SEED = 3


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _st_inputs():
    g = torch.Generator().manual_seed(77)
    Cn, _, _, ctx = ST_CFG
    x = torch.randn((2, Cn, 6, 5), generator=g)
    x2 = torch.randn((2, Cn, 4, 3), generator=g)
    return x.cuda(), x2.cuda(), torch.randn((2, 7, ctx), generator=g).cuda()


def _st(**kw):
    from sd_animation_optical_flow_amd import transformer as T
    Cn, heads, d, ctx = ST_CFG
    return T.SpatialTransformer(T.random_spatial_transformer_state_dict(ST_SEED, Cn, heads, d, ctx), heads, d, **kw)


def _st_refs(hist, hist2, cast=lambda t: t):
    """Two entries of 30 and 12 tokens at batch 2 ("all"); two of 18 and 12 at batch 1, N = 30 in total ("positive")."""
    (k, v), (k2, v2) = hist[0], hist2[0]
    ref_all = [(cast(k), cast(v)), (cast(k2), cast(v2))]
    ref_pos = [(cast(k[:1, :18].contiguous()), cast(v[:1, :18].contiguous())), (cast(k2[:1].contiguous()), cast(v2[:1].contiguous()))]
    return ref_all, ref_pos


def _u0(**kw):
    from sd_animation_optical_flow_amd import unet as UN
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # attention_precision="fp16" names the 192-wide middle head it keeps at fp32
        return UN.UNetModel(UN.random_unet_state_dict(0, UC.U0), UC.U0, prefix="", **kw)


def _u0_refs(kvA, kvB, cast=lambda t: t):
    """Frames A and B at batch 2 ("all"); at batch 1 the first half of A's tokens and the second half of B's, N in total
    ("positive"), per transformer."""
    ref_all = [[(cast(k), cast(v)) for k, v in kvA], [(cast(k), cast(v)) for k, v in kvB]]
    half = lambda t, lo: cast((t[:1, :t.shape[1] // 2] if lo else t[:1, t.shape[1] // 2:]).contiguous())
    ref_pos = [[(half(k, True), half(v, True)) for k, v in kvA], [(half(k, False), half(v, False)) for k, v in kvB]]
    return ref_all, ref_pos


def runs():
    """name -> CPU tensor, for both arms."""
    out = {}

    def keep(name, y, hist):
        out[name] = y.cpu()
        for i, (k, v) in enumerate(hist):
            out[f"{name}.k{i}"], out[f"{name}.v{i}"] = k.cpu(), v.cpu()

    mod = _st()
    x, x2, ctx = _st_inputs()
    y, hist = mod(x, ctx)
    _, hist2 = mod(x2, ctx)
    keep("st.plain", y, hist)
    ref_all, ref_pos = _st_refs(hist, hist2)
    keep("st.all", *mod(x, ctx, reference_kv=ref_all))
    keep("st.positive", *mod(x, ctx, reference_kv=ref_pos))
    out["st.kv_concat"] = torch.tensor(int(mod.kv_concat))

    model = _u0()
    ux, ut, uctx = (t.cuda() for t in UC.u0_inputs())
    eps, kvA = model(ux, ut, uctx)
    _, kvB = model(ux * 0.5 + 0.1, ut, uctx)
    keep("u0.plain", eps, kvA)
    u_all, u_pos = _u0_refs(kvA, kvB)
    keep("u0.all", *model(ux, ut, uctx, reference_kv=u_all))
    keep("u0.positive", *model(ux, ut, uctx, reference_kv=u_pos))
    return out


_CHILD = r"""
import os, sys
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_kv_history as M
torch.save(M.runs(), sys.argv[2])
"""


@pytest.fixture(scope="module")
def arms(cuda, tmp_path_factory):
    """(this process on the segment route, a fresh child with OFX_ST_KV_CONCAT=1)."""
    assert not os.environ.get("OFX_ST_KV_CONCAT") and not os.environ.get("OFX_ST_TORCH_GLUE")
    path = str(tmp_path_factory.mktemp("kv") / "concat.pt")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(HERE), path], env=dict(os.environ, OFX_ST_KV_CONCAT="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return runs(), torch.load(path)


@pytest.mark.parametrize("model", ["st", "u0"])
@pytest.mark.parametrize("mode", ["plain", "all", "positive"])
def test_segment_route_is_bitwise_the_concatenation_route(arms, model, mode):
    """Output and kv_hists of the same call, with the two-entry reference_kv attended in place and under OFX_ST_KV_CONCAT=1."""
    mine, base = arms
    assert int(mine["st.kv_concat"]) == 0 and int(base["st.kv_concat"]) == 1, "the switch did not reach exactly one arm"
    names = [n for n in mine if n.startswith(f"{model}.{mode}")]
    assert sorted(names) == sorted(n for n in base if n.startswith(f"{model}.{mode}")) and len(names) >= 3
    for n in names:
        assert mine[n].dtype == torch.float32 and torch.equal(_bits(mine[n]), _bits(base[n])), n
    if mode != "plain":
        assert not torch.equal(mine[f"{model}.{mode}"], mine[f"{model}.plain"]), "the references changed nothing"


def test_the_routes_the_models_take(cuda):
    """What `plan_kv_route` answers for the calls of `runs()`: segments at the fused head sizes, the concatenation path at u0's
    192-wide middle head."""
    from sd_animation_optical_flow_amd import transformer as T
    mod = _st()
    assert not mod.kv_concat and mod.fused_attention
    x, x2, ctx = _st_inputs()
    _, hist = mod(x, ctx)
    _, hist2 = mod(x2, ctx)
    for cast, want_pos in ((lambda t: t, "segments"), (lambda t: t.half(), "segments+own")):
        ref_all, ref_pos = _st_refs(hist, hist2, cast)
        assert mod._reference_kv(ref_all, 2, 30)[:2] == ("all", "segments")
        assert mod._reference_kv(ref_pos, 2, 30)[:2] == ("positive", want_pos)
    mixed = [_st_refs(hist, hist2)[0][0], _st_refs(hist, hist2, lambda t: t.half())[0][1]]
    mode, route, (k, v) = mod._reference_kv(mixed, 2, 30)
    assert (mode, route) == ("all", "concat") and k.dtype == torch.float32 and tuple(k.shape) == (2, 42, 80)
    assert T.plan_kv_route("all", [torch.float32] * 4, [False, False], 2, 192) == "concat"


def test_the_plan_kept_between_calls_follows_the_tensors(cuda):
    """`_reference_kv` keeps the previous call's plan while every entry is the very same tensor (a sampler's 30 calls per frame):
    a repeated call is bitwise the first, values changed in place are read, and another tensor -- a clone, another dtype, another
    mode -- is planned afresh and gives what a new module gives."""
    mod = _st()
    x, x2, ctx = _st_inputs()
    _, hist = mod(x, ctx)
    _, hist2 = mod(x2, ctx)
    ref_all, ref_pos = _st_refs(hist, hist2)
    first, _ = mod(x, ctx, reference_kv=ref_all)
    assert mod._kv_memo is not None
    again, _ = mod(x, ctx, reference_kv=ref_all)
    assert torch.equal(_bits(again), _bits(first))
    fresh = lambda refs: _st()(x, ctx, reference_kv=refs)[0]
    ref_all[1][0].mul_(2.0)                                        # in place: the same tensor, new values
    changed, _ = mod(x, ctx, reference_kv=ref_all)
    assert not torch.equal(changed, first) and torch.equal(_bits(changed), _bits(fresh(ref_all)))
    other = [(ref_all[0][0].clone() * 0.5, ref_all[0][1]), ref_all[1]]              # another tensor in the first entry
    assert torch.equal(_bits(mod(x, ctx, reference_kv=other)[0]), _bits(fresh(other)))
    halves = [(k.half(), v.half()) for k, v in ref_all]
    assert torch.equal(_bits(mod(x, ctx, reference_kv=halves)[0]), _bits(fresh(halves)))
    assert torch.equal(_bits(mod(x, ctx, reference_kv=ref_pos)[0]), _bits(fresh(ref_pos)))
    assert torch.equal(_bits(mod(x, ctx, reference_kv=ref_pos)[0]), _bits(fresh(ref_pos)))      # "positive" kept too: image 0's row is per call
    del other, halves
    assert torch.equal(_bits(mod(x, ctx)[0]), _bits(_st()(x, ctx)[0]))


def test_kv_dtype_fp16_records_the_fp32_history_rounded(arms):
    mine, _ = arms
    x, _, ctx = _st_inputs()
    y, hist = _st(kv_dtype="fp16")(x, ctx)
    assert torch.equal(_bits(y.cpu()), _bits(mine["st.plain"]))                               # the block's own attention reads fp32
    assert len(hist) == 1
    for t, name in zip(hist[0], ("st.plain.k0", "st.plain.v0")):
        assert t.dtype == torch.float16 and t.is_contiguous() and torch.equal(_bits(t.cpu()), _bits(mine[name].half())), name
    ux, ut, uctx = (t.cuda() for t in UC.u0_inputs())
    model = _u0(kv_dtype="fp16")
    assert model.kv_dtype == "fp16" and all(st.kv_dtype == "fp16" for st in model.st.values())
    eps, kv = model(ux, ut, uctx)
    assert torch.equal(_bits(eps.cpu()), _bits(mine["u0.plain"])) and len(kv) == model.n_transformers
    for i, (k, v) in enumerate(kv):
        for t, name in ((k, f"u0.plain.k{i}"), (v, f"u0.plain.v{i}")):
            assert t.dtype == torch.float16 and torch.equal(_bits(t.cpu()), _bits(mine[name].half())), name


@pytest.mark.parametrize("mode", ["all", "positive"])
def test_fp16_attention_reads_a_half_history_like_its_fp32_original(cuda, mode):
    """attention_precision="fp16": the kernel rounds a float32 history to half as it stages it, and stages a half history as it
    is -- one rounding either way, so the outputs agree bitwise.  (u0 itself cannot show this: its 192-wide middle head keeps fp32
    attention, where a half history is its widened copy and not its original; the next test runs a UNet whose heads are all fused.)"""
    mod = _st(attention_precision="fp16")
    x, x2, ctx = _st_inputs()
    _, hist = mod(x, ctx)
    _, hist2 = mod(x2, ctx)
    pick = 0 if mode == "all" else 1
    y32, _ = mod(x, ctx, reference_kv=_st_refs(hist, hist2)[pick])
    y16, _ = mod(x, ctx, reference_kv=_st_refs(hist, hist2, lambda t: t.half())[pick])
    assert torch.equal(_bits(y16), _bits(y32))
    plain, _ = mod(x, ctx)
    assert not torch.equal(y32, plain)


U_FUSED = dict(UC.U0, channel_mult=(1, 2, 2))          # u0 with a 128-wide middle head: every transformer takes the fused kernel


@pytest.mark.parametrize("mode", ["all", "positive"])
def test_fp16_attention_unet_reads_a_half_history_like_its_fp32_original(cuda, mode):
    """The same on a UNet: u0 with channel_mult (1, 2, 2), whose head sizes (64, 128, 128 in the middle) are all fused, so every
    transformer runs fp16 attention and routes the half history through the segment table.  Also kv_dtype="fp16" end to end: the
    history this model records, fed back, gives the output of feeding the fp32 model's history."""
    from sd_animation_optical_flow_amd import transformer as T
    from sd_animation_optical_flow_amd import unet as UN
    pick = 0 if mode == "all" else 1
    sd = UN.random_unet_state_dict(0, U_FUSED)
    m32 = UN.UNetModel(sd, U_FUSED, prefix="", attention_precision="fp16")
    m16 = UN.UNetModel(sd, U_FUSED, prefix="", attention_precision="fp16", kv_dtype="fp16")
    assert set(m32.attention_precision_of.values()) == {"fp16"} and all(st.d_head in T.FUSED_HEAD_SIZES for st in m32.st.values())
    ux, ut, uctx = (t.cuda() for t in UC.u0_inputs())
    _, kvA = m32(ux, ut, uctx)
    _, kvB = m32(ux * 0.5 + 0.1, ut, uctx)
    _, hA = m16(ux, ut, uctx)
    _, hB = m16(ux * 0.5 + 0.1, ut, uctx)
    assert all(k.dtype == torch.float16 and torch.equal(_bits(k), _bits(k32.half())) for (k, _), (k32, _) in zip(hA, kvA))
    e32, _ = m32(ux, ut, uctx, reference_kv=_u0_refs(kvA, kvB)[pick])
    e16, _ = m32(ux, ut, uctx, reference_kv=_u0_refs(kvA, kvB, lambda t: t.half())[pick])
    own, _ = m16(ux, ut, uctx, reference_kv=_u0_refs(hA, hB)[pick])
    plain, _ = m32(ux, ut, uctx)
    assert torch.equal(_bits(e16), _bits(e32)) and torch.equal(_bits(own), _bits(e32)) and not torch.equal(e32, plain)


@pytest.mark.parametrize("mode", ["all", "positive"])
def test_fp32_attention_reads_a_half_history_as_its_widened_copy(cuda, mode):
    """fp32 attention: feeding hist.half() equals feeding hist.half().float(), on the transformer and on u0 (whose middle head
    widens on the concatenation path)."""
    pick = 0 if mode == "all" else 1
    mod = _st()
    x, x2, ctx = _st_inputs()
    _, hist = mod(x, ctx)
    _, hist2 = mod(x2, ctx)
    y16, _ = mod(x, ctx, reference_kv=_st_refs(hist, hist2, lambda t: t.half())[pick])
    yw, _ = mod(x, ctx, reference_kv=_st_refs(hist, hist2, lambda t: t.half().float())[pick])
    y32, _ = mod(x, ctx, reference_kv=_st_refs(hist, hist2)[pick])
    assert torch.equal(_bits(y16), _bits(yw)) and not torch.equal(y16, y32)
    model = _u0()
    ux, ut, uctx = (t.cuda() for t in UC.u0_inputs())
    _, kvA = model(ux, ut, uctx)
    _, kvB = model(ux * 0.5 + 0.1, ut, uctx)
    e16, _ = model(ux, ut, uctx, reference_kv=_u0_refs(kvA, kvB, lambda t: t.half())[pick])
    ew, _ = model(ux, ut, uctx, reference_kv=_u0_refs(kvA, kvB, lambda t: t.half().float())[pick])
    assert torch.equal(_bits(e16), _bits(ew))
