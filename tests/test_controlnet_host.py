"""ControlNet without a device: the tensor list against the reference's, the float64 restatement against the reference's outputs,
`make_hint`'s value rules, `apply_multi_controlnet`'s weights, windows and caching, and the refusals of `ofx_conv3x3_silu`.
Fixture: tests/golden/controlnet_ref_c0.npz (tests/golden/make_golden_controlnet.py, the reference's own module on the CPU)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import controlnet_check as CC
import sd_ops_check as SC
import transformer_check as TC
from sd_animation_optical_flow_amd import _lib, controlnet as CN
from sd_animation_optical_flow_amd.unet import SD_V15_UNET, unet_tensors

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "controlnet_ref_c0.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dist(gold):
    return dict(zip([str(k) for k in gold["dist_keys"]], [float(v) for v in gold["ref_vs_f64"]]))


def test_c0_tensors_are_the_reference_modules(gold):
    want = [(str(n), tuple(int(v) for v in s[:d])) for n, s, d in zip(gold["names"], gold["shapes"], gold["ndims"])]
    got = CN.controlnet_tensors(CC.C0)
    assert got == want
    assert len(got) == 172 and abs(sum(int(np.prod(s)) for _, s in got) / 1e6 - 4.50) < 0.005
    sd = CN.random_controlnet_state_dict(0, CC.C0)
    assert list(sd) == [k for k, _ in got] and all(tuple(sd[k].shape) == s for k, s in got)
    # the zero_module convolutions are not zeroed
    for k in ("zero_convs.0.0.weight", "input_hint_block.14.weight", "middle_block_out.0.weight"):
        assert float(sd[k].abs().max()) > 0


def test_v15_trunk_is_the_unets_encoder_key_for_key():
    cn = dict(CN.controlnet_tensors(CN.SD_V15_CONTROLNET))
    trunk = [(k, s) for k, s in unet_tensors(dict(SD_V15_UNET, in_channels=4)) if k.startswith(("time_embed.", "input_blocks.", "middle_block."))]
    assert len(trunk) > 200
    for k, s in trunk:
        assert cn[k] == s, k
    own = [k for k in cn if k not in dict(trunk)]
    assert all(k.startswith(("zero_convs.", "input_hint_block.", "middle_block_out.")) for k in own)
    assert len(own) == 2 * (12 + 8 + 1)
    assert cn["input_hint_block.0.weight"] == (16, 3, 3, 3) and cn["input_hint_block.14.weight"] == (320, 256, 3, 3)
    assert cn["zero_convs.11.0.weight"] == (1280, 1280, 1, 1) and cn["middle_block_out.0.bias"] == (1280,)
    assert CN.SD_V15_CONTROLNET == dict(in_channels=4, hint_channels=3, model_channels=320, attention_resolutions=(4, 2, 1), num_res_blocks=2,
                                        channel_mult=(1, 2, 4, 4), num_heads=8, transformer_depth=1, context_dim=768, legacy=False)


def test_unbuilt_options_are_refused():
    for key, val in (("dims", 3), ("use_scale_shift_norm", True), ("resblock_updown", True), ("use_linear_in_transformer", True)):
        with pytest.raises(NotImplementedError):
            CN.controlnet_tensors(dict(CC.C0, **{key: val}))
    with pytest.raises(KeyError):
        CN.controlnet_tensors({k: v for k, v in CC.C0.items() if k != "hint_channels"})


def test_float64_restatement_reproduces_the_reference(gold, dist):
    x, hint, t, context = CC.c0_inputs()
    for k, v in (("x", x), ("timesteps", t), ("context", context)):
        assert np.array_equal(gold[k], v.numpy()), k
    assert int(gold["hint_seed"]) == CC.C0_SEED and float(gold["hint_sum"]) == float(hint.double().sum())
    lay = CN.controlnet_layout(CC.C0)
    results = []
    for seed, _, _, _ in CC.MIX_NETS:
        sd64 = TC.to64(CN.random_controlnet_state_dict(seed, CC.C0))
        outs, guided = CC.controlnet64(sd64, lay, x, hint, t, context)
        results.append(outs)
        if seed != 0:
            continue
        assert [tuple(o.shape) for o in outs] == CC.C0_SHAPES
        outs1, _ = CC.controlnet64(sd64, lay, x, hint[:1], t, context)
        pairs = [("guided_hint", guided)] + [(f"out{i}", o) for i, o in enumerate(outs)] + [(f"out{i}_hint1", o) for i, o in enumerate(outs1)]
        for name, r64 in pairs:
            d = float((torch.from_numpy(gold[name]).double() - r64).abs().max())
            print(f"  {name:12s} |reference - float64| {d:.3e}  stored {dist[name]:.3e}")
            assert d <= dist[name] * (1 + 1e-9) + 1e-12, name
    for p in CC.MIX_P:
        for i, m64 in enumerate(CC.mix64(results, p)):
            name = f"mix{int(round(p * 100))}_{i}"
            d = float((torch.from_numpy(gold[name]).double() - m64).abs().max())
            assert d <= dist[name] * (1 + 1e-9) + 1e-12, name


def test_make_hint_value_rules():
    edges = np.array([[0, 255, 7], [128, 1, 254]], dtype=np.uint8)
    for model in ("canny", "hed"):
        h = CN.make_hint(model, edges, {"low_threshold": 1, "high_threshold": 2}, device="cpu")
        assert h.dtype == torch.float32 and tuple(h.shape) == (1, 3, 2, 3)
        want = torch.from_numpy(edges).float() / 255.0
        assert all(torch.equal(h[0, c], want) for c in range(3))
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 13
    mask = np.array([[0, 127, 128], [255, 1, 200]], dtype=np.uint8)
    h = CN.make_hint("inpaint", img, {"mask": mask}, device="cpu")
    assert tuple(h.shape) == (1, 3, 2, 3) and h.dtype == torch.float32
    want = (torch.from_numpy(img).float() / 255.0).permute(2, 0, 1)
    under = torch.from_numpy(mask > 127)
    assert torch.equal(h[0][:, under], torch.full((3, int(under.sum())), -1.0))          # -1.0 exactly under the mask
    assert torch.equal(h[0][:, ~under], want[:, ~under])                                # v / 255 in fp32 elsewhere
    assert int(under.sum()) == 3                                                         # 127 is outside, 128 inside
    assert np.array_equal(img, np.arange(18, dtype=np.uint8).reshape(2, 3, 3) * 13)      # the caller's image is not written to
    with pytest.raises(KeyError):
        CN.make_hint("inpaint", img, {}, device="cpu")
    with pytest.raises(ValueError):
        CN.make_hint("canny", img, {}, device="cpu")
    with pytest.raises(NotImplementedError):
        CN.make_hint("depth", edges, {}, device="cpu")


class _CountingNet:
    def __init__(self, outs):
        self.outs, self.calls, self.hints = outs, 0, []

    def __call__(self, x, hint, t, ctx):
        self.calls += 1
        self.hints.append(hint)
        return [o.clone() for o in self.outs]


def test_apply_multi_controlnet_weights_windows_and_caching(gold):
    x, _, t, context = CC.c0_inputs()
    stored = [[torch.from_numpy(gold[f"{tag}out{i}"]) for i in range(7)] for tag in ("", "net1_")]
    edges = np.zeros((64, 96), dtype=np.uint8)
    fakes = [_CountingNet(r) for r in stored]
    nets = [CN.SingleControlNet(weight=w, model="canny", args={}, condition=edges, guidance_start=gs, guidance_end=ge, net=f)
            for (_, w, gs, ge), f in zip(CC.MIX_NETS, fakes)]
    for p in CC.MIX_P:
        mixed = CN.apply_multi_controlnet(x, t, context, p, nets)
        assert len(mixed) == 7
        for i, m in enumerate(mixed):
            name = f"mix{int(round(p * 100))}_{i}"
            d = float((m.double() - torch.from_numpy(gold[name]).double()).abs().max())
            # the reference's `r0 * w0 + r1 * w1` and `(r0 * w0).add_(r1, alpha=w1)` on the same fp32 residuals: three roundings each
            assert d <= 4 * SC.U * float(np.abs(gold[name]).max()), (name, d)
    assert [f.calls for f in fakes] == [1, 1]                      # the second call ran no net
    assert tuple(fakes[0].hints[0].shape) == (1, 3, 64, 96)
    assert CC.mix_weights(0.95) == [0.7, 0.0] and CC.mix_weights(0.5) == [0.7, 0.3]
    # the window's edges are inside it (`<` / `>` in :423)
    assert CN.control_weight(nets[1], 0.9) == 0.3 and CN.control_weight(nets[1], 0.0) == 0.3
    assert CN.control_weight(nets[1], 0.9000001) == 0.0
    edge = CN.apply_multi_controlnet(x, t, context, 0.9, nets)
    for i in range(7):                                             # both nets count at 0.9: the mix of p = 0.5
        assert torch.equal(edge[i], CN.apply_multi_controlnet(x, t, context, 0.5, nets)[i])
    nets[0].guidance_start = 0.25
    assert CN.control_weight(nets[0], 0.25) == 0.7 and CN.control_weight(nets[0], 0.2499) == 0.0
    off = CN.apply_multi_controlnet(x, t, context, 0.1, nets)      # net 0 outside its window: only net 1 is left
    assert all(float((o - stored[1][i] * 0.3).abs().max()) < 1e-6 for i, o in enumerate(off))
    # the returned list is fresh: writing to it leaves the cache alone
    before = nets[0].result[0].clone()
    off[0].add_(1.0)
    mixed[0].add_(1.0)
    assert torch.equal(nets[0].result[0], before) and [f.calls for f in fakes] == [1, 1]
    with pytest.raises(ValueError):
        CN.apply_multi_controlnet(x, t, context, 0.5, [CN.SingleControlNet(weight=1.0, model="canny", args={}, condition=edges)])


def test_conv_case_table_covers_what_the_issue_lists():
    cs = CC.CONV_CASES
    assert {c["cin_pad"] for c in cs} >= {4, 16, 32, 96, 256}
    assert {c["cout"] for c in cs} >= {16, 32, 96, 256, 320}
    assert {c["stride"] for c in cs} == {1, 2} and {c["B"] for c in cs} >= {1, 3} and {c["silu"] for c in cs} == {True, False}
    assert {(c["H"], c["W"]) for c in cs} >= {(1, 1), (3, 5), (9, 11), (17, 23), (16, 32)}
    assert any(c["cin"] == 3 for c in cs) and any(c["ldx"] > c["cin_pad"] and c["ldo"] > c["cout"] for c in cs)
    assert any(c["kind"] == "big" and c["silu"] for c in cs)
    assert any(c["stride"] == 2 and c["H"] % 2 and c["W"] % 2 and c["H"] > 1 for c in cs)
    assert len({c["name"] for c in cs}) == len(cs)
    big = next(c for c in cs if c["kind"] == "big")
    _, _, y = CC.conv_reference(*CC.conv_input(big), big)
    assert float(y.max()) > 90 and float(y.min()) < -90


@pytest.mark.parametrize("case", CC.CONV_CASES, ids=[c["name"] for c in CC.CONV_CASES])
def test_planted_bugs_exceed_the_bound(case):
    """The bound is tight enough to tell: a dropped bias, taps shifted by a column and stride-2 sampling of the odd phase, computed on
    the CPU in float64, each miss it; the float64 reference rounded to fp32 is inside it."""
    x, w, bias = CC.conv_input(case)
    ref, bound, _ = CC.conv_reference(x, w, bias, case)
    assert CC.worst_ratio(ref.float(), ref, bound) <= 1.0
    wrong = CC.conv_planted(x, w, bias, case)
    assert ("stride-2-odd-phase" in wrong) == (case["stride"] == 2 and case["H"] > 1)
    for name, bad in wrong.items():
        assert CC.worst_ratio(bad, ref, bound) > 1.0, name


def test_conv3x3_silu_refusals_need_no_device():
    f = _lib.lib().ofx_conv3x3_silu
    buf = (C.c_float * 4096)()
    a = (C.addressof(buf) + 15) // 16 * 16
    ok = dict(x=a, ldx=4, Cin=4, w=a, ldw=64, bias=None, out=a, ldo=16, Cout=16, B=1, H=4, W=4, stride=1, silu=1)

    def call(**kw):
        v = dict(ok, **kw)
        return f(v["x"], v["ldx"], v["Cin"], v["w"], v["ldw"], v["bias"], v["out"], v["ldo"], v["Cout"], v["B"], v["H"], v["W"], v["stride"],
                 v["silu"], None)

    for key in ("x", "w", "out"):
        assert call(**{key: None}) == SC.EINVAL, key
    assert call(stride=3) == SC.EINVAL and call(stride=0) == SC.EINVAL
    assert call(Cin=6, ldx=8) == SC.EINVAL
    assert call(Cout=8, ldo=8) == SC.EINVAL
    assert call(B=0) == SC.EINVAL and call(H=0) == SC.EINVAL and call(W=-1) == SC.EINVAL
    assert call(ldx=0) == SC.EINVAL and call(ldo=12) == SC.EINVAL and call(ldw=32) == SC.EINVAL
    assert call(B=1 << 16, H=1 << 8, W=1 << 8) == SC.EINVAL        # 2^32 pixels
    assert call(ldx=6) == SC.EALIGN                                # a misaligned leading dimension
    assert call(ldo=18) == SC.EALIGN and call(ldw=66) == SC.EALIGN
    assert call(x=a + 4) == SC.EALIGN and call(out=a + 8) == SC.EALIGN and call(w=a + 4) == SC.EALIGN
