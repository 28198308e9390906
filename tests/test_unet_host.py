"""Host side of the UNet (no GPU): the state-dict layout against the reference module's own key list, the float64 restatement
against the real module's stored outputs, the K/V routing, the error paths that need no device, and the arithmetic of
`ofx_groupnorm_cat` simulated in fp32 against its bound."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sd_ops_check as SC   # noqa: E402
import transformer_check as TC   # noqa: E402
import unet_check as UC   # noqa: E402

# float64 evaluations of the restatement on two hosts differ by the order of their BLAS sums: ~1e-15 on values of a few units
F64_NOISE = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "unet_ref_u0.npz"))


@pytest.fixture(scope="module")
def yard(gold):
    return {str(k): float(v) for k, v in zip(gold["dist_keys"], gold["ref_vs_f64"])}


@pytest.fixture(scope="module")
def u0():
    from sd_animation_optical_flow_amd import unet as UN
    sd = UN.random_unet_state_dict(0, UC.U0)
    return UN, sd, TC.to64(sd), UN.unet_layout(UC.U0)


def test_unet_tensors_are_the_reference_modules_keys(gold, u0):
    UN = u0[0]
    mine = UN.unet_tensors(UC.U0)
    names = [str(n) for n in gold["names"]]
    shapes = [tuple(int(v) for v in s[:n]) for s, n in zip(gold["shapes"], gold["ndims"])]
    assert [k for k, _ in mine] == names
    assert [s for _, s in mine] == shapes
    assert len(names) == 326 and abs(sum(int(np.prod(s)) for s in shapes) - 8.7e6) < 0.05e6
    lay = u0[3]
    assert UC.transformer_heads(lay) == [1] * 7
    assert sorted({l[4] for l in UN._layers(lay) if l[0] == "st"}) == [64, 128, 192]
    assert sorted({l[2] for l in UN._layers(lay) if l[0] == "res" and len(l) == 6}) == [128, 192, 320, 384]


def test_sd_v15_layout():
    from sd_animation_optical_flow_amd import unet as UN
    lay = UN.unet_layout(UN.SD_V15_UNET)
    layers = UN._layers(lay)
    st = [l for l in layers if l[0] == "st"]
    res = [l for l in layers if l[0] == "res"]
    assert len(st) == 16 and len(res) == 22
    assert all(l[3] == 8 for l in st) and sorted({l[4] for l in st}) == [40, 80, 160]
    assert len(lay["input"]) == 12 and len(lay["output"]) == 12
    tens = dict(UN.unet_tensors(UN.SD_V15_UNET))
    total = sum(l[3] for l in res)
    assert sum(s[0] for k, s in tens.items() if k.endswith("emb_layers.1.weight")) == total
    assert all(s == (s[0], 1280) for k, s in tens.items() if k.endswith("emb_layers.1.weight"))
    assert tens["input_blocks.0.0.weight"] == (320, 9, 3, 3) and tens["out.2.weight"] == (4, 320, 3, 3)
    assert tens["output_blocks.0.0.in_layers.0.weight"] == (2560,) and tens["output_blocks.5.0.in_layers.0.weight"] == (1920,)
    assert tens["output_blocks.9.0.skip_connection.weight"] == (320, 960, 1, 1)
    assert "output_blocks.2.1.conv.weight" in tens and "output_blocks.5.2.conv.weight" in tens and "input_blocks.3.0.op.weight" in tens
    assert abs(sum(int(np.prod(s)) for s in tens.values()) - 859.5e6) < 0.5e6          # the 860 M parameters of the v1.5 UNet


def _frames64(gold, heads, mode):
    hist = [(torch.from_numpy(gold[f"k{i}"]), torch.from_numpy(gold[f"v{i}"])) for i in range(len(heads))]
    fr = UC.reference_frames(hist, heads, mode)
    return [[(TC.heads_last(k, h).double(), TC.heads_last(v, h).double()) for (k, v), h in zip(fr[0], heads)]]


def test_float64_restatement_against_the_reference_module(gold, yard, u0):
    """Every stored output of the REAL modules within a quarter of the device's bar, i.e. within the yardstick itself."""
    _, _, sd64, lay = u0
    heads = UC.transformer_heads(lay)
    x, t, ctx = (torch.from_numpy(gold[n]) for n in ("x", "timesteps", "context"))
    xs, ts, cs = UC.u0_inputs()
    assert torch.equal(x, xs) and torch.equal(t, ts) and torch.equal(ctx, cs)
    ctl = UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)

    def check(name, mine):
        ref = torch.from_numpy(gold[name])
        dist = float((mine - ref.double()).abs().max())
        print(f"{name}: float64 restatement vs stored reference {dist:.3e}, yardstick {yard[name]:.3e}")
        assert dist <= UC.bar4(yard[name]) / 4 + F64_NOISE, (name, dist)

    out, hist = UC.unet64(sd64, lay, x, t, ctx)
    check("out", out)
    for i, ((k, v), h) in enumerate(zip(hist, heads)):
        check(f"k{i}", TC.heads_first(k, h))
        check(f"v{i}", TC.heads_first(v, h))
    out_all = UC.unet64(sd64, lay, x, t, ctx, reference_kv=_frames64(gold, heads, "all"))[0]
    out_pos = UC.unet64(sd64, lay, x, t, ctx, reference_kv=_frames64(gold, heads, "positive"))[0]
    check("out_refall", out_all)
    check("out_refpos", out_pos)
    check("out_ctl", UC.unet64(sd64, lay, x, t, ctx, control=ctl)[0])
    check("out_ctl_mid", UC.unet64(sd64, lay, x, t, ctx, control=ctl, only_mid_control=True)[0])
    assert torch.equal(out_pos[0], out[0]) and not torch.equal(out_pos[1], out[1]) and not torch.equal(out_all[0], out[0])
    emb = UC.time_embed64(sd64, t, UC.U0["model_channels"])
    for ci, (_, name, _, up) in enumerate(UC.RESBLOCK_CASES):
        xb, skip = UC.resblock_inputs(ci)
        r = UC.resblock64(sd64, name, (xb if skip is None else torch.cat([xb, skip], 1)).double(), emb)
        check(f"rb{ci}", r if up is None else UC.upsample64(sd64, up, r))


def test_reference_kv_goes_to_its_transformer():
    from sd_animation_optical_flow_amd import unet as UN
    frames = [[(f"k{f}.{i}", f"v{f}.{i}") for i in range(7)] for f in range(3)]
    keep = [list(f) for f in frames]
    routed = UN.route_reference_kv(frames, 7)
    assert len(routed) == 7
    for i, ents in enumerate(routed):
        assert ents == [(f"k{f}.{i}", f"v{f}.{i}") for f in range(3)]
    assert frames == keep                                            # the caller's lists are not consumed
    assert UN.route_reference_kv((), 7) == [[]] * 7 and UN.route_reference_kv(None, 7) == [[]] * 7
    assert UN.route_reference_kv([[(1, 2, "layer")] * 7], 7)[6] == [(1, 2)]
    with pytest.raises(ValueError, match="6 entries"):
        UN.route_reference_kv([frames[0], frames[1][:6]], 7)
    with pytest.raises(ValueError, match="16 transformers"):
        UN.route_reference_kv([frames[0]], 16)
    with pytest.raises(ValueError, match=r"reference_kv\[0\]\[2\]"):
        UN.route_reference_kv([[("k", "v")] * 2 + ["k"] + [("k", "v")] * 4], 7)


@pytest.mark.parametrize("key,value", [("use_scale_shift_norm", True), ("resblock_updown", True), ("num_classes", 10),
                                       ("use_linear_in_transformer", True), ("use_spatial_transformer", False),
                                       ("conv_resample", False), ("dims", 3)])
def test_unsupported_options(key, value):
    from sd_animation_optical_flow_amd import unet as UN
    with pytest.raises(NotImplementedError, match=key):
        UN.unet_tensors(dict(UC.U0, **{key: value}))
    with pytest.raises(NotImplementedError, match=key):
        UN.UNetModel({}, dict(UC.U0, **{key: value}))


def test_checkpoint_errors_name_the_key(u0):
    UN, sd, _, _ = u0
    pre = "model.diffusion_model."
    full = {pre + k: v for k, v in sd.items()}
    miss = dict(full)
    del miss[pre + "output_blocks.3.0.skip_connection.weight"]
    with pytest.raises(KeyError, match="output_blocks.3.0.skip_connection.weight"):
        UN.UNetModel(miss, UC.U0)
    bad = dict(full)
    bad[pre + "middle_block.1.proj_in.weight"] = torch.zeros((192, 192))
    with pytest.raises(ValueError, match="middle_block.1.proj_in.weight"):
        UN.UNetModel(bad, UC.U0)
    with pytest.raises(KeyError, match="time_embed.0.weight"):
        UN.UNetModel(sd, UC.U0)                                      # the default prefix is the full checkpoint's
    with pytest.raises(ValueError, match="multiples of 32"):
        UN.UNetModel({}, dict(UC.U0, model_channels=48))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            UN.UNetModel(sd, UC.U0, prefix="")


def test_seeded_weights_do_not_zero_the_zero_modules(u0):
    _, sd, _, _ = u0
    for k in ("out.2.weight", "input_blocks.1.0.out_layers.3.weight", "middle_block.1.proj_out.weight"):
        assert float(sd[k].abs().max()) > 0


def test_timestep_table_is_the_references(u0):
    from sd_animation_optical_flow_amd import ops
    for dim in UC.TS_DIMS + (64,):
        assert torch.equal(ops.timestep_freqs(dim), UC.timestep_freqs(dim))
    ref, bound = UC.timestep_embedding_reference(torch.tensor(UC.TS_T), 65)
    assert tuple(ref.shape) == (4, 65) and float(ref[:, 64].abs().max()) == 0 and float(ref[0, :32].min()) == 1.0


@pytest.mark.parametrize("c", UC.GNC_CASES, ids=[c["name"] for c in UC.GNC_CASES])
def test_groupnorm_cat_arithmetic_meets_its_bound_in_fp32(c):
    """The kernels' arithmetic in kernel order, simulated on the host with fp32 roundings where the kernels round: inside the bound
    on every case of the GPU table, so the bound can be met."""
    x0, x1, e, gamma, beta = UC.gnc_input(c)
    x, ref = UC.gnc_reference(x0, x1, e, gamma, beta, c["groups"])
    sim = UC.gnc_simulate(x0, x1, e, gamma, beta, c["groups"], c["silu"])
    assert bool(torch.isfinite(sim).all())
    worst, used = SC.gn_ratios(sim, x, ref, c["silu"])
    print(f"{c['name']}: simulated |error| / bound {worst:.3f}, measured-term use {used:.3f}")
    assert worst <= 1.0


def test_groupnorm_cat_bound_notices_a_dropped_emb_term():
    c = UC.GNC_CASES[0]
    x0, x1, e, gamma, beta = UC.gnc_input(c)
    x, ref = UC.gnc_reference(x0, x1, e, gamma, beta, c["groups"])
    wrong = UC.gnc_simulate(x0, x1, None, gamma, beta, c["groups"], c["silu"])
    assert SC.gn_ratios(wrong, x, ref, c["silu"])[0] > 1e3
    swapped = UC.gnc_simulate(x0, x1, e.flip(0), gamma, beta, c["groups"], c["silu"])
    assert SC.gn_ratios(swapped, x, ref, c["silu"])[0] > 1e3


def test_emb_linear_bound_holds_for_an_fp32_evaluation():
    g = torch.Generator().manual_seed(3)
    for K, N in ((320, 1280), (1280, 100), (36, 7)):
        x, w, b = torch.randn((3, K), generator=g), torch.randn((N, K), generator=g) / K ** 0.5, torch.randn((N,), generator=g) * 0.05
        for silu in (False, True):
            ref, bound = UC.emb_linear_reference(x, w, b, silu)
            got = torch.nn.functional.linear(torch.nn.functional.silu(x) if silu else x, w, b)
            assert SC._worst((got.double() - ref).abs(), bound) <= 1.0
