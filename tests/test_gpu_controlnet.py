"""ControlNet on the device: `ofx_conv3x3_silu` against float64 case by case with the derived bound (tests/controlnet_check.py),
`ControlNet.forward` and `apply_multi_controlnet` at configuration c0 against the float64 restatement with the bar of four times the
reference's own distance (tests/golden/controlnet_ref_c0.npz), and the input rules.  Every test prints its figures (-s)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import controlnet_check as CC   # noqa: E402
import transformer_check as TC   # noqa: E402
import unet_check as UC   # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "controlnet_ref_c0.npz")


@pytest.fixture(scope="module")
def ops(cuda):
    from sd_animation_optical_flow_amd import ops as O
    return O


@pytest.fixture(scope="module")
def CN(cuda):
    from sd_animation_optical_flow_amd import controlnet
    return controlnet


@pytest.fixture(scope="module")
def yard():
    z = np.load(GOLD)
    return dict(zip([str(k) for k in z["dist_keys"]], [float(v) for v in z["ref_vs_f64"]]))


@pytest.fixture(scope="module")
def refs64(CN):
    """The float64 restatement at c0, computed once: per net the residuals, net 0's guided_hint and its batch-1-hint residuals."""
    x, hint, t, context = CC.c0_inputs()
    lay = CN.controlnet_layout(CC.C0)
    out = {}
    for seed, _, _, _ in CC.MIX_NETS:
        sd64 = TC.to64(CN.random_controlnet_state_dict(seed, CC.C0))
        outs, guided = CC.controlnet64(sd64, lay, x, hint, t, context)
        out[f"net{seed}"] = outs
        if seed == 0:
            out["guided_hint"] = guided
            out["hint1"], _ = CC.controlnet64(sd64, lay, x, hint[:1], t, context)
    return out


@pytest.fixture(scope="module")
def nets(CN):
    return [CN.ControlNet(CN.random_controlnet_state_dict(seed, CC.C0), CC.C0, prefix="") for seed, _, _, _ in CC.MIX_NETS]


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the kernel

@pytest.mark.parametrize("c", CC.CONV_CASES, ids=[c["name"] for c in CC.CONV_CASES])
def test_conv3x3_silu_against_float64(ops, c):
    x, w, bias = CC.conv_input(c)
    ref, bound, y = CC.conv_reference(x, w, bias, c)
    wp = ops.pack_conv_weight(w)                                   # [cout, Kpad]: a 3-channel weight is padded to 4 with zeros
    B, Ho, Wo, _ = ref.shape
    out = torch.full((B, Ho, Wo, c["ldo"]), CC.SENTINEL, device="cuda")
    xd = x.cuda()
    got = ops.conv3x3_silu(xd, wp.cuda(), bias.cuda(), c["cout"], stride=c["stride"], silu=c["silu"], out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    o = out.cpu()
    assert torch.equal(xd.cpu(), x)                                # the input is not written to
    if c["ldo"] > c["cout"]:
        assert bool((o[..., c["cout"]:] == CC.SENTINEL).all()), "the slack of an output row was written"
    o = o[..., :c["cout"]]
    assert bool(torch.isfinite(o).all())
    worst = CC.worst_ratio(o, ref, bound)
    print(f"{c['name']}: |error| / bound {worst:.4f}   max |y64| {float(y.abs().max()):.1f}")
    assert worst <= 1.0
    if c["kind"] == "big":
        assert float(y.max()) > 90 and float(y.min()) < -90
    if c["ldo"] == c["cout"]:                                      # without `out`: the same bits in a fresh tensor
        assert torch.equal(ops.conv3x3_silu(xd, wp.cuda(), bias.cuda(), c["cout"], stride=c["stride"], silu=c["silu"]).cpu(), o)
    for name, bad in CC.conv_planted(x, w, bias, c).items():       # the bound tells a wrong kernel from a right one
        assert CC.worst_ratio(bad, ref, bound) > 1.0, name


def test_conv3x3_silu_wrapper_refuses(ops):
    x = torch.zeros((1, 4, 4, 16), device="cuda")
    w = torch.zeros((16, 160), device="cuda")
    with pytest.raises(RuntimeError):
        ops.conv3x3_silu(x.cpu(), w, None, 16)
    with pytest.raises(RuntimeError):
        ops.conv3x3_silu(x, torch.zeros((16, 150), device="cuda"), None, 16)       # not a packed 3x3 weight
    with pytest.raises(RuntimeError):
        ops.conv3x3_silu(x[..., :8].contiguous(), w, None, 16)                      # x holds fewer channels than the weight
    with pytest.raises(RuntimeError):
        ops.conv3x3_silu(x, w, None, 16, out=torch.zeros((1, 4, 4, 8), device="cuda"))
    from sd_animation_optical_flow_amd._lib import OfxError
    with pytest.raises(OfxError):
        ops.conv3x3_silu(x, w, None, 16, stride=3)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) ControlNet.forward at c0

def _check(tag, got, ref64, yardstick):
    d = float((got.double().cpu() - ref64).abs().max())
    bar = UC.bar4(yardstick)
    print(f"  {tag:14s} |device - float64| {d:.3e}   bar {bar:.3e}   ratio {d / bar:.3f}")
    assert bool(torch.isfinite(got).all()) and d <= bar, tag


def test_forward_c0_against_float64(nets, refs64, yard):
    x, hint, t, context = (v.cuda() for v in CC.c0_inputs())
    net = nets[0]
    assert not net.stem_glue
    outs = net.forward(x, hint, t, context)
    assert [tuple(o.shape) for o in outs] == CC.C0_SHAPES and all(o.is_contiguous() and o.dtype == torch.float32 for o in outs)
    guided = net.hint_stem(hint).permute(0, 3, 1, 2)
    _check("guided_hint", guided, refs64["guided_hint"], yard["guided_hint"])
    for i, o in enumerate(outs):
        _check(f"out{i}", o, refs64["net0"][i], yard[f"out{i}"])
    outs1 = net(x, hint[:1], t, context)                           # a hint of batch 1 broadcasts; the stem runs once
    for i, o in enumerate(outs1):
        _check(f"out{i}_hint1", o, refs64["hint1"][i], yard[f"out{i}_hint1"])
    # one map for both images: in the epilogue of input_blocks.0.0 (batch 2) or as one broadcast add (batch 1), the same bits
    rep = net(x, hint[:1].expand(2, -1, -1, -1).contiguous(), t, context)
    for a, b in zip(rep, outs1):
        assert torch.equal(a, b)
    assert torch.equal(x.cpu(), CC.c0_inputs()[0]) and torch.equal(hint.cpu(), CC.c0_inputs()[1])


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import controlnet_check as CC
from sd_animation_optical_flow_amd import controlnet as CN
net = CN.ControlNet(CN.random_controlnet_state_dict(0, CC.C0), CC.C0, prefix="")
assert net.stem_glue
x, hint, t, context = (v.cuda() for v in CC.c0_inputs())
outs = net(x, hint, t, context)
np.savez(sys.argv[2], guided_hint=net.hint_stem(hint).permute(0, 3, 1, 2).cpu().numpy(), **{f"out{i}": o.cpu().numpy() for i, o in enumerate(outs)})
"""


def test_torch_glue_stem_in_a_fresh_process(cuda, refs64, yard, tmp_path):
    """OFX_CNET_TORCH_GLUE=1 is read once per process, so the glue stem (F.conv2d + F.silu) runs in a child: same float64
    references, same bar."""
    path = str(tmp_path / "glue.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(HERE), path], env=dict(os.environ, OFX_CNET_TORCH_GLUE="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(path)
    _check("guided_hint", torch.from_numpy(z["guided_hint"]), refs64["guided_hint"], yard["guided_hint"])
    for i in range(7):
        _check(f"out{i}", torch.from_numpy(z[f"out{i}"]), refs64["net0"][i], yard[f"out{i}"])


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) apply_multi_controlnet

def test_apply_multi_controlnet_on_the_device(CN, nets, refs64, yard):
    x, hint, t, context = (v.cuda() for v in CC.c0_inputs())
    # the nets' residuals are preset from the full hint (two maps), as the fixture's were; the caching path is run below
    cn = [CN.SingleControlNet(weight=w, model="canny", args={}, condition=None, guidance_start=gs, guidance_end=ge, net=net,
                              result=net(x, hint, t, context)) for (_, w, gs, ge), net in zip(CC.MIX_NETS, nets)]
    mixed = None
    for p in CC.MIX_P:
        mixed = CN.apply_multi_controlnet(x, t, context, p, cn)
        for i, (m, m64) in enumerate(zip(mixed, CC.mix64([refs64["net0"], refs64["net1"]], p))):
            name = f"mix{int(round(p * 100))}_{i}"
            _check(name, m, m64, yard[name])
    assert all(m.data_ptr() != r.data_ptr() for m, r in zip(mixed, cn[0].result))
    # the mix is what UNetModel.forward(control=) takes: c0 mirrors U0
    from sd_animation_optical_flow_amd.unet import UNetModel, random_unet_state_dict
    unet = UNetModel(random_unet_state_dict(0, UC.U0), UC.U0, prefix="")
    ux, ut, uctx = (v.cuda() for v in UC.u0_inputs())
    plain, _ = unet(ux, ut, uctx)
    eps, _ = unet(ux, ut, uctx, control=mixed)
    assert tuple(eps.shape) == tuple(plain.shape) and bool(torch.isfinite(eps).all()) and not torch.equal(eps, plain)
    # from a condition image: the hint is made and the net run on first use only
    edges = (torch.rand((8 * CC.C0_H, 8 * CC.C0_W), generator=torch.Generator().manual_seed(5)) > 0.9).to(torch.uint8).numpy() * 255
    one = [CN.SingleControlNet(weight=0.5, model="hed", args={}, condition=edges, net=nets[0])]
    first = CN.apply_multi_controlnet(x, t, context, 0.3, one)
    cached = one[0].result
    want = nets[0](x, CN.make_hint("hed", edges, {}), t, context)
    assert all(torch.equal(a, b * 0.5) for a, b in zip(first, want))
    again = CN.apply_multi_controlnet(x, t, context, 0.4, one)
    assert one[0].result is cached and all(torch.equal(a, b) for a, b in zip(first, again))


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) input rules

def test_input_rules_raise_before_any_launch(CN, nets):
    x, hint, t, context = (v.cuda() for v in CC.c0_inputs())
    net = nets[0]
    with pytest.raises(ValueError):
        net(x, hint[:, :, :-8], t, context)                        # a hint not 8x the latent
    with pytest.raises(ValueError):
        net(x, hint[:, :, ::2, ::2].contiguous(), t, context)
    with pytest.raises(ValueError):
        net(x[:, :, :6], hint[:, :, :48], t, context)              # a latent not a multiple of 4
    with pytest.raises(RuntimeError):
        net(x.cpu(), hint, t, context)                             # CPU tensors
    with pytest.raises(RuntimeError):
        net(x, hint.cpu(), t, context)
    with pytest.raises(RuntimeError):
        net(x, hint, t, context[:, :, :32].contiguous())           # wrong context width
    with pytest.raises(RuntimeError):
        net(x, hint[:, :2], t, context)                            # wrong hint channels
    with pytest.raises(RuntimeError):
        net(x, torch.cat([hint, hint[:1]]), t, context)            # a hint batch that is neither 1 nor B
    with pytest.raises(RuntimeError):
        net(x, hint, t[:1], context)
    sd = CN.random_controlnet_state_dict(0, CC.C0)
    lacking = {k: v for k, v in sd.items() if k != "zero_convs.3.0.bias"}
    with pytest.raises(KeyError, match="zero_convs.3.0.bias"):
        CN.ControlNet(lacking, CC.C0, prefix="")
    with pytest.raises(KeyError, match="control_model.time_embed.0.weight"):
        CN.ControlNet(sd, CC.C0)                                   # the default prefix is the checkpoint's "control_model."
    bad = dict(sd)
    bad["input_hint_block.14.weight"] = torch.zeros((64, 256, 1, 1))
    with pytest.raises(ValueError, match="input_hint_block.14.weight"):
        CN.ControlNet(bad, CC.C0, prefix="")
    with pytest.raises(NotImplementedError):
        CN.ControlNet(sd, dict(CC.C0, dims=3), prefix="")
    with pytest.raises(ValueError):
        CN.ControlNet(sd, CC.C0, prefix="", precision="fp8")
