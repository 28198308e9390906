"""`UNetModel(precision=)` on the device, configuration u0 (B = 2, 8 x 12 latent, as tests/test_gpu_unet.py): every precision against
the float64 restatement `unet_check.unet64`.

Bars.  "fp16": twice the stored distance of the reference's own mode for this stage -- its UNet under torch.autocast -- from
float64, per output (tests/golden/unet_ref_u0_autocast.npz, make_golden_unet_autocast.py).  The device performs a subset of
autocast's roundings (the operands of the contractions; autocast also rounds every layer's output and runs attention in half) and
must not be worse than the reference's mode; the factor two, not `bar4`'s four, allows for the yardstick being one sample of a
rounding error.  "bf16x6": `unet_check.bar4` of the fp32 yardstick (tests/golden/unet_ref_u0.npz) -- the arithmetic is fp32-level
by construction.  "bf16x3": the fp16 bar -- about 16 mantissa bits per product, finer than fp16's 11.  "fp32": the bits of a model
built without the argument.  Every test prints the measured distances (-s)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import transformer_check as TC   # noqa: E402
import unet_check as UC   # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "unet_ref_u0.npz")
GOLD_AUTOCAST = os.path.join(HERE, "golden", "unet_ref_u0_autocast.npz")
OUTS = ("out", "out_refall", "out_refpos", "out_ctl", "out_ctl_mid")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def yard32(gold):
    return {str(k): float(v) for k, v in zip(gold["dist_keys"], gold["ref_vs_f64"])}


@pytest.fixture(scope="module")
def yard16():
    g = np.load(GOLD_AUTOCAST)
    return {str(k): float(v) for k, v in zip(g["dist_keys"], g["autocast_vs_f64"])}


def bar2(yardstick):
    """The fp16 device's bar: twice the distance of the reference under autocast from float64 (header)."""
    return 2.0 * float(yardstick)


@pytest.fixture(scope="module")
def setup(cuda, gold):
    from sd_animation_optical_flow_amd import unet as UN
    sd = UN.random_unet_state_dict(0, UC.U0)
    lay = UN.unet_layout(UC.U0)
    heads = UC.transformer_heads(lay)
    hist = [(torch.from_numpy(gold[f"k{i}"]), torch.from_numpy(gold[f"v{i}"])) for i in range(len(heads))]
    return dict(UN=UN, sd=sd, lay=lay, heads=heads, hist=hist, models={}, runs={})


@pytest.fixture(scope="module")
def refs64(gold, setup):
    """The float64 restatement of the five stored runs, computed once and left unchanged."""
    sd64, lay, heads = TC.to64(setup["sd"]), setup["lay"], setup["heads"]
    x, t, ctx = (torch.from_numpy(gold[n]) for n in ("x", "timesteps", "context"))
    ctl = UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)
    f64 = lambda mode: [[(TC.heads_last(k, h).double(), TC.heads_last(v, h).double())
                         for (k, v), h in zip(UC.reference_frames(setup["hist"], heads, mode)[0], heads)]]
    out, hist = UC.unet64(sd64, lay, x, t, ctx)
    r = {"out": out}
    for i, ((k, v), h) in enumerate(zip(hist, heads)):
        r[f"k{i}"], r[f"v{i}"] = TC.heads_first(k, h), TC.heads_first(v, h)
    r["out_refall"] = UC.unet64(sd64, lay, x, t, ctx, reference_kv=f64("all"))[0]
    r["out_refpos"] = UC.unet64(sd64, lay, x, t, ctx, reference_kv=f64("positive"))[0]
    r["out_ctl"] = UC.unet64(sd64, lay, x, t, ctx, control=ctl)[0]
    r["out_ctl_mid"] = UC.unet64(sd64, lay, x, t, ctx, control=ctl, only_mid_control=True)[0]
    return r


def _model(setup, precision):
    """One model per precision for the module; None: built without the argument."""
    if precision not in setup["models"]:
        kw = {} if precision is None else dict(precision=precision)
        m = setup["UN"].UNetModel(setup["sd"], UC.U0, prefix="", **kw)
        assert not m.torch_glue and m.precision == (precision or "fp32")
        assert all(st.precision == m.precision for st in m.st.values())
        setup["models"][precision] = m
    return setup["models"][precision]


def _runs(setup, gold, precision):
    """The five scenarios (and the plain run's history, in the reference's layout) of one precision, run once."""
    if precision in setup["runs"]:
        return setup["runs"][precision]
    from sd_animation_optical_flow_amd.transformer import to_reference_layout
    model, heads, lay = _model(setup, precision), setup["heads"], setup["lay"]
    x, t, ctx = (torch.from_numpy(gold[n]).cuda() for n in ("x", "timesteps", "context"))
    ctl = [c.cuda() for c in UC.control_residuals(lay, UC.U0_B, UC.U0_H, UC.U0_W)]
    keep = [c.clone() for c in ctl]
    fa, fp = UC.reference_frames(setup["hist"], heads, "all"), UC.reference_frames(setup["hist"], heads, "positive")
    n_before = [len(f) for f in fa + fp]
    out, hist = model(x, t, ctx)
    res = {"out": out}
    for i, ((k, v), h) in enumerate(zip(hist, heads)):
        res[f"k{i}"], res[f"v{i}"] = to_reference_layout(k, h), to_reference_layout(v, h)
    res["out_refall"] = model(x, t, ctx, reference_kv=fa)[0]
    res["out_refpos"] = model(x, t, ctx, reference_kv=fp)[0]
    res["out_ctl"] = model(x, t, ctx, control=ctl)[0]
    res["out_ctl_mid"] = model(x, t, ctx, control=ctl, only_mid_control=True)[0]
    assert [len(f) for f in fa + fp] == n_before                                     # reference_kv is not consumed ...
    assert len(ctl) == len(keep) and all(torch.equal(a, b) for a, b in zip(ctl, keep))   # ... and control neither consumed nor written
    setup["runs"][precision] = res
    return res


def _hold(tag, res, refs64, bars):
    assert sorted(res) == sorted(refs64)
    dist = {name: float((res[name].detach().cpu().double() - refs64[name]).abs().max()) for name in sorted(res)}
    for name, d in dist.items():                                                     # every figure is printed before any is judged
        print(f"{tag} {name}: device vs float64 {d:.3e}; bar {bars[name]:.3e}")
    for name, d in dist.items():
        assert d <= bars[name], (tag, name, d, bars[name])


def test_fp16_against_float64(setup, gold, refs64, yard16):
    res = _runs(setup, gold, "fp16")
    _hold("fp16", res, refs64, {k: bar2(v) for k, v in yard16.items()})
    exact = _runs(setup, gold, "fp32")
    for name in res:
        assert not torch.equal(res[name], exact[name]), name             # the fp16 kernels ran
    # a second call repeats the bits
    model = _model(setup, "fp16")
    x, t, ctx = (torch.from_numpy(gold[n]).cuda() for n in ("x", "timesteps", "context"))
    out2, hist2 = model(x, t, ctx)
    from sd_animation_optical_flow_amd.transformer import to_reference_layout
    assert torch.equal(out2, res["out"])
    for i, ((k, v), h) in enumerate(zip(hist2, setup["heads"])):
        assert torch.equal(to_reference_layout(k, h), res[f"k{i}"]) and torch.equal(to_reference_layout(v, h), res[f"v{i}"])


def test_default_precision_is_untouched(setup, gold):
    default, named = _runs(setup, gold, None), _runs(setup, gold, "fp32")
    assert _model(setup, None).precision == "fp32"
    for name in default:
        assert torch.equal(default[name], named[name]), name


@pytest.mark.parametrize("precision", ["bf16x3", "bf16x6"])
def test_split_bf16_against_float64(setup, gold, refs64, yard16, yard32, precision):
    res = _runs(setup, gold, precision)
    bars = {k: UC.bar4(v) for k, v in yard32.items() if k in res} if precision == "bf16x6" else {k: bar2(v) for k, v in yard16.items()}
    _hold(precision, res, refs64, bars)
    exact = _runs(setup, gold, "fp32")
    assert not torch.equal(res["out"], exact["out"])


_CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import transformer_check as TC, unet_check as UC
from sd_animation_optical_flow_amd import unet as UN
from sd_animation_optical_flow_amd.transformer import to_reference_layout
g, refs = np.load(sys.argv[2]), np.load(sys.argv[3])
model = UN.UNetModel(UN.random_unet_state_dict(0, UC.U0), UC.U0, prefix="", precision="fp16")
assert model.torch_glue and model.precision == "fp16"
assert all(st.torch_glue and not st.fused_attention and st.precision == "fp16" for st in model.st.values())
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


def test_fp16_torch_glue_path_in_a_fresh_process(cuda, yard16, refs64):
    """OFX_UNET_TORCH_GLUE=1 and OFX_ST_TORCH_GLUE=1 are read once per process, so both glue compositions (the UNet's and the
    transformers') run in a child with precision="fp16": the same float64 references, the same bars."""
    env = dict(os.environ, OFX_UNET_TORCH_GLUE="1", OFX_ST_TORCH_GLUE="1")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "refs64.npz")
        np.savez(path, **{k: v.numpy() for k, v in refs64.items()})
        r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(HERE), GOLD, path], env=env, capture_output=True, text=True,
                           timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("ERR ")]
    assert sorted(ln[1] for ln in lines) == sorted(refs64)
    for _, name, err in lines:
        print(f"fp16 glue path {name}: device vs float64 {float(err):.3e}; bar {bar2(yard16[name]):.3e}")
        assert float(err) <= bar2(yard16[name]), name
