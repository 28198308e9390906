"""-m gpu: the CLIP text encoder on the HIP kernels -- `ofx_clip_embed` bit for bit against torch, `ofx_quick_gelu` against float64
within the derived bound (tests/text_encoder_check.py), and `ClipTextEncoder` at configuration t0 against the float64 restatement
with the bar of four times the reference's own distance (tests/golden/clip_text_ref_t0.npz): outputs, hidden states, causality,
T = 20, `conditioning` with and without dedupe, and the torch-glue switch.  Every test prints its figures (-s)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import text_encoder_check as XC   # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "clip_text_ref_t0.npz")


@pytest.fixture(scope="module")
def ops(cuda):
    from sd_animation_optical_flow_amd import ops as O
    return O


@pytest.fixture(scope="module")
def TE(cuda):
    from sd_animation_optical_flow_amd import text_encoder
    return text_encoder


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    out = {k: z[k] for k in z.files}
    out["dist"] = dict(zip([str(k) for k in z["dist_keys"]], [float(v) for v in z["ref_dist"]]))
    return out


@pytest.fixture(scope="module")
def sd(TE):
    return TE.random_clip_text_state_dict(0, XC.T0)


@pytest.fixture(scope="module")
def refs64(sd, gold):
    """The float64 restatement on the golden tokens, computed once: per clip_skip the [2,231,128] output."""
    sd64 = XC.to64(sd)
    return {skip: XC.forward_tokens64(sd64, XC.T0, gold["tokens"], skip) for skip in XC.T0_SKIPS}


@pytest.fixture(scope="module")
def encoders(TE, sd):
    """(clip_skip, dedupe) -> encoder."""
    return {(skip, dd): TE.ClipTextEncoder(sd, XC.T0, prefix="", clip_skip=skip, dedupe=dd) for skip in XC.T0_SKIPS for dd in (True, False)}


def _check(tag, got, ref64, yardstick):
    d = float((got.double().cpu() - ref64).abs().max())
    bar = XC.bar4(yardstick)
    print(f"  {tag:26s} |device - float64| {d:.3e}   bar {bar:.3e}   ratio {d / bar:.3f}")
    assert bool(torch.isfinite(got).all()) and d <= bar, tag
    return d / bar


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the kernels

@pytest.mark.parametrize("c", XC.EMBED_CASES, ids=[c["name"] for c in XC.EMBED_CASES])
def test_clip_embed_is_torchs_bits(ops, c):
    ids, tok, pos = XC.embed_input(c)
    ref, ok = XC.embed_reference(ids, tok, pos, c)
    out = torch.full((c["rows"], c["ldo"]), XC.SENTINEL, device="cuda")
    dids, dtok, dpos = ids.cuda(), tok.cuda(), pos.cuda()
    got = ops.clip_embed(dids, dtok, dpos, c["T"], out=out[:, :c["C"]])
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    o = out.cpu()
    if c["ldo"] > c["C"]:
        assert bool((o[:, c["C"]:] == XC.SENTINEL).all()), "the padding columns of an output row were written"
    o = o[:, :c["C"]]
    assert torch.equal(o[ok].view(torch.int32), ref[ok].view(torch.int32))         # the bits, not the values
    assert int((~ok).sum()) == (2 if c["bad"] else 0) and bool(torch.isnan(o[~ok]).all())
    assert torch.equal(dtok.cpu(), tok) and torch.equal(dpos.cpu(), pos) and torch.equal(dids.cpu(), ids)
    T = c["T"]
    if c["ldo"] == c["C"] and not c["bad"] and c["rows"] % T == 0:         # without `out`: the same bits in a fresh [S,T,C] tensor
        fresh = ops.clip_embed(dids.view(-1, T), dtok, dpos, T)
        assert tuple(fresh.shape) == (c["rows"] // T, T, c["C"]) and torch.equal(fresh.cpu().view(-1, c["C"]), ref)


def test_clip_embed_wrapper_refuses(ops):
    ids = torch.zeros((4,), dtype=torch.int32, device="cuda")
    tok, pos = torch.zeros((8, 16), device="cuda"), torch.zeros((4, 16), device="cuda")
    with pytest.raises(RuntimeError):
        ops.clip_embed(ids.cpu(), tok, pos, 4)
    with pytest.raises(RuntimeError):
        ops.clip_embed(ids.long(), tok, pos, 4)                    # int32 ids, as the reference feeds
    with pytest.raises(RuntimeError):
        ops.clip_embed(ids, tok.t(), pos, 4)                       # not contiguous
    with pytest.raises(RuntimeError):
        ops.clip_embed(ids, tok, pos, 5)                           # fewer positions than T
    with pytest.raises(RuntimeError):
        ops.clip_embed(ids, tok, pos[:, :8].contiguous(), 4)       # the tables disagree on C
    with pytest.raises(RuntimeError):
        ops.clip_embed(ids, tok, pos, 4, out=torch.zeros((4, 8), device="cuda"))
    with pytest.raises(RuntimeError):
        ops.quick_gelu(torch.zeros((4, 8)))
    with pytest.raises(RuntimeError):
        ops.quick_gelu(torch.zeros((8, 4), device="cuda").t())
    with pytest.raises(RuntimeError):
        ops.quick_gelu(torch.zeros((4, 8), device="cuda"), out=torch.zeros((4, 4), device="cuda"))
    from sd_animation_optical_flow_amd._lib import OfxError
    with pytest.raises(OfxError):
        ops.quick_gelu(torch.zeros((4, 6), device="cuda"))         # n % 4


@pytest.mark.parametrize("c", XC.QGELU_CASES, ids=[c["name"] for c in XC.QGELU_CASES])
def test_quick_gelu_against_float64(ops, c):
    rows, n = c["rows"], c["n"]
    for kind in XC.QGELU_SETS:
        x = XC.qgelu_input(c, kind)
        ref, bound = XC.qgelu_reference(x)
        xin = torch.full((rows, c["ldx"]), XC.SENTINEL, device="cuda")
        xin[:, :n] = x.cuda()
        out = torch.full((rows, c["ldo"]), XC.SENTINEL, device="cuda")
        got = ops.quick_gelu(xin[:, :n], out=out[:, :n])           # out of place
        assert got.data_ptr() == out.data_ptr()
        inplace = xin.clone()
        ops.quick_gelu(inplace[:, :n], out=inplace[:, :n])         # in place
        torch.cuda.synchronize()
        assert torch.equal(xin.cpu()[:, :n], x) and bool((xin.cpu()[:, n:] == XC.SENTINEL).all())
        for tag, t in (("out of place", out.cpu()), ("in place", inplace.cpu())):
            assert bool((t[:, n:] == XC.SENTINEL).all()), f"{kind} {tag}: columns >= n were written"
            o = t[:, :n]
            assert bool(torch.isfinite(o).all()), f"{kind} {tag}"
            worst = XC.worst_ratio(o, ref, bound)
            print(f"{c['name']} {kind:7s} {tag:12s} |error| / bound {worst:.4f}")
            assert worst <= 1.0, f"{kind} {tag}"
        assert torch.equal(out.cpu()[:, :n], inplace.cpu()[:, :n])
        if kind == "sweep":
            assert float(x.view(-1)[1]) == -80.0 and float(out.cpu()[:, :n].reshape(-1)[1]) == 0.0      # -0 or 0, not NaN
        if c["ldx"] == n:                                          # without `out`: the same bits in a fresh tensor
            assert torch.equal(ops.quick_gelu(xin).cpu(), out.cpu()[:, :n])


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the encoder at t0

def test_outputs_against_float64_both_dedupe_settings(encoders, refs64, gold):
    tokens = torch.from_numpy(gold["tokens"])
    for (skip, dd), enc in encoders.items():
        assert not enc.torch_glue
        got = enc.forward_tokens(tokens)
        assert tuple(got.shape) == (2, 231, 128) and got.is_contiguous() and got.dtype == torch.float32 and got.is_cuda
        _check(f"clip_skip {skip} dedupe {dd}", got, refs64[skip], gold["dist"][f"out_skip{skip}"])
        # the empty chunk [bos, eos, pad...] occurs three times (prompt 1's third, prompt 2's second and third): four distinct sequences
        assert enc.embed_rows == (4 if dd else 6) * 77
        assert enc.layers_run == {0: 3, 2: 2, 3: 1}[skip]
    # the reference's own fp32 output: one yardstick from float64, the device at most four, so at most five apart (1.25 bars)
    d =float((encoders[(0, True)].forward_tokens(tokens).cpu().double() - torch.from_numpy(gold["out_skip0"]).double()).abs().max())
    print(f"  device vs the reference's fp32 output {d:.3e}")
    assert d <= XC.bar4(gold["dist"]["out_skip0"]) * 1.25


def test_hidden_states_layer_by_layer(encoders, sd, gold):
    ids = gold["tokens"].reshape(6, 77)
    _, yard = XC.fp32_yardsticks(sd, XC.T0, ids, 0)
    _, hs64 = XC.clip_text64(XC.to64(sd), XC.T0, ids, 0, hidden_states=True)
    for dd in (True, False):
        out, hs = encoders[(0, dd)].encode_ids(torch.from_numpy(ids), hidden_states=True)
        assert len(hs) == XC.T0["layers"] + 1 and tuple(out.shape) == (6, 77, 128)
        for i, (h, h64, y) in enumerate(zip(hs, hs64, yard)):
            _check(f"hidden_states[{i}] dedupe {dd}", h, h64, y)
    _, hs2 = encoders[(3, True)].encode_ids(torch.from_numpy(ids), hidden_states=True)
    assert len(hs2) == 2                                           # clip_skip 3 of three layers: layers past the first are not run


def test_causality(encoders, sd, gold):
    """Changing the id at position 10 of one sequence leaves positions 0..9 of it and every other sequence within the bar; some
    position >= 10 moves by more than 1000 x the bar."""
    enc = encoders[(0, False)]
    ids = torch.from_numpy(gold["tokens"].reshape(6, 77)).clone()
    base = enc.encode_ids(ids).cpu()
    changed = ids.clone()
    changed[1, 10] = (int(ids[1, 10]) + 123) % XC.T0_BOS
    assert int(changed[1, 10]) != int(ids[1, 10])
    got = enc.encode_ids(changed)
    y, _ = XC.fp32_yardsticks(sd, XC.T0, changed, 0)
    bar = XC.bar4(y)
    _check("changed id, all positions", got, XC.clip_text64(XC.to64(sd), XC.T0, changed, 0), y)
    got = got.cpu()
    before = float((got[1, :10] - base[1, :10]).abs().max())
    others = float((got[[0, 2, 3, 4, 5]] - base[[0, 2, 3, 4, 5]]).abs().max())
    after = float((got[1, 10:] - base[1, 10:]).abs().max())
    print(f"  positions 0..9 moved {before:.3e}, other sequences {others:.3e}, positions >= 10 {after:.3e}; bar {bar:.3e}")
    assert before <= bar and others <= bar and after > 1000 * bar


def test_sequences_of_20_tokens(encoders, sd):
    """The causal bias and r % T are not hard-wired to 77."""
    g = torch.Generator().manual_seed(20)
    ids = torch.randint(0, XC.T0["vocab"], (4, 20), generator=g)
    y, _ = XC.fp32_yardsticks(sd, XC.T0, ids, 0)
    ref = XC.clip_text64(XC.to64(sd), XC.T0, ids, 0)
    for dd in (True, False):
        got = encoders[(0, dd)].encode_ids(ids)
        assert tuple(got.shape) == (4, 20, 128)
        _check(f"T = 20 dedupe {dd}", got, ref, y)
    assert tuple(encoders[(0, True)].causal_bias(20).shape) == (20, 20)
    _check("T = 20 from a list", encoders[(0, True)].encode_ids(ids.tolist()), ref, y)
    _check("T = 20 from device ids", encoders[(0, True)].encode_ids(ids.cuda()), ref, y)
    with pytest.raises(ValueError):
        encoders[(0, True)].encode_ids(torch.full((1, 20), XC.T0["vocab"]))        # an id past the table, on the host
    with pytest.raises(ValueError):
        encoders[(0, True)].encode_ids([[0, -1, 3, 4]])
    with pytest.raises(ValueError):
        encoders[(0, True)].encode_ids(torch.zeros((1, 78), dtype=torch.int64))    # more tokens than positions
    with pytest.raises(RuntimeError):
        encoders[(0, True)].encode_ids(torch.zeros((20,), dtype=torch.int64))


def test_conditioning_encodes_a_short_pair_as_three_sequences(TE, encoders, sd, gold):
    tc = TE.chunk_tokens([[5, 9, 200, 31]], XC.T0_BOS, XC.T0_EOS, XC.T0_PAD)
    tu = TE.chunk_tokens([[77, 3]], XC.T0_BOS, XC.T0_EOS, XC.T0_PAD)
    sd64 = XC.to64(sd)
    y, _ = XC.fp32_yardsticks(sd, XC.T0, torch.cat([tc, tu]).reshape(6, 77), 0)
    for dd in (True, False):
        enc = encoders[(0, dd)]
        calls = enc.embed_calls
        ctx, uctx = enc.conditioning(tc, tu)
        assert enc.embed_calls == calls + 1                        # one pass for both prompts
        assert enc.embed_rows == (3 if dd else 6) * 77             # the rows that reached ofx_clip_embed
        for t in (ctx, uctx):
            assert tuple(t.shape) == (1, 231, 128) and t.is_contiguous() and t.dtype == torch.float32 and t.is_cuda
        _check(f"context dedupe {dd}", ctx, XC.forward_tokens64(sd64, XC.T0, tc), y)
        _check(f"unconditional dedupe {dd}", uctx, XC.forward_tokens64(sd64, XC.T0, tu), y)
        bar = XC.bar4(y)
        assert float((ctx - enc.forward_tokens(tc)).abs().max()) <= bar and float((uctx - enc.forward_tokens(tu)).abs().max()) <= bar
    # from prompts, through the tokenizer interface
    class Tok:
        bos_token_id, eos_token_id, pad_token_id = XC.T0_BOS, XC.T0_EOS, XC.T0_PAD

        def __call__(self, texts, truncation=False, add_special_tokens=False):
            return {"input_ids": [[int(s) for s in t.split()] for t in texts]}

    enc = encoders[(0, True)]
    assert float((enc.encode(["5_9 200_31"], Tok()) - enc.forward_tokens(tc)).abs().max()) <= XC.bar4(y)
    with pytest.raises(RuntimeError):
        enc.conditioning(tc, tu[:, :2])


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import text_encoder_check as XC
from sd_animation_optical_flow_amd import text_encoder as TE
tokens = torch.from_numpy(np.load(sys.argv[2])["tokens"])
sd = TE.random_clip_text_state_dict(0, XC.T0)
out = {}
for skip in XC.T0_SKIPS:
    enc = TE.ClipTextEncoder(sd, XC.T0, prefix="", clip_skip=skip)
    assert enc.torch_glue
    out[f"out_skip{skip}"] = enc.forward_tokens(tokens).cpu().numpy()
np.savez(sys.argv[3], **out)
"""


def test_torch_glue_in_a_fresh_process(cuda, refs64, gold, tmp_path):
    """OFX_CLIP_TORCH_GLUE=1 is read once per process, so the glue (F.embedding, torch's sigmoid) runs in a child: same float64
    references, same bar."""
    path = str(tmp_path / "glue.npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(HERE), GOLD, path], env=dict(os.environ, OFX_CLIP_TORCH_GLUE="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(path)
    for skip in XC.T0_SKIPS:
        _check(f"glue clip_skip {skip}", torch.from_numpy(z[f"out_skip{skip}"]), refs64[skip], gold["dist"][f"out_skip{skip}"])
