"""The CLIP text encoder without a device: `chunk_tokens` against the tokens the reference fed its transformer, the float64
restatement against the reference's outputs, planted mistakes against the device's bar, the loader's rules, and the refusals of
`ofx_clip_embed` / `ofx_quick_gelu`.
Fixture: tests/golden/clip_text_ref_t0.npz (tests/golden/make_golden_text_encoder.py, the reference's own embedder on the CPU)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sd_ops_check as SC
import text_encoder_check as XC
from sd_animation_optical_flow_amd import _lib, text_encoder as TE

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_text_ref_t0.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dist(gold):
    return dict(zip([str(k) for k in gold["dist_keys"]], [float(v) for v in gold["ref_dist"]]))


@pytest.fixture(scope="module")
def sd():
    return TE.random_clip_text_state_dict(0, XC.T0)


def test_t0_tensors_are_the_librarys(gold, sd):
    want = [(str(n), tuple(int(v) for v in s[:d])) for n, s, d in zip(gold["names"], gold["shapes"], gold["ndims"])]
    got = TE.clip_text_tensors(XC.T0)
    assert got == want and len(got) == 2 + 16 * 3 + 2
    assert list(sd) == [k for k, _ in got] and all(tuple(sd[k].shape) == s for k, s in got)
    assert not any("position_ids" in k for k, _ in got)
    v15 = dict(TE.clip_text_tensors())
    assert TE.SD_V15_CLIP_TEXT == dict(vocab=49408, width=768, heads=12, layers=12, intermediate=3072, positions=77)
    assert len(v15) == 2 + 16 * 12 + 2 and v15["embeddings.token_embedding.weight"] == (49408, 768)
    assert v15["encoder.layers.11.mlp.fc1.weight"] == (3072, 768) and v15["embeddings.position_embedding.weight"] == (77, 768)
    assert abs(sum(int(np.prod(s)) for s in v15.values()) / 1e6 - 123.06) < 0.01       # the text tower of ViT-L/14


def test_chunk_tokens_reproduces_the_references_tokens(gold):
    raw = [[int(v) for v in row[:n]] for row, n in zip(gold["raw_ids"], gold["raw_len"])]
    assert raw == XC.t0_inputs() and [len(r) for r in raw] == [100, 5]
    got = TE.chunk_tokens(raw, XC.T0_BOS, XC.T0_EOS, XC.T0_PAD)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, 3, 77)
    assert np.array_equal(got.numpy(), gold["tokens"])
    # the short prompt's chunks 2 and 3 are the constant [bos, eos, pad...]
    assert got[1, 1].tolist() == [XC.T0_BOS, XC.T0_EOS] + [XC.T0_PAD] * 75 and torch.equal(got[1, 1], got[1, 2])


@pytest.mark.parametrize("n", [0, 75, 76, 225, 300])
def test_chunk_tokens_lengths(n):
    bos, eos, pad = 1000, 1001, 1002
    raw = list(range(n))
    t = TE.chunk_tokens([raw], bos, eos, pad)
    assert tuple(t.shape) == (1, 3, 77) and t.dtype == torch.int32
    kept = raw[:225]                                               # ids beyond 225 are dropped
    for f in range(3):
        piece = kept[75 * f:75 * (f + 1)]
        row = t[0, f].tolist()
        assert row[0] == bos and row[1:1 + len(piece)] == piece
        assert row[1 + len(piece)] == eos                          # where eos lands: right after the piece, position 76 when full
        assert row[2 + len(piece):] == [pad] * (75 - len(piece))
    assert sorted(v for v in t.flatten().tolist() if v < 1000) == kept
    t2 = TE.chunk_tokens([raw, [0, 1, 2]], bos, eos, pad, chunks=2, chunk_len=4)
    assert tuple(t2.shape) == (2, 2, 6) and t2[1].tolist() == [[bos, 0, 1, 2, eos, pad], [bos, eos, pad, pad, pad, pad]]


def test_tokenize_prompts_follows_the_references_interface():
    class Tok:
        bos_token_id, eos_token_id, pad_token_id = 7, 8, 9
        seen = None

        def __call__(self, texts, truncation=None, add_special_tokens=None):
            Tok.seen = (list(texts), truncation, add_special_tokens)
            return {"input_ids": [[len(w) for w in t.split()] for t in texts]}

    t = TE.tokenize_prompts(["a_bb ccc", ""], Tok())
    assert Tok.seen == (["a bb ccc", ""], False, False)            # '_' becomes a space (hack.py:37)
    assert t[0, 0, :6].tolist() == [7, 1, 2, 3, 8, 9] and t[1, 0, :3].tolist() == [7, 8, 9] and tuple(t.shape) == (2, 3, 77)
    with pytest.raises(TypeError):
        TE.tokenize_prompts("one prompt", Tok())


def test_float64_restatement_reproduces_the_reference(gold, dist, sd):
    sd64 = XC.to64(sd)
    for skip in XC.T0_SKIPS:
        name = f"out_skip{skip}"
        z64 = XC.forward_tokens64(sd64, XC.T0, gold["tokens"], skip)
        assert tuple(z64.shape) == (2, 231, 128)
        d = float((torch.from_numpy(gold[name]).double() - z64).abs().max())
        print(f"  {name}: |reference - float64| {d:.3e}  stored {dist[name]:.3e}")
        assert d <= dist[name] * (1 + 1e-9) + 1e-12, name
        assert 1e-7 < dist[name] < 1e-5                            # fp32 rounding of a three-layer tower, not a disagreement
    # hidden_states has layers + 1 entries and clip_skip picks from its end
    out, hs = XC.clip_text64(sd64, XC.T0, gold["tokens"].reshape(6, 77), 0, hidden_states=True)
    assert len(hs) == XC.T0["layers"] + 1
    assert len(XC.clip_text64(sd64, XC.T0, gold["tokens"].reshape(6, 77), 3, hidden_states=True)[1]) == 2
    assert torch.equal(XC.clip_text64(sd64, XC.T0, gold["tokens"].reshape(6, 77), 1), out)      # clip_skip 1 is the default


def test_planted_mistakes_land_far_beyond_the_device_bar(gold, dist, sd):
    """The bar discriminates: each planted mistake in the restatement moves the output by at least PLANTED_FACTOR x the device's
    bar (four times ref_dist).  clip_skip off by one is planted at clip_skip 2 (at 0 it would be clip_skip 1, the same function)."""
    sd64 = XC.to64(sd)
    for plant in XC.PLANTED:
        skip = 2 if plant == "clip-skip-off-by-one" else 0
        right = XC.forward_tokens64(sd64, XC.T0, gold["tokens"], skip)
        wrong = XC.forward_tokens64(sd64, XC.T0, gold["tokens"], skip, plant=plant)
        bar = XC.bar4(dist[f"out_skip{skip}"])
        d = float((wrong - right).abs().max())
        print(f"  {plant:22s} moves the output by {d:.3e} = {d / bar:.0f} x the bar {bar:.3e}")
        assert d >= XC.PLANTED_FACTOR * bar, plant


def test_loader_rules(sd):
    plain = TE.load_clip_text_tensors(sd, XC.T0, prefix="")
    assert list(plain) == list(sd) and all(torch.equal(plain[k], sd[k]) and plain[k].dtype == torch.float32 for k in sd)
    ckpt = {f"cond_stage_model.transformer.text_model.{k}": v.double() for k, v in sd.items()}
    ckpt["cond_stage_model.transformer.text_model.embeddings.position_ids"] = torch.arange(77)[None]      # ignored
    ckpt["model.diffusion_model.out.2.bias"] = torch.zeros(4)
    with_tm = TE.load_clip_text_tensors(ckpt, XC.T0)               # the default prefix is the SD checkpoint's
    assert all(torch.equal(with_tm[k], sd[k]) for k in sd) and len(with_tm) == len(sd)
    no_tm = TE.load_clip_text_tensors({f"cond_stage_model.transformer.{k}": v for k, v in sd.items()}, XC.T0)
    assert all(torch.equal(no_tm[k], sd[k]) for k in sd)
    # the constructor raises each of these before it asks for a device
    lacking = {k: v for k, v in sd.items() if k != "encoder.layers.1.mlp.fc2.bias"}
    with pytest.raises(KeyError, match="encoder.layers.1.mlp.fc2.bias"):
        TE.ClipTextEncoder(lacking, XC.T0, prefix="")
    with pytest.raises(KeyError, match="embeddings.token_embedding.weight"):
        TE.ClipTextEncoder(sd, XC.T0)                              # nothing under the default prefix
    bad = dict(sd)
    bad["encoder.layers.0.self_attn.q_proj.weight"] = torch.zeros((128, 64))
    with pytest.raises(ValueError, match="encoder.layers.0.self_attn.q_proj.weight"):
        TE.ClipTextEncoder(bad, XC.T0, prefix="")
    with pytest.raises(ValueError, match="multiple of heads"):
        TE.ClipTextEncoder(sd, dict(XC.T0, heads=3), prefix="")
    with pytest.raises(ValueError, match="head size 32"):
        TE.ClipTextEncoder(sd, dict(XC.T0, heads=4), prefix="")    # 32 is not a fused head size
    with pytest.raises(ValueError, match="clip_skip"):
        TE.ClipTextEncoder(sd, XC.T0, prefix="", clip_skip=5)      # hidden_states has 4 entries
    with pytest.raises(ValueError, match="clip_skip"):
        TE.ClipTextEncoder(sd, XC.T0, prefix="", clip_skip=-1)
    for extra in (dict(hidden_act="gelu"), dict(causal=False), dict(pre_ln=False), dict(projection_dim=64)):
        with pytest.raises(NotImplementedError):
            TE.clip_text_tensors(dict(XC.T0, **extra))
    assert TE.clip_text_tensors(dict(XC.T0, hidden_act="quick_gelu")) == TE.clip_text_tensors(XC.T0)
    with pytest.raises(KeyError):
        TE.clip_text_tensors({k: v for k, v in XC.T0.items() if k != "positions"})


def test_case_tables_cover_what_the_issue_lists():
    e = {(c["rows"], c["T"], c["C"], c["ldo"]) for c in XC.EMBED_CASES}
    assert e == {(1, 1, 4, 4), (77, 77, 128, 128), (462, 77, 768, 768), (10, 5, 128, 160), (70000, 77, 4, 4)}
    assert sum(c["bad"] for c in XC.EMBED_CASES) == 1
    for c in XC.EMBED_CASES:
        ids, tok, pos = XC.embed_input(c)
        ref, ok = XC.embed_reference(ids, tok, pos, c)
        assert int(ids[-1]) == c["vocab"] - 1 and (c["rows"] == 1 or int(ids[0]) == 0)
        assert int((~ok).sum()) == (2 if c["bad"] else 0) and bool(torch.isnan(ref[~ok]).all()) and bool(torch.isfinite(ref[ok]).all())
        if c["bad"]:
            assert sorted(int(ids[r]) for r in XC.EMBED_BAD_ROWS) == [-1, c["vocab"]]
    q = {(c["rows"], c["n"], c["ldx"], c["ldo"]) for c in XC.QGELU_CASES}
    assert q == {(1, 4, 4, 4), (77, 512, 512, 512), (462, 3072, 3072, 3072), (33, 128, 192, 160)}


def test_quick_gelu_bound_admits_fp32_and_rejects_mistakes():
    """The derived bound holds a CPU fp32 evaluation of the kernel's formula and the rounded float64 reference, and rejects 1.702
    -> 1.7, the tanh-form gelu and a dropped x; at -80 the fp32 exponential overflows and the quotient is a zero."""
    c = XC.QGELU_CASES[1]
    for kind in XC.QGELU_SETS:
        x = XC.qgelu_input(c, kind)
        ref, bound = XC.qgelu_reference(x)
        assert bool(torch.isfinite(ref).all())
        assert XC.worst_ratio(ref.float(), ref, bound) <= 1.0, kind
        cpu32 = x / (1.0 + torch.exp(-(torch.tensor(1.702, dtype=torch.float32) * x)))
        assert bool(torch.isfinite(cpu32).all()) and XC.worst_ratio(cpu32, ref, bound) <= 1.0, kind
        if kind in ("normal", "sweep"):
            x64 = x.double()
            assert XC.worst_ratio(x64 * torch.sigmoid(1.7 * x64), ref, bound) > 1.0
            assert XC.worst_ratio(torch.nn.functional.gelu(x64, approximate="tanh"), ref, bound) > 1.0
            assert XC.worst_ratio(torch.sigmoid(1.702 * x64), ref, bound) > 1.0
    x = XC.qgelu_input(c, "sweep")
    assert float(x.view(-1)[1]) == -80.0 and float(x.min()) == -100.0 and float(x.max()) == 100.0
    assert float(torch.exp(torch.tensor(80.0 * 1.702, dtype=torch.float32))) == float("inf")
    assert float(torch.tensor(-80.0) / (1.0 + torch.exp(torch.tensor(80.0 * 1.702, dtype=torch.float32)))) == 0.0


def test_c_entries_refuse_bad_arguments_without_a_device():
    L = _lib.lib()
    buf = (C.c_float * 4096)()
    a = (C.addressof(buf) + 15) // 16 * 16
    ok = dict(ids=a, tok=a, pos=a, out=a, ldo=8, rows=4, T=2, C=8, vocab=16)

    def embed(**kw):
        v = dict(ok, **kw)
        return L.ofx_clip_embed(v["ids"], v["tok"], v["pos"], v["out"], v["ldo"], v["rows"], v["T"], v["C"], v["vocab"], None)

    for key in ("ids", "tok", "pos", "out"):
        assert embed(**{key: None}) == SC.EINVAL, key
    assert embed(rows=-1) == SC.EINVAL and embed(T=0) == SC.EINVAL and embed(C=0) == SC.EINVAL and embed(vocab=0) == SC.EINVAL
    assert embed(ldo=4) == SC.EINVAL                               # ldo < C
    assert embed(C=6, ldo=8) == SC.EALIGN and embed(ldo=10) == SC.EALIGN
    assert embed(tok=a + 4) == SC.EALIGN and embed(pos=a + 8) == SC.EALIGN and embed(out=a + 4) == SC.EALIGN and embed(ids=a + 2) == SC.EALIGN
    assert embed(rows=0) == 0                                      # a successful no-op: nothing is launched
    assert embed(rows=0, tok=None) == SC.EINVAL                    # the arguments are still checked

    okq = dict(x=a, ldx=8, out=a, ldo=8, rows=4, n=8)

    def qg(**kw):
        v = dict(okq, **kw)
        return L.ofx_quick_gelu(v["x"], v["ldx"], v["out"], v["ldo"], v["rows"], v["n"], None)

    assert qg(x=None) == SC.EINVAL and qg(out=None) == SC.EINVAL
    assert qg(rows=-1) == SC.EINVAL and qg(n=0) == SC.EINVAL and qg(ldx=4) == SC.EINVAL and qg(ldo=4) == SC.EINVAL
    assert qg(n=6) == SC.EALIGN and qg(ldx=10) == SC.EALIGN and qg(ldo=10) == SC.EALIGN
    assert qg(x=a + 4) == SC.EALIGN and qg(out=a + 8) == SC.EALIGN
    assert qg(rows=0) == 0 and qg(rows=0, n=6) == SC.EALIGN
