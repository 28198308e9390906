"""`RaftEngine(precision="fp16")` as far as the host can tell: the launcher's plan (ofx_conv2d_plan: the launcher's own validation
and rule, no operand read, no device) for the fp16 arithmetic on the GRU gate, norm-on-load and epilogue-statistics descriptors --
the case tables of gru_f16_check.py and test_gpu_encoder_norm_f16.py, and every convolution of the basic network's forward at the
benchmark's size and at a single pair -- what that arithmetic still rejects, the flags and the Python surface.  No GPU: the
descriptors carry dummy, aligned, never-dereferenced pointers."""
import ctypes as C
import inspect
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gru_check as gc   # noqa: E402
import gru_f16_check as gf   # noqa: E402
import test_gpu_encoder_norm_f16 as EN   # noqa: E402

PTR = 0x10000                       # non-null, 16-byte aligned, never dereferenced
EINVAL = -1
F16, F16_EPI = gf.PREC_F16, gf.PREC_F16_EPI      # the arithmetic a plan reports / the descriptor value that asks for the new epilogues
TILES = {(128, 128), (128, 64), (64, 64)}


def _lib():
    from sd_animation_optical_flow_amd import _lib
    return _lib


def _desc(B, H, W, c0, cout, kh, kw=None, stride=1, tile=0, precision=F16_EPI, **over):
    kw = kh if kw is None else kw
    d = _lib().ConvDesc()
    d.in0, d.ld0, d.c0, d.w = PTR, c0, c0, PTR
    d.out, d.ldo = PTR, cout
    d.B, d.Hin, d.Win = B, H, W
    d.Hout, d.Wout = (H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1
    d.Cout, d.KH, d.KW, d.stride, d.padH, d.padW = cout, kh, kw, stride, kh // 2, kw // 2
    d.tile, d.precision = tile, precision
    for name, v in over.items():
        setattr(d, name, v)
    return d


def _query(d, stats_cap=0, pool=0):
    p = _lib().ConvPlan()
    return _lib().lib().ofx_conv2d_plan(C.byref(d), stats_cap, pool, C.byref(p)), p


@pytest.mark.parametrize("c", gf.CASES, ids=gf.IDS)
def test_every_gate_case_plans_in_fp16_onto_the_kernel_it_is_there_for(c):
    """Before the gate epilogues existed in this arithmetic every one of these was OFX_EINVAL."""
    d = gc.descriptor(c, lambda name: PTR)
    assert d.precision == F16_EPI
    st, p = _query(d)
    assert st == 0, c["name"]
    got = dict(bm=p.bm, bn=p.bn, bk=p.bk, ks=p.ks, ksplit=p.ksplit, prec=p.prec, mode=p.mode)
    assert p.path == 0 and got == c["plan"], (c["name"], got)
    # the Winograd operands are ignored, as for every arithmetic but fp32
    d.wino_w = d.wino4_w = PTR
    st, q = _query(d)
    assert st == 0 and q.path == 0 and (q.bm, q.bn, q.bk, q.mode) == (p.bm, p.bn, p.bk, p.mode)


def test_gate_table_reaches_every_tile_schedule_and_mask():
    sigs = {gc.signature(c) for c in gf.CASES}
    for epi in gf.ZRQ:
        assert {(s[1], s[2], s[3]) for s in sigs if s[0] == epi and s[7] == 2} >= {(128, 128, 16), (128, 64, 16), (64, 64, 16)}   # halo patch
        assert {(s[1], s[2], s[3]) for s in sigs if s[0] == epi and s[7] == 1} >= {(128, 128, 32), (128, 64, 32), (64, 64, 32)}   # scalar coordinates
        assert {s[7] for s in sigs if s[0] == epi} == {0, 1, 2}
        for mode in (0, 1, 2):
            assert {s[8] for s in sigs if s[0] == epi and s[7] == mode} == {False, True}, (epi, mode)       # whole tiles and masked ones
    assert all(s[4] == F16 and s[5] == 1 and not s[6] for s in sigs)
    assert {c["map"] for c in gf.CASES} == {"W", "R", "D"} and {c["layout"] for c in gf.CASES} == {"basic", "tiny"}


@pytest.mark.parametrize("layout,epi,filt,mp", sorted({(c["layout"], c["epi"], c["filt"], c["map"]) for c in gf.CASES}))
def test_gate_oracle_inputs_and_an_fp32_evaluation(layout, epi, filt, mp):
    """The input condition holds before and after rounding (`reference` asserts it); an fp32 evaluation over the rounded operands is
    one admissible summation order of exact products -- inside the bound.  (At K = 1280 the bound, K 2^-24 M, is as wide as the
    operand rounding itself, ~2^-11.5 sqrt(K) of an rms product: unlike f16_check's small-K cases it cannot tell rounded from unrounded
    operands; that the fp16 kernel ran is held on the device by the bits differing from the fp32 launch.)"""
    r = gf.reference(layout, epi, filt, mp)
    base = gc.reference(layout, epi, filt, mp)
    assert base.unsaturated >= 0.75 and r.unsaturated >= 0.75 and max(base.vmax, r.vmax) < 8
    c = next(c for c in gf.CASES if (c["layout"], c["epi"], c["filt"], c["map"]) == (layout, epi, filt, mp))
    v32 = (gc._conv(r.x.float(), r.w.float(), filt, mp).float() + r.add.float()).double()     # operands rounded, float32 result
    assert not gc.violates(r, r.gates(v32), gf.K_of(c))
    wrong = {k: torch.roll(v, 1, 0) for k, v in r.out.items()}           # ... and the bound is no formality: another row's gates are outside
    assert gc.violates(r, wrong, gf.K_of(c))


def test_norm_on_load_and_statistics_cases_plan_in_fp16():
    for tile, ch, plans in EN.NORM_CASES:
        for (H, W), want in plans.items():
            assert EN._plan_of(3, H, W, ch, 96, 3, 1, tile, True)[0] == want, (tile, ch, H, W)
    for c in EN.STATS_CASES:
        need = c["B"] * c["rows"] * c["cout"] * 2
        got = EN._plan_of(c["B"], c["H"], c["W"], c["cin"], c["cout"], c["k"], c["stride"], c["tile"], c["norm"], stats_cap=need)
        assert got == (c["plan"], c["rows"]), (c["name"], got)
        # a buffer one float short: no statistics, the same kernel
        assert EN._plan_of(c["B"], c["H"], c["W"], c["cin"], c["cout"], c["k"], c["stride"], c["tile"], c["norm"], stats_cap=need - 1) == (c["plan"], 0)
    # every fp16 tile with and without the fused norm, on and off the patch; both arms compiled at a lower occupancy
    plans = {(c["plan"], c["norm"]) for c in EN.STATS_CASES}
    assert {p[:2] for p, _ in plans} == TILES and {p[3] for p, _ in plans} == {0, 1, 2} and {n for _, n in plans} == {False, True}
    norm32 = {want[:3] for _, _, pl in EN.NORM_CASES for want in pl.values() if want[2] == 32}
    assert {(128, 128, 32), (128, 64, 32)} <= norm32


def test_what_fp16_still_rejects():
    base = dict(B=2, H=8, W=16, c0=64, cout=64, kh=3)
    ok = lambda **kw: _query(_desc(**dict(base, **kw)))[0]
    gru = dict(aux_z=PTR, aux_rh=PTR, aux_h=PTR, ldh=64)
    flow = dict(aux_coords=PTR, aux_h=PTR, aux_flow4=PTR, cout=2)
    assert ok() == 0 and ok(epi=1, **gru) == 0 and ok(epi=2, **gru) == 0 and ok(nmean=PTR, nrstd=PTR) == 0
    assert _query(_desc(**base), stats_cap=1 << 40)[0] == 0
    assert ok(splitk_ws=PTR, splitk_ws_bytes=1 << 40) == EINVAL                      # split-K ...
    assert ok(epi=1, splitk_ws=PTR, splitk_ws_bytes=1 << 40, **gru) == EINVAL        # ... with a gate epilogue too
    assert _query(_desc(**dict(base, precision=0, splitk_ws=PTR, splitk_ws_bytes=1 << 40)))[1].ksplit > 1
    assert ok(tile=2032064064) == EINVAL and ok(tile=2032064064, epi=2, **gru) == EINVAL   # the paired pipelines (KS = 2)
    assert ok(epi=3, **flow) == EINVAL and ok(precision=0, epi=3, **flow) == 0       # OFX_EPI_FLOW: the small network's
    assert _query(_desc(1, 16, 16, 256, 256, 1), pool=1)[0] == EINVAL                # the pooled volume
    assert _query(_desc(1, 16, 16, 256, 256, 1, precision=0), pool=1)[0] == 0
    assert ok(nz=2) == EINVAL                                                        # batched GEMM
    assert ok(nmean=PTR, nrstd=PTR, epi=1, **gru) == EINVAL                          # (any arithmetic: the fused norm has the plain epilogue only)
    assert ok(epi=1, aux_z=PTR, aux_rh=PTR, aux_h=PTR, ldh=48, cout=96) == EINVAL    # a z | r split inside a 32-column sub-tile
    # OFX_PREC_F16 itself keeps every rejection it documents: the new epilogues are asked for with OFX_PREC_F16_EPI
    assert ok(precision=F16) == 0
    assert ok(precision=F16, epi=1, **gru) == EINVAL and ok(precision=F16, epi=2, **gru) == EINVAL
    assert ok(precision=F16, nmean=PTR, nrstd=PTR) == EINVAL
    assert _query(_desc(**dict(base, precision=F16)), stats_cap=1 << 40)[0] == EINVAL
    assert ok(precision=F16 | 512) == EINVAL and ok(precision=256) == EINVAL and ok(precision=6) == EINVAL
    from sd_animation_optical_flow_amd import ops
    assert ops.CONV_PRECISIONS["fp16_epi"] == F16_EPI == 261 and ops.CONV_PRECISIONS["fp16"] == F16
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ofx.h")).read()
    assert "#define OFX_PREC_F16_EPI (OFX_PREC_F16 | 256)" in hdr


def basic_forward_convs(B, H, W):
    """Every ofx_conv2d descriptor of the basic network's forward (raft_engine.cpp: run_encoder for fnet -- instance norm -- and
    cnet -- folded BatchNorm --, run_recurrence, conv_tanh_relu, the mask head) on B pairs of H x W frames, as
    (name, keyword arguments of _desc, wants statistics)."""
    out = []
    for enc, inorm in (("fnet", True), ("cnet", False)):
        chunk = max(1, min(64, ((1 << 31) - 4096) // ((H // 2) * (W // 2) * 64 * 4)))      # images per encoder pass (enc_chunk)
        n = min(2 * B if inorm else B, chunk)
        plain = {} if inorm else dict(act=1)
        out.append((f"{enc}.conv1", dict(B=n, H=H, W=W, c0=4, cout=64, kh=7, stride=2, **plain), inorm))
        h, w, cin, stem_raw = H // 2, W // 2, 64, inorm
        for li, dim in ((1, 64), (2, 96), (3, 128)):
            for bi in range(2):
                s = 2 if (li > 1 and bi == 0) else 1
                p = f"{enc}.layer{li}.{bi}"
                nm = dict(nmean=PTR, nrstd=PTR)
                out.append((p + ".conv1", dict(B=n, H=h, W=w, c0=cin, cout=dim, kh=3, stride=s, **(nm if stem_raw else {}), **plain), inorm))
                if s == 2:
                    out.append((p + ".down", dict(B=n, H=h, W=w, c0=cin, cout=dim, kh=1, stride=2), inorm))
                h, w = h // s, w // s
                out.append((p + ".conv2", dict(B=n, H=h, W=w, c0=dim, cout=dim, kh=3, **(nm if inorm else dict(act=1, res=PTR, ldres=dim))), inorm))
                cin, stem_raw = dim, False
        if inorm:
            out.append((f"{enc}.conv2", dict(B=n, H=h, W=w, c0=128, cout=256, kh=1), False))
        else:
            out.append((f"{enc}.conv2.tanh", dict(B=n, H=h, W=w, c0=128, cout=128, kh=1, act=3, ldo=384), False))
            out.append((f"{enc}.conv2.relu", dict(B=n, H=h, W=w, c0=128, cout=128, kh=1, act=1, ldo=384), False))
    h, w = H // 8, W // 8
    u = dict(B=B, H=h, W=w)
    for i, co in enumerate((256, 128, 256, 128)):
        k = dict(kh=1, kw=5) if i < 2 else dict(kh=5, kw=1)
        out.append((f"gru.inp{i}", dict(c0=128, ld0=384, cout=co, ldo=768, **k, **u), False))
    out += [("convf1", dict(c0=16, cout=128, kh=1, kw=7, act=1, **u), False), ("convf2", dict(c0=128, cout=64, kh=3, act=1, ldo=256, **u), False),
            ("convc1", dict(c0=336, cout=256, kh=1, act=1, **u), False), ("convc2", dict(c0=256, cout=192, kh=3, act=1, ldo=256, **u), False),
            ("conv", dict(c0=256, cout=126, kh=3, act=1, ldo=384, **u), False)]
    for pass_, k in ((1, dict(kh=1, kw=5)), (2, dict(kh=5, kw=1))):
        out.append((f"gru.zr{pass_}", dict(c0=256, ld0=384, cout=256, epi=1, addend=PTR, ldadd=768, aux_z=PTR, aux_rh=PTR, aux_h=PTR, ldh=384, **k, **u), False))
        out.append((f"gru.q{pass_}", dict(c0=128, ld0=128, in1=PTR, ld1=384, c1=128, cout=128, epi=2, addend=PTR, ldadd=768, aux_z=PTR, aux_h=PTR,
                                         ldh=384, **k, **u), False))
    out += [("fh1", dict(c0=128, ld0=384, cout=256, kh=3, act=1, **u), False), ("mask0", dict(c0=128, ld0=384, cout=256, kh=3, act=1, **u), False),
            ("mask2", dict(c0=256, cout=576, kh=1, **u), False)]
    return out


@pytest.mark.parametrize("B,H,W", [(64, 512, 768), (1, 512, 768), (2, 128, 160), (1, 136, 168)])
def test_every_convolution_of_the_basic_forward_plans_in_fp16(B, H, W):
    """No split-K workspace in this mode: every descriptor runs unsplit on one of the three fp16 tiles; the gate layers of a batch
    that fills the chip take the 128-row tiles on the halo patch."""
    modes = {0: 0, 1: 0, 2: 0}
    for name, kw, stats in basic_forward_convs(B, H, W):
        st, p = _query(_desc(precision=F16_EPI, wino_w=PTR, wino4_w=PTR, **kw), stats_cap=(1 << 40) if stats else 0)
        assert st == 0, name
        assert p.path == 0 and p.prec == F16 and (p.bm, p.bn) in TILES and p.bk in (16, 32) and p.ks == 1 and p.ksplit == 1, name
        modes[p.mode] += 1
        st32, p32 = _query(_desc(precision=0, **kw), stats_cap=(1 << 40) if stats else 0)
        assert st32 == 0, name
        if stats:
            assert (p.stats_rows > 0) == (p32.stats_rows > 0), name
        if B == 64 and name.startswith("gru."):
            assert (p.bm, p.bk, p.mode) == (128, 16, 2), (name, p.bm, p.bn, p.bk, p.mode)
    print(f"B {B} {H}x{W}: launches by schedule: general {modes[0]}, scalar {modes[1]}, patch {modes[2]}")
    assert modes[2] > 0 or (H // 8) % 8 or (W // 8) % 8                  # (a 17 x 21 map has no whole patch at any encoder stage)


def test_flags_and_python_surface():
    from sd_animation_optical_flow_amd import ofgen, pdcnet_of, raft
    assert "fp16" in raft.PRECISIONS and raft.PRECISIONS["fp16"] == raft.FLAG_F16 == 4096
    assert {k: raft.PRECISIONS[k] for k in ("fp32", "bf16x3", "bf16x6")} == {"fp32": 0, "bf16x3": 16, "bf16x6": 64}
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ofx.h")).read()
    assert "#define OFX_RAFT_F16 4096" in hdr
    L = _lib().lib()
    # the workspace query accepts the flag (alone and with the independent volume modes) and the layout does not depend on it
    base = L.ofx_raft_workspace_bytes_mode(None, 0, 2, 128, 160, 0)
    assert base > 0
    for extra in (0, 512, 1024, 8, 2 | 32, 2048):
        assert L.ofx_raft_workspace_bytes_mode(None, 0, 2, 128, 160, 4096 | extra) == L.ofx_raft_workspace_bytes_mode(None, 0, 2, 128, 160, extra) > 0
    assert L.ofx_raft_workspace_bytes_mode(None, 0, 2, 128, 160, 8192) == 0
    assert L.ofx_raft_workspace_bytes_mode(None, 3, 2, 128, 160, 4096) == L.ofx_raft_workspace_bytes_mode(None, 3, 2, 128, 160, 0) > 0
    # docstrings state what is and is not rounded
    doc = raft.RaftEngine.__init__.__doc__
    for needle in ("'fp16'", "OPERANDS", "activations in memory", "correlation volume", "flow head", "upsample", "SUBSET of autocast"):
        assert needle in doc, needle
    assert "fp16" in pdcnet_of.create_of_algo.__doc__
    assert inspect.signature(ofgen.create_of_algo).parameters["precision"].default == "fp32"
    assert inspect.signature(ofgen.RAFT_2.__init__).parameters["mixed_precision"].default is False
    # the precision is looked at before the checkpoint is read
    with pytest.raises(ValueError, match="precision"):
        pdcnet_of.create_of_algo("/nonexistent/checkpoint.pth", precision="fp17")
    with pytest.raises(ValueError, match="precision"):
        ofgen.create_of_algo("/nonexistent/checkpoint.pth", precision="half")


def test_small_network_rejects_fp16_before_the_device():
    from sd_animation_optical_flow_amd import ofgen, raft
    from sd_animation_optical_flow_amd.weights import load_checkpoint
    sd = load_checkpoint("random-small:0")
    with pytest.raises(ValueError, match="fp32"):
        raft.RaftEngine(sd, precision="fp16")
    with pytest.raises(ValueError, match="fp32"):
        ofgen.RAFT_2(model=sd, mixed_precision=True)
    with pytest.raises(ValueError, match="fp32"):
        ofgen.RAFT_2(model="random-small:0", mixed_precision=True)


def test_bf16_and_f16_flags_together_are_rejected():
    """OFX_RAFT_F16 with OFX_RAFT_BF16X3 / _BF16X6 is OFX_EINVAL.  One precision per engine: the Python surface cannot express the
    combination (distinct flag bits, one key of PRECISIONS per engine); the header states the rule; the C entry points are held
    to it with raw flags on the device by tests/test_gpu_raft_f16.py (an engine handle needs a device)."""
    from sd_animation_optical_flow_amd import raft
    assert raft.FLAG_F16 & (raft.FLAG_BF16X3 | raft.FLAG_BF16X6 | raft.FLAG_VOL_BF16X3 | raft.FLAG_VOL_BF16X6 | raft.FLAG_FLOW_INIT) == 0
    assert len(set(raft.PRECISIONS.values())) == len(raft.PRECISIONS)
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "ofx.h")).read()
    assert "With OFX_RAFT_BF16X3 or _BF16X6: OFX_EINVAL" in hdr
    with pytest.raises(ValueError, match="precision"):
        raft.RaftEngine(load_basic(), precision="fp16+bf16x3")


def load_basic():
    from sd_animation_optical_flow_amd.weights import load_checkpoint
    return load_checkpoint("random:0")
