"""The case table, the oracle and the checker of the split-bf16 direct convolutions' plain epilogue (bf16_check.py), as far as the
host can tell: every case reaches the plan it names under every precision, the table reaches every split-bf16 instantiation on
every A-side schedule it has, the conditions the bound rests on hold for the seeds chosen, every simulated bug is caught at every
case it concerns with the constants in force, and the rejections that are specific to these arithmetics.  CPU only; needs the
built library (ofx_conv2d_plan is pure: no device)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bf16_check as bc
import wino_check as wc

PTR = 0x10000                       # non-null, 256-byte aligned, never dereferenced
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECS = sorted(bc.FAMILY)
FAMS = ("x3", "x6")
CASE_FAM = [(c, f) for c in bc.CASES for f in FAMS]
CASE_FAM_IDS = [f"{c['name']}-{f}" for c, f in CASE_FAM]
K_FAM = {"x3": wc.K_DIRECT_BF16X3, "x6": wc.K_DIRECT_BF16X6}


def _plan(d, stats_cap=0, pool=0):
    from sd_animation_optical_flow_amd import _lib
    p = _lib.ConvPlan()
    return _lib.lib().ofx_conv2d_plan(C.byref(d), stats_cap, pool, C.byref(p)), p


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", bc.CASES, ids=bc.IDS)
def test_every_case_reaches_the_plan_it_names(c, prec):
    st, p = _plan(bc.descriptor(c, prec, lambda name: PTR))
    assert st == 0 and p.path == 0, (st, p.path)
    assert p.mode in (0, 2)                                              # these arithmetics have no scalar-coordinate schedule
    assert (p.bm, p.bn, p.bk, int(p.mode == 2)) == c["plan"][prec], (c["name"], prec, (p.bm, p.bn, p.bk, p.mode))
    # no paired pipelines and no split-K instance in these arithmetics, whatever workspace the descriptor carries
    assert p.prec == prec and p.ks == 1 and p.ksplit == 1
    Ho, Wo = bc.out_hw(c)
    assert p.ntiles == -(-c["cout"] // p.bn)
    if p.mode == 2:
        assert p.mtiles == c["B"] * -(-c["H"] // 8) * -(-c["W"] // 16)
        if c["name"].startswith("patch-over"):
            assert p.mtiles == 4 and (c["H"] % 8, c["W"] % 16) == (1, 1)   # four overhanging patches
    else:
        assert p.mtiles == -(-(c["B"] * Ho * Wo) // p.bm)


def test_the_workspace_cases_carry_a_workspace_that_fp32_would_use():
    ws = [c for c in bc.CASES if c["extra"].get("ws")]
    assert {c["name"] for c in ws} == {"gather-auto-ws", "small-grid-auto-ws"}
    d = bc.descriptor(bc.case("small-grid-auto-ws"), 0, lambda name: PTR)
    st, p = _plan(d)
    assert st == 0 and p.ksplit > 1                                      # the same descriptor in fp32 splits K: the workspace is no formality
    for prec in PRECS:
        d = bc.descriptor(bc.case("small-grid-auto-ws"), prec, lambda name: PTR)
        assert d.splitk_ws == PTR and d.splitk_ws_bytes == bc.WS_BYTES and _plan(d)[1].ksplit == 1


def _ktiles():
    """The split-bf16 rows of kTiles in conv.hip: {(bm, bn, bk, prec)}."""
    src = open(os.path.join(ROOT, "sd_animation_optical_flow_amd", "csrc", "conv.hip")).read()
    table = src[src.index("const TileInst kTiles[]"):]
    table = table[:table.index("};")]
    rows = re.findall(r"OFX_TILE\((\d+), (\d+), \d+, \d+, (\d+), (\d+), (\d+), (true|false)\)", table)
    assert all(ks == "1" and sk == "false" for _, _, _, prec, ks, sk in rows if int(prec) in bc.FAMILY)
    return {(int(bm), int(bn), int(bk), int(prec)) for bm, bn, bk, prec, _, _ in rows if int(prec) in bc.FAMILY}


def test_the_table_reaches_every_split_bf16_instantiation_on_every_schedule_it_has():
    tiles = _ktiles()
    assert len(tiles) == 13
    # which of them have a halo-patch form: asked of the launcher, on a layer that qualifies for it (3x3, whole 8x16 patches, 32 channels)
    patchable = set()
    for bm, bn, bk, prec in tiles:
        c = bc._c("probe", 2, 8, 16, 32, bn, 3, 3, None, tile=bk * 1000000 + bm * 1000 + bn)
        st, p = _plan(bc.descriptor(c, prec, lambda name: PTR))
        assert st == 0 and (p.bm, p.bn, p.bk, p.prec) == (bm, bn, bk, prec)
        if p.mode == 2:
            patchable.add((bm, bn, bk, prec))
    assert len(patchable) == 8
    cov = bc.covered()
    assert {s[:4] for s in cov if s[4] == 0} == tiles                    # the general gather: all 13
    assert {s[:4] for s in cov if s[4] == 1} == patchable                # the halo patch: each of the 8 that have one
    assert {s[:4] for s in cov} == tiles                                 # and nothing the library does not have


def test_the_pre_split_twin_shares_the_plan_except_on_the_bk32_tile():
    other = [c["name"] for c in bc.CASES if not bc.same_plan(c)]
    assert other == ["bk32-k324", "bk32-3x3-c48"]
    for name in other:
        assert bc.case(name)["plan"][1][2] == 32 and bc.case(name)["plan"][2][2] == 16
        assert bc.case(name)["plan"][3] == bc.case(name)["plan"][4]


def test_the_shapes_have_the_seams_they_are_there_for():
    c = bc.case
    assert bc.k_of(c("gather-64x64")) == 36 and 36 % 16 and (10 * 14) % 64 and (10 * 14) % 128 and 72 % 64      # K, M and N ragged
    assert bc.k_of(c("bk32-k324")) % 32 == 4
    assert c("bk32-3x3-c48")["c0"] % 32 == 16                            # a tap straddles 32-chunks
    assert bc.out_hw(c("stride2-3x3-96")) == (6, 7) and bc.out_hw(c("stride2-1x1")) == (5, 3) and bc.out_hw(c("stem-7x7-s2")) == (8, 12)
    assert not bool(bc.inputs("stem-7x7-s2", "x3")["x"][..., 3].any())   # Cin 3 + a zero channel
    assert bc.ldo_of(c("out-slice-126")) == 384 and c("out-slice-126")["cout"] == 126
    assert [bc.seam_axis(c(n)) for n in ("patch-3x3-128x64", "patch-1x5-128x128-x2", "patch-5x1-128x128-x2", "patch-1x5-seam-128x128-x2",
                                         "patch-over-128x64")] == [None, None, "y", "x", "x"]
    for name in ("patch-1x5-128x128-x2", "patch-5x1-128x128-x2", "patch-1x5-seam-128x128-x2"):
        assert (c(name)["c0"], c(name)["c1"]) == (32, 32)


@pytest.mark.parametrize("c,fam", CASE_FAM, ids=CASE_FAM_IDS)
def test_the_conditions_of_the_bound_hold_for_the_seeds_chosen(c, fam):
    """`reference` asserts them itself (|shift| + |addend| + |res| <= M's convolution part, unsaturated activations, exact three-way
    splits, lo == 0 of the exact cases, M >> |ref| of the spread cases); here they are looked at again, with the figures."""
    r = bc.reference(c["name"], fam)
    e = c["extra"]
    print(f"{c['name']} {fam}: |v| < 2 at {r.unsaturated:.3f}, min M {float(r.mag.min()):.3g}, mean M / mean |out| {float(r.mag.mean() / r.out.abs().mean()):.3g}")
    assert tuple(r.out.shape) == (c["B"], *bc.out_hw(c), c["cout"]) and r.out.dtype == torch.float64
    assert bool(torch.isfinite(r.out).all()) and float(r.mag.min()) > 0
    if e.get("act") in ("tanh", "sigmoid"):
        assert r.unsaturated >= 0.75
    for parts, whole in ((r.xp, r.x), (r.wp, r.t["w"])):
        assert len(parts) == (2 if fam == "x3" else 3)
        assert all(torch.equal(p, p.bfloat16().float()) for p in parts)  # every piece is a bfloat16 value
        if fam == "x6":
            assert torch.equal(sum(p.double() for p in parts), whole.double())
    if e.get("exact"):
        assert not bool(r.xp[-1].any()) and not bool(r.wp[-1].any())
        assert fam == "x3" or bool(r.xp[1].any())                        # x6: 16 mantissa bits, the mid piece is in use
        assert float(torch.as_tensor(r.extra).max()) == 0.0              # the accumulation bound alone
    if e.get("spread"):
        assert r.cancel > 16
        ex = torch.frexp(r.x[r.x != 0])[1]
        assert int(ex.max()) - int(ex.min()) >= 24                       # operands spread over 2^-12 ... 2^12
    if e.get("norm"):
        assert bool((r.x >= 0).all()) and 0.3 < float((r.x == 0).double().mean()) < 0.7 and r.t["nmean"].shape == (c["B"], c["c0"])


@pytest.mark.parametrize("c,fam", CASE_FAM, ids=CASE_FAM_IDS)
def test_the_checker_catches_every_simulated_bug(c, fam):
    r, K = bc.reference(c["name"], fam), K_FAM[fam]
    bugs = bc.simulated_bugs(c, fam)
    assert set(bugs) == bc.bugs_for(c, fam)
    print(f"{c['name']} {fam}: " + ", ".join(f"{k} {bc.ratio(r, v):.3g}" for k, v in bugs.items()))
    missed = [name for name, got in bugs.items() if not bc.violates(r, got, K)]
    assert not missed, missed
    # ... while the fp32 rounding of the right answer passes, as do the products the kernel forms summed in float64 (x6: the
    # derived term covers the three it drops) and in float32 (one admissible order of the fp32 accumulation)
    assert not bc.violates(r, r.out.float(), K)
    assert not bc.violates(r, r.epilogue(bc.products(c, r.xp, r.wp, fam))[1], K)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    acc32 = sum(F.conv2d(nchw(r.xp[i]), r.wp[j], stride=c["stride"], padding=(c["kh"] // 2, c["kw"] // 2)) for i, j in bc.PRODUCTS[fam])
    ev32 = r.epilogue(acc32.permute(0, 2, 3, 1).double())[1]
    print(f"{c['name']} {fam}: a float32 evaluation of the products stands at {bc.ratio(r, ev32):.3g} of {K}")
    assert not bc.violates(r, ev32, K)
    # half the allowance passes, three times the allowance does not
    allow = r.slope * K * wc.EPS * r.mag
    assert not bc.violates(r, r.out + 0.5 * allow, K) and not bc.violates(r, r.out - 0.5 * allow, K)
    assert bc.violates(r, r.out + 3.0 * allow, K)


def test_every_simulated_bug_is_exercised_in_both_families():
    common = {"lower_a_dropped_in_the_last_chunk", "lower_a_dropped_for_a_border_tap", "lower_a_dropped_in_the_second_segment",
              "lower_b_of_the_last_group_from_its_neighbour", "norm_applied_after_the_split", "columns_slipped_by_a_sub_tile"}
    seen = {f: set().union(*(bc.bugs_for(c, f) for c in bc.CASES)) for f in FAMS}
    assert seen["x3"] == common and seen["x6"] == common | {"mm_dropped", "lh_dropped"}
    # where each concerns the schedules: the chunk and weight-group bugs on the gather and the patch of every tile, the rest where it applies
    for f in FAMS:
        for bug in ("lower_a_dropped_in_the_last_chunk", "lower_b_of_the_last_group_from_its_neighbour"):
            sig = {bc.signature(c, p) for c in bc.CASES for p in PRECS if bc.FAMILY[p] == f and bug in bc.bugs_for(c, f)}
            assert sig == {s for s in bc.covered() if bc.FAMILY[s[3]] == f}, (f, bug)
        assert sum("lower_a_dropped_for_a_border_tap" in bc.bugs_for(c, f) for c in bc.CASES) >= 4
        assert sum("lower_a_dropped_in_the_second_segment" in bc.bugs_for(c, f) for c in bc.CASES) == 3
        assert sum("norm_applied_after_the_split" in bc.bugs_for(c, f) for c in bc.CASES) == 2
    assert all("mm_dropped" in bc.bugs_for(c, "x6") for c in bc.CASES)


def test_the_constants_are_wino_checks():
    assert [bc.K_of(p) for p in PRECS] == [wc.K_DIRECT_BF16X3] * 2 + [wc.K_DIRECT_BF16X6] * 2
    assert bc.DROPPED == 2.0 ** -26 + 2.0 ** -36 and bc.NORM_ULP == wc.EPS
    assert bc.DROPPED / wc.EPS < 0.26                                    # the derived term is a quarter of one unit of K
    from sd_animation_optical_flow_amd import ops
    assert {k: v for k, v in ops.CONV_PRECISIONS.items() if k.startswith("bf16")} == bc.PRECISIONS


def _with(d, **kw):
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_rejections_specific_to_the_split_bf16_arithmetics():
    from sd_animation_optical_flow_amd import raft
    from sd_animation_optical_flow_amd.weights import load_checkpoint
    base = bc.case("patch-3x3-128x64")
    desc = lambda prec, **kw: _with(bc.descriptor(base, prec, lambda name: PTR), **kw)
    gemm = bc._c("gemm", 1, 16, 16, 64, 128, 1, 1, None)
    batched = lambda prec: _with(bc.descriptor(gemm, prec, lambda name: PTR), nz=2, a_zs=16 * 16 * 64, w_zs=128 * 64, o_zs=16 * 16 * 128)
    # bf16x6_w finds its lo groups behind the WHOLE pre-split matrix of ONE problem: a batched GEMM is rejected, in that precision only
    assert [_plan(batched(p))[0] for p in (1, 2, 3, 4)] == [0, 0, 0, EINVAL]
    # beyond the five arithmetics
    assert _plan(desc(6))[0] == EINVAL and _plan(desc(-1))[0] == EINVAL
    # the paired-pipeline marker and a Winograd operand are not errors here: the split-bf16 modes ignore both and run their own tiles
    st, p = _plan(desc(1, tile=2032064064))
    assert st == 0 and (p.bm, p.bn, p.bk, p.ks, p.prec) == (64, 64, 16, 1, 1)
    st, p = _plan(desc(3, wino_w=PTR, wino4_w=PTR))
    assert st == 0 and p.path == 0 and p.prec == 3
    # the fused norm keeps its own rule: one segment
    two = bc.descriptor(bc.case("patch-1x5-128x128-x2"), 1, lambda name: PTR)
    two.nmean = two.nrstd = PTR
    assert _plan(two)[0] == EINVAL
    # OFX_EPI_FLOW: only the small network sends it through the conv launcher, and that network refuses the split-bf16 flags before
    # any device call -- no bf16 engine reaches that epilogue (bf16_check.py's header), so the table has no flow case
    sd = load_checkpoint("random-small:0")
    for kw in ({"precision": "bf16x3"}, {"precision": "bf16x6"}, {"volume_precision": "bf16x3"}, {"volume_precision": "bf16x6"}):
        with pytest.raises(ValueError, match="fp32"):
            raft.RaftEngine(sd, **kw)
    src = open(os.path.join(ROOT, "sd_animation_optical_flow_amd", "csrc", "raft_engine.cpp")).read()
    unsupported = re.search(r"constexpr int S_UNSUPPORTED = ([^;]*);", src).group(1)
    assert "OFX_RAFT_BF16X3" in unsupported and "OFX_RAFT_BF16X6" in unsupported
    assert src.count(".epi = OFX_EPI_FLOW") == 1 and src.index(".epi = OFX_EPI_FLOW") < src.index("S_UNSUPPORTED")   # the small network's fh2
