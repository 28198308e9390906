"""The case table, the oracle and the checker of the direct kernels' GRU gate epilogues (gru_check.py), and the launcher's
rejection of a z | r split inside a 32-column sub-tile.  CPU only; needs the built library (ofx_conv2d_plan is pure: no device)."""
import ctypes as C

import pytest
import torch

import gru_check as gc
import wino_check as wc

PTR = 0x10000                       # non-null, 256-byte aligned, never dereferenced
EINVAL = -1
ZR, Q = gc.EPI_ZR, gc.EPI_Q


def _plan(d):
    from sd_animation_optical_flow_amd import _lib
    p = _lib.ConvPlan()
    return _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 0, C.byref(p)), p


@pytest.mark.parametrize("c", gc.CASES, ids=gc.IDS)
def test_every_case_reaches_the_plan_it_names(c):
    st, p = _plan(gc.descriptor(c, lambda name: PTR, PTR))
    assert st == 0 and p.path == 0, (st, p.path)
    assert dict(bm=p.bm, bn=p.bn, bk=p.bk, ks=p.ks, ksplit=p.ksplit, prec=p.prec, mode=p.mode) == c["plan"]
    s = gc.spec(c["layout"], c["epi"], c["filt"])
    B, H, W = gc.MAPS[c["map"]]
    if p.mode == 2 and gc.masked(c):                                     # overhanging patches: R gives four of 8x16, two of 16x16
        assert p.mtiles == (2 if p.bm == 256 else 4) and c["map"] == "R"
    assert p.ntiles == -(-s["cout"] // p.bn)
    if c["layout"] == "small" and c["epi"] == ZR and (p.bm, p.bn) == (64, 64):
        assert p.ntiles == 3 and p.bn < s["hd"] < 2 * p.bn               # the z | r boundary inside N tile 1


def _required():
    """The instantiation rows of the table, restated by hand: (epi, bm, bn, bk, prec, ks, split-K, mode, masked)."""
    req = set()

    def row(epis, bm, bn, bk, where, prec=0, ks=1, sk=False):
        for epi in epis:
            for mode, masked in where:
                req.add((epi, bm, bn, bk, prec, ks, sk, mode, masked))

    both, scalar, patch, gather = (ZR, Q), ((1, False), (1, True)), ((2, False), (2, True)), ((0, False), (0, True))
    whole_patch = ((2, False), (1, True))                                # the 8x8 patch on W and D, scalar coordinates on R
    row(both, 64, 64, 32, scalar, ks=2)                                  # basic: auto and 2032064064
    row(both, 64, 64, 32, whole_patch, sk=True)
    row(both, 64, 64, 32, whole_patch)
    row(both, 64, 64, 16, scalar)
    for bm, bn in ((128, 128), (128, 64), (256, 64)):
        row(both, bm, bn, 16, patch)
    for bn in (128, 64):
        row(both, 128, bn, 32, scalar)
    row((ZR,), 128, 192, 16, patch)                                      # small
    row((ZR,), 128, 96, 16, patch)
    row(both, 128, 32, 32, scalar)
    row((ZR,), 64, 64, 32, gather, ks=2)                                 # tiny
    row((ZR,), 64, 64, 32, gather, sk=True)
    row((ZR,), 128, 64, 16, gather)
    row((Q,), 128, 32, 32, gather)
    for prec in (1, 2, 3, 4):                                            # the split-bf16 arithmetics
        row(both, 64, 64, 16, gather, prec=prec)
        row(both, 128, 128, 16, patch, prec=prec)
        row(both, 128, 64, 16, patch, prec=prec)
    row((Q,), 128, 128, 16, ((2, False), (0, True)), prec=1)             # 96 of 128 columns
    return req


def test_the_table_covers_every_instantiation_row():
    missing = _required() - gc.covered()
    assert not missing, sorted(missing)
    assert {c["plan"]["ksplit"] for c in gc.CASES} == {1, 3, 4}
    assert {(c["layout"], c["map"]) for c in gc.CASES} >= {("basic", m) for m in "WRD"} | {(l, m) for l in ("small", "tiny") for m in "WR"}
    # the three maps are what their names say
    assert gc.MAPS == {"W": (1, 8, 16), "R": (1, 9, 17), "D": (2, 16, 16)}


REF_KEYS = sorted({(c["layout"], c["epi"], c["filt"], c["map"], c["prec"] in gc.PREC_X3) for c in gc.CASES})


@pytest.mark.parametrize("key", REF_KEYS, ids=["-".join(str(k) for k in key) for key in REF_KEYS])
def test_no_case_saturates_its_gates(key):
    r = gc.reference(*key)                                               # (asserts the condition itself)
    print(key, f"|v| < 2: {r.unsaturated:.3f}, max |v| {r.vmax:.2f}")
    assert r.unsaturated >= 0.75 and r.vmax < 8


def _expected_bugs(c):
    p, s = c["plan"], gc.spec(c["layout"], c["epi"], c["filt"])
    names = {"rh_with_h_of_column_n"} if c["epi"] == ZR else {"z_of_the_next_row"}
    if c["epi"] == ZR and s["hd"] % p["bn"]:
        names.add("zr_exchanged_in_the_straddling_tile")
    if p["ksplit"] > 1:
        names.add("splitk_partial_dropped")
    if p["ks"] == 2:
        names.add("odd_k_chunks_dropped")
    if c["layout"] != "small":
        names.add("addend_at_the_wrong_offset")
    if c["map"] == "R":
        names.add("unwritten_on_the_masked_rows")
    if c["prec"] in gc.PREC_X3:
        names |= {"hi_lo_dropped", "lo_hi_dropped"}
    return names


@pytest.mark.parametrize("c", gc.CASES, ids=gc.IDS)
def test_the_checker_catches_every_simulated_bug(c):
    r, K = gc.ref_of(c), gc.K_of(c["prec"])
    bugs = gc.simulated_bugs(c)
    assert set(bugs) == _expected_bugs(c)
    missed = [name for name, got in bugs.items() if not gc.violates(r, got, K)]
    assert not missed, missed
    # ... while the float32 rounding of the right answer, and half the allowance on the pre-activation, pass
    assert not gc.violates(r, {k: v.float() for k, v in r.out.items()}, K)
    assert not gc.violates(r, r.gates(r.v + 0.5 * K * wc.EPS * r.mag), K)
    assert not gc.violates(r, r.gates(r.v - 0.5 * K * wc.EPS * r.mag), K)
    assert gc.violates(r, r.gates(r.v + 40.0 * K * wc.EPS * r.mag), K)    # (the gates do not swallow the pre-activation's error)


def test_every_simulated_bug_is_exercised():
    seen = set()
    for c in gc.CASES:
        seen |= _expected_bugs(c)
    assert seen == {"rh_with_h_of_column_n", "z_of_the_next_row", "zr_exchanged_in_the_straddling_tile", "splitk_partial_dropped",
                    "odd_k_chunks_dropped", "addend_at_the_wrong_offset", "unwritten_on_the_masked_rows", "hi_lo_dropped", "lo_hi_dropped"}


def test_the_split_bf16_constants_hold_their_conditions():
    assert wc.K_DIRECT_BF16X6 <= 3 * wc.K_DIRECT                         # fp32-accurate: test_conv2d_bf16x6_mode_is_fp32_accurate's criterion
    assert wc.K_DIRECT_BF16X3 > 0 and gc.K_of(0) == wc.K_DIRECT and gc.K_of(2) == wc.K_DIRECT_BF16X3 and gc.K_of(4) == wc.K_DIRECT_BF16X6


def test_the_cpu_split_is_the_librarys():
    """The oracle's bfloat16 split (torch's round-to-nearest-even cast, twice / three times) against the pre-split weight formats."""
    from sd_animation_optical_flow_amd import ops
    g = torch.Generator().manual_seed(5)
    w = torch.randn((64, 72, 3, 3), generator=g) * torch.exp(4.0 * torch.randn((64, 72, 3, 3), generator=g))
    wp = ops.pack_conv_weight(w)
    assert torch.equal(ops.split_conv_weight(wp).view(torch.int16).reshape(-1, 8), gc.split_weight_bits(wp))
    assert torch.equal(ops.split_conv_weight3(wp).view(torch.int16), gc.split_weight3_bits(wp))
    hi, mid, lo = gc.split3(wp)
    assert torch.equal(hi.double() + mid.double() + lo.double(), wp.double())   # three pieces are exact
    h2, l2 = gc.split2(wp)
    assert torch.equal(h2, hi) and torch.equal(l2, mid)


@pytest.mark.parametrize("cout,status", [(96, EINVAL), (80, EINVAL), (48, EINVAL), (64, 0), (192, 0), (256, 0)])
@pytest.mark.parametrize("tile", [0, 32128032, 16128064])
def test_a_zr_split_inside_a_32_column_sub_tile_is_rejected(cout, status, tile):
    """GRU_ZR decides z half or r half once per 32-column sub-tile: hd = Cout / 2 must be a multiple of 32 (hd 48 planned to a
    128x32 tile whose sub-tile at 32 stored r columns 48..63 as z, into the next row of aux_z)."""
    from sd_animation_optical_flow_amd import _lib
    d = _lib.ConvDesc()
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = 1, 8, 16, 8, 16, cout
    d.KH, d.KW, d.stride, d.padH, d.padW = 3, 3, 1, 1, 1
    d.in0 = d.w = d.aux_z = d.aux_rh = d.aux_h = PTR
    d.ld0 = d.c0 = 64
    d.ldh, d.epi, d.tile = cout, ZR, tile
    st, p = _plan(d)
    assert st == status
    d.epi = Q                                                            # the q epilogue has no halves: any Cout
    assert _plan(d)[0] == 0
