"""The case table, the oracle and the checker of the fp32 direct convolutions' plain epilogue (fp32_check.py), as far as the host can
tell: every case reaches exactly the plan it names, the table reaches every fp32 row of kTiles -- parsed out of conv.hip, not
remembered -- on every A-side schedule the row has and in each of the three kernel families, the conditions the bound rests on hold
for the seeds chosen, float32 evaluations of the reference on the CPU stay inside the bound, and every simulated bug stands outside
it at every case it lists.  CPU only; needs the built library (ofx_conv2d_plan is pure: no device)."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import fp32_check as fc
import wino_check as wc

PTR = 0x10000                       # non-null, 256-byte aligned, never dereferenced
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, S, P = fc.GATHER, fc.SCALAR, fc.PATCH


def _plan(d):
    from sd_animation_optical_flow_amd import _lib
    p = _lib.ConvPlan()
    return _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 0, C.byref(p)), p


def _plan_of(c):
    return _plan(fc.descriptor(c, lambda name: PTR, PTR))


def _probe(row, mp, c0, cout, filt, **kw):
    """A descriptor outside the table, on `row`: -> (status, plan)."""
    n = len(fc.CASES)
    try:
        fc._c("probe", mp, c0, cout, filt, row, 0, ksplit=2 if fc.ROWS[row][5] else 1, **kw)
        return _plan_of(fc.CASES[-1])
    finally:
        del fc.CASES[n:]


@pytest.mark.parametrize("c", fc.CASES, ids=fc.IDS)
def test_every_case_reaches_the_plan_it_names(c):
    st, p = _plan_of(c)
    assert st == 0 and p.path == 0 and p.prec == 0, (st, p.path, p.prec)
    print(f"{c['name']}: {p.bm}x{p.bn} BK {p.bk} KS {p.ks} ksplit {p.ksplit} {fc.MODE_NAME[p.mode]}, {p.mtiles} x {p.ntiles} tiles")
    assert (p.bm, p.bn, p.bk, p.ks, p.ksplit, p.mode) == c["plan"], c["name"]
    assert (p.bm, p.bn, p.bk, p.ks, p.ksplit > 1) == fc.row_key(c["row"])
    assert p.ntiles == -(-c["cout"] // p.bn)
    if p.mode == P:
        ph, pw = fc.patch_hw(c)
        assert p.mtiles == c["B"] * -(-c["H"] // ph) * -(-c["W"] // pw)
        assert c["stride"] == 1 and (c["c0"] + c["c1"]) % p.bk == 0 and c["c0"] % p.bk == 0      # what the schedule can serve
    else:
        assert p.mtiles == -(-fc.rows_of(c) // p.bm)
    if p.mode == S:                                                      # every chunk inside one tap and one segment
        assert (c["c0"] + c["c1"]) % p.bk == 0 and c["c0"] % p.bk == 0
    if c["extra"].get("ws"):
        assert p.ksplit > 1 and c["tile"] == 0                           # a workspace only where the plan uses it
        assert 65536 + p.mtiles * p.ntiles * p.ksplit * 64 * 64 * 4 <= fc.WS_BYTES


def _ktiles():
    """The fp32 rows of kTiles in conv.hip: [(bm, bn, bk, ks, sk)]."""
    src = open(os.path.join(ROOT, "sd_animation_optical_flow_amd", "csrc", "conv.hip")).read()
    table = src[src.index("const TileInst kTiles[]"):]
    table = table[:table.index("};")]
    assert table.count("OFX_TILE(") == len(re.findall(r"OFX_TILE\(\d+, \d+, \d+, \d+, \d+, \d+, \d+, (?:true|false)\)", table))
    rows = re.findall(r"OFX_TILE\((\d+), (\d+), \d+, \d+, (\d+), (\d+), (\d+), (true|false)\)", table)
    return [(int(bm), int(bn), int(bk), int(ks), sk == "true") for bm, bn, bk, prec, ks, sk in rows if int(prec) == 0]


def has_patch(bm, bn, bk, ks, sk):
    """tile_has_patch of conv.hip at PREC 0, restated."""
    return ks == 1 and ((bm == 128 and bk == 16 and not sk and bn in (64, 96, 128, 192)) or (bm == 64 and bn == 64 and bk == 32) or
                        (bm == 256 and bn == 64 and bk == 16 and not sk))


def has_scalar(bm, bn, bk, ks, sk):
    """tile_has_scalar of conv.hip at PREC 0, restated."""
    return bn != 192


def schedules(key):
    return {G} | ({S} if has_scalar(*key) else set()) | ({P} if has_patch(*key) else set())


def test_the_table_reaches_every_fp32_row_of_ktiles_on_every_schedule_and_in_every_family():
    tiles = _ktiles()
    assert len(tiles) == 12 and len(set(tiles)) == 12
    by_key = {fc.row_key(row): row for row in fc.ROWS}
    assert set(by_key) == set(tiles), "kTiles has an fp32 row that fp32_check.ROWS does not name, or the reverse"
    # the restatement against the launcher: a layer that qualifies for the halo patch (3x3, whole patches, 64 channels) and one that
    # qualifies only for scalar coordinates (the same at stride 2) get those schedules exactly where the restated rules say
    for key, row in by_key.items():
        auto = fc.ROWS[row][0] == 0
        st, p = _probe(row, "W", 64, 64, "3x3", auto=auto)
        assert st == 0 and (p.bm, p.bn, p.bk, p.ks, p.ksplit > 1) == key, (row, st)
        assert p.mode == (P if has_patch(*key) else S if has_scalar(*key) else G), (row, p.mode)
        st, p = _probe(row, "D", 64, 64, "3x3", stride=2, auto=auto)
        assert st == 0 and (p.bm, p.bn, p.bk, p.ks, p.ksplit > 1) == key, (row, st)
        assert p.mode == (S if has_scalar(*key) else G), (row, p.mode)
    # ... and over the table: the modes ofx_conv2d_plan returns per row are the schedules the restatement gives the row
    planned = {row: set() for row in fc.ROWS}
    for c in fc.CASES:
        planned[c["row"]].add(_plan_of(c)[1].mode)
    assert planned == {row: schedules(fc.row_key(row)) for row in fc.ROWS}
    cov = fc.covered()
    lines = []
    for row in fc.ROWS:
        key = fc.row_key(row)
        for mode in sorted(schedules(key)):
            n = {f: sum(c["row"] == row and c["plan"][5] == mode and c["fam"] == f for c in fc.CASES) for f in fc.FAMILIES}
            lines.append(f"{row:>11} {fc.MODE_NAME[mode]:>6}: " + ", ".join(f"{f} {n[f]}" for f in fc.FAMILIES))
            assert (row, "plain", mode) in cov, f"no OFX_EPI_PLAIN case on {row} {fc.MODE_NAME[mode]}"
        for fam in fc.FAMILIES:
            modes = {m for r, f, m in cov if r == row and f == fam}
            assert modes, f"no {fam} case on {row}"
            assert modes <= schedules(key)
            if fam != "plain":                                           # the patch where the row has one, and a schedule off it
                assert (P in modes) == has_patch(*key) and modes - {P}, (row, fam, modes)
    print("\n".join(lines))
    assert sum(len(schedules(fc.row_key(row))) for row in fc.ROWS) == 30


def test_removing_the_only_cover_of_a_row_and_schedule_is_noticed():
    """The coverage is a property of the table, not of its length: without `p-128x192-patch-200` the 128x192 row has no plain case on
    the halo patch."""
    only = [c for c in fc.CASES if (c["row"], c["fam"], c["plan"][5]) == ("128x192", "plain", P)]
    assert [c["name"] for c in only] == ["p-128x192-patch-200"]
    rest = {(c["row"], c["fam"], c["plan"][5]) for c in fc.CASES if c is not only[0]}
    assert ("128x192", "plain", P) not in rest


def test_the_table_holds_what_it_is_there_for():
    c = fc.case
    plans = lambda *names: [c(n)["plan"] for n in names]
    # 128x96 on the patch and the gather at Cout 96 and a ragged 200 (three N tiles); 128x192 without a scalar schedule; 128x32
    for name in ("p-128x96-patch-96", "p-128x96-patch-200", "p-128x96-gather-96", "p-128x96-gather-200"):
        assert c(name)["plan"][:2] == (128, 96) and c(name)["cout"] in (96, 200)
    assert -(-200 // 96) == 3 and 200 % 96 == 8 and 200 % 192 == 8
    assert not has_scalar(*fc.row_key("128x192")) and c("p-128x192-gather-x2")["c1"] == 32
    assert {x["cout"] for x in fc.CASES if x["row"] == "128x32"} == {2, 24}
    # 256x64: whole and overhanging 16x16 patches, and off the patch on both other schedules
    assert (fc.MAPS["D"][1] % 16, fc.MAPS["D"][2] % 16) == (0, 0) and (fc.MAPS["Q"][1] % 16, fc.MAPS["Q"][2] % 16) == (1, 2)
    assert [p[5] for p in plans("p-256x64-patch", "p-256x64-patch-over", "p-256x64-scalar-1x1", "p-256x64-scalar-s2", "p-256x64-gather")] == [P, P, S, S, G]
    assert fc.rows_of(c("p-256x64-scalar-1x1")) == 306                   # two 256-row tiles, the second ragged
    # split-K: the three schedules, ksplit 2, 3 and 4, ragged M and N
    sk = [x for x in fc.CASES if x["plan"][4] > 1]
    assert {x["plan"][5] for x in sk} == {G, S, P} and {x["plan"][4] for x in sk} == {2, 3, 4}
    assert all(x["tile"] == 0 and x["extra"]["ws"] for x in sk)
    for name, chunks in (("sk3-patch", 18), ("sk2-patch", 15), ("sk4-scalar", 27), ("sk2-gather", 13)):
        assert -(-fc.k_of(c(name)) // 32) == chunks
    assert c("sk2-gather")["c0"] % 32 and fc.rows_of(c("sk2-gather")) % 64 and c("sk2-gather")["cout"] % 64
    assert fc.rows_of(c("sk4-scalar")) == 153 and c("sk4-scalar")["cout"] == 120
    assert c("sk3-patch")["c0"] // 32 == 2                               # two slabs for three splits: the third parks a zero tile
    # paired pipelines: forced and automatic; one chunk, exactly two, an odd count
    ks2 = [x for x in fc.CASES if x["plan"][3] == 2]
    assert {x["tile"] for x in ks2} == {0, 2032064064} and not any(x["extra"].get("ws") for x in ks2)
    assert [-(-fc.k_of(c(n)) // 32) for n in ("ks2-forced-one-chunk", "ks2-forced-k36", "ks2-auto-9-chunks", "n-ks2-forced")] == [1, 2, 9, 3]
    # K edges
    assert fc.k_of(c("p-128x128-gather")) == 36 and fc.rows_of(c("p-128x128-gather")) == 140
    assert fc.k_of(c("p-128x128k32-k324")) % 32 == 4 and c("p-128x128k32-c48")["c0"] % 32 == 16
    # strides and taps
    assert fc.out_hw(c("p-128x128-scalar-s2")) == (9, 9) and fc.out_hw(c("auto-1x1-s2")) == (5, 9) and fc.out_hw(c("auto-stem-7x7-s2")) == (9, 9)
    assert not bool(fc.inputs("auto-stem-7x7-s2")["x"][..., 3].any())
    # two segments: a BK 16 and a BK 32 row, in the patch and off it
    two = {(x["plan"][2], x["plan"][5] == P) for x in fc.CASES if x["c1"]}
    assert two == {(16, True), (16, False), (32, True), (32, False)}
    assert any(x["c1"] and x["plan"][:3] in ((128, 128, 32), (128, 64, 32), (128, 32, 32)) for x in fc.CASES)
    # epilogue: ldadd > Cout, the out-slice on the gather, the patch and the 96- and 192-wide tiles
    assert all(fc.ldadd_of(c(n)) > c(n)["cout"] for n in ("e-addend-shift-gather", "e-addend-shift-patch"))
    sl = [x for x in fc.CASES if x["extra"].get("ldo")]
    assert all((x["cout"], fc.ldo_of(x), fc.out_off_of(x)) == (126, 384, 64) for x in sl)
    assert {(x["plan"][1], x["plan"][5]) for x in sl} == {(64, G), (128, P), (96, P), (192, G)}
    # sizes: nothing beyond 2x16x16 / 1x17x18 rows, channels 4 ... 96 (+ 32) but for the K-edge GEMM
    for x in fc.CASES:
        assert x["B"] * x["H"] * x["W"] <= 512
        assert x["c0"] in range(4, 97) or (x["c0"] == 324 and x["map"] == "E"), x["name"]
        assert x["c1"] in (0, 32)


def _with(d, **kw):
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_what_the_plan_does_not_admit():
    """fp32_check.py's header, held: Cout 72 never splits K; a tile that names a chunk length, or paired pipelines, that its row
    does not exist with is OFX_EINVAL, not another row."""
    d = _with(fc.descriptor(fc.case("sk4-scalar"), lambda name: PTR, PTR), Cout=72)
    st, p = _plan(d)
    assert st == 0 and (p.bm, p.bn, p.bk, p.ks, p.ksplit) == (128, 32, 32, 1, 1)
    base = fc.case("p-128x128-gather")
    for tile in (32128096, 32128192, 32256064, 16128032, 48064064, 2016064064, 2016128128, 2032128128):
        st, _ = _plan(_with(fc.descriptor(base, lambda name: PTR), tile=tile))
        assert st == EINVAL, tile
    for tile in (128096, 128192, 256064, 128032, 64064, 128128, 2000064064):   # no chunk length named: the row's own
        st, p = _plan(_with(fc.descriptor(base, lambda name: PTR), tile=tile))
        assert st == 0 and (p.bm * 1000 + p.bn) == tile % 1000000, tile
    # two segments are whole 32-channel chunks, so they qualify for scalar coordinates wherever the tile has them
    two = fc.case("p-128x128k32-scalar-x2")
    assert _plan(fc.descriptor(two, lambda name: PTR))[0] == 0
    assert _plan(_with(fc.descriptor(two, lambda name: PTR), c0=16, ld0=16))[0] != 0
    assert _plan(_with(fc.descriptor(two, lambda name: PTR), c1=48, ld1=48))[0] != 0
    # every forcing value of ROWS names its row as it stands
    for row, (tile, *key) in fc.ROWS.items():
        if tile:
            st, p = _plan(_with(fc.descriptor(base, lambda name: PTR), tile=tile))
            assert st == 0 and (p.bm, p.bn, p.bk, p.ks, p.ksplit > 1) == tuple(key), row


@pytest.mark.parametrize("c", fc.CASES, ids=fc.IDS)
def test_the_conditions_of_the_bound_hold_for_the_seeds_chosen(c):
    """`reference` asserts them itself; here they are looked at again, with the figures, and the oracle is held to
    wino_check.reference wherever that one applies (stride 1, no norm, no res, ReLU or no activation)."""
    r = fc.reference(c["name"])
    e, t = c["extra"], r.t
    print(f"{c['name']}: |v| < 2 at {r.unsaturated:.3f}, min M {float(r.mag.min()):.3g}, mean M / mean |out| {float(r.mag.mean() / r.out.abs().mean()):.3g}")
    assert tuple(r.out.shape) == (c["B"], *fc.out_hw(c), c["cout"]) and r.out.dtype == torch.float64
    assert bool(torch.isfinite(r.out).all()) and float(r.mag.min()) > 0
    side = sum((t[n].double().abs() for n in ("shift", "addend", "res") if t[n] is not None), torch.zeros_like(r.mag))
    assert bool((side <= r.mag - side).all())
    if e.get("act") in ("tanh", "sigmoid"):
        assert r.unsaturated >= 0.75 and r.slope == (1.0 if e["act"] == "tanh" else 0.25)
        assert float(torch.as_tensor(r.extra).min()) == wc.ACT_ULP
    if e.get("spread"):
        assert r.cancel > 16
        ex = torch.frexp(r.x[r.x != 0])[1]
        assert int(ex.max()) - int(ex.min()) >= 24                       # operands spread over 2^-12 ... 2^12
    if e.get("norm"):
        assert bool((r.x >= 0).all()) and 0.3 < float((r.x == 0).double().mean()) < 0.7 and t["nmean"].shape == (c["B"], c["c0"])
        assert float(torch.as_tensor(r.extra).max()) > 0
    elif e.get("act") not in ("tanh", "sigmoid"):
        assert float(torch.as_tensor(r.extra).max()) == 0.0              # the accumulation bound alone
    if c["stride"] == 1 and not e.get("norm") and not e.get("res") and e.get("act") in (None, "relu"):
        nchw = lambda v: None if v is None else v.permute(0, 3, 1, 2)
        ref, mag = wc.reference(nchw(t["x"]), t["w"], c["kh"], c["kw"], t["scale"], t["shift"], nchw(t["addend"]), e.get("act") == "relu")
        assert torch.allclose(nchw(r.out), ref, rtol=0, atol=1e-12) and torch.allclose(nchw(r.mag), mag, rtol=1e-13, atol=0)


def _f32(c, r, chunked):
    """The reference's convolution evaluated in float32 on the CPU: F.conv2d, or BK-wide chunks summed in the kernel's order."""
    nchw = r.x.permute(0, 3, 1, 2).contiguous()
    kw = dict(stride=c["stride"], padding=(c["kh"] // 2, c["kw"] // 2))
    if not chunked:
        return F.conv2d(nchw, r.t["w"], **kw).permute(0, 2, 3, 1)
    acc = None
    for keep in fc.chunk_masks(c, c["plan"][2]):
        part = F.conv2d(nchw, fc._masked(r.t["w"], keep), **kw)
        acc = part if acc is None else acc + part
    return acc.permute(0, 2, 3, 1)


_margins = {}


@pytest.mark.parametrize("c", fc.CASES, ids=fc.IDS)
def test_the_checker_catches_every_simulated_bug_and_passes_float32(c):
    r = fc.reference(c["name"])
    bugs = fc.simulated_bugs(c)
    assert set(bugs) == fc.bugs_for(c) and "last_chunk_dropped" in bugs
    ratios = {k: fc.ratio(r, v) for k, v in bugs.items()}
    _margins[c["name"]] = ratios
    print(f"{c['name']}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    missed = [name for name, got in bugs.items() if not fc.violates(r, got)]
    assert not missed, missed
    # ... while float32 evaluations of the right answer pass: its rounding, F.conv2d, and chunks of BK summed in the kernel's order
    assert not fc.violates(r, r.out.float())
    for chunked in (False, True):
        ev = r.epilogue(_f32(c, r, chunked).double())[1]
        print(f"{c['name']}: a float32 evaluation ({'chunked' if chunked else 'F.conv2d'}) stands at {fc.ratio(r, ev):.3g} of {fc.K_FP32}")
        assert not fc.violates(r, ev)
    # half the allowance passes, three times the allowance does not
    allow = r.slope * fc.K_FP32 * wc.EPS * r.mag
    assert not fc.violates(r, r.out + 0.5 * allow) and not fc.violates(r, r.out - 0.5 * allow)
    assert fc.violates(r, r.out + 3.0 * allow + 3.0 * torch.as_tensor(r.extra))


def test_every_simulated_bug_concerns_at_least_two_cases_and_the_narrowest_margin():
    names = {"last_chunk_dropped", "split_partial_missing", "split_partial_twice", "second_pipeline_dropped", "second_segment_four_off",
             "halo_staged_zero", "padding_normalised", "norm_relu_missing", "scale_after_shift", "res_before_activation",
             "columns_slipped_by_a_sub_tile"}
    count = {n: sum(n in fc.bugs_for(c) for c in fc.CASES) for n in names}
    assert set().union(*(fc.bugs_for(c) for c in fc.CASES)) == names
    assert all(v >= 2 for v in count.values()), count
    # where each concerns the table
    assert count["last_chunk_dropped"] == len(fc.CASES)
    assert count["split_partial_missing"] == count["split_partial_twice"] == sum(c["plan"][4] > 1 for c in fc.CASES)
    assert [c["name"] for c in fc.CASES if c["plan"][3] == 2 and "second_pipeline_dropped" not in fc.bugs_for(c)] == ["ks2-forced-one-chunk"]
    assert count["second_segment_four_off"] == sum(bool(c["c1"]) for c in fc.CASES)
    assert [c["name"] for c in fc.CASES if c["extra"].get("norm") and "padding_normalised" not in fc.bugs_for(c)] == ["n-128x64-scalar-1x1"]
    assert {fc.patch_hw(c) for c in fc.CASES if "halo_staged_zero" in fc.bugs_for(c)} == {(16, 16), (8, 16), (8, 8)}
    assert {fc.seam_axis(c) for c in fc.CASES if "halo_staged_zero" in fc.bugs_for(c)} == {"x", "y"}
    assert {c["plan"][1] for c in fc.CASES if "columns_slipped_by_a_sub_tile" in fc.bugs_for(c)} >= {96, 192}
    # the narrowest margin of the table: the smallest worst ratio of any bug at any case, against the constant
    worst = min(((fc.ratio(fc.reference(c["name"]), v), k, c["name"]) for c in fc.CASES for k, v in fc.simulated_bugs(c).items()))
    print(f"narrowest margin: {worst[1]} at {worst[2]} stands at {worst[0]:.4g} x 2^-24 M against K = {fc.K_FP32}")
    assert worst[0] > 100 * fc.K_FP32


def test_the_constants_are_wino_checks():
    assert fc.K_FP32 == wc.K_DIRECT == 11.0 and fc.NORM_ULP == wc.EPS
    from sd_animation_optical_flow_amd import ops
    assert ops.CONV_PRECISIONS["fp32"] == 0
