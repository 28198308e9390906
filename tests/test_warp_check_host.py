"""tests/warp_check.py on the CPU: the tables reach the branches they claim, every table meets the exemption cap, the fp32
restatements of oracle/warp_oracle.py stay inside the float64 bounds, and the checkers catch planted bugs at every case."""
import numpy as np
import pytest

import warp_check as wc
from oracle import warp_oracle as WO

U8_TABLES = dict(wc.ROUTE_TABLES, per_frame=wc.PER_FRAME_U8, bicubic=wc.BICUBIC_U8)
FLOAT_TABLES = {"f32-" + m: t for m, t in wc.FLOAT_CASES.items()}
ALL_TABLES = dict(U8_TABLES, **FLOAT_TABLES)

_inputs = {}


def inputs(c):
    if c not in _inputs:
        _inputs[c] = wc.make_inputs(c)
    return _inputs[c]


def correct_output(c):
    frame, flow = inputs(c)
    r, _, _ = wc.warp_reference(frame, flow, c.sign, c.mode)
    return wc.simulate_u8(r) if c.dtype == "u8" else r.astype(np.float32)


def test_the_route_rule_sends_every_case_where_its_table_says():
    for name, table in ALL_TABLES.items():
        for c in table + wc.CV2_CASES + [wc.STRIDE_WARP]:
            got = wc.route(c.H, c.W, c.B, c.C, c.per_frame, c.dtype, c.mode)
            if c.route is not None:
                assert got == c.route, (c.name, got)
    # the instantiations no earlier test launched
    gen = [c for t in ALL_TABLES.values() for c in t if c.route == "generic"]
    for dtype, mode, chans in (("u8", "bilinear", {1, 2, 4}), ("u8", "bicubic", {1, 2, 3, 4}), ("f32", "bilinear", {1, 2, 3, 4}), ("f32", "bicubic", {1, 2, 3, 4})):
        assert {c.C for c in gen if c.dtype == dtype and c.mode == mode} >= chans
    assert {(c.dtype, c.C) for c in wc.CV2_CASES} >= {("u8", 1), ("u8", 2), ("u8", 4), ("f32", 2), ("f32", 3), ("f32", 4)}
    assert any(c.dtype == "u8" and c.C == 3 and c.per_frame for c in wc.CV2_CASES)
    # per-frame frames on every route but the shared one, at B = 2, 3 and 5
    for rt in ("generic", "x4", "u8c3"):
        assert {c.B for c in wc.PER_FRAME_U8 if c.route == rt} >= {2, 3, 5}
    # the shared-frame kernel's 64 x 16 tile is crossed in both directions, and a ragged group of the x4 kernel exists
    assert any(c.W > 64 and c.H > 16 and c.W % 64 and c.H % 16 for c in wc.SHARED_U8)
    assert all(c.W % 4 for c in wc.X4_U8) and all(c.W % 4 == 0 for c in wc.U8C3_U8 + wc.SHARED_U8)
    for t in ALL_TABLES.values():
        assert {c.sign for c in t} == {1.0, -1.0}
    # the second grid-stride trips
    s = wc.STRIDE_WARP
    assert s.B * s.H * s.W > wc.GRID_CAP and s.B * s.H * s.W < wc.GRID_CAP * 1.01
    r = wc.STRIDE_RESIZE
    assert r.B * r.Hd * r.Wd * r.C > wc.GRID_CAP and r.B * r.Hd * r.Wd * r.C < wc.GRID_CAP * 1.01


@pytest.mark.parametrize("table", sorted(ALL_TABLES))
def test_the_planted_pixels_reach_every_branch(table):
    for c in ALL_TABLES[table]:
        _, flow = inputs(c)
        missing = wc.expected_branches(c) - wc.branches(c, flow)
        assert not missing, (c.name, sorted(missing))
        assert np.isfinite(flow).all()
    big = [c for c in ALL_TABLES[table] if c.B * c.H * c.W >= 24]
    assert big and all(wc.expected_branches(c) >= set(wc.BRANCHES) - {"inside"} for c in big)


@pytest.mark.parametrize("table", sorted(U8_TABLES))
def test_every_uint8_table_meets_the_exemption_cap_and_the_oracle_passes(table):
    total = exempt = 0
    for c in U8_TABLES[table]:
        frame, flow = inputs(c)
        n, cap = wc.check_u8(wc.oracle_warp(frame, flow, c.sign, c.mode), *wc.warp_reference(frame, flow, c.sign, c.mode), c.name)
        assert n <= cap
        wc.check_u8(correct_output(c), *wc.warp_reference(frame, flow, c.sign, c.mode), c.name)
        total, exempt = total + frame.shape[-1] * flow[..., 0].size, exempt + n
    print(f"{table}: {exempt} exempt of {total} bytes")


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_the_fp32_oracle_stays_inside_the_float64_bound(mode):
    worst = 0.0
    for c in wc.FLOAT_CASES[mode]:
        frame, flow = inputs(c)
        ratio, _, _ = wc.check_warp(wc.oracle_warp(frame, flow, c.sign, mode), frame, flow, c.sign, mode, c.name)
        worst = max(worst, ratio)
    print(f"{mode}: worst |error| / bound of the fp32 oracle {worst:.3f}")
    assert 0.01 < worst <= 1.0                                  # a bound the fp32 restatement never comes near would check nothing


def test_the_cubic_weight_error_covers_the_fp32_weights():
    t = np.concatenate([np.linspace(0, 1, 4097)[:-1], np.random.default_rng(1).random(20000)]).astype(np.float32)
    w, e = wc.cubic64(t)
    w32 = np.stack(WO.cubic_coeffs(t), -1).astype(np.float64)
    ratio = np.abs(w32 - w) / e
    assert ratio.max() <= 1.0 and e.max() < 64 * wc.U and np.abs(w.sum(-1) - 1).max() < 1e-15, (ratio.max(), e.max() / wc.U)
    assert (wc.cubic64(np.float32(0))[0] == [0, 1, 0, 0]).all() and (wc.cubic64(np.float32(0.5))[0] == [-0.09375, 0.59375, 0.59375, -0.09375]).all()


def invisible(bug, c):
    """Where a bug cannot show.  The buggy output is asserted to EQUAL the correct one there, so this cannot hide a blind checker.
    A frame of one pixel is symmetric: sampling at p + f and at p - f weighs it the same."""
    return bug == "sign" and c.H == 1 and c.W == 1


@pytest.mark.parametrize("bug", wc.WARP_BUGS)
def test_the_checker_catches_a_planted_bug_at_every_case(bug):
    seen = 0
    for table, cases in ALL_TABLES.items():
        for c in cases:
            if not wc.bug_concerns(bug, c):
                continue
            frame, flow = inputs(c)
            out = wc.buggy_output(c, frame, flow, bug)
            if invisible(bug, c):
                assert np.array_equal(out, correct_output(c)), (bug, c.name, "listed as invisible but the outputs differ")
                continue
            with pytest.raises(AssertionError):
                wc.check_warp(out, frame, flow, c.sign, c.mode, c.name)
            seen += 1
    assert seen >= 6, (bug, seen)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_resize_oracle_passes_and_planted_bugs_fail():
    invisible = {("zero_border", "6x6-to-6x6-b1-c4"), ("no_half", "6x6-to-6x6-b1-c4"), ("no_half", "1x1-to-5x3-b1-c4"),
                 ("zero_border", "5x3-to-1x1-b1-c4"), ("zero_border", "96x64-to-12x8-b1-c4")}
    # t = 0 puts no weight on a clamped tap; one source pixel has no offset to drop; 8 to 1 samples 8d + 2 .. 8d + 5, never the border
    worst = 0.0
    for c in wc.RESIZE_CASES:
        img = wc.resize_inputs(c)
        r, bound = wc.resize_reference(img, c.Hd, c.Wd)
        worst = max(worst, wc.check_float(wc.oracle_resize(img, c.Hd, c.Wd), r, bound, c.name))
        if (c.Hs, c.Ws) == (c.Hd, c.Wd):
            assert np.array_equal(r.astype(np.float32), img) and (bound >= 0).all()
        for bug in wc.RESIZE_BUGS:
            out = wc.resize_reference(img, c.Hd, c.Wd, bug)[0].astype(np.float32)
            if (bug, c.name) in invisible:
                assert np.array_equal(out, r.astype(np.float32)), (bug, c.name)
                continue
            with pytest.raises(AssertionError):
                wc.check_float(out, r, bound, c.name)
    print(f"resize_cubic: worst |error| / bound of the fp32 oracle {worst:.3f}")
    assert 0.01 < worst <= 1.0


def _fb_fp32(fw, bw, sigma):
    """fb_conf_kernel in numpy fp32, through the oracle's bilinear warp."""
    conf, logc = [], []
    B, H, W, _ = fw.shape
    inv = np.float32(1.0) / (np.float32(2.0) * np.float32(sigma) * np.float32(sigma))
    for b in range(B):
        mx = np.arange(W, dtype=np.float32)[None, :] + fw[b, :, :, 0]
        my = np.arange(H, dtype=np.float32)[:, None] + fw[b, :, :, 1]
        with np.errstate(over="ignore", invalid="ignore"):       # 1e30: the squares overflow; the oracle's int cast is out of range
            e = fw[b] + WO.warp_bilinear(bw[b], mx, my)
            lc = -(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) * inv
            logc.append(lc)
            conf.append(np.exp(lc))
    return np.stack(conf), np.stack(logc)


def test_fb_confidence_reference_tables_and_planted_bugs():
    worst = [0.0, 0.0]
    for c in wc.FB_CASES:
        fw, bw, planted = wc.fb_inputs(c)
        assert wc.fb_branches(fw) >= set(wc.FB_BRANCHES), (c.name, set(wc.FB_BRANCHES) - wc.fb_branches(fw))
        assert not np.array_equal(bw[0], bw[1]) and not np.array_equal(bw[1], bw[2])
        ref = wc.fb_reference(fw, bw, c.sigma)
        z = planted["zero"]
        assert ref["conf"][z] == 1.0 and ref["logc"][z] == 0 and ref["dlogc"][z] == 0
        assert ref["overflow"][planted["1e30"]] and not ref["overflow"][planted["1e6"]] and ref["conf"][planted["1e6"]] == 0
        assert np.median(ref["conf"][0]) > 0.9          # the consistent item: conf near 1
        conf, logc = _fb_fp32(fw, bw, c.sigma)
        rc, rl = wc.check_fb(conf, logc, ref, c.name)
        worst = [max(worst[0], rc), max(worst[1], rl)]
        for bug in wc.FB_BUGS:
            bad = wc.fb_reference(fw, bw, c.sigma, bug)
            with np.errstate(over="ignore"):
                bconf, blogc = bad["conf"].astype(np.float32), np.where(bad["overflow"], -np.inf, bad["logc"]).astype(np.float32)
            with pytest.raises(AssertionError):
                wc.check_fb(bconf, blogc, ref, c.name)
            with pytest.raises(AssertionError):                 # conf alone, which is what generate_mask thresholds
                wc.check_fb(bconf, logc, ref, c.name)
    print(f"fb_confidence: worst |error| / bound of an fp32 evaluation: conf {worst[0]:.3f}, logc {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


def test_travel_mask_reference_agrees_with_the_oracle_and_meets_the_cap():
    for c in wc.TRAVEL_CASES:
        conf, flow, dist, travel = wc.travel_inputs(c)
        assert (conf == np.float32(0.9)).sum() >= c.B * 4 and (conf < np.float32(0.9)).mean() > 0.2
        raw, tout = wc.travel_oracle(conf, flow, dist, travel, c.thres, c.mode)
        assert 0.05 < (raw == 255).mean() < 0.95 and ((tout == 0) & (raw == 0)).sum() == 0
        if c.mode == "cv2_cubic":
            continue
        ref = wc.travel_reference(conf, flow, dist, travel, c.thres, c.mode)
        assert ref["far"].any() and (~ref["far"] & ~ref["low"]).any()
        ratio, n, cap = wc.check_travel(raw, tout, ref, c.name)
        assert n <= cap and ratio <= 1.0
        with pytest.raises(AssertionError):                     # item 0's travel map for every item
            r2, t2 = wc.travel_oracle(conf, flow, dist, np.repeat(travel[:1], c.B, 0), c.thres, c.mode)
            wc.check_travel(r2, t2, ref, c.name)
