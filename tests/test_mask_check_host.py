"""tests/mask_check.py on the CPU: every case takes the route its table names (asked of the library's own plan, ofx_mask_plan, which
issues no HIP call), its inputs leave the mask unsaturated, its stamps come out as the element, and every simulated bug changes the
output of every case it concerns.  Then the plan itself, swept over batch sizes, shapes, element sizes and alignment."""
import itertools

import numpy as np
import pytest

import mask_check as mc
from oracle import mask_oracle as MO

PAIRS = [(c, k) for c in mc.CASES for k in c.ksizes]
IDS = [f"{c.name}-k{k}" for c, k in PAIRS]

_made = {}


def made(c, ksize):
    """inputs, per source the bitmap of the compared images' batch and the oracle's mask of the compared images: made once."""
    key = (c.name, ksize)
    if key not in _made:
        inp = (mc.conf_inputs if c.src == "conf" else mc.edge_inputs)(c, ksize)
        imgs = mc.compared(c, ksize)
        bits = {s: (mc.conf_bits(inp.conf, s) if c.src == "conf" else mc.edge_bits(inp.image)) for s in mc.sources(c)}
        want = {s: mc.oracle_dilate(bits[s], ksize, imgs) for s in mc.sources(c)}
        _made[key] = (inp, imgs, bits, want)
    return _made[key]


def test_every_case_takes_the_route_its_table_names():
    for c, k in PAIRS:
        for s in mc.sources(c):
            got, p = mc.planned_route(c, k, s)
            assert got == mc.expected_route(c, k), (c.name, k, got, p)
            if got[0] == "rows":
                assert p.threads == (512 if p.band == 64 else 256) and p.lds <= 65536
                if got[2] == "planes":
                    assert p.nplanes == mc.distinct_widths(k) and p.lds <= 49152, (c.name, k, p)
    # 8 distinct half widths are the most that run as planes; 29x29 at 16-row bands crosses 48 KiB between W = 928 and 932
    assert [mc.distinct_widths(k) for k in (27, 29, 31)] == [8, 8, 9]
    assert mc.plan(0, 2, 20, 928, 29)[1].lds == 48144 and mc.plan(0, 2, 20, 928, 29)[1].nplanes == 8
    assert mc.plan(0, 2, 20, 932, 29)[1].nplanes == -1
    routes = {mc.expected_route(c, k) for c, k in PAIRS if c.src == "conf"}
    assert {(r[1], r[2]) for r in routes if r[0] == "rows"} >= {(64, "planes"), (64, "direct"), (32, "planes"), (32, "direct"), (16, "planes"), (16, "direct")}
    assert {r[3] for r in routes if r[0] == "rows"} == {0, 1}
    for src in ("conf", "edges"):
        assert {mc.expected_route(c, k)[0] for c, k in PAIRS if c.src == src} >= {"narrow", "wide"}
    assert any(c.B != 1 and c.B % 8 for c in mc.CASES if c.kernel == "rows") and any(c.B != 1 and c.B % 8 for c in mc.CASES if c.kernel == "tile")
    # partial last bands at every band height, a ragged last XCD group, both tile kernels with more than one tile across and down
    for c in mc.CONF_CASES:
        if c.kernel == "rows" and c.H > c.band:
            assert c.H % c.band, c.name
    assert {c.band for c in mc.CONF_CASES if c.kernel == "rows" and c.H > c.band} == {16, 32, 64}
    assert any(c.xcd and c.B % 8 for c in mc.CONF_CASES)
    assert all(c.W > 64 and c.H > 32 for c in mc.CASES if c.name in ("tiles", "tiles-offset", "edges"))
    assert any(c.offset for c in mc.CONF_CASES) and any(c.offset for c in mc.EDGE_CASES)
    assert {(c.H, c.W)[i] for c in mc.EDGE_CASES for i in (0, 1)} >= {1, 2}


def test_the_benchmark_shape_keeps_its_kernel():
    st, p = mc.plan(mc.SRC_LT, 64, 768, 512, 7)
    assert st == 0 and (p.kernel, p.band, p.threads, p.nplanes, p.xcd) == ("rows", 64, 512, 2, 1), p
    st, p = mc.plan(mc.SRC_LT, 64, 512, 768, 7)
    assert st == 0 and (p.kernel, p.band, p.threads, p.nplanes, p.xcd) == ("rows", 64, 512, 2, 1), p


@pytest.mark.parametrize("c,ksize", PAIRS, ids=IDS)
def test_inputs_are_unsaturated_stamped_and_differ_across_the_batch(c, ksize):
    inp, imgs, bits, want = made(c, ksize)
    r = ksize // 2
    for s in mc.sources(c):
        share = float((want[s] == 255).mean())
        assert 0.05 <= share <= 0.95, (c.name, ksize, s, share)
        assert set(np.unique(want[s])) == {0, 255}
    # every seam of the route that has room for a stamp carries one; borders and corners always do
    seam_kinds = {k for _, _, _, k in inp.stamps}
    assert {"corner", "top", "bottom", "left", "right"} <= seam_kinds | set(inp.missing) and "corner" in seam_kinds
    if r >= 1:
        lost = [k for k in inp.missing if k.startswith(("col", "row"))]
        assert not lost, (c.name, ksize, lost)
    assert {b for b, _, _, _ in inp.stamps} == set(range(c.B))
    # a stamp's window is the element, clipped (at the threshold: under !(conf > t) only)
    for s in mc.sources(c):
        for b, y, x, kind in inp.stamps:
            if b not in imgs:
                continue
            win, el = mc.stamp_window(want[s][imgs.index(b)], y, x, ksize)
            empty = c.src == "conf" and s == mc.SRC_LT and (b, y, x) == inp.at_thres
            assert np.array_equal(win, np.zeros_like(el) if empty else el), (c.name, ksize, s, b, y, x, kind)
    if c.src == "conf":
        assert inp.conf[inp.at_thres] == mc.THRES and (inp.conf == mc.THRES).sum() >= 1
        assert (bits[mc.SRC_LT] != bits[mc.SRC_NGT]).any()
        data = inp.conf
    else:
        data = inp.image
        assert 0 < (inp.mask != 0).mean() < 0.1 and len(np.unique(inp.mask)) > 4
    for a, b in itertools.combinations(imgs, 2):
        assert not np.array_equal(data[a], data[b]), (c.name, a, b)
        assert not np.array_equal(want[mc.sources(c)[0]][imgs.index(a)], want[mc.sources(c)[0]][imgs.index(b)])


def test_the_edge_inputs_carry_the_planted_grey_values_the_wrap_and_the_borders():
    c = next(c for c in mc.EDGE_CASES if c.name == "edges")
    for ksize in c.ksizes:
        inp = mc.edge_inputs(c, ksize)
        lap = mc.laplacian_abs(inp.image[0])
        grey = (((lap & 255) * np.array(mc.GREY_W)).sum(-1) + (1 << 14)) >> 15
        assert np.array_equal(grey > mc.EDGE_THRES, MO.laplacian_edges(inp.image[0], mc.EDGE_THRES) != 0)
        sp = inp.specials
        assert set(sp) == {f"ch{ch}-{w}" for ch in range(3) for w in ("at", "above")} | {"wrap256", "lap1020"}, sorted(sp)
        for ch, d0, d1 in mc.threshold_bumps():
            y, x = sp[f"ch{ch}-at"]
            assert grey[y, x + 1] == mc.EDGE_THRES and lap[y, x + 1, ch] == d0 and lap[y, x + 1].sum() == d0
            y, x = sp[f"ch{ch}-above"]
            assert grey[y, x + 1] == mc.EDGE_THRES + 1 and lap[y, x + 1, ch] == d1 and lap[y, x + 1].sum() == d1
        assert [(d0, d1) for _, d0, d1 in mc.threshold_bumps()] == [(68, 69), (34, 35), (179, 180)]
        y, x = sp["wrap256"]
        assert lap[y, x, 0] == 256 and grey[y - 1:y + 2, x - 1:x + 2].max() <= mc.EDGE_THRES
        y, x = sp["lap1020"]
        assert (lap[y, x] == 1020).all() and grey[y, x] == 252
        # edges on all four borders and in a corner region of some image: reflect101 is exercised
        e = mc.edge_bits(inp.image)
        assert e[:, 0].any() and e[:, -1].any() and e[:, :, 0].any() and e[:, :, -1].any()
        assert any(k == "corner" for _, _, _, k in inp.stamps)
    for c in mc.EDGE_CASES:                                     # the thin shapes: edges exist, on the border by necessity
        if min(c.H, c.W) <= 2:
            assert mc.edge_bits(mc.edge_inputs(c, 7).image).any(), c.name


def test_numpy_reflect_is_reflect101_at_one_and_two_pixels():
    """The oracle pads with numpy's 'reflect'; the kernel's reflect101 maps -1 -> 1 and n -> n - 2, and a line of one pixel onto
    itself.  For n = 2 that is -1 -> 1, 2 -> 0; for n = 1 everything -> 0."""
    assert np.pad(np.array([5, 9]), 1, mode="reflect").tolist() == [9, 5, 9, 5]
    assert np.pad(np.array([5]), 1, mode="reflect").tolist() == [5, 5, 5]


def _masks(c, ksize, s, bug):
    inp, imgs, bits, want = made(c, ksize)
    other = bits[mc.SRC_NGT if s == mc.SRC_LT else mc.SRC_LT] if c.src == "conf" else None
    return mc.buggy(bug, c, ksize, bits[s], other, imgs), want[s]


def test_the_block_dilation_without_cuts_is_the_oracle():
    for c, k in PAIRS[::3]:
        inp, imgs, bits, want = made(c, k)
        s = mc.sources(c)[0]
        got = np.stack([mc._dilate_blocks(bits[s][b], MO.ellipse_kernel(k), (), ()) for b in imgs])
        assert np.array_equal(got, want[s]), (c.name, k)


@pytest.mark.parametrize("bug", [b for b in mc.BUGS if not b.startswith("halo_reset")])
def test_every_simulated_bug_changes_the_mask_of_every_case_it_concerns(bug):
    seen = 0
    for c, k in PAIRS:
        if not mc.bug_concerns(bug, c, k):
            continue
        for s in mc.sources(c):
            got, want = _masks(c, k, s, bug)
            assert got.shape == want.shape and not np.array_equal(got, want), (bug, c.name, k, s)
            with pytest.raises(AssertionError):
                mc.first_difference(got, want, c.name)
            seen += 1
    assert seen >= 10, (bug, seen)


def test_the_log_confidence_reset_bugs():
    seen = 0
    for c, k in PAIRS:
        if not mc.bug_concerns("halo_reset", c, k):
            continue
        inp, imgs, bits, _ = made(c, k)
        for s in mc.sources(c):
            want = mc.oracle_reset(inp.logc, bits[s], imgs)
            assert (want == 0).any() and (want != 0).any()
            for b in imgs:                                      # the oracle's own generate_mask gives the same reset
                if s == mc.SRC_LT:
                    assert np.array_equal(MO.generate_mask(inp.conf[b], inp.logc[b], float(mc.THRES), k)[1], want[imgs.index(b)])
            # the literal bug cannot show: asserted equal, so that it cannot hide a blind checker
            assert np.array_equal(mc.buggy_reset("halo_reset", c, k, inp.logc, bits[s], imgs), want), (c.name, k)
            if mc.bug_concerns("halo_reset_origin", c, k):
                assert not np.array_equal(mc.buggy_reset("halo_reset_origin", c, k, inp.logc, bits[s], imgs), want), (c.name, k)
            seen += 1
    assert seen >= 10


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan, swept

SWEEP_B = (1, 16, 64, 512, 4096)
SWEEP_H = (1, 2, 64, 768, 4096)
SWEEP_W = (4, 512, 3264, 3268, 3872, 3876, 4096, 4100, 1, 3, 53, 117, 3875, 4099)
SWEEP_K = tuple(range(1, 32, 2))


def sweep_failures(plan_fn):
    """Every (B, H, W, ksize, aligned, src) whose plan fails or breaks a limit, with the reason."""
    bad = []
    for B, H, W, k, al in itertools.product(SWEEP_B, SWEEP_H, SWEEP_W, SWEEP_K, (True, False)):
        for src in (mc.SRC_LT, mc.SRC_NGT, mc.SRC_EDGES):
            st, p = plan_fn(src, B, H, W, k, al)
            why = None
            if st != 0:
                why = f"status {st}"
            elif p.kernel == "rows":
                if src == mc.SRC_EDGES or W % 4 or W > 4096 or not al:
                    why = "rows kernel for a shape it does not serve"
                elif p.lds > 65536 or (p.nplanes > 0 and p.lds > 49152) or p.nplanes > 8:
                    why = f"LDS {p.lds}, {p.nplanes} planes"
                elif p.band not in (16, 32, 64) or p.threads != (512 if p.band == 64 else 256) or p.xcd != (1 if B >= 16 else 0):
                    why = f"band {p.band}, {p.threads} threads, xcd_map {p.xcd}"
                elif p.workgroups != (-(-B // 8) * 8 if p.xcd else B) * -(-H // p.band):
                    why = f"{p.workgroups} workgroups"
            elif p.kernel not in ("narrow", "wide") or (p.kernel == "narrow") != (k <= 9) or p.band != 32 or p.threads != 256 or p.lds != 0:
                why = f"tile route {p}"
            elif p.workgroups != -(-W // (56 if k <= 9 else 64)) * -(-H // 32) * B:
                why = f"{p.workgroups} workgroups"
            if why:
                bad.append(((B, H, W, k, al, src), why))
    return bad


def test_the_plan_succeeds_and_fits_over_the_sweep():
    bad = sweep_failures(mc.plan)
    assert not bad, (len(bad), bad[:5])
    # the shapes that a batch of 512 used to be refused: now bands of 32
    for k, W in ((7, 3876), (7, 4096), (31, 3268), (31, 4096)):
        st, p = mc.plan(mc.SRC_LT, 512, 2, W, k)
        assert st == 0 and (p.kernel, p.band) == ("rows", 32), (k, W, p)
    # and below those widths nothing changed
    assert mc.plan(mc.SRC_LT, 512, 2, 3872, 7)[1].band == 64 and mc.plan(mc.SRC_LT, 512, 2, 3264, 31)[1].band == 64


def test_the_plan_rejects_what_the_entry_points_reject():
    for args in ((0, 0, 8, 8, 7, 1), (0, 1, 0, 8, 7, 1), (0, 1, 8, 0, 7, 1), (0, 1, 8, 8, 8, 1), (0, 1, 8, 8, 33, 1), (0, 1, 8, 8, 0, 1), (2, 1, 8, 8, 7, 1)):
        assert mc.plan(*args)[0] == -1, args
    assert mc.plan(mc.SRC_EDGES, 65536, 8, 8, 7)[0] == -1 and mc.plan(mc.SRC_EDGES, 65535, 8, 8, 7)[0] == 0
    from sd_animation_optical_flow_amd import _lib
    assert _lib.lib().ofx_mask_plan(0, 1, 8, 8, 7, 1, None) == -1
