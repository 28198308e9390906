"""The bit-plane mask kernels (mask_bits.hip) restated for their tests: one case table that names the route every case must take
(asserted against the library's own plan, ofx_mask_plan, never against a Python restatement of the launcher), inputs whose masks
stay UNSATURATED, stamps on every seam of a route, and CPU functions that return what a broken kernel would.  Not a conftest:
imported by name, like warp_check.py.  Plain numpy; tests/test_mask_check_host.py proves on the CPU that the inputs have the
properties claimed here and that every simulated bug changes the output of every case it concerns.  The reference is
oracle/mask_oracle.py throughout and every comparison is bit for bit.

Why the inputs look as they do.  A uniform-random confidence against a threshold of 0.8 or more has so many low pixels that any
element from 7x7 up dilates the mask to all 255: such a case checks the comparison and the log-confidence reset, nothing of the
dilation.  Here the confidence is high everywhere except on a sparse Bernoulli set of low pixels of density 0.35 / area, `area`
being the cells of the element that fall inside min(H, ksize) rows: a pixel then stays 0 with a probability of about
exp(-0.35) = 0.70 (measured: 0.62 to 0.89 over these tables), whatever the element.  The inputs are made per (case, ksize).

Stamps.  A stamp is one low pixel with every other pixel within 2r + 1 of it high (r = ksize // 2): the output window of
(2r+1) x (2r+1) around it is exactly the element, clipped to the image.  Each case centres stamps on the seams of its route
(`seams`): the columns where two tiles (56 or 64 wide), two 32-pixel words or two 256-pixel chunks of the band kernel meet, the
rows where two tiles (32) or two bands (16, 32, 64) meet, and the image's borders and corners.  The seam stamps go into the images
a test compares (`compared`); every other image of the batch gets one stamp at a random place.  One stamp of image 0 holds exactly
the threshold: low under `!(conf > t)`, high under `conf < t`, so its window is the element under one convention and empty under
the other.

Simulated bugs (`BUGS`, `buggy`): see each one's line in `buggy`.  `halo_reset` is the literal "log_conf reset on halo rows too":
a band then also zeroes the low pixels of its halo rows, which their own band zeroes anyway, so the result is THE SAME and the host
test asserts that equality; what a kernel gets wrong when it takes halo rows for its own is the row origin, and `halo_reset_origin`
is that bug: the reset lands r rows below every low pixel of a band's bitmap.

Edge source (ofx_expand_mask).  A flat or linearly ramped BGR image has a zero Laplacian inside (a slope of 1 leaves |2| on the
borders under reflect101: grey 1, no edge).  A bump of +d in one channel of one pixel gives |Laplacian| 4d there and d on its four
neighbours (2d on a neighbour that lies on the border, whose reflection counts the bump twice).  Stamps are bumps of 15 in channel 1
(grey 35 at the centre, at most 18 around it: one edge pixel; in an image one pixel wide or high the centre sees 2d and the bump is
20: grey 23 and 12).  Image 0 also carries, for
each channel weight (channel 0 takes the "R" weight 9798, then 19235, 3735), the two bumps whose neighbours' grey value is exactly
edge_thres and edge_thres + 1, a bump of 64 in channel 0 (|Laplacian| 256 wraps to 0: no edge at the centre, grey 19 around it: no
edge at all; without the wrap grey 77) and a pixel of 255 among four of 0 (|Laplacian| 1020 -> 252).
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from oracle import mask_oracle as MO

SRC_LT, SRC_NGT, SRC_EDGES = 0, 1, 3
KERNELS = {0: "rows", 1: "narrow", 2: "wide"}
THRES = np.float32(0.9)
EDGE_THRES = 20
GREY_W = (MO.R2Y, MO.G2Y, MO.B2Y)


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's plan

Route = namedtuple("Route", "kernel band threads nplanes xcd lds workgroups")


def plan(src, B, H, W, ksize, aligned=True):
    """ofx_mask_plan -> (status, Route).  No device is touched."""
    from sd_animation_optical_flow_amd import _lib
    r = _lib.MaskRoute()
    st = _lib.lib().ofx_mask_plan(int(src), int(B), int(H), int(W), int(ksize), 1 if aligned else 0, C.byref(r))
    return st, Route(KERNELS.get(r.kernel, r.kernel), r.band_rows, r.threads, r.nplanes, r.xcd_map, r.lds_bytes, r.workgroups)


def half_widths(ksize):
    """Half width per row of the oracle's element."""
    return [int(row.sum() - 1) // 2 for row in MO.ellipse_kernel(ksize)]


def distinct_widths(ksize):
    return len({h for h in half_widths(ksize) if h > 0})


# ---------------------------------------------------------------------------------------------------------------------------------
# cases

# kernel: 'rows' or 'tile' (narrow for ksize <= 9, wide above); band: rows per workgroup; direct: the ksizes that must run without
# planes; offset: elements the confidence (4 bytes each) or the mask (1 byte each) starts after an aligned allocation
Case = namedtuple("Case", "name src B H W ksizes kernel band xcd direct offset all_images")


def _c(name, src, B, H, W, ksizes, kernel, band, xcd=0, direct=(), offset=0, all_images=()):
    return Case(name, src, B, H, W, tuple(ksizes), kernel, band, xcd, frozenset(direct), offset, frozenset(all_images))


CONF_CASES = [
    # 260 x ceil(100 / 64) = 520 >= 512: bands of 64 and 36 rows, 512 threads; 260 = 32 * 8 + 4: a ragged last XCD group
    _c("rows64", "conf", 260, 100, 36, (1, 3, 7, 9, 15, 31), "rows", 64, xcd=1, direct=(31,), all_images=(7,)),
    # 172 x 2 < 512 <= 172 x 3: bands of 32, 32 and 6 rows
    _c("rows32", "conf", 172, 70, 36, (1, 3, 7, 9, 15, 31), "rows", 32, xcd=1, direct=(31,)),
    # bands of 16 and 4 rows; 8 distinct half widths at 27 and 29, 9 at 31; 29x29 planes: 48144 bytes at W = 928, 49792 at 932
    _c("rows16-w928", "conf", 2, 20, 928, (7, 11, 27, 29, 31), "rows", 16, direct=(31,)),
    _c("rows16-w932", "conf", 2, 20, 932, (29,), "rows", 16, direct=(29,)),
    # the batch asks for bands of 64, which need 65952 bytes (7x7) and more of LDS at this width: bands of 32
    _c("rows-wide-frames", "conf", 512, 2, 3876, (7, 31), "rows", 32, xcd=1, direct=(7, 31)),
    _c("tiles", "conf", 3, 70, 117, (1, 3, 7, 9, 11, 15, 31), "tile", 32),
    # W % 4 == 0, but the confidence starts 4 bytes after a 16-byte boundary
    _c("tiles-offset", "conf", 3, 70, 116, (7, 15), "tile", 32, offset=1),
]
EDGE_CASES = [
    _c("edges", "edges", 3, 70, 117, (7, 15), "tile", 32),
    _c("edges-offset", "edges", 3, 70, 117, (7,), "tile", 32, offset=1),
    _c("edges-h1", "edges", 3, 1, 70, (7, 15), "tile", 32),
    _c("edges-w1", "edges", 3, 70, 1, (7, 15), "tile", 32),
    _c("edges-h2", "edges", 3, 2, 67, (7, 15), "tile", 32),
    _c("edges-w2", "edges", 3, 67, 2, (7, 15), "tile", 32),
]
CASES = CONF_CASES + EDGE_CASES


def aligned(c):
    return c.offset == 0


def sources(c):
    return (SRC_LT, SRC_NGT) if c.src == "conf" else (SRC_EDGES,)


def expected_route(c, ksize):
    """(kernel, band, 'planes' | 'direct' | None, xcd_map) the table claims."""
    if c.kernel == "rows":
        return "rows", c.band, "direct" if ksize in c.direct else "planes", c.xcd
    return ("narrow" if ksize <= 9 else "wide"), 32, None, 0


def planned_route(c, ksize, src=None):
    st, p = plan(sources(c)[0] if src is None else src, c.B, c.H, c.W, ksize, aligned(c))
    assert st == 0, (c.name, ksize, st)
    mode = None if p.kernel != "rows" else ("direct" if p.nplanes < 0 else "planes")
    return (p.kernel, p.band, mode, p.xcd), p


def compared(c, ksize):
    """The images a test compares with the oracle: all of a small batch and where the case says so, else 0, 7, 8 and B - 1."""
    if c.B <= 8 or ksize in c.all_images:
        return list(range(c.B))
    return sorted({0, 7, 8, c.B - 1} & set(range(c.B)))


def seams(c, ksize):
    """-> (column seams, row seams) of the route: x (or y) such that pixels x - 1 and x belong to different tiles, words or bands."""
    kernel, band, _, _ = expected_route(c, ksize)
    step = {"rows": 32, "narrow": 56, "wide": 64}[kernel]
    return list(range(step, c.W, step)), list(range(band, c.H, band))


# ---------------------------------------------------------------------------------------------------------------------------------
# stamps

def _cheb(a, b):
    return max(abs(a[0] - b[0]), abs(a[1] - b[1]))


def wanted_stamps(c, ksize):
    """[(kind, [(y, x), ...])]: for every kind of seam the positions that would serve it, best first."""
    H, W = c.H, c.W
    cols, rows = seams(c, ksize)
    my, mx = H // 2, W // 2
    borders = [("corner", [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]), ("corner2", [(H - 1, W - 1), (H - 1, 0), (0, W - 1)]),
               ("top", [(0, mx), (0, mx // 2)]), ("bottom", [(H - 1, mx), (H - 1, mx // 2)]),
               ("left", [(my, 0), (my // 2, 0)]), ("right", [(my, W - 1), (my // 2, W - 1)])]
    out = []                                                    # the seams first: they have the fewest places to go
    col_kinds = sorted({x for x in cols if x in (32, 56, 64, 112, 256)} | set(cols[:1]))
    for x in col_kinds:                                         # one stamp on either side of the seam
        ys = [my, my // 2, (my + H) // 2, 0, H - 1]
        out.append((f"col{x - 1}", [(y, x - 1) for y in ys]))
        out.append((f"col{x}", [(y, x) for y in ys]))
    for y in rows:
        xs = [mx, mx // 2, (mx + W) // 2, 3, W - 4, 0, W - 1]
        out.append((f"row{y - 1}", [(y - 1, x) for x in xs if 0 <= x < W]))
        out.append((f"row{y}", [(y, x) for x in xs if 0 <= x < W]))
    return out + borders


def place_stamps(c, ksize, rng):
    """-> (stamps [(b, y, x, kind)], missing kinds).  Two stamps of an image are more than 2r + 1 apart (Chebyshev)."""
    r = ksize // 2
    imgs = compared(c, ksize)
    taken = {b: [] for b in range(c.B)}
    stamps, missing = [], []
    turn = 0
    for kind, spots in wanted_stamps(c, ksize):
        done = False
        for k in range(len(imgs)):
            b = imgs[(turn + k) % len(imgs)]
            for p in spots:
                if all(_cheb(p, q) > 2 * r + 1 for q in taken[b]):
                    taken[b].append(p)
                    stamps.append((b, p[0], p[1], kind))
                    done = True
                    break
            if done:
                break
        turn += 1
        if not done:
            missing.append(kind)
    for b in range(c.B):                                        # at least one per image
        if not taken[b]:
            p = (int(rng.integers(c.H)), int(rng.integers(c.W)))
            taken[b].append(p)
            stamps.append((b, p[0], p[1], "any"))
    return stamps, missing


def stamp_window(out_b, y, x, ksize):
    """The (2r+1)^2 window of one image's mask around (y, x) and the element, both clipped to the image -> (window != 0, element != 0)."""
    r = ksize // 2
    H, W = out_b.shape
    y0, y1, x0, x1 = max(y - r, 0), min(y + r + 1, H), max(x - r, 0), min(x + r + 1, W)
    el = MO.ellipse_kernel(ksize)[y0 - (y - r):y1 - (y - r), x0 - (x - r):x1 - (x - r)]
    return out_b[y0:y1, x0:x1] != 0, el != 0


# ---------------------------------------------------------------------------------------------------------------------------------
# confidence inputs

def element_area(H, ksize):
    k = MO.ellipse_kernel(ksize)
    m = min(H, ksize)
    top = ksize // 2 - m // 2
    return int(k[top:top + m].sum())


ConfInputs = namedtuple("ConfInputs", "conf logc stamps missing at_thres")


def conf_inputs(c, ksize):
    """conf, logc f32 [B,H,W]; stamps [(b, y, x, kind)]; at_thres: the (b, y, x) of the stamp that holds exactly THRES."""
    rng = np.random.default_rng(1000 * ksize + c.H * 7 + c.W + c.B)
    B, H, W = c.B, c.H, c.W
    r = ksize // 2
    conf = (0.92 + 0.08 * rng.random((B, H, W))).astype(np.float32)
    low = rng.random((B, H, W)) < 0.35 / element_area(H, ksize)
    conf[low] = (0.88 * rng.random(int(low.sum()))).astype(np.float32)
    at = rng.random((B, H, W)) < 0.1 / element_area(H, ksize)   # a few values exactly at the threshold: low only under !(conf > t)
    conf[at] = THRES
    stamps, missing = place_stamps(c, ksize, rng)
    for b, y, x, _ in stamps:
        win = conf[b, max(y - 2 * r - 1, 0):y + 2 * r + 2, max(x - 2 * r - 1, 0):x + 2 * r + 2]
        win[win <= THRES] = np.float32(0.95)
    for b, y, x, _ in stamps:
        conf[b, y, x] = np.float32(0.25)
    at_thres = next(((b, y, x) for b, y, x, kind in stamps if b == 0 and kind not in ("corner", "any")), stamps[0][:3])
    conf[at_thres] = THRES
    logc = np.log(conf + np.float32(1e-3)).astype(np.float32)
    return ConfInputs(conf, logc, stamps, missing, at_thres)


def conf_bits(conf, src):
    return conf < THRES if src == SRC_LT else ~(conf > THRES)


# ---------------------------------------------------------------------------------------------------------------------------------
# edge inputs

def grey_of(g, ch):
    return (g * GREY_W[ch] + (1 << (MO.GRAY_SHIFT - 1))) >> MO.GRAY_SHIFT


def threshold_bumps(edge_thres=EDGE_THRES):
    """[(channel, d at the threshold, d one above it)]: the largest d whose grey value is edge_thres and the smallest one above."""
    out = []
    for ch in range(3):
        d = max(g for g in range(256) if grey_of(g, ch) == edge_thres)
        assert grey_of(d + 1, ch) == edge_thres + 1
        out.append((ch, d, d + 1))
    return out


EdgeInputs = namedtuple("EdgeInputs", "image mask stamps missing specials")


def edge_inputs(c, ksize):
    """image u8 [B,H,W,3] BGR, mask u8 [B,H,W] (sparse, any byte), stamps, and image 0's special bumps {name: (y, x)}."""
    rng = np.random.default_rng(2000 * ksize + c.H * 7 + c.W + c.B)
    B, H, W = c.B, c.H, c.W
    r = ksize // 2
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    image = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        base = (40 + 0 * ys, 10 + ys, 10 + xs)[b % 3]           # flat, a ramp down the rows, a ramp along them
        image[b] = base[..., None]
    stamps, missing = place_stamps(c, ksize, rng)
    objects = {b: [] for b in range(B)}                         # (y, x, reach): pixels whose Laplacian the object touches

    def free(b, y, x, reach):
        if not (0 <= y < H and 0 <= x < W):
            return False
        if any(_cheb((y, x), (sy, sx)) <= 2 * r + 1 + reach + 1 for sb, sy, sx, _ in stamps if sb == b):
            return False
        return all(_cheb((y, x), (oy, ox)) > reach + oreach + 1 for oy, ox, oreach in objects[b])

    def bump(b, y, x, ch, d):
        v = int(image[b, y, x, ch])
        v = v + d if v + d <= 255 else v - d
        assert 0 <= v <= 255, (b, y, x, ch, d)
        image[b, y, x, ch] = v

    for b, y, x, _ in stamps:
        bump(b, y, x, 1, 15 if min(H, W) >= 2 else 20)
    specials = {}
    if H >= 8 and W >= 8:
        todo = [(f"ch{ch}-at", ch, d0) for ch, d0, _ in threshold_bumps()] + [(f"ch{ch}-above", ch, d1) for ch, _, d1 in threshold_bumps()]
        todo += [("wrap256", 0, 64), ("lap1020", None, 255)]
        spots = [(int(y), int(x)) for y, x in zip(rng.integers(2, H - 2, 4000), rng.integers(2, W - 2, 4000))]
        for name, ch, d in todo:
            p = next((p for p in spots if free(0, p[0], p[1], 2)), None)
            if p is None:
                continue
            y, x = p
            if ch is None:
                image[0, y - 1:y + 2, x - 1:x + 2] = 0
                image[0, y, x] = 255
                objects[0].append((y, x, 2))
            else:
                bump(0, y, x, ch, d)
                objects[0].append((y, x, 1))
            specials[name] = p
    # sparse random bumps everywhere else, borders included: strong ones (an edge on the centre and around it)
    n = max(2, int(0.35 / element_area(H, ksize) * H * W / 3))
    for b in range(B):
        planted = 0
        for y, x in zip(rng.integers(0, H, 4 * n), rng.integers(0, W, 4 * n)):
            if planted < n and free(b, int(y), int(x), 1):
                bump(b, int(y), int(x), int(rng.integers(3)), int(rng.choice([45, 100, 120])))
                objects[b].append((int(y), int(x), 1))
                planted += 1
    mask = np.where(rng.random((B, H, W)) < 0.03, rng.integers(1, 256, (B, H, W)), 0).astype(np.uint8)
    return EdgeInputs(image, mask, stamps, missing, specials)


def laplacian_abs(img):
    """|Laplacian| per channel before the wrap, reflect101 borders: int64 [H,W,3]."""
    v = img.astype(np.int64)
    p = np.pad(v, ((1, 1), (1, 1), (0, 0)), mode="reflect")
    return np.abs(p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:] - 4 * v)


def edge_bits(image, edge_thres=EDGE_THRES):
    return np.stack([MO.laplacian_edges(im, edge_thres) for im in image]) != 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle and the simulated bugs

def oracle_dilate(bits, ksize, images=None):
    """bits bool [B,H,W] -> u8 {0,255} [len(images),H,W] through mask_oracle.dilate."""
    k = MO.ellipse_kernel(ksize)
    idx = range(bits.shape[0]) if images is None else images
    return np.stack([MO.dilate(np.where(bits[b], np.uint8(255), np.uint8(0)), k) for b in idx])


def oracle_reset(logc, bits, images=None):
    idx = list(range(bits.shape[0])) if images is None else list(images)
    lc = logc[idx].copy()
    lc[bits[idx]] = 0
    return lc


BUGS = ("half_width", "column_seam", "halo_rows", "previous_image", "other_compare", "all_255", "halo_reset", "halo_reset_origin")


def narrowed_row(c, ksize):
    """The row of the element the half_width bug narrows: the narrowest one an image of H rows can reach (the first of them)."""
    r = ksize // 2
    hw = half_widths(ksize)
    return min((i for i in range(ksize) if abs(i - r) <= c.H - 1), key=lambda i: (hw[i], i))


def bug_concerns(bug, c, ksize):
    r = ksize // 2
    cols, rows = seams(c, ksize)
    if bug == "half_width":
        return half_widths(ksize)[narrowed_row(c, ksize)] <= c.W - 1
    if bug == "column_seam":
        return r >= 1 and bool(cols)
    if bug == "halo_rows":
        return r >= 1 and bool(rows)
    if bug == "previous_image":
        return c.B >= 2
    if bug == "other_compare":
        return c.src == "conf"
    if bug == "halo_reset":
        return c.src == "conf" and r >= 1
    if bug == "halo_reset_origin":
        return c.src == "conf" and r >= 1 and c.H > r            # r rows below a low pixel of the top rows is inside the image
    return True


def _dilate_blocks(bits_b, kern, col_cuts, row_cuts):
    """Each block of the image dilated on its own: nothing crosses a cut."""
    H, W = bits_b.shape
    out = np.zeros((H, W), np.uint8)
    ye = [0] + list(row_cuts) + [H]
    xe = [0] + list(col_cuts) + [W]
    src = np.where(bits_b, np.uint8(255), np.uint8(0))
    for y0, y1 in zip(ye[:-1], ye[1:]):
        for x0, x1 in zip(xe[:-1], xe[1:]):
            out[y0:y1, x0:x1] = MO.dilate(np.ascontiguousarray(src[y0:y1, x0:x1]), kern)
    return out


def buggy(bug, c, ksize, bits, other_bits=None, images=None):
    """The mask [len(images),H,W] a kernel with `bug` would write for the source bitmap `bits` [B,H,W].
    half_width       one row of the element (`narrowed_row`) is one cell narrower on either side (a row of one cell: empty)
    column_seam      no dilation across the column seams of the route
    halo_rows        no dilation across the row seams of the route (the halo rows of a band or tile are missing)
    previous_image   image b is computed from image b - 1 (b >= 1)
    other_compare    `<` and `!(>)` swapped: the source bitmap of the other convention (other_bits)
    all_255          every byte 255"""
    idx = list(range(bits.shape[0])) if images is None else list(images)
    kern = MO.ellipse_kernel(ksize)
    r = ksize // 2
    cols, rows = seams(c, ksize)
    if bug == "half_width":
        kern = kern.copy()
        i = narrowed_row(c, ksize)
        on = np.flatnonzero(kern[i])
        kern[i, on[0]] = kern[i, on[-1]] = 0
    if bug == "all_255":
        return np.full((len(idx),) + bits.shape[1:], 255, np.uint8)
    if bug == "other_compare":
        bits = other_bits
    out = []
    for b in idx:
        src = bits[b - 1] if bug == "previous_image" and b >= 1 else bits[b]
        out.append(_dilate_blocks(src, kern, cols if bug == "column_seam" else (), rows if bug == "halo_rows" else ()))
    return np.stack(out)


def buggy_reset(bug, c, ksize, logc, bits, images=None):
    """log_conf after a reset that also runs over the halo rows of every band / tile row of the route:
    halo_reset         ... at the right pixels (the same result: every low pixel is zeroed once more)
    halo_reset_origin  ... with the band's first OUTPUT row as the origin of its bitmap rows: r rows too low"""
    idx = list(range(bits.shape[0])) if images is None else list(images)
    r = ksize // 2
    H = bits.shape[1]
    _, rows = seams(c, ksize)
    lc = oracle_reset(logc, bits, idx)
    edges = [0] + list(rows) + [H]
    for y0, y1 in zip(edges[:-1], edges[1:]):
        for row in range(0, y1 - y0 + 2 * r):                   # bitmap rows of the band, halo included
            y = y0 - r + row
            if not 0 <= y < H:
                continue
            dst = y if bug == "halo_reset" else y0 + row
            if 0 <= dst < H:
                lc[:, dst][bits[idx][:, y]] = 0
    return lc


def first_difference(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got != want
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {i}: got {got[i]!r}, want {want[i]!r}")
