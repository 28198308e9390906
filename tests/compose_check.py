"""Shared by tests/test_compose_host.py (CPU) and tests/test_gpu_compose.py: the histogram form of the greedy multi-reference
composition (`ofx_compose_refs`, warp_mask.hip) restated in numpy, the case table, and the float64 reference of the sampled frame.

The reference's loop (ofgen_keyframe_inpaint.py:995-1024; `oracle.mask_oracle.compose`) thresholds the confidences to 0 / 1, and in
each of N rounds sums every plane, draws the arg-max, warps that reference whole, merges it where its plane is 1 and subtracts the
plane from all planes, clipped at 0.  With 0 / 1 planes that is bit logic on the per-pixel pattern b_p = sum_s (conf_s(p) > thres)
<< s, so everything but the warp is a function of the 256-bin histogram of b_p:

    count_r(s)  = sum of hist[b] over patterns b with bit s set and no already-drawn bit set      (a drawn s counts 0)
    order[r]    = the lowest s with the largest count_r(s)                                          (np.argmax: first maximum)
    table[b]    = the first order[r] whose bit is set in b, order[0] for b == 0 (the first warp is copied whole, :1010-1011)
    select[p]   = table[b_p]  (order[0] everywhere with first_only: generate_ai_frame_with_ref_both never merges, :900-908)
    mask[p]     = 255 where b_p != 0

`histogram_compose` is that, `oracle_compose` the reference loop through the oracle; the host test holds one against the other.
"""
from collections import namedtuple

import numpy as np

import warp_check as WC

MAX_REFS = 8


def patterns(conf, thres):
    """conf f32 [N,H,W] -> b_p u8 [H,W]; the compare is fp32 (a NaN is not confident)."""
    with np.errstate(invalid="ignore"):
        bits = np.asarray(conf, np.float32) > np.float32(thres)
    out = np.zeros(conf.shape[1:], np.uint8)
    for s in range(conf.shape[0]):
        out |= (bits[s].astype(np.uint8) << s).astype(np.uint8)
    return out


def histogram_compose(conf, thres, first_only=False):
    """-> dict(pattern u8 [H,W], hist i64 [256], order, counts (lists of N ints), table u8 [256], select u8 [H,W], mask u8 [H,W])."""
    n = conf.shape[0]
    assert 1 <= n <= MAX_REFS
    pat = patterns(conf, thres)
    hist = np.bincount(pat.ravel(), minlength=256).astype(np.int64)
    b = np.arange(256)
    order, counts, drawn = [], [], 0
    for _ in range(n):
        free = (b & drawn) == 0
        c = [int(hist[free & (((b >> s) & 1) == 1)].sum()) for s in range(n)]
        s = int(np.argmax(c))
        order.append(s)
        counts.append(c[s])
        drawn |= 1 << s
    table = np.full(256, order[0], np.uint8)
    if not first_only:
        for r in reversed(range(n)):
            table[((b >> order[r]) & 1) == 1] = order[r]
    return dict(pattern=pat, hist=hist, order=order, counts=counts, table=table, select=table[pat],
                mask=np.where(pat != 0, 255, 0).astype(np.uint8))


def flow_mat(flow, conf):
    """(flow [N,H,W,2], conf [N,H,W]) -> the reference's f32 [N,1,H,W,3]."""
    return np.concatenate([flow, conf[..., None]], -1)[:, None].astype(np.float32)


def oracle_compose(flow, conf, frames, thres, mode="cv2_cubic"):
    """The reference loop: -> (ret u8 [H,W,3], mask u8 [H,W] (255 = some reference confident), order list)."""
    from oracle import mask_oracle as MO
    with np.errstate(invalid="ignore"):
        ret, mask2, order = MO.compose(flow_mat(flow, conf), list(frames), None, thres, warp_mode=mode, expand=False)
    return ret, 255 - mask2, order


def oracle_selected(flow, frames, select, mode="cv2_cubic"):
    """The oracle's warp of every reference, gathered by `select`: what one sample per pixel must give (cv2_cubic: bit for bit)."""
    warped = WC.oracle_warp(frames, flow, 1.0, mode)                       # [N,H,W,3]
    return np.take_along_axis(warped, select[None, :, :, None].astype(np.int64), 0)[0]


def float64_selected(flow, frames, select, mode):
    """warp_check's float64 warp of the reference `select` names, values and bounds gathered per pixel:
    -> (r, bound f64 [1,H,W,3], exact bool [1,H,W])."""
    r, bound, exact = WC.warp_reference(frames, flow, 1.0, mode)
    idx = select[None].astype(np.int64)
    g4 = lambda a: np.take_along_axis(a, idx[..., None], 0)
    return g4(r), g4(bound), np.take_along_axis(exact, idx, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases

Case = namedtuple("Case", "name N H W thres seed kind")

# kind: how the confidence planes are made (`make_inputs`)
HOST_CASES = [
    Case("n1-9x7", 1, 9, 7, 0.6, 11, "random"),
    Case("n2-12x10", 2, 12, 10, 0.6, 12, "random"),
    Case("n3-48x40", 3, 48, 40, 0.6, 7, "block"),
    Case("n8-20x24", 8, 20, 24, 0.5, 14, "random"),
    Case("tie-n3-8x8", 3, 8, 8, 0.5, 15, "tie"),
    Case("nowhere-n3-10x6", 3, 10, 6, 0.5, 16, "nowhere"),
    Case("equal-thres-n2-6x6", 2, 6, 6, 0.75, 17, "equal"),
    Case("nan-n3-7x9", 3, 7, 9, 0.5, 18, "nan"),
    Case("none-confident-n3-5x5", 3, 5, 5, 0.5, 19, "none"),
    Case("all-patterns-n8-16x16", 8, 16, 16, 0.5, 20, "all"),
]

# the GPU shapes: the vector tails (H*W % 4 != 0 takes the one-pixel loop), a multiple of 4, more than one workgroup with a
# ragged edge (33*257 = 8481 pixels = 34 workgroups of 256), all 256 patterns
GPU_CASES = [
    Case("1x1-n1", 1, 1, 1, 0.5, 31, "random"),
    Case("3x5-n2", 2, 3, 5, 0.5, 32, "random"),
    Case("48x40-n3", 3, 48, 40, 0.6, 7, "block"),
    Case("33x257-n3", 3, 33, 257, 0.6, 34, "block"),
    Case("all-patterns-n8-16x16", 8, 16, 16, 0.5, 20, "all"),
]

# bilinear and bicubic are checked with warp_check's uint8 tie rule, whose cap on exempt bytes (5e-4 of the bytes, at least 1) the
# float64 reference must meet on its own.  The bilinear window is about 3e-4 of random bytes, so the shapes above do with a seed
# chosen on the CPU.  The bicubic bound carries the weight errors and its window is about 3e-3 (warp_check.BICUBIC_U8): no seed
# brings 48x40 or 33x257 under the cap, so bicubic runs on small frames that still take every path of the two kernels -- both
# vector tails, two workgroups with a ragged edge (9*31 = 279 pixels, one-pixel loop), the 16-byte loop over more than one workgroup
# (16*36 = 576 pixels, three workgroups of samples) and the 16-byte loop with all patterns.
# Seeds: the first of base, base + 1, ... under the cap with and without first_only (test_compose_host.py asserts it).
FLOAT_CASES = {
    "bilinear": [
        Case("1x1-n1", 1, 1, 1, 0.5, 100, "random"),
        Case("3x5-n2", 2, 3, 5, 0.5, 110, "random"),
        Case("48x40-n3", 3, 48, 40, 0.6, 120, "block"),
        Case("33x257-n3", 3, 33, 257, 0.6, 130, "block"),
        Case("all-patterns-n8-16x16", 8, 16, 16, 0.5, 140, "all"),
    ],
    "bicubic": [
        Case("1x1-n1", 1, 1, 1, 0.5, 200, "random"),
        Case("3x5-n2", 2, 3, 5, 0.5, 210, "random"),
        Case("9x31-n3", 3, 9, 31, 0.6, 221, "block"),
        Case("16x36-n3", 3, 16, 36, 0.6, 240, "block"),          # H*W % 4 == 0: the 16-byte loop, three workgroups of samples
        Case("all-patterns-n8-16x16", 8, 16, 16, 0.5, 235, "all"),
    ],
}
FLOAT_PARAMS = [(mode, c) for mode, cases in FLOAT_CASES.items() for c in cases]


def make_inputs(c):
    """-> (flow f32 [N,H,W,2], conf f32 [N,H,W], frames u8 [N,H,W,3])."""
    rng = np.random.default_rng(c.seed)
    N, H, W = c.N, c.H, c.W
    flow = (rng.standard_normal((N, H, W, 2)) * 2).astype(np.float32)
    conf = rng.random((N, H, W)).astype(np.float32)
    frames = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    if c.kind == "block":                           # the last-but-one reference wins the first round
        conf[N - 2, H // 5:H * 3 // 5, W // 8:W * 7 // 8] = 0.99
    elif c.kind == "tie":                           # references 1 and 2 confident on the same number of pixels, 0 on fewer
        conf[:] = 0
        conf[0, :2] = 1
        conf[1, :4] = 1
        conf[2, 4:] = 1
    elif c.kind == "nowhere":                       # reference 1 is confident nowhere: the last round draws index 0 again
        conf[1] = 0.1
        conf[0, :, :2] = 0.9
    elif c.kind == "equal":                         # confidence == thres is not confident (strict compare)
        conf[0, :3] = np.float32(c.thres)
        conf[1, 3:] = np.float32(c.thres)
        conf[1, 0] = np.nextafter(np.float32(c.thres), np.float32(2))
    elif c.kind == "nan":
        conf[0, ::2] = np.nan
        conf[2, :, 1] = np.nan
    elif c.kind == "none":
        conf *= np.float32(c.thres) * np.float32(0.99)
    elif c.kind == "all":                           # pixel p holds pattern p
        p = np.arange(H * W).reshape(H, W)
        for s in range(N):
            conf[s] = ((p >> s) & 1).astype(np.float32)
    return flow, conf, frames
