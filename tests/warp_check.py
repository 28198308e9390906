"""The output stage restated for its tests: the backward warp (warp_mask.hip, warp_fast.hip), cv2-style cubic resize, the
forward-backward confidence and the travel mask, each as a float64 reference with a derived per-element bound, the case tables
that reach every branch of the kernels, and the checkers.  Not a conftest: imported by name, like pyramid_check.py.  Plain numpy,
runs on any machine; tests/test_warp_check_host.py proves on the CPU that the checkers catch planted bugs.

Notation: u = 2^-24 (fp32 unit roundoff).  All bounds are first order in u; nothing in them is fitted to a device's output.

Coordinates.  The sample position is the fp32 number the kernels and oracle.warp_oracle._maps agree on,
    mx = float32(float64(x) + sign * float64(f)),
(fb_confidence: float32(x) + f in fp32, the same value for the inputs used here).  x0 = floor(mx) and fx = mx - x0 are exact in fp32;
from there on the reference is float64.

Bilinear.  r = sum_i v_i w_i over the four taps (zero outside), w = (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy.  The kernel rounds each
weight three times (1-fx, 1-fy, the product), each product v_i w_i once, and the first product passes through three additions:
    |out - r| <= K_BIL u sum_i |v_i| w_i,    K_BIL = 3 + 1 + 3 = 7.
(The shared-frame kernel of warp_fast.hip contracts products and sums into FMAs: fewer roundings, same bound.)  On the CPU
warp_oracle.warp_bilinear (fp32, no FMA) reaches 0.56 of it over the tables below.

Cubic weights (ofx_cubic_coeffs, ofx_internal.h; Keys, A = -0.75; every operation rounded on its own).  `cubic64` evaluates the same
Horner steps in float64 and carries the running absolute error of each step: an operation whose exact result is p adds u |p| to the
error its operands bring, a product a b brings |a| e_b + |b| e_a, a sum e_a + e_b.  t is exact; t1 = t + 1 and 1 - t are rounded (u |.|).
    w0:  t1 = t + 1; p1 = A t1; p2 = p1 - 5A; p3 = p2 t1; p4 = p3 + 8A; p5 = p4 t1; w0 = p5 - 4A                 (7 roundings)
    w1:  q1 = (A+2) t; q2 = q1 - (A+3); q3 = q2 t; q4 = q3 t; w1 = q4 + 1                                       (5 roundings)
    w2:  the same in 1 - t                                                                                        (6 roundings)
    w3:  ((1 - w0) - w1) - w2: the three errors above plus u (|1 - w0| + |1 - w0 - w1| + |w3|)                 (3 roundings)
giving e_k, the absolute error of weight k (between 1 u and 56 u over [0, 1); the fp32 weights of warp_oracle.cubic_coeffs reach 0.67 of it).

Bicubic warp and resize_cubic.  out = sum_k1 wy_k1 (sum_k2 v wx_k2), accumulated as row = row + v wx, acc = acc + row wy from zero.
A tap's product v wx is rounded once and passes through at most three additions of `row` (the first addition, to zero, is exact);
row wy is rounded once and passes through at most three additions of `acc`:  K_CUB = 1 + 3 + 1 + 3 = 8, and per element
    |out - r| <= K_CUB u sum |v| |wx| |wy|  +  sum |v| (e_x |wy| + |wx| e_y).
The warp zeroes taps outside the frame; resize_cubic clamps them (replicate), and its source coordinate ((x + 0.5) scale - 0.5) is
float64 in the kernel and here, the fraction rounded to fp32 once.

uint8 outputs of the float modes: the tie rule.  With r the float64 value and `bound` the bound above, a byte is EXEMPT iff
|frac(r) - 0.5| <= bound: there it may be floor(r) or ceil(r) (clipped to 0..255).  Everywhere else it equals clip(rint(r), 0, 255).
Pixels whose fractions fx, fy are both in {0, 0.5} have exact fp32 arithmetic (weights are multiples of 1/1024, taps are bytes;
bilinear: any multiple of 1/4, see exact_pixels): they are never exempt and must be round-half-even of r; the tables plant such
pixels on taps whose sum ends in .5 with an even floor, where round-half-up gives the other byte.  The exempt bytes of a case are
counted from the float64 reference alone and may not exceed max(1, 5e-4 N) of its N values (the bilinear window is 2 * 7u * 255 =
2.1e-4 wide; 1.5e-4 of 33 360 values were measured when the rule was set); the seeds of the tables are chosen so that every case
meets it, and the host test asserts that.  The cubic bound carries the weight errors and its window is some ten times wider, so the
uint8 bicubic cases are small ones whose cap is a single byte.

cv2_cubic stays bit-exact against warp_oracle.warp_cv2_cubic.

fb_confidence.  s = the float64 bilinear sample of bw[b] at p + fw(p), |ds| <= 7u mag;  e = fw + s is rounded once:
de = ds + u |e|.  lc = -(ex^2 + ey^2) inv with inv = float32(1 / (2 sigma^2)): the squares, the sum and the product are rounded once
each, so
    |d lc| <= inv (2 |ex| dex + 2 |ey| dey + dex^2 + dey^2) + 3 u |lc|,
    |d conf| <= conf |d lc| + E_EXP u conf + FLOOR,
E_EXP and FLOOR being the ones sd_ops_check.py measured and states.  Where ex^2 + ey^2 is beyond fp32 (|fw| = 1e30) the kernel's
squares overflow: there conf must be 0 and logc below -1e30 or -inf, and nothing may be NaN.

travel_mask.  t = warp(travel)(p + flow) + dist, rounded once: |dt| <= warp bound + u |t|.  Pixels whose confidence is below 0.9 (fp32
compare) give raw = 255, travel = 0; t > thres gives raw = 255, travel = 0.  Pixels with |t - thres| <= dt are exempt (either side),
under the same cap.

Worst ratios measured on an MI355X (gfx950) over tests/test_gpu_warp_float64.py, 2026-10-20 (the tests print them, run with -s to
re-measure).  A ratio is |error| / bound over the elements, inside when <= 1; exempt values are counted from the float64 reference
and set against the sum of the cases' caps.
    uint8 bilinear, generic kernel (C = 1, 2, 4; C = 3 at W < 4 or H < 2)      0 exempt bytes of 850      (caps add up to 16)
    uint8 bilinear, warp_u8c3_x4_kernel                                        0 of 20 664                (12)
    uint8 bilinear, warp_bilinear_u8c3_kernel                                  2 of 21 096                (12)
    uint8 bilinear, warp_bilinear_shared_kernel                                4 of 35 208                (18)
    uint8 bilinear, a frame per item (generic, x4, u8c3)                       3 of 35 441                (24)
    uint8 bicubic, C = 1..4                                                    3 of 4 020                 (8)
        every byte outside the exemption equals clip(rint(r)); the x4 and u8c3 kernels equal the generic kernel byte for byte
    float32 bilinear, 64 cases                                                 0.486
    float32 bicubic, 64 cases                                                  0.298
    warp_kernel<float, 1, bilinear>, second grid-stride trip (2 100 000 px)    0.562
    resize_cubic, 10 cases and the second trip (2 108 288 outputs)             0.307
    fb_confidence                                                              conf 0.357, logc 0.474
    travel_mask, bilinear / bicubic, B = 2                                     0.409 / 0.191, no exempt pixel (cap 1 each)
  The warp, resize and logc ratios equal those of the fp32 CPU oracle (test_warp_check_host.py prints them): with contraction off
  warp_mask.hip rounds where numpy does.  No case exposed a defect in a kernel.
"""
from collections import namedtuple

import numpy as np

from sd_ops_check import E_EXP, FLOOR

U = 2.0 ** -24
K_BIL = 7.0
K_CUB = 8.0
CUBIC_A = -0.75
CAP_SHARE = 5e-4
GRID_CAP = 256 * 8192                     # threads of warp_kernel / resize_cubic_kernel before the grid-stride loop makes a second trip


def cap(n):
    return max(1, int(CAP_SHARE * n))


# ---------------------------------------------------------------------------------------------------------------------------------
# the dispatch of launch_warp (warp_mask.hip), restated

def route(H, W, B, C, per_frame, dtype="u8", mode="bilinear"):
    """The kernel ops.warp runs (sizes far below the 32-bit limits the launcher also checks; torch allocations are aligned):
    'shared'   warp_bilinear_shared_kernel: u8, C = 3, bilinear, one shared frame, B >= 4, W % 4 == 0
    'u8c3'     warp_bilinear_u8c3_kernel:   u8, C = 3, bilinear, W % 4 == 0, H >= 2
    'x4'       warp_u8c3_x4_kernel:         u8, C = 3, bilinear or cv2_cubic, W >= 4, H >= 2
    'generic'  warp_kernel<T, C, MODE>:     everything else"""
    if dtype != "u8" or C != 3 or mode == "bicubic":
        return "generic"
    if mode == "bilinear":
        if not per_frame and B >= 4 and W % 4 == 0:
            return "shared"
        if W % 4 == 0 and H >= 2 and H * W * 3 >= 8:
            return "u8c3"
    return "x4" if (W >= 4 and H >= 2) else "generic"


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 restatements

def coords(flow, sign):
    """flow f32 [B,H,W,2] -> (mx, my) f32 [B,H,W]: float32(float64(x) + sign * float64(f))."""
    _, H, W, _ = flow.shape
    xs = np.arange(W, dtype=np.float64)[None, None, :]
    ys = np.arange(H, dtype=np.float64)[None, :, None]
    mx = (xs + np.float64(sign) * flow[..., 0].astype(np.float64)).astype(np.float32)
    my = (ys + np.float64(sign) * flow[..., 1].astype(np.float64)).astype(np.float32)
    return mx, my


def _split(m, trunc=False):
    """fp32 coordinate -> (integer part int64, clamped like the kernels; fraction float64).  Exact."""
    m0 = (np.trunc(m) if trunc else np.floor(m)).astype(np.float32)
    f = (m - m0).astype(np.float32)
    return np.clip(m0, -1.0e6, 1.0e6).astype(np.int64), f.astype(np.float64)


def _gather(frames, per_frame, yi, xi, replicate=False):
    """frames [nf,H,W,C]; yi, xi int64 [B,H,W] -> float64 [B,H,W,C], zeros outside (or the clamped tap)."""
    _, H, W, _ = frames.shape
    B = yi.shape[0]
    bsel = np.arange(B)[:, None, None] if per_frame else 0
    v = frames[bsel, np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)].astype(np.float64)
    if replicate:
        return v
    ok = (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W)
    return np.where(ok[..., None], v, 0.0)


def exact_pixels(mx, my, mode="bicubic"):
    """Pixels whose fp32 arithmetic is exact for byte taps: both fractions in {0, 0.5}; bilinear: any multiple of 1/4 (weights are
    multiples of 1/16 there, every product and sum fits 24 bits; the cubic weights of 1/4 are multiples of 1/256 and row * wy may not)."""
    _, fx = _split(mx)
    _, fy = _split(my)
    q = 4.0 if mode == "bilinear" else 2.0
    return (fx * q == np.floor(fx * q)) & (fy * q == np.floor(fy * q))


def bilinear64(frames, per_frame, mx, my, bug=None):
    """-> (r, bound) float64 [B,H,W,C].  `bug` plants a defect (the host tests' simulated devices)."""
    W = frames.shape[2]
    x0, fx = _split(mx, bug == "trunc")
    y0, fy = _split(my, bug == "trunc")
    rep = bug == "replicate"
    v00, v01 = _gather(frames, per_frame, y0, x0, rep), _gather(frames, per_frame, y0, x0 + 1, rep)
    v10, v11 = _gather(frames, per_frame, y0 + 1, x0, rep), _gather(frames, per_frame, y0 + 1, x0 + 1, rep)
    if bug == "swap":
        last = (x0 == W - 1)[..., None]
        v00, v01 = np.where(last, v01, v00), np.where(last, v00, v01)
        v10, v11 = np.where(last, v11, v10), np.where(last, v10, v11)
    gx, gy = 1.0 - fx, 1.0 - fy
    w01x = gx if bug == "weight" else fx
    w = [(gx * gy)[..., None], (w01x * gy)[..., None], (gx * fy)[..., None], (fx * fy)[..., None]]
    r = v00 * w[0] + v01 * w[1] + v10 * w[2] + v11 * w[3]
    mag = np.abs(v00) * w[0] + np.abs(v01) * w[1] + np.abs(v10) * w[2] + np.abs(v11) * w[3]
    return r, K_BIL * U * np.abs(mag)


def cubic64(t):
    """Keys weights of the fp32 fraction t in float64 and the running error of ofx_cubic_coeffs: (w, e), each [..., 4]."""
    t = np.asarray(t, np.float64)
    A = CUBIC_A
    t1 = t + 1.0
    e_t1 = U * np.abs(t1)
    p1 = A * t1
    e = abs(A) * e_t1 + U * np.abs(p1)
    p2 = p1 - 5 * A
    e = e + U * np.abs(p2)
    p3 = p2 * t1
    e = e * np.abs(t1) + np.abs(p2) * e_t1 + U * np.abs(p3)
    p4 = p3 + 8 * A
    e = e + U * np.abs(p4)
    p5 = p4 * t1
    e = e * np.abs(t1) + np.abs(p4) * e_t1 + U * np.abs(p5)
    w0 = p5 - 4 * A
    e0 = e + U * np.abs(w0)

    def mid(s, e_s):
        q1 = (A + 2) * s
        e = (A + 2) * e_s + U * np.abs(q1)
        q2 = q1 - (A + 3)
        e = e + U * np.abs(q2)
        q3 = q2 * s
        e = e * np.abs(s) + np.abs(q2) * e_s + U * np.abs(q3)
        q4 = q3 * s
        e = e * np.abs(s) + np.abs(q3) * e_s + U * np.abs(q4)
        w = q4 + 1.0
        return w, e + U * np.abs(w)

    w1, e1 = mid(t, np.zeros_like(t))
    s = 1.0 - t
    w2, e2 = mid(s, U * np.abs(s))
    a, b = 1.0 - w0, 1.0 - w0 - w1
    w3 = b - w2
    e3 = e0 + e1 + e2 + U * (np.abs(a) + np.abs(b) + np.abs(w3))
    return np.stack([w0, w1, w2, w3], -1), np.stack([e0, e1, e2, e3], -1)


def bicubic64(frames, per_frame, mx, my, bug=None):
    """-> (r, bound) float64 [B,H,W,C]."""
    x0, fx = _split(mx, bug == "trunc")
    y0, fy = _split(my, bug == "trunc")
    wx, ex = cubic64(fx)
    wy, ey = cubic64(fy)
    r = mag = wterm = 0.0
    for k1 in range(4):
        for k2 in range(4):
            v = _gather(frames, per_frame, y0 - 1 + k1, x0 - 1 + k2, bug == "replicate")
            a, b = wx[..., k2][..., None], wy[..., k1][..., None]
            r = r + v * a * b
            mag = mag + np.abs(v) * np.abs(a) * np.abs(b)
            wterm = wterm + np.abs(v) * (ex[..., k2][..., None] * np.abs(b) + np.abs(a) * ey[..., k1][..., None])
    return r, K_CUB * U * mag + wterm


def _frames4(frame):
    return (frame if frame.ndim == 4 else frame[None]), frame.ndim == 4


def warp_reference(frame, flow, sign, mode, bug=None):
    """frame [H,W,C] (shared) or [B,H,W,C], uint8 or float32; flow f32 [B,H,W,2] -> (r, bound, exact [B,H,W]).
    bug: None | 'trunc' | 'swap' | 'replicate' | 'sign' | 'frame0' | 'channels' | 'weight' ('half_up' is a rounding: simulate_u8)."""
    frames, per_frame = _frames4(frame)
    mx, my = coords(flow, 1.0 if bug == "sign" else sign)
    if bug == "frame0":
        frames, per_frame = frames[:1], False
    r, bound = (bilinear64 if mode == "bilinear" else bicubic64)(frames, per_frame, mx, my, bug)
    if bug == "channels":
        r = np.concatenate([r[..., 1:2], r[..., 0:1], r[..., 2:]], -1)
    return r, bound, exact_pixels(mx, my, mode)


def simulate_u8(r, half_up=False):
    return np.clip(np.floor(r + 0.5) if half_up else np.rint(r), 0, 255).astype(np.uint8)


def oracle_warp(frame, flow, sign, mode):
    """oracle.warp_oracle's fp32 restatement over the batch (cv2_cubic: the bit-exact reference)."""
    from oracle import warp_oracle as WO
    frames, per_frame = _frames4(frame)
    out = []
    with np.errstate(invalid="ignore"):                          # its int cast of a 1e30 coordinate: out of range either way
        for b in range(flow.shape[0]):
            mx, my = WO._maps(flow[b], sign)
            out.append(WO._MODES[mode](frames[b if per_frame else 0], mx, my))
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# checkers

def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def check_float(out, r, bound, what):
    """|out - r| <= bound per element (no NaN); returns the worst |error| / bound."""
    out = np.asarray(out, np.float64)
    assert out.shape == r.shape, (what, out.shape, r.shape)
    err = np.abs(out - r)
    bad = ~(err <= bound)
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outside the bound; first at {i}: got {out[i]!r}, float64 {r[i]!r}, "
                             f"bound {bound[i]:.3e}, error {err[i]:.3e}")
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def exempt_bytes(r, bound, exact):
    return (np.abs(r - np.floor(r) - 0.5) <= bound) & ~exact[..., None]


class CapExceeded(Exception):
    """A case whose float64 reference exempts more values than the cap allows: a defect of the table, not of the output."""


def check_u8(out, r, bound, exact, what):
    """The tie rule.  Returns (exempt bytes, cap)."""
    assert out.dtype == np.uint8 and out.shape == r.shape, (what, out.dtype, out.shape, r.shape)
    ex = exempt_bytes(r, bound, exact)
    n, c = int(ex.sum()), cap(r.size)
    if n > c:
        raise CapExceeded(f"{what}: {n} exempt bytes of {r.size}, cap {c}: choose another seed")
    o = out.astype(np.float64)
    want = np.clip(np.rint(r), 0, 255)
    lo, hi = np.clip(np.floor(r), 0, 255), np.clip(np.ceil(r), 0, 255)
    bad = np.where(ex, (o != lo) & (o != hi), o != want)
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} bytes wrong; first at {i}: got {int(out[i])}, float64 {r[i]!r}, "
                             f"bound {bound[i]:.3e}, {'exempt' if ex[i] else 'exact pixel' if exact[i[:3]] else 'plain'}")
    return n, c


def check_warp(out, frame, flow, sign, mode, what):
    """Either dtype.  Returns (worst ratio or None for uint8, exempt bytes, cap)."""
    r, bound, exact = warp_reference(frame, flow, sign, mode)
    if frame.dtype == np.uint8:
        n, c = check_u8(out, r, bound, exact, what)
        return None, n, c
    return check_float(out, r, bound, what), 0, 0


def same_bytes(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    bad = a.view(np.uint32) != b.view(np.uint32) if a.dtype == np.float32 else a != b
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.size} differ; first at {i}: got {a[i]!r}, want {b[i]!r}")


# ---------------------------------------------------------------------------------------------------------------------------------
# warp case tables

Case = namedtuple("Case", "name H W B C sign per_frame dtype mode seed route")

BRANCHES = ("x0=-1", "x0=W-1", "y0=-1", "y0=H-1", "last_pair", "all_out", "far", "huge", "tie", "inside")


def case(name, H, W, B, C, sign, per_frame, dtype, mode, seed, rt=None):
    return Case(f"{name}-{H}x{W}-b{B}-c{C}-{'neg' if sign < 0 else 'pos'}{'-perframe' if per_frame else ''}", H, W, B, C, sign, per_frame,
                dtype, mode, seed, rt)


def make_inputs(c):
    """-> (frame, flow).  Random bytes (floats: bytes * 0.37 - 20) and flows, with planted pixels: samples on the four
    frame edges with one tap column or row outside, the bottom-right pixels of every item sampling the frame's last pixel pair and
    beyond, a row pointing left out of the frame, far (* 40) and 1e30 flows, and exact ties on taps whose sum ends in .5."""
    rng = np.random.default_rng(c.seed)
    H, W, B, C, sg = c.H, c.W, c.B, c.C, c.sign
    nf = B if c.per_frame else 1
    frames = rng.integers(0, 256, (nf, H, W, C), dtype=np.uint8)
    amp = np.array([min(3.0, W / 4.0), min(3.0, H / 4.0)], np.float32)
    flow = (rng.standard_normal((B, H, W, 2)).astype(np.float32) * amp).astype(np.float32)

    def aim(b, y, x, sx, sy):
        flow[b, y, x] = (sg * (sx - x), sg * (sy - y))          # dyadic numbers: the sample position is exactly (sx, sy)

    if B * H >= 3:                                              # a row pointing left out of the frame
        for x in range(W):
            aim(B - 1, 0, x, -3.25, 0.0)
    big = H * W >= 4
    q = 0.25 if c.mode == "bilinear" else 0.5                  # fractions whose fp32 arithmetic is exact (exact_pixels)
    reserved = set()
    if big:                                                     # the end of every item's frame: last pixel pair, and beyond it
        for b in range(B):
            aim(b, H - 1, W - 1, W - 2 + q, H - 2 + 0.5)
            aim(b, H - 1, W - 2, W - 1 + q, H - 1 + q)
            reserved |= {(b, H - 1, W - 1), (b, H - 1, W - 2)}
    slots = ((int(i) // (H * W), int(i) % (H * W) // W, int(i) % W) for i in rng.permutation(B * H * W))
    slots = (s for s in slots if s not in reserved)
    # exact ties in the frame the item samples: r = a + 0.5 with a even (half-even: a, half-up: a + 1)
    a = (10 + 4 * np.arange(C)).astype(np.uint8)

    def tie2(b, y, x):
        f = frames[b if c.per_frame else 0]
        if c.mode == "bilinear":
            if W >= 2:
                f[0, 0], f[0, 1] = a, a + 1                     # (a + a + 1) / 2
            else:
                f[0, 0] = 2 * a + 1                             # the right tap is outside
        elif W >= 3:
            f[0, 0], f[0, 1], f[0, 2] = a, a + 1, 2 * a + 1     # cubic weights of 1/2: (19 a + 19 (a + 1) - 3 (2a + 1)) / 32
        aim(b, y, x, 0.5, 0.0)

    def tie4(b, y, x):
        f = frames[b if c.per_frame else 0]
        f[H - 2, W - 2], f[H - 2, W - 1], f[H - 1, W - 2], f[H - 1, W - 1] = a, a, a + 1, a + 1
        aim(b, y, x, W - 2 + 0.5, H - 2 + 0.5)

    def far(b, y, x):
        flow[b, y, x] = (68.5, -91.25)

    def huge(b, y, x):
        flow[b, y, x] = (1e30, -1e30)

    plants = [tie2, lambda b, y, x: aim(b, y, x, -q, y), lambda b, y, x: aim(b, y, x, W - 1 + q, y),
              lambda b, y, x: aim(b, y, x, x, -q), lambda b, y, x: aim(b, y, x, x, H - 1 + q)]
    if not big:
        plants += [lambda b, y, x: aim(b, y, x, W - 2 + q, H - 2 + 0.5)]
    plants += [far, huge]
    if H >= 3 and W >= 2 and c.mode == "bilinear":             # four taps, clear of the two-tap tie's
        plants += [tie4]
    for p, (b, y, x) in zip(plants, slots):
        p(b, y, x)
    frame = frames if c.per_frame else frames[0]
    if c.dtype == "f32":
        frame = (frame.astype(np.float32) * np.float32(0.37) - np.float32(20)).astype(np.float32)
    return np.ascontiguousarray(frame), flow


def branches(c, flow):
    """The branches of the kernels the flows of a case reach (from the sample positions alone)."""
    mx, my = coords(flow, c.sign)
    x0, fx = _split(mx)
    y0, fy = _split(my)
    H, W = c.H, c.W
    xin, yin = (x0 >= -1) & (x0 <= W - 1), (y0 >= -1) & (y0 <= H - 1)
    xc = np.clip(x0, 0, max(W - 2, 0))
    got = {"x0=-1": (x0 == -1) & (fx > 0) & yin, "x0=W-1": (x0 == W - 1) & yin, "y0=-1": (y0 == -1) & (fy > 0) & xin,
           "y0=H-1": (y0 == H - 1) & xin,
           "last_pair": (xc == W - 2) & ((np.clip(y0, 0, H - 1) == H - 1) | (np.clip(y0 + 1, 0, H - 1) == H - 1)) & xin & yin,
           "all_out": ~(xin & yin), "far": (np.abs(flow).max(-1) > 40) & (np.abs(flow).max(-1) < 1e6), "huge": np.abs(flow).max(-1) >= 1e29,
           "tie": ((fx == 0.5) | (fy == 0.5)) & exact_pixels(mx, my) & xin & yin,
           "inside": (x0 >= 0) & (x0 < W - 1) & (y0 >= 0) & (y0 < H - 1)}
    out = {k for k, m in got.items() if m.any()}
    if c.per_frame and not all(got["last_pair"][b].any() for b in range(c.B)):
        out.discard("last_pair")
    return out


def expected_branches(c):
    """What make_inputs must reach: everything, except what a frame of one or two pixels has no room for."""
    want = set(BRANCHES)
    big = c.H * c.W >= 4
    order = ["tie", "x0=-1", "x0=W-1", "y0=-1", "y0=H-1"] + ([] if big else ["last_pair"]) + ["far", "huge"]      # make_inputs' plants
    slots = c.B * c.H * c.W - (2 * c.B if big else 0)
    want -= set(order[slots:])
    if c.H < 2 or c.W < 2:
        want.discard("inside")
    if c.W < 2:
        want.discard("last_pair")                               # no pixel pair in a row
    if "far" not in want:
        want.discard("all_out")                                 # the planted pixels may take the whole out-pointing row
    return want


def _u8_cases(name, shapes, C, per_frame, mode, rt, seed0):
    out = []
    for i, s in enumerate(shapes):
        H, W, B = s
        sign = 1.0 if i % 2 == 0 else -1.0
        for k, sg in enumerate((sign, -sign) if i == len(shapes) - 1 else (sign,)):
            out.append(case(name, H, W, B, C, sg, per_frame, "u8", mode, seed0 + 10 * i + k, rt))
    return out


# uint8 bilinear, one table per route (B = 3 where the route allows it; 8 items of 1x1 carry the planted pixels)
GENERIC_U8 = (_u8_cases("generic", [(5, 3, 3), (1, 8, 3), (1, 1, 8)], 1, False, "bilinear", "generic", 100)
              + _u8_cases("generic", [(5, 3, 3), (1, 8, 3), (1, 1, 8)], 2, False, "bilinear", "generic", 200)
              + _u8_cases("generic", [(5, 3, 3), (1, 8, 3), (1, 1, 8)], 4, False, "bilinear", "generic", 300)
              + _u8_cases("generic", [(5, 3, 3), (1, 8, 3), (1, 1, 8)], 3, False, "bilinear", "generic", 400))
X4_U8 = _u8_cases("x4", [(2, 5, 3), (9, 7, 2), (17, 66, 3)], 3, False, "bilinear", "x4", 500)
U8C3_U8 = _u8_cases("u8c3", [(2, 4, 3), (9, 4, 2), (17, 68, 3)], 3, False, "bilinear", "u8c3", 600)
SHARED_U8 = _u8_cases("shared", [(1, 8, 4), (9, 4, 4), (17, 68, 5)], 3, False, "bilinear", "shared", 700)
ROUTE_TABLES = {"generic": GENERIC_U8, "x4": X4_U8, "u8c3": U8C3_U8, "shared": SHARED_U8}

# per-frame key frames: every route but shared-fast, B = 2, 3, 5, a different frame per item
PER_FRAME_U8 = ([case("generic", H, W, B, C, sg, True, "u8", "bilinear", 800 + 7 * i, "generic")
                 for i, (H, W, B, C, sg) in enumerate([(5, 3, 2, 1, 1.0), (1, 8, 3, 3, -1.0), (1, 1, 5, 4, 1.0), (5, 3, 5, 2, -1.0)])]
                + [case("x4", H, W, B, 3, sg, True, "u8", "bilinear", 850 + 7 * i, "x4")
                   for i, (H, W, B, sg) in enumerate([(2, 5, 2, 1.0), (9, 7, 3, -1.0), (17, 66, 5, 1.0)])]
                + [case("u8c3", H, W, B, 3, sg, True, "u8", "bilinear", 900 + 7 * i, "u8c3")
                   for i, (H, W, B, sg) in enumerate([(2, 4, 2, -1.0), (9, 4, 3, 1.0), (17, 68, 5, -1.0)])])

# uint8 bicubic: C = 1..4, shared and per-frame (always warp_kernel<uint8_t, C, BICUBIC>)
# The cubic bound carries the weight errors: its window is some ten times the bilinear one (about 3e-3 of random bytes), so these
# cases are small (more than one workgroup, cap 1); seed 1000 is the first one tried and every case meets the cap with it.
BICUBIC_U8 = [case("bicubic", H, W, 3, C, sg, pf, "u8", "bicubic", 1000, "generic")
              for C in (1, 2, 3, 4) for pf, (H, W), sg in ((False, (9, 11), 1.0), (True, (5, 7), -1.0))]

# float32 bilinear and bicubic: C = 1..4, shared and per-frame, both signs, four shapes
FLOAT_SHAPES = [(45, 37, 2), (1, 8, 3), (5, 3, 3), (1, 1, 8)]
FLOAT_CASES = {mode: [case(mode, H, W, B, C, sg, pf, "f32", mode, 2000 + 1000 * m + 100 * C + 10 * i + 2 * pf + (sg < 0), "generic")
                      for C in (1, 2, 3, 4) for pf in (False, True) for sg in (1.0, -1.0) for i, (H, W, B) in enumerate(FLOAT_SHAPES)]
               for m, mode in enumerate(("bilinear", "bicubic"))}

# cv2_cubic, bit-exact against the oracle
CV2_CASES = ([case("cv2", 45, 37, 2, C, sg, False, "u8", "cv2_cubic", 4000 + C) for C, sg in ((1, 1.0), (2, -1.0), (4, 1.0))]
             + [case("cv2", H, W, 3, 3, sg, True, "u8", "cv2_cubic", 4010 + H) for (H, W), sg in (((45, 37), -1.0), ((5, 3), 1.0), ((9, 8), 1.0))]
             + [case("cv2", 45, 37, 2, C, sg, pf, "f32", "cv2_cubic", 4020 + C) for C, sg, pf in ((2, 1.0, False), (3, -1.0, True), (4, 1.0, False))])

# the grid-stride second trip of warp_kernel<float, 1, BILINEAR>
STRIDE_WARP = Case("stride-700x1000-b3-c1", 700, 1000, 3, 1, 1.0, False, "f32", "bilinear", 5000, "generic")

WARP_BUGS = ("half_up", "trunc", "swap", "replicate", "sign", "frame0", "channels", "weight")


def bug_concerns(bug, c):
    """Whether case c belongs to the table a planted bug must fail on."""
    if bug == "half_up":
        return c.dtype == "u8"
    if bug in ("swap", "weight"):
        return c.mode == "bilinear"
    if bug == "sign":
        return c.sign < 0
    if bug == "frame0":
        return c.per_frame
    if bug == "channels":
        return c.C >= 2
    return True


def buggy_output(c, frame, flow, bug):
    r, _, _ = warp_reference(frame, flow, c.sign, c.mode, None if bug == "half_up" else bug)
    if c.dtype == "u8":
        return simulate_u8(r, bug == "half_up")
    return r.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# resize_cubic

ResizeCase = namedtuple("ResizeCase", "name Hs Ws Hd Wd B C seed")
RESIZE_CASES = [ResizeCase(f"{hs}x{ws}-to-{hd}x{wd}-b{b}-c{c}", hs, ws, hd, wd, b, c, 6000 + i) for i, (hs, ws, hd, wd, b, c) in enumerate(
    [(12, 8, 96, 64, 1, 4), (96, 64, 12, 8, 1, 4), (7, 5, 20, 13, 1, 4), (20, 13, 7, 5, 1, 4), (1, 1, 5, 3, 1, 4), (5, 3, 1, 1, 1, 4),
     (6, 6, 6, 6, 1, 4), (12, 8, 96, 64, 3, 4), (12, 8, 96, 64, 1, 1), (12, 8, 96, 64, 1, 3)])]
STRIDE_RESIZE = ResizeCase("stride-8x8-to-728x724-c4", 8, 8, 728, 724, 1, 4, 6100)
RESIZE_BUGS = ("zero_border", "no_half")


def resize_inputs(c):
    rng = np.random.default_rng(c.seed)
    return (rng.standard_normal((c.B, c.Hs, c.Ws, c.C)) * 3.0 + 0.5).astype(np.float32)


def resize_reference(img, Hd, Wd, bug=None):
    """img f32 [B,Hs,Ws,C] -> (r, bound) float64 [B,Hd,Wd,C]: cv2.resize(INTER_CUBIC), clamped taps."""
    B, Hs, Ws, C = img.shape

    def axis(n_out, n_in):
        scale = np.float64(n_in) / np.float64(n_out)
        d = np.arange(n_out, dtype=np.float64)
        f = d * scale if bug == "no_half" else (d + 0.5) * scale - 0.5
        s = np.floor(f)
        w, e = cubic64((f - s).astype(np.float32))
        idx = s.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :]
        ok = (idx >= 0) & (idx < n_in)
        if bug == "zero_border":
            w, e = np.where(ok, w, 0.0), np.where(ok, e, 0.0)
        return np.clip(idx, 0, n_in - 1), w, e

    ix, wx, ex = axis(Wd, Ws)
    iy, wy, ey = axis(Hd, Hs)
    src = img.astype(np.float64)
    r = mag = wterm = 0.0
    for k1 in range(4):
        rows = src[:, iy[:, k1]]
        b, eb = np.abs(wy[:, k1])[None, :, None, None], ey[:, k1][None, :, None, None]
        for k2 in range(4):
            v = rows[:, :, ix[:, k2]]
            a, ea = np.abs(wx[:, k2])[None, None, :, None], ex[:, k2][None, None, :, None]
            r = r + v * wx[:, k2][None, None, :, None] * wy[:, k1][None, :, None, None]
            mag = mag + np.abs(v) * a * b
            wterm = wterm + np.abs(v) * (ea * b + a * eb)
    return r, K_CUB * U * mag + wterm


def oracle_resize(img, Hd, Wd):
    from oracle import warp_oracle as WO
    return np.stack([WO.resize_cubic(img[b], Hd, Wd) for b in range(img.shape[0])])


# ---------------------------------------------------------------------------------------------------------------------------------
# fb_confidence

FbCase = namedtuple("FbCase", "name H W B sigma seed")
FB_CASES = [FbCase(f"{h}x{w}-b3-sigma{s}", h, w, 3, s, 7000 + 10 * i + j) for i, (h, w) in enumerate([(16, 24), (1, 8), (5, 3)])
            for j, s in enumerate((0.5, 3.0, 10.0))]
FB_BUGS = ("bw0", "sigma4")
FB_BRANCHES = ("zero", "left", "right", "top", "bottom", "all_out", "1e6", "1e30", "consistent")


def fb_inputs(c):
    """-> (fw, bw, planted) f32 [B,H,W,2]: item 0 consistent (bw = -fw of a smooth field, resampled by the kernel), item 1 the same
    plus noise, item 2 unrelated; a different bw per item; planted pixels: zero flows, samples leaving on each side with one tap column
    or row still inside, samples wholly outside, |fw| = 1e6 and 1e30.  `planted` maps a branch name to its (b, y, x)."""
    rng = np.random.default_rng(c.seed)
    H, W, B = c.H, c.W, c.B
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    fw = np.zeros((B, H, W, 2), np.float32)
    bw = np.zeros((B, H, W, 2), np.float32)
    ax, ay = min(1.0, (W - 1) / 8.0), min(1.0, (H - 1) / 8.0)    # a frame of one row has no room for a vertical flow
    for b in range(B):
        smooth = np.stack([ax * (0.8 * np.sin(0.17 * xs + 0.1 * ys + b) + 0.3), ay * (0.6 * np.cos(0.13 * ys - 0.07 * xs + 2 * b) - 0.2)], -1)
        fw[b] = smooth.astype(np.float32)
        bw[b] = (-smooth).astype(np.float32)
    noise = rng.standard_normal((H, W, 2))
    bw[1] += (0.05 * noise).astype(np.float32)
    fw[2] += (rng.standard_normal((H, W, 2)) * 1.5).astype(np.float32)
    bw[2] = (rng.standard_normal((H, W, 2)) * 2.0).astype(np.float32)
    slots = [(b, y, x) for b in range(B) for y in range(H) for x in range(W)]
    slots = [slots[i] for i in rng.permutation(len(slots))]
    planted = {}

    def put(name, fn):
        b, y, x = slots.pop()
        fw[b, y, x] = fn(y, x)
        planted[name] = (b, y, x)
        return b, y, x

    b, y, x = put("zero", lambda y, x: (0.0, 0.0))
    bw[b, y, x] = 0.0
    put("left", lambda y, x: (-0.25 - x, 0.0))
    put("right", lambda y, x: (W - 1 + 0.25 - x, 0.0))
    put("top", lambda y, x: (0.0, -0.25 - y))
    put("bottom", lambda y, x: (0.0, H - 1 + 0.25 - y))
    put("all_out", lambda y, x: (-3.5 - x, 2.0))
    put("1e6", lambda y, x: (1e6, -1e6))
    put("1e30", lambda y, x: (-1e30, 1e30))
    return fw, bw, planted


def fb_reference(fw, bw, sigma, bug=None):
    """-> dict(conf, dconf, logc, dlogc, overflow): float64 [B,H,W] (overflow: bool, the kernel's squares leave fp32)."""
    B, H, W, _ = fw.shape
    mx = (np.arange(W, dtype=np.float32)[None, None, :] + fw[..., 0]).astype(np.float32)
    my = (np.arange(H, dtype=np.float32)[None, :, None] + fw[..., 1]).astype(np.float32)
    s, ds = bilinear64(bw[:1] if bug == "bw0" else bw, bug != "bw0", mx, my)
    e = fw.astype(np.float64) + s
    de = ds + U * np.abs(e)
    s2 = np.float32(sigma) * np.float32(sigma)
    inv = np.float64(np.float32(1.0) / (np.float32(2.0) * (s2 * s2 if bug == "sigma4" else s2)))
    q = e[..., 0] ** 2 + e[..., 1] ** 2
    lc = -q * inv
    dlc = inv * (2 * np.abs(e[..., 0]) * de[..., 0] + 2 * np.abs(e[..., 1]) * de[..., 1] + de[..., 0] ** 2 + de[..., 1] ** 2) + 3 * U * np.abs(lc)
    conf = np.exp(lc)
    return dict(conf=conf, dconf=conf * dlc + E_EXP * U * conf + FLOOR, logc=lc, dlogc=dlc, overflow=q > 1e37)


def check_fb(conf, logc, ref, what):
    """Returns the worst ratios (conf, logc) over the pixels whose squares stay inside fp32."""
    conf, logc = np.asarray(conf, np.float64), np.asarray(logc, np.float64)
    assert not np.isnan(conf).any() and not np.isnan(logc).any(), f"{what}: NaN"
    ov = ref["overflow"]
    if ov.any():
        assert (conf[ov] == 0).all(), f"{what}: conf != 0 where |e|^2 overflows: {conf[ov]}"
        assert (logc[ov] < -1e30).all(), f"{what}: logc not very negative where |e|^2 overflows: {logc[ov]}"
    fin = ~ov
    rc = check_float(conf[fin], ref["conf"][fin], ref["dconf"][fin], what + " conf")
    rl = check_float(logc[fin], ref["logc"][fin], ref["dlogc"][fin], what + " logc")
    return rc, rl


def fb_branches(fw):
    B, H, W, _ = fw.shape
    mx = np.arange(W, dtype=np.float32)[None, None, :] + fw[..., 0]
    my = np.arange(H, dtype=np.float32)[None, :, None] + fw[..., 1]
    x0, fx = _split(mx)
    y0, fy = _split(my)
    xin, yin = (x0 >= -1) & (x0 <= W - 1), (y0 >= -1) & (y0 <= H - 1)
    mag = np.abs(fw).max(-1)
    got = {"zero": mag == 0, "left": (x0 == -1) & (fx > 0) & yin, "right": (x0 == W - 1) & (fx > 0) & yin, "top": (y0 == -1) & (fy > 0) & xin,
           "bottom": (y0 == H - 1) & (fy > 0) & xin, "all_out": ~(xin & yin) & (mag < 100), "1e6": (mag >= 1e6) & (mag < 1e7), "1e30": mag >= 1e30,
           "consistent": np.zeros_like(xin)}
    got["consistent"][0] = xin[0] & yin[0]
    return {k for k, m in got.items() if m.any()}


# ---------------------------------------------------------------------------------------------------------------------------------
# travel_mask and dilate

TravelCase = namedtuple("TravelCase", "name H W B mode thres seed")
TRAVEL_CASES = [TravelCase("cv2_cubic-33x29-b3", 33, 29, 3, "cv2_cubic", 25.0, 8000), TravelCase("bilinear-33x29-b2", 33, 29, 2, "bilinear", 25.0, 8001),
                TravelCase("bicubic-33x29-b2", 33, 29, 2, "bicubic", 25.0, 8002)]
DILATE_CASES = [(20, 70, 3), (33, 130, 3)]
DILATE_KSIZES = (3, 7, 15, 31)


def travel_inputs(c):
    """-> conf, flow, dist, travel (f32; a different travel map per item; conf planted at exactly 0.9, where `<` must not fire)."""
    from oracle import mask_oracle as MO
    rng = np.random.default_rng(c.seed)
    B, H, W = c.B, c.H, c.W
    conf = (0.8 + 0.2 * rng.random((B, H, W))).astype(np.float32)
    conf[:, 3::11, 2::9] = np.float32(0.9)
    conf[:, 0, 0] = np.float32(0.9)
    flow = (rng.standard_normal((B, H, W, 2)) * 4).astype(np.float32)
    dist = np.stack([MO.travel_distance(flow[b], conf[b]) for b in range(B)])
    travel = (rng.random((B, H, W)) * 30).astype(np.float32)
    return conf, flow, dist, travel


def travel_oracle(conf, flow, dist, travel, thres, mode):
    """mask_oracle.confidence_to_mask before its dilation, per item: (raw, travel_out)."""
    from oracle import warp_oracle as WO
    raws, outs = [], []
    for b in range(conf.shape[0]):
        low = conf[b] < np.float32(0.9)
        t = (WO.warp_frame(travel[b], flow[b], mode=mode) + dist[b]).astype(np.float32)
        t[low] = 0
        far = t > np.float32(thres)
        raws.append(np.where(low | far, np.uint8(255), np.uint8(0)))
        t[far] = 0
        outs.append(t)
    return np.stack(raws), np.stack(outs)


def travel_reference(conf, flow, dist, travel, thres, mode):
    """-> dict(t, dt, low, far, exempt): float64 / bool [B,H,W]."""
    w, dw, _ = warp_reference(travel[..., None], flow, 1.0, mode)
    t = w[..., 0] + dist.astype(np.float64)
    dt = dw[..., 0] + U * np.abs(t)
    low = conf < np.float32(0.9)
    th = np.float64(np.float32(thres))
    return dict(t=t, dt=dt, low=low, far=~low & (t > th), exempt=~low & (np.abs(t - th) <= dt))


def check_travel(raw, tout, ref, what):
    """Returns (worst ratio of travel_out, exempt pixels, cap)."""
    tout = np.asarray(tout, np.float64)
    low, far, ex = ref["low"], ref["far"], ref["exempt"]
    n, c = int(ex.sum()), cap(ex.size)
    if n > c:
        raise CapExceeded(f"{what}: {n} exempt pixels of {ex.size}, cap {c}: choose another seed")
    zero = (low | far) & ~ex
    assert ((raw == 255) == (low | far))[~ex].all(), f"{what}: raw mask differs on {int((((raw == 255) != (low | far)) & ~ex).sum())} pixels"
    assert np.isin(raw, (0, 255)).all() and ((raw[ex] == 255) == (tout[ex] == 0)).all(), f"{what}: raw and travel disagree on an exempt pixel"
    assert (tout[zero] == 0).all(), f"{what}: travel not reset on {int((tout[zero] != 0).sum())} pixels"
    keep = ~(low | far) & ~ex
    ratio = check_float(tout[keep], ref["t"][keep], ref["dt"][keep], what + " travel")
    inside = (tout[ex] == 0) | (np.abs(tout[ex] - ref["t"][ex]) <= ref["dt"][ex])
    assert inside.all(), f"{what}: an exempt pixel's travel is neither 0 nor inside the bound"
    return ratio, n, c


def dilate_inputs(H, W, B, seed=9000):
    rng = np.random.default_rng(seed + H)
    return ((rng.random((B, H, W)) > 0.97) * rng.integers(1, 256, (B, H, W))).astype(np.uint8)
