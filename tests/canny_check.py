"""TEST INFRASTRUCTURE -- `cv2.Canny(image, threshold1, threshold2)` (aperture 3, L2gradient=False) restated for 1- and 3-channel
8-bit images, and the inputs the Canny tests share.  No device.

PARITY UNPINNED, like oracle/keyframe_oracle.py whose single-channel `canny` this must equal bit for bit (tests/test_canny_host.py):
OpenCV 4.x imgproc/src/canny.cpp written down on integers.

    gradient      3x3 Sobel with replicated borders per channel, norm |dx| + |dy|; with 3 channels a pixel keeps the (dx, dy, norm)
                  of the channel with the largest norm -- channels are scanned in memory order and a later one replaces an earlier
                  one only when its norm is strictly larger, so a tie keeps the lowest channel index
    suppression   the 15-bit tan(22.5 deg) direction test on a magnitude map with a one-pixel zero border; m > low is a candidate,
                  m > high a strong pixel
    hysteresis    a candidate survives when it is 8-connected, through candidates, to a strong pixel; 255 or 0, no dilation
    thresholds    numbers, floored (cvFloor); low > high are swapped
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import keyframe_oracle as KO   # noqa: E402

TILE = 32          # the hysteresis kernel's tile
SWEEP_BATCH = 8    # sweeps per host check


def thresholds(low, high) -> tuple:
    low, high = int(math.floor(low)), int(math.floor(high))
    return (high, low) if low > high else (low, high)


def gradient(img: np.ndarray):
    """(dx, dy) int32 [H,W] of a [H,W] or [H,W,3] image: per channel Sobel, then the channel choice."""
    if img.ndim == 2:
        return KO._sobel16(img)
    assert img.ndim == 3 and img.shape[2] == 3
    dx, dy = KO._sobel16(img[..., 0])
    norm = np.abs(dx) + np.abs(dy)
    for c in (1, 2):
        cx, cy = KO._sobel16(img[..., c])
        cn = np.abs(cx) + np.abs(cy)
        take = cn > norm                                         # strictly larger: a tie keeps the earlier channel
        dx, dy, norm = np.where(take, cx, dx), np.where(take, cy, dy), np.where(take, cn, norm)
    return dx, dy


def canny_map(img: np.ndarray, low: int, high: int) -> np.ndarray:
    """Non-maximum suppression: 2 = strong, 0 = candidate, 1 = no edge (the codes of keyframe_oracle.canny_map)."""
    H, W = img.shape[:2]
    dx, dy = gradient(img)
    dx, dy = dx.astype(np.int64), dy.astype(np.int64)
    mag = np.zeros((H + 2, W + 2), dtype=np.int64)
    mag[1:-1, 1:-1] = np.abs(dx) + np.abs(dy)
    m = mag[1:-1, 1:-1]
    x, y = np.abs(dx), np.abs(dy) << 15
    tg22x = x * KO.TG22
    tg67x = tg22x + (x << 16)
    neg = (dx ^ dy) < 0
    up_d = np.where(neg, mag[:-2, 2:], mag[:-2, :-2])            # (row - 1, col - s) and (row + 1, col + s), s = -1 where the signs differ
    down_d = np.where(neg, mag[2:, :-2], mag[2:, 2:])
    horiz = y < tg22x
    vert = ~horiz & (y > tg67x)
    diag = ~horiz & ~vert
    is_max = (horiz & (m > mag[1:-1, :-2]) & (m >= mag[1:-1, 2:])) | (vert & (m > mag[:-2, 1:-1]) & (m >= mag[2:, 1:-1])) | \
             (diag & (m > up_d) & (m > down_d))
    out = np.ones((H, W), dtype=np.uint8)
    cand = is_max & (m > low)
    out[cand] = 0
    out[cand & (m > high)] = 2
    return out


def hysteresis(mp: np.ndarray) -> np.ndarray:
    from scipy import ndimage
    lab, n = ndimage.label(mp != 1, structure=np.ones((3, 3), dtype=int))
    keep = np.zeros(n + 1, dtype=bool)
    keep[np.unique(lab[mp == 2])] = True
    keep[0] = False
    return np.where(keep[lab], 255, 0).astype(np.uint8)


def canny_u8(img: np.ndarray, low, high) -> np.ndarray:
    """cv2.Canny(img, low, high) for uint8 [H,W] or [H,W,3] -> uint8 [H,W], 255 or 0."""
    assert img.dtype == np.uint8
    low, high = thresholds(low, high)
    return hysteresis(canny_map(img, low, high))


def sweep_count(mp: np.ndarray) -> int:
    """A model of the device's hysteresis: every sweep, each TILE x TILE tile takes its pixels and a one-pixel apron as the map
    stood before the sweep and grows its strong pixels through its candidates until it is stable.  -> the number of sweeps up to
    and including the first that moves nothing (the one whose flag the host reads as 0)."""
    from scipy import ndimage
    mp = mp.copy()
    H, W = mp.shape
    eight = np.ones((3, 3), dtype=int)
    sweeps = 0
    while True:
        sweeps += 1
        before = np.pad(mp, 1, constant_values=1)
        moved = False
        for y0 in range(0, H, TILE):
            for x0 in range(0, W, TILE):
                h, w = min(TILE, H - y0), min(TILE, W - x0)
                t = before[y0:y0 + h + 2, x0:x0 + w + 2]
                inner = np.zeros(t.shape, dtype=bool)
                inner[1:-1, 1:-1] = True
                grow = (t == 2) | ((t == 0) & inner)             # apron candidates are not grown, apron strong pixels seed
                lab, n = ndimage.label(grow, structure=eight)
                keep = np.zeros(n + 1, dtype=bool)
                keep[np.unique(lab[t == 2])] = True
                keep[0] = False
                new = keep[lab] & inner & (t == 0)
                if new.any():
                    mp[y0:y0 + h, x0:x0 + w][new[1:-1, 1:-1]] = 2
                    moved = True
        if not moved:
            return sweeps


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs

SERP = 160         # 5 x 5 hysteresis tiles


def serpentine(c: int, strong: int) -> np.ndarray:
    """One 6-pixel-wide path of grey level c through all five 32-row groups of a 160x160 image: a horizontal band per group at rows
    32r+16 .. 32r+21, columns 8 .. 151, consecutive bands joined by a vertical band alternately at the right end (x 146 .. 151) and
    the left end (x 8 .. 13); the piece at rows 16 .. 21, columns 8 .. 19 is raised to `strong`."""
    img = np.zeros((SERP, SERP), dtype=np.uint8)
    for r in range(5):
        img[32 * r + 16:32 * r + 22, 8:152] = c
        if r < 4:
            xs = slice(146, 152) if r % 2 == 0 else slice(8, 14)
            img[32 * r + 16:32 * (r + 1) + 22, xs] = c
    img[16:22, 8:20] = strong
    return img


def with_isolated_band(img: np.ndarray, level: int = 30) -> np.ndarray:
    """The image plus a band at rows 96 .. 99, columns 60 .. 99: candidates that touch no strong pixel."""
    out = img.copy()
    out[96:100, 60:100] = level
    return out


def colour_serpentine(c: int = 30, strong: int = 60, blue: bool = True) -> np.ndarray:
    """[160,160,3] in cv2 channel order: R is the weak serpentine (level c throughout), B is level `strong` on the strong piece (or
    zero with blue=False), G is zero.  The only strong pixels come from B winning the channel choice.  Behind the piece B falls
    to zero in steps of 10, a column each: a hard end would win the choice in the column next to it with a horizontal gradient,
    fail the suppression there and cut R's candidates off from the strong pixels (the map then has 32 pixels on)."""
    img = np.zeros((SERP, SERP, 3), dtype=np.uint8)
    img[..., 2] = serpentine(c, c)
    if blue:
        img[16:22, 8:20, 0] = strong
        for k, v in enumerate(range(strong - 10, 0, -10)):
            img[16:22, 20 + k, 0] = v
    return img


def tie_case() -> np.ndarray:
    """A 3x3 colour image whose centre has equal norms in channels 0 and 1 with gradients of different direction, and a smaller
    norm in channel 2: the choice must be channel 0's."""
    img = np.zeros((3, 3, 3), dtype=np.uint8)
    img[:, 2, 0] = 50                                            # channel 0: dx = 200, dy = 0
    img[2, :, 1] = 50                                            # channel 1: dx = 0, dy = 200
    img[:, 0, 2] = 40                                            # channel 2: dx = -160, dy = 0
    return img


def seeded_images(H: int, W: int, channels: int, seed: int, n: int = 1) -> np.ndarray:
    """n images [n,H,W] or [n,H,W,3]: smooth blobs with some noise on top, edges of every strength."""
    g = np.random.default_rng(seed)
    shape = (n, H, W) + ((3,) if channels == 3 else ())
    coarse = g.integers(0, 256, size=(n, (H + 7) // 8 + 1, (W + 7) // 8 + 1) + shape[3:]).astype(np.float64)
    up = np.repeat(np.repeat(coarse, 8, axis=1), 8, axis=2)[:, :H, :W]
    noise = g.normal(0.0, 6.0, size=shape)
    return np.clip(up + noise, 0, 255).astype(np.uint8)
