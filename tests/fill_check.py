"""Helper (not a test): numpy restatement of the reference's `fill_mask_input` (guided_ldm_inpainting.py:161-176) as Pillow's
integer arithmetic, step by step:

    paste        Image.new('RGBa').paste(image.convert('RGBA').convert('RGBa'), mask=ImageOps.invert(mask))      Paste.c
    blur_rgba    ImageFilter.GaussianBlur(radius) on the 4-channel image, every channel like an 'L' plane       BoxBlur.c
    unpremultiply  .convert('RGBA') of an 'RGBa' image                                                          Convert.c
    alpha_composite  Image.alpha_composite (in place on the accumulator)                                        AlphaComposite.c
    fill_mask_input  the chain, .convert('RGB') at the end

Pinned against the real Pillow by tests/golden/make_golden_fill.py (tests/golden/fill_mask_pil.npz) and, where Pillow is
importable, against live Pillow by tests/test_fill_host.py.  The single-channel box blur is oracle/handoff_oracle.py's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import handoff_oracle as HO  # noqa: E402

STAGES = ((256, 1), (64, 1), (16, 2), (4, 4), (2, 2), (0, 1))      # (GaussianBlur radius, alpha_composite repeats)
GOLDEN = os.path.join(ROOT, "tests", "golden", "fill_mask_pil.npz")


def div255(a):
    """Paste.c DIV255 on an integer array."""
    t = a + 128
    return ((t >> 8) + t) >> 8


def paste(image: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """image u8 [H,W,3], mask u8 [H,W] (255 = repaint) -> premultiplied RGBa u8 [H,W,4]: the opaque source pasted onto zeros through
    255 - mask, colours and alpha alike."""
    inv = 255 - mask.astype(np.int64)
    out = np.empty(mask.shape + (4,), np.uint8)
    out[..., :3] = div255(image.astype(np.int64) * inv[..., None])
    out[..., 3] = div255(255 * inv)                                # == inv
    return out


def blur_rgba(a: np.ndarray, radius: float) -> np.ndarray:
    """GaussianBlur(radius) of u8 [H,W,4]: the four channels are blurred alike and independently (radius 0: a copy)."""
    return np.stack([HO.gaussian_blur_u8(np.ascontiguousarray(a[..., c]), radius) for c in range(a.shape[-1])], axis=-1)


def unpremultiply(a: np.ndarray) -> np.ndarray:
    """'RGBa' -> 'RGBA': c unchanged at alpha 0 or 255, else min(255, 255 * c // alpha)."""
    al = a[..., 3].astype(np.int64)
    c = a[..., :3].astype(np.int64)
    q = np.minimum(255, 255 * c // np.maximum(al, 1)[..., None])
    keep = ((al == 0) | (al == 255))[..., None]
    out = a.copy()
    out[..., :3] = np.where(keep, c, q)
    return out


def _shift255(a):
    return (a + (a >> 8)) >> 8


def alpha_composite(dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    """Image.alpha_composite(dst, src) on straight-alpha u8 [H,W,4] (7 precision bits, all uint32 in the C source)."""
    d, s = dst.astype(np.int64), src.astype(np.int64)
    sa, da = s[..., 3], d[..., 3]
    outa255 = sa * 255 + da * (255 - sa)
    coef1 = sa * 255 * 255 * 128 // np.maximum(outa255, 1)
    coef2 = 255 * 128 - coef1
    out = np.empty_like(d)
    out[..., :3] = _shift255(s[..., :3] * coef1[..., None] + d[..., :3] * coef2[..., None] + (0x80 << 7)) >> 7
    out[..., 3] = _shift255(outa255 + 0x80)
    return np.where((sa == 0)[..., None], d, out).astype(np.uint8)


def fill_mask_input(image: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """image u8 [H,W,3] (any channel order), mask u8 [H,W] = the blurred 'L' mask -> the filled frame u8 [H,W,3]."""
    pasted = paste(image, mask)
    acc = np.zeros_like(pasted)
    for radius, repeats in STAGES:
        src = unpremultiply(blur_rgba(pasted, radius))
        for _ in range(repeats):
            acc = alpha_composite(acc, src)
    return np.ascontiguousarray(acc[..., :3])


# ---- the same with the real Pillow (golden generation and the live comparison) ----------------------------------------------------
def pil_fill_mask_input(image: np.ndarray, mask: np.ndarray) -> np.ndarray:
    from PIL import Image, ImageFilter, ImageOps
    img, m = Image.fromarray(image, "RGB"), Image.fromarray(mask, "L")
    pasted = Image.new("RGBa", img.size)
    pasted.paste(img.convert("RGBA").convert("RGBa"), mask=ImageOps.invert(m))
    acc = Image.new("RGBA", img.size)
    for radius, repeats in STAGES:
        layer = pasted.filter(ImageFilter.GaussianBlur(radius)).convert("RGBA")
        for _ in range(repeats):
            acc.alpha_composite(layer)
    return np.array(acc.convert("RGB"))


def pil_blur_rgba(a: np.ndarray, radius: float) -> np.ndarray:
    from PIL import Image, ImageFilter
    return np.array(Image.fromarray(a, "RGBa").filter(ImageFilter.GaussianBlur(radius)))


def random_case(seed: int, H: int, W: int, kind: str = "blobs"):
    """(image u8 [H,W,3], blurred mask u8 [H,W]).  kind: 'blobs' (rectangles + speckle, blurred at radius 4 like the sampler's
    mask), 'noise' (every value), 'full' (all 255), 'none' (all 0)."""
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "full":
        return image, np.full((H, W), 255, np.uint8)
    if kind == "none":
        return image, np.zeros((H, W), np.uint8)
    if kind == "noise":
        return image, rng.integers(0, 256, (H, W), dtype=np.uint8)
    mask = np.zeros((H, W), np.uint8)
    for _ in range(3):
        y, x = rng.integers(0, H), rng.integers(0, W)
        mask[max(0, y - 5):y + 5, max(0, x - 8):x + 8] = 255
    mask[rng.random((H, W)) < 0.02] = 255
    return image, HO.gaussian_blur_u8(mask, 4.0)
