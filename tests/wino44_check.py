"""Cases, float64 references and the bound of the fused Winograd F(4x4,3x3) kernel's tests (not a conftest: imported by name).

Every case is forced with TILE_WINOGRAD4 and checked elementwise with wino_check's operand-scaled bound |err| <= K 2^-24 M.
K_F43 follows wino_check's rule: at most 2x the largest ratio measured on MI355X over this file's own cases (CASES and the five
engine-layer descriptors).
"""
import math

import torch

import wino_check as wc

# measured maximum of |err| / (2^-24 M) over CASES + ENGINE_LAYERS on MI355X: 72.5 (fh1; F(2x2,3x3) over the same cases: 3.89)
K_F43 = 145.0

# (name, B, H, W, (c0, c1), Cout, distribution, relu, scale/shift, (ldo, offset) or None)
CASES = [
    # one patch, one slab, Cout tails
    ("one_patch_co1", 1, 16, 32, (16, 0), 1, "normal", False, False, None),
    ("one_patch_co33", 1, 16, 32, (16, 0), 33, "normal", True, False, None),
    ("one_patch_co64", 1, 16, 32, (16, 0), 64, "normal", False, True, None),
    ("one_patch_co65", 1, 16, 32, (16, 0), 65, "normal", True, True, None),
    # several patches: zero padding on every border, interior halos shared between patches (8 workgroups: a multiple of 8)
    ("patches_2x2x2", 2, 32, 64, (32, 0), 64, "relu", True, True, None),
    # patch rows against columns
    ("three_patch_rows", 1, 48, 32, (16, 0), 64, "tanh", False, False, None),
    ("three_patch_cols", 1, 16, 96, (16, 0), 64, "normal", True, False, None),
    # two input segments, one split off a 64-channel boundary
    ("segments_96_32", 1, 16, 32, (96, 32), 126, "relu", True, True, None),
    ("segments_32_16", 1, 16, 32, (32, 16), 126, "normal", False, False, None),
    # strided destination with a channel offset
    ("strided_dst", 1, 16, 32, (16, 0), 126, "tanh", True, True, (192, 33)),
    # the XCD remap's other two classes: 9 and 13 workgroups
    ("groups_9", 1, 48, 96, (16, 0), 64, "normal", False, True, None),
    ("groups_13", 13, 16, 32, (16, 0), 33, "relu", True, False, None),
]

# the engine's five layers (name, (c0, c1), Cout, relu), at B = 2, 32x64
ENGINE_LAYERS = [
    ("convc2", (256, 0), 192, True),
    ("conv", (192, 64), 126, True),
    ("convf2", (128, 0), 64, True),
    ("fh1", (128, 0), 256, True),
    ("mask0", (128, 0), 256, True),
]


def draw(shape, dist, g):
    x = torch.randn(shape, generator=g)
    if dist == "relu":
        return torch.relu(x)
    if dist == "tanh":
        return torch.tanh(x)
    return x


def make(case, seed):
    """-> dict of the case's CPU tensors: x0, x1 (NCHW, x1 None), w (OIHW), scale, shift (None), ref and mag (NCHW float64)."""
    name, B, H, W, (c0, c1), co, dist, relu, affine, dst = case
    g = torch.Generator().manual_seed(seed)
    x0 = draw((B, c0, H, W), dist, g)
    x1 = draw((B, c1, H, W), dist, g) if c1 else None
    w = torch.randn((co, c0 + c1, 3, 3), generator=g) / math.sqrt(9 * (c0 + c1))
    scale = (torch.rand((co,), generator=g) + 0.5) if affine else None
    shift = torch.randn((co,), generator=g) * 0.1 if affine else None
    x = x0 if x1 is None else torch.cat([x0, x1], 1)
    ref, mag = wc.reference(x, w, 3, 3, scale=scale, shift=shift, relu=relu)
    return dict(x0=x0, x1=x1, w=w, scale=scale, shift=shift, ref=ref, mag=mag, relu=relu, co=co, dst=dst, shape=(B, H, W))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().cpu()


def run(ops, c, tile, ops_w=None, joined=False):
    """One launch of case `c` (make()) on the device with `tile`; -> (NCHW cpu result, the whole destination or None).
    ops_w: the cached device operands (packed, F(2x2), F(4x4)).  joined: the two segments as one tensor (the same convolution;
    every route but the forced F(4x4) one refuses segments that are not whole 32-channel chunks)."""
    wp, u2, u4 = ops_w
    B, H, W = c["shape"]
    co = c["co"]
    kw = dict(act="relu" if c["relu"] else None, wino_w=u2, wino4_w=u4, tile=tile)
    if c["scale"] is not None:
        kw.update(scale=c["scale"].cuda(), shift=c["shift"].cuda())
    if c["x1"] is not None and joined:
        c = dict(c, x0=torch.cat([c["x0"], c["x1"]], 1), x1=None)
    if c["x1"] is not None:
        kw["x2"] = nhwc(c["x1"])
    if c["dst"]:
        ld, off = c["dst"]
        dst = torch.full((B, H, W, ld), float("nan"), device="cuda")
        ops.conv2d_nhwc(nhwc(c["x0"]), wp, 3, 3, co, out=dst, out_off=off, **kw)
        return nchw(dst[..., off:off + co]), dst
    return nchw(ops.conv2d_nhwc(nhwc(c["x0"]), wp, 3, 3, co, **kw)), None


def operands(ops, w):
    return ops.pack_conv_weight(w).cuda(), ops.wino_conv_weight(w).cuda(), ops.wino44_conv_weight(w).cuda()
