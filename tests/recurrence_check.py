"""Float64 references, operand-scaled bounds and exact output contracts for the kernels of the RAFT iteration that are not
convolutions: the flow head (flow_head.hip, and the OFX_EPI_FLOW epilogue of ofx_conv2d), the 4-level radius-4 correlation lookup
(corr.hip) and the convex upsample (upsample_inl.h).  Not a conftest: imported by name, like wino_check.py, whose bound it uses:
|out - ref| <= K 2^-24 M + extra + TINY, with M the magnitude of the operation and `extra` half an ulp of a rounded coordinate.
"""
import torch
import torch.nn.functional as F

import wino_check as wc

EPS = wc.EPS
# K per kernel: at most 2x the largest |err| / (2^-24 M) measured on MI355X over tests/test_gpu_recurrence_kernels.py (beyond the
# `extra` each check allows).  Measured maxima:
#   flow head (coords1)                                    0.866
#   OFX_EPI_FLOW of ofx_conv2d (coords1)                   2.10
#   4-level radius-4 lookup, blocked kernel                3.26
#   convex upsample (M with the exponent-argument term)    6.87
K_FLOW_HEAD = 1.7
K_FLOW_CONV = 4.2
K_LOOKUP = 6.5
K_UPSAMPLE = 13.7

RADIUS, LEVELS, RD = 4, 4, 9
STRIP_H, STRIP_W = 4, 8              # flow_head.hip: kPR x kPW output pixels per strip


def half_ulp32(x):
    """Half an ulp of fp32(x), elementwise, as float64 (x any float dtype): the largest error of rounding x to fp32."""
    x32 = x.float().abs()
    _, e = torch.frexp(x32)                      # x = m 2^e, m in [0.5, 1): ulp = 2^(e - 24)
    h = torch.ldexp(torch.ones_like(x32, dtype=torch.float64), (e - 25).to(torch.int64))
    return torch.where(x32 == 0, torch.zeros_like(h), h)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


# ---------------------------------------------------------------------------------------------------------------------------------
# flow head

def flow_head_branch(B, h, w):
    """The launch branch ofx_flow_head_launch takes: one wave per workgroup, four-wave workgroups, or the grid-stride loop."""
    strips = B * -(-h // STRIP_H) * -(-w // STRIP_W)
    return "wave" if strips <= 1024 else "quad" if strips <= 256 * 16 * 4 else "stride"


def grid32(B, h, w):
    """coords0 [B,h,w,2] fp32: (x, y) per pixel."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys], -1)[None].expand(B, h, w, 2).contiguous()


def flow_head_reference(x, wt, bias, coords):
    """x [B,h,w,>=256] NHWC, wt OIHW [2,256,3,3], bias [2], coords [B,h,w,2] -> (coords + (conv + bias), M) in float64, NHWC.
    M = conv(|x|, |w|) + |bias|: the magnitude of delta, whose error the coordinate add carries over unchanged."""
    xn = x[..., :256].permute(0, 3, 1, 2)
    delta, mag = wc.reference(xn, wt, 3, 3, shift=bias)
    return coords.double() + delta.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def check_coords(c1, ref, mag, K, what):
    """The updated coordinates: the delta's error plus half an ulp of the coordinate (its one rounding)."""
    return wc.check(c1, ref, mag, K, what, extra=half_ulp32(ref))


def frows_expected(flow, fill):
    """The contract of frows [B,h,w,16] for the flow [B,h,w,2] the kernel left in hx: slot s (floats 2s, 2s+1) of pixel x holds the
    flow of pixel x + s - 3 where that pixel is inside the row; every other float keeps `fill` (a [B,h,w,16] tensor)."""
    out = fill.clone()
    w = flow.shape[2]
    for s in range(7):
        d = s - 3
        lo, hi = max(0, -d), min(w, w - d)           # pixels x whose neighbour x + d is inside the image
        if lo < hi:
            out[:, :, lo:hi, 2 * s:2 * s + 2] = flow[:, :, lo + d:hi + d]
    return out


def check_flow_contract(c1, hx, flow_off, frows, hx_before, frows_before, what):
    """The exact part of the flow head's output contract: hx_flow = coords1 - grid bit for bit (fp32), frows as frows_expected,
    every other channel of hx unchanged."""
    B, h, w, _ = c1.shape
    flow = c1.float() - grid32(B, h, w)
    assert same_bits(hx[..., flow_off:flow_off + 2], flow), f"{what}: hx flow slot is not coords1 - grid"
    other = torch.ones(hx.shape[-1], dtype=torch.bool)
    other[flow_off:flow_off + 2] = False
    assert same_bits(hx[..., other], hx_before[..., other]), f"{what}: hx channels outside the flow slot were written"
    exp = frows_expected(flow, frows_before)
    if not same_bits(frows, exp):
        bad = (bits(frows) != bits(exp)).nonzero()[0].tolist()
        raise AssertionError(f"{what}: frows differ from the contract at {bad}: got {float(frows[tuple(bad)])}, "
                             f"want {float(exp[tuple(bad)])}")


# ---------------------------------------------------------------------------------------------------------------------------------
# correlation lookup (levels 4, radius 4)

def window_start(c, l):
    """The kernel's window origin at level l: floor(c / 2^l) - r (the 10 x 10 window of block loads starts there)."""
    return int(torch.floor(torch.tensor(c, dtype=torch.float32) / 2 ** l)) - RADIUS


def overlap(c, l, n):
    """Columns (or rows) of the n-wide level-l map that the 9 taps of coordinate c touch with nonzero weight, and on which side the
    window hangs off the map ('lo' / 'hi' / 'in')."""
    s = float(torch.tensor(c, dtype=torch.float32)) / 2 ** l
    f0 = int(torch.floor(torch.tensor(s)))
    last = f0 + RADIUS + (1 if s > f0 else 0)
    first = f0 - RADIUS
    inside = max(0, min(last, n - 1) - max(first, 0) + 1)
    side = "lo" if first < 0 else "hi" if last > n - 1 else "in"
    return inside, side


def lookup_reference(pyr, coords, B, h, w):
    """pyr: the kernel's fp32 pyramid unblocked, level l [M, h_l, w_l]; coords [M,2] (x, y) -> (ref, M, extra) [M, 324] in float64:
    CorrBlock.__call__ (corr.py:29-50) sampling level l at (x / 2^l + i - r, y / 2^l + j - r) into channel l*81 + i*9 + j, bilinear
    with zeros outside.  M = sum over the four taps of weight x |value|.  extra: the fractional offset fx = x / 2^l - floor(x / 2^l)
    rounds in fp32 where x / 2^l is negative and finer than fx (in (-1, 0), say); there the bound allows half an ulp of fx times
    the sensitivity of the sample to it, (1 - fy)(|v00| + |v01|) + fy (|v10| + |v11|), and the same for fy."""
    M = coords.shape[0]
    c = coords.double()
    off = torch.arange(-RADIUS, RADIUS + 1, dtype=torch.float64)
    refs, mags, extras = [], [], []
    for l, p in enumerate(pyr):
        hl, wl = p.shape[1], p.shape[2]
        flat = p.double().reshape(M, hl * wl)
        xs, ys = c[:, 0] / 2 ** l, c[:, 1] / 2 ** l
        x0, y0 = torch.floor(xs), torch.floor(ys)
        fx, fy = (xs - x0).view(M, 1, 1), (ys - y0).view(M, 1, 1)
        ex, ey = (torch.where(f.float().double() != f, half_ulp32(f), torch.zeros_like(f)) for f in (fx, fy))
        X = (x0.view(M, 1, 1) + off.view(1, RD, 1)).expand(M, RD, RD)     # i: x offset (slow)
        Y = (y0.view(M, 1, 1) + off.view(1, 1, RD)).expand(M, RD, RD)     # j: y offset (fast)

        def tap(dx, dy):
            xi, yi = X + dx, Y + dy
            ok = (xi >= 0) & (xi < wl) & (yi >= 0) & (yi < hl)
            idx = (yi.clamp(0, hl - 1) * wl + xi.clamp(0, wl - 1)).long().reshape(M, -1)
            v = torch.gather(flat, 1, idx).reshape(M, RD, RD)
            return torch.where(ok, v, torch.zeros_like(v))
        v00, v01, v10, v11 = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
        w00, w01, w10, w11 = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy
        refs.append(v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11)
        mags.append(v00.abs() * w00 + v01.abs() * w01 + v10.abs() * w10 + v11.abs() * w11)
        dfx = (1 - fy) * (v00.abs() + v01.abs()) + fy * (v10.abs() + v11.abs())
        dfy = (1 - fx) * (v00.abs() + v10.abs()) + fx * (v01.abs() + v11.abs())
        extras.append(ex * dfx + ey * dfy)
    cat = lambda ts: torch.cat([t.reshape(M, RD * RD) for t in ts], 1)
    return cat(refs), cat(mags), cat(extras)


# ---------------------------------------------------------------------------------------------------------------------------------
# convex upsample

def upsample_reference(coords, mask, transposed=False):
    """coords [B,h,w,2] fp32, mask [B,h,w,576] -> (ref, M) [B,8h,8w,2] in float64 from the same fp32 inputs.
    M = sum_k a_k |8 (c_k - x_k)| (1 + |z_k|): a_k the exact softmax weight of neighbour k, z_k = logit - max its exponent argument.
    v_exp_f32 evaluates 2^(z log2 e), so the rounding of that argument makes a relative error of the order of |z| 2^-24 in a_k, the
    exponential itself and the hardware reciprocal a few ulp more: all of it scales with this M.  `transposed` (a simulated bug):
    the 3x3 neighbours in transposed order."""
    B, h, w, _ = coords.shape
    lg = mask.double().reshape(B, h, w, 9, 64)
    z = lg - lg.max(dim=3, keepdim=True).values
    a = torch.softmax(lg, dim=3)
    f = 8.0 * (coords.double() - grid32(B, h, w).double())                      # [B,h,w,2]
    nb = F.unfold(f.permute(0, 3, 1, 2), [3, 3], padding=1).reshape(B, 2, 9, h, w).permute(0, 3, 4, 2, 1)   # [B,h,w,9,2]
    if transposed:
        nb = nb[:, :, :, [3 * (k % 3) + k // 3 for k in range(9)]]
    ref = torch.einsum("bhwks,bhwkc->bhwsc", a, nb)
    mag = torch.einsum("bhwks,bhwkc->bhwsc", a * (1 + z.abs()), nb.abs())
    fine = lambda t: t.reshape(B, h, w, 8, 8, 2).permute(0, 1, 3, 2, 4, 5).reshape(B, 8 * h, 8 * w, 2)
    return fine(ref), fine(mag)
