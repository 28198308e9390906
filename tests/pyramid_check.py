"""The correlation pyramid's builders, restated for their tests: which kernels a shape takes (the rule of ofx_corr_volume and
ofx_corr_pool_launch in corr.hip), the blocked layout, the exact pooling arithmetic of every path and the float64 reference of
level 0.  Not a conftest: imported by name, like recurrence_check.py.  Everything here is plain torch and runs on any device.

What is checked, and how
  level 0       the batched volume GEMM (conv.hip, kEpiVolPool or the plain epilogue; corr_split.hip), fed by block_rows_kernel:
                against the float64 product of the same fp32 feature maps, |out - ref| <= K_VOL 2^-24 M + TINY with
                M = (|f1| . |f2|) / 16 (wino_check.check).
  levels 1..3   BIT FOR BIT against `expected_pyramid` of the level 0 the device stored.  Every pooling step on every path adds four
                stored fp32 values in a fixed order and multiplies by 0.25 (exact): the pooled levels are deterministic functions of
                level 0, so a tolerance would only hide a wrong neighbour or a differently rounded step that happens to lie near
                the right value.
  layout        padding elements of a blocked slice are +0.0 at exactly the positions `blocked_map` names (the lookup reads them as
                the zeros outside the map); no sentinel survives inside a slice of a level that was asked for; levels that were not
                asked for and the guard floats behind every buffer keep their sentinels.

The pooling order per path (read from the kernels; a b on the upper row, c d below)
  level 1, fused into the GEMM (h % 8 == 0 and w % 16 == 0; conv.hip, VOLPOOL epilogue): s1 = v + v[lane ^ 1], s2 = s1 + s1[lane ^ 8]
                on the values it has just stored: ((a + b) + (c + d)) * 0.25.
  level 1, ofx_corr_volume_split (corr_split.hip, park): ((a + b) + (c + d)) * 0.25 on the accumulators it stores, in every arithmetic.
  level 1, pyramid_pool_kernel from level 0 (every other shape): (((a + b) + c) + d) * 0.25.
  levels 2, 3, pyramid_pool_kernel (LDS) and pyramid_pool_reg_kernel (registers): (((a + b) + c) + d) * 0.25, each from the level
                above as stored.
No step was found that is not an exact function of the stored values, so no pooled level falls back to the float64 bound.

Deliberately not covered: the launcher's fall-back to the LDS kernel for wps > 64 or wb1 > 64 (a level 0 of 17 GB or more), the LDS
kernel's refusal of maps above 64 KiB of LDS (about 10 GB), and the OFX_POOL_* environment knobs (read once per process).
"""
from collections import namedtuple

import torch

import wino_check as wc

EPS = wc.EPS
# K_VOL: at most 2x the largest |err| / (2^-24 M) of level 0 measured on MI355X over tests/test_gpu_corr_pyramid.py (the generic
# batched GEMM of ofx_corr_volume over VOLUME_CASES and STRIDE_CASE; the largest cases on sampled source pixels).  Measured maximum:
#   level 0 of ofx_corr_volume                             24.87
K_VOL = 49.0

SENT = 0x7FC0FFEE                    # a quiet NaN with a payload: kept bit for bit wherever nothing may be written
GUARD = 64                           # floats behind every buffer
D = 256                              # feature channels: the volume is scaled by 1 / sqrt(D) = 2^-4

POOL_GRID_CAP = 256 * 64             # workgroups of pyramid_pool_reg_kernel
POOL_PAIR = 4                        # adjacent 1 KB pieces per wave and trip
LIM31 = (1 << 31) - 64

PoolPath = namedtuple("PoolPath", "fused register wb1 wps lds_bytes nwaves stride dims slices")


def slice_floats(hl, wl):
    """Floats of one pixel's slice of an hl x wl level: whole 4 x 8 blocks (ofx_corr_slice_floats)."""
    return ((hl + 3) // 4) * ((wl + 7) // 8) * 32


def pool_path(h, w, levels, B=1, split=False):
    """The kernels ofx_corr_volume (split: ofx_corr_volume_split) runs for B maps of h x w and `levels` levels.
    fused      level 1 comes out of the GEMM: h % 8 == 0 and w % 16 == 0, level 0's slice whole 128-column tiles and level 1 of one
               pair inside 32-bit byte offsets (the split entry takes no other shape)
    register   levels 2 and 3 by pyramid_pool_reg_kernel: fused, h1 % 16 == 0, w1 % 32 == 0, levels >= 3, fewer than 2^26 waves,
               2 <= wps <= 64 and 2 <= wb1 <= 64 (wps = slice1 / 256 waves per slice, wb1 blocks per row of level 1)
    lds_bytes  dynamic LDS of pyramid_pool_kernel (the three row-major maps), whichever kernel runs
    nwaves     waves of the register kernel's work (one per 64 float4 of level 1); stride: its grid-stride loop makes a second trip,
               nwaves > 16384 workgroups x 4 waves x 4 pieces"""
    dims = [(h >> l, w >> l) for l in range(4)]
    slices = [slice_floats(*d) if d[0] > 0 and d[1] > 0 else 0 for d in dims]
    n = h * w
    fused = levels >= 2 and h % 8 == 0 and w % 16 == 0 and slices[0] % 128 == 0 and n * slices[1] * 4 < LIM31
    if split:
        assert fused and n >= 64 and n * n * 4 < LIM31, "ofx_corr_volume_split refuses this shape"
    (h1, w1) = dims[1]
    wb1 = (w1 + 7) // 8
    f4 = slices[1] // 4
    wps = f4 // 64
    nwaves = B * n * f4 // 64
    register = (fused and levels >= 3 and h1 % 16 == 0 and w1 % 32 == 0 and nwaves < (1 << 26) and 2 <= wps <= 64 and 2 <= wb1 <= 64)
    lds = 4 * sum(a * b for a, b in dims[1:])
    grid = min((B * n * f4 + 255) // 256, POOL_GRID_CAP)
    stride = register and nwaves > grid * 4 * POOL_PAIR
    return PoolPath(fused, register, wb1, wps, lds, nwaves, stride, dims, slices)


def blocked_map(hl, wl):
    """int64 [slice_floats(hl, wl)]: for every float of a blocked slice the row-major index y * wl + x of the element it holds, or
    -1 for padding.  corr.hip: element (y, x) sits at ((y / 4) * ceil(wl / 8) + x / 8) * 32 + (y % 4) * 8 + x % 8."""
    wb = (wl + 7) // 8
    out = torch.full((slice_floats(hl, wl),), -1, dtype=torch.int64)
    ys, xs = torch.meshgrid(torch.arange(hl), torch.arange(wl), indexing="ij")
    pos = ((ys // 4) * wb + xs // 8) * 32 + (ys % 4) * 8 + xs % 8
    out[pos.reshape(-1)] = (ys * wl + xs).reshape(-1)
    return out


def unblock(level, hl, wl):
    """Blocked slices [M, slice] -> row-major [M, hl, wl], through blocked_map (on the tensor's device)."""
    bm = blocked_map(hl, wl)
    where = torch.empty(hl * wl, dtype=torch.int64)
    valid = (bm >= 0).nonzero().reshape(-1)
    where[bm[valid]] = valid
    return level.index_select(1, where.to(level.device)).reshape(-1, hl, wl)


def block(rowmajor, fill=0.0):
    """Row-major [M, hl, wl] -> blocked slices [M, slice] with `fill` in the padding (the layout the kernels write)."""
    M, hl, wl = rowmajor.shape
    bm = blocked_map(hl, wl)
    out = torch.full((M, bm.numel()), fill, dtype=rowmajor.dtype)
    valid = (bm >= 0).nonzero().reshape(-1)
    out[:, valid] = rowmajor.reshape(M, hl * wl)[:, bm[valid]]
    return out


def _quads(t):
    h2, w2 = t.shape[1] // 2, t.shape[2] // 2           # an odd last row or column is floored away
    return (t[:, 0:2 * h2:2, 0:2 * w2:2], t[:, 0:2 * h2:2, 1:2 * w2:2], t[:, 1:2 * h2:2, 0:2 * w2:2], t[:, 1:2 * h2:2, 1:2 * w2:2])


def pool_seq(t):
    """(((a + b) + c) + d) * 0.25 in fp32 over 2x2 windows of row-major [M, hl, wl]: avg_pool2d's window sum."""
    a, b, c, d = _quads(t)
    return (((a + b) + c) + d) * 0.25


def pool_pair(t):
    """((a + b) + (c + d)) * 0.25 in fp32: rows first, then the two row sums."""
    a, b, c, d = _quads(t)
    return ((a + b) + (c + d)) * 0.25


def expected_pyramid(level0, path, levels):
    """Row-major levels 1 .. levels - 1 from the device's own level 0 (row-major [M, h, w], fp32), in the order each path uses (see
    the module docstring): level 1 by pool_pair where the GEMM wrote it (path.fused; the split entry always), by pool_seq from
    pyramid_pool_kernel; levels 2 and 3 by pool_seq on either pooling kernel."""
    assert level0.dtype == torch.float32
    out, t = [], level0
    for l in range(1, levels):
        t = (pool_pair if (l == 1 and path.fused) else pool_seq)(t)
        out.append(t)
    return out


def _pairs(f1, f2):
    B, h, w, d = f1.shape
    assert d == D and f2.shape[0] in (1, B) and tuple(f2.shape[1:]) == (h, w, d)
    return B, h, w


def level0_reference(f1, f2):
    """f1 [B,h,w,256], f2 [B or 1,h,w,256] fp32 (NHWC; one f2 map: shared by every pair) -> (ref, M) [B*h*w, h, w] float64:
    corr[b, i, j] = <f1[b, i], f2[b, j]> / 16 (RAFT/core/corr.py:52-60) and its magnitude (|f1| . |f2|) / 16."""
    B, h, w = _pairs(f1, f2)
    a, b = f1.double().reshape(B, h * w, D), f2.double().reshape(-1, h * w, D)
    ref = torch.matmul(a, b.transpose(1, 2)) / 16.0
    mag = torch.matmul(a.abs(), b.abs().transpose(1, 2)) / 16.0
    return ref.reshape(B * h * w, h, w), mag.reshape(B * h * w, h, w)


def level0_reference_rows(f1, f2, rows):
    """The rows (source pixels m = b h w + i) of level0_reference named by `rows`: (ref, M) [len(rows), h, w]."""
    B, h, w = _pairs(f1, f2)
    n = h * w
    a, b = f1.reshape(B * n, D), f2.reshape(-1, n, D)
    refs, mags = [], []
    for m in rows:
        x, y = a[m].double(), b[(m // n) % b.shape[0]].double()
        refs.append((y @ x) / 16.0)
        mags.append((y.abs() @ x.abs()) / 16.0)
    return torch.stack(refs).reshape(-1, h, w), torch.stack(mags).reshape(-1, h, w)


def sample_rows(B, h, w):
    """A fixed sample of source pixels: the first and last, both sides of every image boundary, and a few inside each image."""
    n = h * w
    rows = {0, B * n - 1}
    for b in range(B):
        rows |= {b * n, b * n + n - 1, b * n + n // 3, b * n + (5 * n) // 7 + 1, b * n + w - 1, b * n + w}
    return sorted(r for r in rows if 0 <= r < B * n)


# ---------------------------------------------------------------------------------------------------------------------------------
# buffers and the exact checks

def sentinel(n, device="cpu"):
    return torch.full((n,), SENT, dtype=torch.int32, device=device).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def level_buffers(B, h, w, device="cpu"):
    """Four flat level buffers of M * slice_l + GUARD floats, every float the sentinel."""
    p = pool_path(h, w, 4, B)
    return [sentinel(B * h * w * s + GUARD, device) for s in p.slices]


def level_view(buf, M):
    return buf[:buf.numel() - GUARD].view(M, -1)


def restated_buffers(level0, path, levels):
    """What a correct call leaves in `level_buffers`, from a row-major level 0 [M, h, w] (CPU): the restatement the checker's own
    tests start from."""
    M, h, w = level0.shape
    bufs = [sentinel(M * s + GUARD) for s in path.slices]
    for l, t in enumerate([level0] + expected_pyramid(level0, path, levels)):
        level_view(bufs[l], M)[:] = block(t)
    return bufs


def _first(mask):
    return mask.nonzero()[0].tolist()


def check_layout(bufs, B, h, w, levels, what):
    """Guards intact, unasked levels untouched, no sentinel inside an asked level, padding +0.0 where blocked_map says.  Returns
    the row-major levels [M, hl, wl] that were asked for."""
    path = pool_path(h, w, levels, B)
    M = B * h * w
    out = []
    for l in range(4):
        buf = bufs[l]
        assert buf.numel() == M * path.slices[l] + GUARD
        assert same_bits(buf[-GUARD:], sentinel(GUARD, buf.device)), f"{what}: level {l}: write past the end of the buffer"
        lv = level_view(buf, M)
        if l >= levels:
            assert bool((bits(lv) == SENT).all()), f"{what}: level {l} was not asked for and was written"
            continue
        left = bits(lv) == SENT
        assert not bool(left.any()), f"{what}: level {l}: sentinel left inside a slice at {_first(left)}"
        hl, wl = path.dims[l]
        pad = (blocked_map(hl, wl) < 0).nonzero().reshape(-1).to(buf.device)
        if pad.numel():
            nz = bits(lv.index_select(1, pad)) != 0
            if bool(nz.any()):
                m, k = _first(nz)
                raise AssertionError(f"{what}: level {l}: padding float {int(pad[k])} of slice {m} is not +0.0")
        out.append(unblock(lv, hl, wl))
    return out


def check_pooled(got, path, levels, what):
    """Levels 1 .. levels - 1 of `got` (row-major, as check_layout returns them) equal expected_pyramid(got[0]) bit for bit."""
    exp = expected_pyramid(got[0], path, levels)
    for l in range(1, levels):
        g, e = got[l], exp[l - 1]
        assert g.shape == e.shape, (what, l, g.shape, e.shape)
        diff = bits(g) != bits(e)
        if bool(diff.any()):
            i = _first(diff)
            raise AssertionError(f"{what}: level {l}: {int(diff.sum())} of {diff.numel()} elements are not the pooled level {l - 1}; "
                                 f"first at {i}: got {float(g[tuple(i)])!r}, want {float(e[tuple(i)])!r}")


def check_pyramid(bufs, B, h, w, levels, what, split=False):
    """check_layout + check_pooled; returns the row-major levels."""
    got = check_layout(bufs, B, h, w, levels, what)
    check_pooled(got, pool_path(h, w, levels, B, split), levels, what)
    return got


def check_level0(out, ref, mag, what, K=None):
    """Level 0 (or rows of it) inside K_VOL of the float64 product; returns the worst ratio."""
    return wc.check(out, ref, mag, K_VOL if K is None else K, what)


def feature_maps(B, h, w, seed, shared=False):
    """fp32 NHWC feature maps with a long-tailed per-channel scale and a DC offset per channel: (f1 [B,h,w,256], f2 [B or 1, ...])."""
    g = torch.Generator().manual_seed(seed)
    chs = torch.exp(torch.randn((1, 1, 1, D), generator=g))
    dc = torch.randn((1, 1, 1, D), generator=g) * 0.5
    f1 = (torch.randn((B, h, w, D), generator=g) + dc) * chs
    f2 = (torch.randn((1 if shared else B, h, w, D), generator=g) + dc) * chs
    return f1.contiguous(), f2.contiguous()
