"""The 4-level correlation pyramid, path by path: block_rows_kernel and the batched volume GEMM with and without the kEpiVolPool
epilogue (conv.hip), pyramid_pool_kernel and pyramid_pool_reg_kernel (corr.hip), and the pooling launcher as corr_split.hip enters
it -- through ofx_corr_volume and ofx_corr_volume_split.

Level 0 is checked against the float64 product of the same fp32 feature maps with the operand-scaled bound of pyramid_check.py;
levels 1 to 3 are checked BIT FOR BIT against the pooling of the level 0 the device stored, in the order each path uses
(pyramid_check.py names it per path and says why no tolerance is involved); padding elements must be +0.0 where the layout puts
them, no sentinel may survive inside a level that was asked for, and every level that was not asked for, every guard float behind a
buffer and both feature maps must come back untouched.  The case lists are fixed; CPU tests assert what they cover with the
launcher's rule restated in pyramid_check.pool_path, that the rule agrees with the launcher's own plan of the fused GEMM, and that
the checker catches the kernel bugs it is meant to catch.
"""
import ctypes as C

import pytest
import torch

import pyramid_check as pc
import wino_check as wc

GUARD = pc.GUARD
BIG_BYTES = 100e6                    # level 0 above this: checked on the device, against float64 on sampled source pixels

# worst ratios seen by this module's GPU tests (read by hand when K_VOL in pyramid_check.py is re-measured)
MEASURED = {}


def _note(kernel, ratio):
    MEASURED[kernel] = max(MEASURED.get(kernel, 0.0), ratio)
    print(f"MEASURED {kernel} {MEASURED[kernel]:.4g}")


# (B, h, w, levels)
UNFUSED_CASES = [
    (2, 8, 8, 4),                    # level 3 is 1x1
    (1, 9, 15, 4),
    (1, 13, 11, 4),
    (2, 9, 29, 4),
    (1, 23, 70, 4),
    (3, 12, 20, 4),
    (1, 8, 24, 4),                   # h % 8 == 0, w % 16 != 0
    (1, 12, 16, 4),                  # w % 16 == 0, h % 8 != 0
    (1, 68, 122, 4),                 # slices above one trip of the LDS kernel's loops: 8704 floats of level 0, 2304 of level 1
    (1, 17, 19, 3),
    (2, 10, 12, 2),
]
FUSED_LDS_CASES = [
    (2, 8, 16, 4),
    (1, 24, 16, 4),
    (2, 16, 48, 4),
    (1, 40, 32, 4),
    (1, 32, 48, 4),
    (1, 8, 128, 4),
    (1, 72, 64, 4),                  # 1152 floats of level 1: two trips of the load from the blocked level 1
    (2, 16, 32, 3),
    (2, 16, 32, 2),                  # the pooling launcher returns at once
]
FUSED_REG_CASES = [
    (2, 32, 64, 4),
    (1, 96, 64, 4),
    (1, 64, 64, 3),
    (1, 32, 128, 4),
    (1, 32, 192, 4),                 # wb1 = 12, wps = 6
    (1, 32, 320, 4),                 # wb1 = 20, wps = 10
    (1, 160, 64, 4),                 # wps = 10
]
STRIDE_CASE = (17, 64, 64, 4)        # 278528 waves: the register kernel's grid-stride loop makes a second trip (1.1 GB of level 0)
VOLUME_CASES = UNFUSED_CASES + FUSED_LDS_CASES + FUSED_REG_CASES
SPLIT_CASES = [(3, 8, 16, 4), (2, 32, 48, 4), (2, 32, 64, 4), (1, 32, 192, 4), (2, 16, 32, 2)]
PLANES = {1: "fp32", 2: "bf16x3", 3: "bf16x6"}


def _id(c):
    return "x".join(map(str, c[:3])) + f"-L{c[3]}"


def _guarded(t):
    """A host copy of t followed by GUARD sentinel floats, and the same on the device: (host flat, device flat, device view)."""
    host = pc.sentinel(t.numel() + GUARD)
    host[:t.numel()] = t.reshape(-1)
    dev = host.cuda()
    return host, dev, dev[:t.numel()].view(t.shape)


def _build(case, f1, f2, planes=0, shared=False):
    """ofx_corr_volume (planes = 0) or ofx_corr_volume_split into sentinel-filled, guarded level buffers on the device.  All four
    level pointers are handed over whatever `levels` says; the feature maps must come back bit for bit."""
    from sd_animation_optical_flow_amd import _lib
    B, h, w, levels = case
    h1, d1, v1 = _guarded(f1)
    h2, d2, v2 = _guarded(f2)
    bufs = pc.level_buffers(B, h, w, "cuda")
    arr = (C.c_void_p * 4)(*[b.data_ptr() for b in bufs])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if planes:
        _lib.check(_lib.lib().ofx_corr_volume_split(C.c_void_p(v1.data_ptr()), C.c_void_p(v2.data_ptr()), arr, B, h, w, pc.D, levels,
                                                    planes, 1 if shared else 0, stream), "ofx_corr_volume_split")
    else:
        _lib.check(_lib.lib().ofx_corr_volume(C.c_void_p(v1.data_ptr()), C.c_void_p(v2.data_ptr()), arr, B, h, w, pc.D, levels, stream),
                   "ofx_corr_volume")
    torch.cuda.synchronize()
    assert pc.same_bits(d1.cpu(), h1) and pc.same_bits(d2.cpu(), h2), f"{case}: a feature map or its guard was written"
    return bufs


def _is_big(case):
    B, h, w, _ = case
    return B * h * w * pc.slice_floats(h, w) * 4 > BIG_BYTES


def _check(case, bufs, what, split=False):
    """The exact checks, on the device for a big case and on the host otherwise; returns the row-major levels."""
    B, h, w, levels = case
    if not _is_big(case):
        bufs = [b.cpu() for b in bufs]
    return pc.check_pyramid(bufs, B, h, w, levels, what, split)


def _check_level0(case, level0, f1, f2, what):
    B, h, w, _ = case
    if _is_big(case):
        rows = pc.sample_rows(B, h, w)
        out = level0[torch.tensor(rows, device=level0.device)].cpu()
        ref, mag = pc.level0_reference_rows(f1, f2, rows)
    else:
        out = level0
        ref, mag = pc.level0_reference(f1, f2)
    _note("vol", pc.check_level0(out, ref, mag, what))


@pytest.mark.gpu
@pytest.mark.parametrize("case", VOLUME_CASES, ids=_id)
def test_corr_volume_pyramid_against_float64_and_its_own_level0(cuda, case):
    B, h, w, levels = case
    f1, f2 = pc.feature_maps(B, h, w, 31)
    bufs = _build(case, f1, f2)
    got = _check(case, bufs, f"volume {case}")
    _check_level0(case, got[0], f1, f2, f"volume {case} level 0")


@pytest.mark.gpu
def test_corr_volume_pyramid_through_the_grid_stride_loop(cuda):
    case = STRIDE_CASE
    B, h, w, levels = case
    assert pc.pool_path(h, w, levels, B).stride and _is_big(case)
    f1, f2 = pc.feature_maps(B, h, w, 32)
    bufs = _build(case, f1, f2)
    got = _check(case, bufs, f"volume {case}")
    _check_level0(case, got[0], f1, f2, f"volume {case} level 0")
    del bufs, got
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["pairs", "shared"])
@pytest.mark.parametrize("case", SPLIT_CASES, ids=_id)
def test_corr_volume_split_pools_its_own_level0(cuda, case, shared):
    """ofx_corr_volume_split in its three arithmetics: the pooling contract, the layout and the guards (the bounds of its level 0 in
    bf16x3 / bf16x6 stay with test_gpu_ops.py); in fp32 every level is ofx_corr_volume's bit for bit."""
    B, h, w, levels = case
    f1, f2 = pc.feature_maps(B, h, w, 33, shared)
    f2e = f2.expand(B, h, w, pc.D).contiguous()
    ref_bufs = _build(case, f1, f2e)
    for planes, name in PLANES.items():
        bufs = _build(case, f1, f2, planes, shared)
        _check(case, bufs, f"split {name} {case} shared={shared}", split=True)
        if planes == 1:
            for l in range(4):
                assert pc.same_bits(bufs[l], ref_bufs[l]), f"split fp32 {case} shared={shared}: level {l} is not ofx_corr_volume's"
        del bufs


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: what the case lists cover, by the launcher's rule

def _paths(cases, split=False):
    return [(c, pc.pool_path(c[1], c[2], c[3], c[0], split)) for c in cases]


def test_pyramid_cases_cover_every_path_level_count_and_residue():
    un, fl, fr = _paths(UNFUSED_CASES), _paths(FUSED_LDS_CASES), _paths(FUSED_REG_CASES)
    st = _paths([STRIDE_CASE])
    # every combination of {fused, unfused} x {register, LDS} that exists (the register kernel needs the fused level 1)
    assert all(not p.fused and not p.register for _, p in un)
    assert all(p.fused and not p.register for _, p in fl)
    assert all(p.fused and p.register and not p.stride for _, p in fr)
    assert all(p.fused and p.register and p.stride for _, p in st) and st[0][1].nwaves > 262144
    for group in (un, fl):
        assert {c[3] for c, _ in group} == {2, 3, 4}
    assert {c[3] for c, _ in fr} == {3, 4}                                  # (two levels never reach a pooling kernel when fused)
    assert all(p.lds_bytes <= 64 * 1024 for _, p in un + fl)
    # fused LDS cases that miss the register kernel on each of its shape conditions
    assert any(p.dims[1][0] % 16 and not p.dims[1][1] % 32 for _, p in fl) and any(p.dims[1][1] % 32 and not p.dims[1][0] % 16 for _, p in fl)
    assert any(c[3] < 3 for c, _ in fl)
    # h % 8 == 0 without w % 16 == 0 and the reverse stay unfused
    assert any(c[1] % 8 == 0 and c[2] % 16 for c, _ in un) and any(c[1] % 8 and c[2] % 16 == 0 for c, _ in un)
    allc = un + fl + fr + st
    levels_of = lambda c, p: [p.dims[l] for l in range(c[3])]
    assert {hl % 4 for c, p in allc for hl, _ in levels_of(c, p)} == {0, 1, 2, 3}
    assert {wl % 8 for c, p in allc for _, wl in levels_of(c, p)} == set(range(8))
    # partial blocks written by store_blocked at every pooled level, and read back from a fused level 1's children
    for l in (1, 2, 3):
        assert any(c[3] > l and (p.dims[l][0] % 4 or p.dims[l][1] % 8) for c, p in un)
    assert any(c[3] > 2 and (p.dims[2][0] % 4 or p.dims[2][1] % 8) for c, p in fl)
    # an odd height and an odd width floored away at each of levels 0, 1, 2
    for l in (0, 1, 2):
        assert any(c[3] > l + 1 and p.dims[l][0] % 2 for c, p in allc), l
        assert any(c[3] > l + 1 and p.dims[l][1] % 2 for c, p in allc), l
    assert any(c[3] == 4 and p.dims[3] == (1, 1) for c, p in allc)
    # more than one image with slices that hold padding
    assert any(c[0] > 1 and p.dims[1][1] % 8 for c, p in un)
    # the LDS kernel's loops beyond one trip of the workgroup: level 0 read (1024 items of 8 floats), store_blocked and the load of a
    # blocked level 1 (256 lanes x 4 floats)
    assert any(p.slices[0] > 8192 for _, p in un) and any(p.slices[1] > 1024 for _, p in un) and any(p.slices[1] > 1024 for _, p in fl)
    # the register kernel's reciprocals: wb1 and wps that are no powers of two, at least four distinct wb1
    pow2 = lambda n: n & (n - 1) == 0
    assert any(not pow2(p.wb1) for _, p in fr) and any(not pow2(p.wps) for _, p in fr)
    assert len({p.wb1 for _, p in fr}) >= 4 and len({p.wps for _, p in fr}) >= 3
    assert {(c[2], p.wb1) for c, p in fr} >= {(192, 12), (320, 20)} and any(p.wps == 10 for _, p in fr)
    # big and small: both ways of checking run
    assert any(_is_big(c) for c in FUSED_REG_CASES) and any(not _is_big(c) for c in FUSED_REG_CASES)
    assert any(_is_big(c) for c in UNFUSED_CASES) and not any(_is_big(c) for c in FUSED_LDS_CASES)


def test_split_cases_cover_both_pooling_kernels_and_the_early_return():
    sp = _paths(SPLIT_CASES, split=True)
    assert all(p.fused for _, p in sp)
    assert any(p.register for _, p in sp) and any(not p.register and c[3] >= 3 for c, p in sp) and any(c[3] == 2 for c, _ in sp)
    assert any(p.register and p.wb1 & (p.wb1 - 1) for _, p in sp)
    assert any(c[0] > 2 for c, _ in sp) and any(c[0] == 1 for c, _ in sp)
    assert set(PLANES) == {1, 2, 3}


def test_blocked_map_is_the_layout_the_library_documents():
    from sd_animation_optical_flow_amd import _lib, ops
    for hl, wl in [(1, 1), (1, 3), (2, 7), (4, 8), (5, 9), (11, 35), (16, 32), (23, 70)]:
        n = pc.slice_floats(hl, wl)
        assert n == _lib.lib().ofx_corr_slice_floats(hl, wl) == ops.corr_slice_floats(hl, wl)
        bm = pc.blocked_map(hl, wl)
        assert bm.numel() == n and int((bm >= 0).sum()) == hl * wl and sorted(bm[bm >= 0].tolist()) == list(range(hl * wl))
        wb = (wl + 7) // 8
        for y, x in ((0, 0), (hl - 1, wl - 1), (hl // 2, wl // 3)):
            assert int(bm[((y // 4) * wb + x // 8) * 32 + (y % 4) * 8 + x % 8]) == y * wl + x
        t = torch.arange(3 * hl * wl, dtype=torch.float32).reshape(3, hl, wl) + 1.0
        blk = pc.block(t)
        assert torch.equal(pc.unblock(blk, hl, wl), t) and torch.equal(ops.corr_unblock(blk, hl, wl), t)
        assert float(blk.sum()) == float(t.sum())


def test_pool_path_agrees_with_the_launchers_plan_of_the_fused_gemm():
    """ofx_conv2d_plan(want_pool = 1) on the descriptor ofx_corr_volume builds: valid, the 128x128 tile, never the patch schedule,
    for every case pool_path calls fused; and the launcher's own validation refuses the epilogue where level 0's slice is not whole
    128-column tiles."""
    from sd_animation_optical_flow_amd import _lib
    PTR = 0x10000

    def plan(B, h, w):
        n, nb = h * w, pc.slice_floats(h, w)
        d = _lib.ConvDesc()
        d.in0, d.ld0, d.c0, d.w = PTR, pc.D, pc.D, PTR
        d.out, d.ldo = PTR, nb
        d.nz, d.a_zs, d.w_zs, d.o_zs = B, n * pc.D, nb * pc.D, n * nb
        d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = 1, h, w, h, w, nb
        d.KH = d.KW = d.stride = 1
        p = _lib.ConvPlan()
        return _lib.lib().ofx_conv2d_plan(C.byref(d), 0, 1, C.byref(p)), p
    for c, path in _paths(FUSED_LDS_CASES + FUSED_REG_CASES + [STRIDE_CASE] + SPLIT_CASES):
        st, p = plan(*c[:3])
        assert path.fused and st == 0, c
        assert (p.path, p.bm, p.bn, p.ksplit) == (0, 128, 128, 1) and p.mode != 2, (c, p.bm, p.bn, p.mode)
        assert p.mtiles == -(-c[1] * c[2] // 128) and p.ntiles * 128 == path.slices[0], c
    for c, path in _paths(UNFUSED_CASES):
        assert not path.fused
        if path.slices[0] % 128:
            assert plan(*c[:3])[0] != 0, c


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the checker passes the restated arithmetic and catches each simulated bug

def _restated(case, seed=7):
    """A pyramid as a correct device would leave it: level 0 the float64 product rounded once to fp32, pooled by the restatement."""
    B, h, w, levels = case
    f1, f2 = pc.feature_maps(B, h, w, seed)
    ref, mag = pc.level0_reference(f1, f2)
    path = pc.pool_path(h, w, levels, B)
    return ref, mag, path, pc.restated_buffers(ref.float(), path, levels)


def _put(bufs, l, rowmajor):
    pc.level_view(bufs[l], rowmajor.shape[0])[:] = pc.block(rowmajor)


PLANT_CASES = [(2, 9, 29, 4), (1, 16, 32, 4)]       # unfused with odd sizes and padding at every level; fused


@pytest.mark.parametrize("case", PLANT_CASES, ids=_id)
def test_pyramid_checker_passes_the_restatement_and_catches_the_other_order(case):
    B, h, w, levels = case
    ref, mag, path, bufs = _restated(case)
    got = pc.check_pyramid(bufs, B, h, w, levels, "restated")
    assert pc.check_level0(got[0], ref, mag, "restated level 0") <= 1.0 < pc.K_VOL      # one rounding: half an ulp of |ref| <= M
    assert pc.same_bits(got[0], ref.float())
    for l in (1, 2, 3):
        right = pc.pool_pair if (l == 1 and path.fused) else pc.pool_seq
        wrong = pc.pool_seq if right is pc.pool_pair else pc.pool_pair
        assert pc.same_bits(got[l], right(got[l - 1])) and not pc.same_bits(got[l], wrong(got[l - 1]))
        bad = [b.clone() for b in bufs]
        _put(bad, l, wrong(got[l - 1]))
        with pytest.raises(AssertionError, match=f"level {l}: .* not the pooled level {l - 1}"):
            pc.check_pyramid(bad, B, h, w, levels, "other order")
    # a float64 bound over the pooled levels would have let the other order through: it is inside a few ulps
    assert (pc.pool_seq(got[0]).double() - pc.pool_pair(got[0]).double()).abs().max() < 1e-5 * float(got[0].abs().max())


def test_pyramid_checker_catches_simulated_kernel_bugs():
    case = PLANT_CASES[0]
    B, h, w, levels = case
    M = B * h * w
    ref, mag, path, bufs = _restated(case)
    got = pc.check_pyramid(bufs, B, h, w, levels, "restated")
    dims = path.dims
    assert dims[0][0] % 2 and dims[0][1] % 2 and (dims[1][1] + 7) // 8 >= 2

    def fails(bad, pattern):
        with pytest.raises(AssertionError, match=pattern):
            pc.check_pyramid(bad, B, h, w, levels, "planted")

    def with_level(l, rowmajor):
        bad = [b.clone() for b in bufs]
        _put(bad, l, rowmajor)
        return bad
    # level 3 averaged straight from sixteen level-1 values
    h3, w3 = dims[3]
    l3 = got[1][:, :4 * h3, :4 * w3].reshape(M, h3, 4, w3, 4).sum((2, 4)) * 0.0625
    assert not pc.same_bits(l3, got[3]) and (l3 - got[3]).abs().max() < 1e-5 * float(got[1].abs().max())
    fails(with_level(3, l3), "level 3: .* not the pooled level 2")
    # a pooled value taken from the block to the right
    l1 = got[1].clone()
    l1[:, 1, 2] = got[1][:, 1, 10]
    fails(with_level(1, l1), "level 1: .* not the pooled level 0")
    # the floored-away last row pooled in: the last level-1 row from rows h - 2, h - 1 instead of h - 3, h - 2
    l1 = got[1].clone()
    l1[:, -1:, :] = pc.pool_seq(got[0][:, h - 2:h, :])
    fails(with_level(1, l1), "level 1: .* not the pooled level 0")
    # ... and the floored-away last column
    l1 = got[1].clone()
    l1[:, :, -1:] = pc.pool_seq(got[0][:, :, w - 2:w])
    fails(with_level(1, l1), "level 1: .* not the pooled level 0")
    # one nonzero padding float (a stray value, and a negative zero), at each level that has padding
    for l in range(4):
        pad = (pc.blocked_map(*dims[l]) < 0).nonzero().reshape(-1)
        assert pad.numel()
        for v in (1e-30, -0.0):
            bad = [b.clone() for b in bufs]
            pc.level_view(bad[l], M)[M // 2, int(pad[len(pad) // 2])] = v
            fails(bad, f"level {l}: padding float {int(pad[len(pad) // 2])} of slice {M // 2} is not")
    # one sentinel left inside a slice; one guard float overwritten; a level that was not asked for written
    for l in range(4):
        bad = [b.clone() for b in bufs]
        pc.level_view(bad[l], M)[M - 1, 5] = pc.sentinel(1)[0]
        fails(bad, f"level {l}: sentinel left inside a slice")
        bad = [b.clone() for b in bufs]
        bad[l][-GUARD] = 0.0
        fails(bad, f"level {l}: write past the end")
    three = pc.restated_buffers(got[0], pc.pool_path(h, w, 3, B), 3)
    pc.check_pyramid(three, B, h, w, 3, "three levels")
    with pytest.raises(AssertionError, match="level 3 was not asked for"):
        pc.check_pyramid(bufs, B, h, w, 3, "three levels")
    # level 0 off by 3 K_VOL ulps of M in one element; a dropped channel; the 1/16 scale applied twice
    out = got[0].clone().double()
    out[M // 3, 2, 3] += 3 * pc.K_VOL * pc.EPS * mag[M // 3, 2, 3]
    with pytest.raises(AssertionError, match="1 of"):
        pc.check_level0(out, ref, mag, "planted")
    assert bool(wc.violations(ref / 16.0, ref, mag, pc.K_VOL).any())
    f1, f2 = pc.feature_maps(B, h, w, 7)
    f1[..., 255] = 0
    assert bool(wc.violations(pc.level0_reference(f1, f2)[0], ref, mag, pc.K_VOL).any())
    # the sampled rows are the full reference's rows
    rows = pc.sample_rows(B, h, w)
    f1, f2 = pc.feature_maps(B, h, w, 7)
    r_ref, r_mag = pc.level0_reference_rows(f1, f2, rows)
    assert torch.allclose(r_ref, ref[rows], rtol=1e-13, atol=1e-13) and torch.allclose(r_mag, mag[rows], rtol=1e-13, atol=1e-13)
    assert {0, h * w - 1, h * w, M - 1} <= set(rows)
