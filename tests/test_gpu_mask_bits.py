"""The bit-plane mask kernels (mask_bits.hip) on the device, bit for bit against oracle/mask_oracle.py, on every route of the
launcher and with masks that stay unsaturated: tests/mask_check.py holds the cases, the inputs and what they prove
(tests/test_mask_check_host.py proves it on the CPU).  Every case asserts the route the library's own plan reports for the
pointers it passes."""
import numpy as np
import pytest
import torch

import mask_check as mc

pytestmark = pytest.mark.gpu

CONF_PAIRS = [(c, k) for c in mc.CONF_CASES for k in c.ksizes]
EDGE_PAIRS = [(c, k) for c in mc.EDGE_CASES for k in c.ksizes]


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def _on_device(a, offset, dev):
    """A contiguous device copy of `a` that starts `offset` elements after an aligned allocation."""
    flat = torch.zeros(a.size + 16, dtype=torch.from_numpy(a[:0]).dtype, device=dev)
    assert flat.data_ptr() % 16 == 0
    t = flat[offset:offset + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() == flat.data_ptr() + offset * a.itemsize
    return t


def _aligned16(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


@pytest.mark.parametrize("c,ksize", CONF_PAIRS, ids=[f"{c.name}-k{k}" for c, k in CONF_PAIRS])
def test_generate_mask_on_every_route(cuda, c, ksize):
    ops = _ops()
    inp = mc.conf_inputs(c, ksize)
    imgs = mc.compared(c, ksize)
    conf = _on_device(inp.conf, c.offset, cuda)
    assert _aligned16(conf) == mc.aligned(c)
    for src in (mc.SRC_LT, mc.SRC_NGT):
        st, p = mc.plan(src, c.B, c.H, c.W, ksize, _aligned16(conf))
        mode = None if p.kernel != "rows" else ("direct" if p.nplanes < 0 else "planes")
        assert st == 0 and (p.kernel, p.band, mode, p.xcd) == mc.expected_route(c, ksize), (c.name, ksize, p)
        bits = mc.conf_bits(inp.conf, src)
        want = mc.oracle_dilate(bits, ksize, imgs)
        zeros = float((want == 0).mean())
        print(f"{c.name} k{ksize} src{src}: {p}, {len(imgs)} images compared, {zeros:.2f} of the mask is 0")
        assert 0.05 <= zeros <= 0.95
        lc = _on_device(inp.logc, c.offset, cuda)
        out = ops.generate_mask(conf, lc, float(mc.THRES), ksize, cmp_gt=src == mc.SRC_NGT)
        out_nolog = ops.generate_mask(conf, None, float(mc.THRES), ksize, cmp_gt=src == mc.SRC_NGT)
        what = f"{c.name} k{ksize} src{src}"
        mc.first_difference(out[imgs].cpu().numpy(), want, what + " mask")
        mc.first_difference(out_nolog[imgs].cpu().numpy(), want, what + " mask, no log_conf")
        # the reset over the whole batch: zero on the low pixels, untouched elsewhere
        mc.first_difference(lc.cpu().numpy().view(np.uint32), mc.oracle_reset(inp.logc, bits).view(np.uint32), what + " log_conf")
        assert np.array_equal(conf.cpu().numpy(), inp.conf)
        # every image's bytes are 0 or 255 and its stamp came out (the images the oracle was not run on)
        rest = out.cpu().numpy()
        assert np.isin(rest, (0, 255)).all()
        for b, y, x, _ in inp.stamps:
            win, el = mc.stamp_window(rest[b], y, x, ksize)
            empty = src == mc.SRC_LT and (b, y, x) == inp.at_thres
            assert np.array_equal(win, np.zeros_like(el) if empty else el), (what, "stamp", b, y, x)


@pytest.mark.parametrize("c,ksize", EDGE_PAIRS, ids=[f"{c.name}-k{k}" for c, k in EDGE_PAIRS])
def test_expand_mask_on_both_tile_kernels(cuda, c, ksize):
    ops = _ops()
    inp = mc.edge_inputs(c, ksize)
    st, p = mc.plan(mc.SRC_EDGES, c.B, c.H, c.W, ksize, False)
    assert st == 0 and (p.kernel, p.band, None, p.xcd) == mc.expected_route(c, ksize), (c.name, ksize, p)
    mask = _on_device(inp.mask, c.offset, cuda)
    assert (mask.data_ptr() % 8 == 0) == (c.offset == 0)
    image = torch.from_numpy(inp.image).to(cuda)
    want = inp.mask | mc.oracle_dilate(mc.edge_bits(inp.image, mc.EDGE_THRES), ksize)
    zeros = float((want == 0).mean())
    print(f"{c.name} k{ksize}: {p}, {zeros:.2f} of the output is 0")
    assert 0.05 <= zeros <= 0.95
    out = ops.expand_mask(mask, image, mc.EDGE_THRES, ksize)
    mc.first_difference(out.cpu().numpy(), want, f"{c.name} k{ksize}")
    assert np.array_equal(mask.cpu().numpy(), inp.mask)
    # rows that start on an 8-byte boundary take the 8-byte store and those that do not the byte tail: both occur
    starts = {(mask.data_ptr() + (b * c.H + y) * c.W) % 8 for b in range(c.B) for y in range(c.H)}
    if c.W >= 16 and c.W % 8:
        assert 0 in starts and len(starts) > 1
