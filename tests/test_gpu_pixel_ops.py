"""The small per-pixel kernels of warp_mask.hip at batched, ragged shapes: flow_magnitude, travel_distance, merge_images, mix_frames
and conf_sum, each against numpy / oracle/mask_oracle.py.  Everything but conf_sum is bit for bit."""
import numpy as np
import pytest
import torch

from oracle import mask_oracle as MO

pytestmark = pytest.mark.gpu

B, H, W = 3, 37, 53                                             # ragged: no multiple of a wavefront, a workgroup or a vector


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = g != w
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at {i}: got {got[i]!r}, want {want[i]!r}")


def test_flow_magnitude_is_numpys_bits(cuda):
    ops = _ops()
    rng = np.random.default_rng(51)
    flow = (rng.standard_normal((B, H, W, 2)) * 6).astype(np.float32)
    tiny = np.float32(2.0 ** -149)
    planted = [(0.0, 0.0), (-0.0, 0.0), (3.0, 4.0), (tiny, 0.0), (tiny, tiny), (1e-30, 2e-30), (1e-20, -1e-20), (2.0 ** -126, 2.0 ** -127),
               (1e-19, 1e-19), (1.5e19, 1.0e19), (1.8e19, 1.8e19), (3e38, 0.0), (1e30, -1e30), (-1e25, 1e-25), (np.inf, 1.0), (1e-3, 1e3)]
    flat = flow.reshape(-1, 2)
    for i, v in enumerate(planted):
        flat[17 * i + 5] = v
    with np.errstate(over="ignore", under="ignore"):
        fx, fy = flow[..., 0], flow[..., 1]
        want = np.sqrt(fx * fx + fy * fy)
    assert want.dtype == np.float32 and np.isinf(want).sum() >= 3 and (want == 0).sum() >= 3
    with np.errstate(over="ignore", under="ignore"):
        ss = fx * fx + fy * fy
    assert ((ss > 0) & (ss < np.float32(2.0 ** -126))).any()   # a denormal sum of squares: flushed to zero it would give 0
    got = ops.flow_magnitude(torch.from_numpy(flow).to(cuda)).cpu().numpy()
    _same(got, want, "flow_magnitude")
    one = ops.flow_magnitude(torch.from_numpy(flow[0, 0, :1]).to(cuda)).cpu().numpy()       # a single pixel
    _same(one, want[0, 0, :1], "flow_magnitude, one pixel")


def test_travel_distance_batched(cuda):
    ops = _ops()
    rng = np.random.default_rng(52)
    flow = (rng.standard_normal((B, H, W, 2)) * 5).astype(np.float32)
    flow[1, 3, 4] = (0.0, 0.0)
    flow[2, 0, 0] = (1e6, -1e6)
    conf = (0.8 + 0.2 * rng.random((B, H, W))).astype(np.float32)
    conf[:, 2::7, 1::5] = np.float32(0.9)                       # exactly the floor: `<` must not fire
    want = np.stack([MO.travel_distance(flow[b], conf[b]) for b in range(B)])
    assert (want == 0).mean() > 0.2 and (want[conf == np.float32(0.9)] > 0).all()
    got = ops.travel_distance(torch.from_numpy(flow).to(cuda), torch.from_numpy(conf).to(cuda)).cpu().numpy()
    _same(got, want, "travel_distance")


@pytest.mark.parametrize("C", [1, 3, 4])
def test_merge_and_mix_batched(cuda, C):
    ops = _ops()
    rng = np.random.default_rng(53 + C)
    a = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    b = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
    a[0, 0, :8], b[0, 0, :8] = 255, 0                           # the ends of the byte range under every weight
    a[0, 1, :8], b[0, 1, :8] = 0, 255
    mk = rng.choice(np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8), (B, H, W))
    assert not np.array_equal(mk[0], mk[1]) and not np.array_equal(a[1], a[2])
    t = lambda x: torch.from_numpy(x).to(cuda)
    want = np.stack([MO.merge_images(a[i], b[i], mk[i]) for i in range(B)])
    assert (want == a).all(-1).any() and (want == b).all(-1).any()
    _same(ops.merge_images(t(a), t(b), t(mk)).cpu().numpy(), want, f"merge_images C={C}")
    for ppw in (0.0, 0.0005, 0.3, 1.0):
        want = np.stack([MO.mix_propagated_ai_frame(a[i], b[i], mk[i], ppw) for i in range(B)])
        if ppw < 0.001:
            assert np.array_equal(want, a)                      # the reference returns the raw frame
        _same(ops.mix_frames(t(a), t(b), t(mk), ppw).cpu().numpy(), want, f"mix_frames C={C} ppw={ppw}")


@pytest.mark.parametrize("chan", [0, 2])
def test_conf_sum_over_more_than_one_slice(cuda, chan):
    """H * W = 4690 > 4096: two slices per image add into one double.  The sum of n float32 values in float64, in any order, is
    within n * 2^-53 * sum|x| of the exact one (each of the n - 1 additions rounds once, to first order); the reference here is
    an extended-precision sum rounded to double once (2^-53 |sum| more)."""
    ops = _ops()
    N, h, w, nchan = 3, 70, 67, 3
    assert h * w > 4096
    rng = np.random.default_rng(54)
    x = (rng.standard_normal((N, h, w, nchan)) * 100).astype(np.float32)
    x[1, :, :, chan] = np.abs(x[1, :, :, chan])
    got = ops.conf_sum(torch.from_numpy(x).to(cuda), chan).cpu().numpy()
    sel = x[..., chan].astype(np.float64).reshape(N, -1)
    want = np.array([float(np.sum(sel[n].astype(np.longdouble))) for n in range(N)])
    bound = h * w * 2.0 ** -53 * np.abs(sel).sum(1) + 2.0 ** -53 * np.abs(want)
    assert got.dtype == np.float64 and (np.abs(got - want) <= bound).all(), (got, want, bound)
    others = [float(x[..., k].astype(np.float64).sum()) for k in range(nchan) if k != chan]
    assert all(abs(got.sum() - o) > 1.0 for o in others)        # another channel's sum is far away
