"""The output stage's kernels against float64, case table by case table (tests/warp_check.py holds the restatements, the bounds and
the tables; tests/test_warp_check_host.py shows on the CPU that these checkers catch planted bugs).  Every test prints the worst
|error| / bound it saw and the exempt values against their cap: run with -s to re-measure."""
import numpy as np
import pytest
import torch

import warp_check as wc
from oracle import mask_oracle as MO

pytestmark = pytest.mark.gpu


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_warp(c, frame, flow):
    return _ops().warp(dev(frame), dev(flow), mode=c.mode, sign=c.sign).cpu().numpy()


def check_table(cases, agree=False):
    """Every case through ops.warp and the float64 checker; agree: the C = 3 kernels of warp_mask.hip against its generic kernel run on
    the frame with a fourth channel appended, byte for byte.  Returns (worst ratio, exempt values, their caps)."""
    worst, exempt, caps = 0.0, 0, 0
    for c in cases:
        assert wc.route(c.H, c.W, c.B, c.C, c.per_frame, c.dtype, c.mode) == c.route, c.name
        frame, flow = wc.make_inputs(c)
        out = run_warp(c, frame, flow)
        ratio, n, cap = wc.check_warp(out, frame, flow, c.sign, c.mode, c.name)
        worst, exempt, caps = max(worst, ratio or 0.0), exempt + n, caps + cap
        if agree and c.C == 3 and c.route in ("x4", "u8c3"):
            f4 = np.concatenate([frame, frame[..., :1]], -1)
            assert wc.route(c.H, c.W, c.B, 4, c.per_frame) == "generic"
            wc.same_bytes(out, run_warp(c, f4, flow)[..., :3], c.name + ": fast kernel against the generic one")
    return worst, exempt, caps


@pytest.mark.parametrize("route", ["generic", "x4", "u8c3", "shared"])
def test_uint8_bilinear_tie_rule_route_by_route(cuda, route):
    _, exempt, caps = check_table(wc.ROUTE_TABLES[route], agree=True)
    print(f"\nuint8 bilinear, {route}: {exempt} exempt bytes, caps add up to {caps}")


def test_uint8_bilinear_per_frame_key_frames(cuda):
    _, exempt, caps = check_table(wc.PER_FRAME_U8, agree=True)
    print(f"\nuint8 bilinear, a frame per item: {exempt} exempt bytes, caps add up to {caps}")


def test_uint8_bicubic_tie_rule(cuda):
    _, exempt, caps = check_table(wc.BICUBIC_U8)
    print(f"\nuint8 bicubic: {exempt} exempt bytes, caps add up to {caps}")


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_float_warp_against_float64(cuda, mode):
    worst, _, _ = check_table(wc.FLOAT_CASES[mode])
    print(f"\nfloat32 {mode}: worst |error| / bound {worst:.3f} over {len(wc.FLOAT_CASES[mode])} cases")


def test_cv2_cubic_stays_bit_exact(cuda):
    for c in wc.CV2_CASES:
        frame, flow = wc.make_inputs(c)
        wc.same_bytes(run_warp(c, frame, flow), wc.oracle_warp(frame, flow, c.sign, "cv2_cubic"), c.name)


def test_warp_kernel_takes_its_second_grid_stride_trip(cuda):
    c = wc.STRIDE_WARP
    assert c.B * c.H * c.W > 256 * 8192
    frame, flow = wc.make_inputs(c)
    ratio, _, _ = wc.check_warp(run_warp(c, frame, flow), frame, flow, c.sign, c.mode, c.name)
    print(f"\nwarp_kernel<float, 1, bilinear> over {c.B * c.H * c.W} pixels: worst |error| / bound {ratio:.3f}")


def test_resize_cubic_against_float64(cuda):
    ops, worst = _ops(), 0.0
    for c in wc.RESIZE_CASES + [wc.STRIDE_RESIZE]:
        img = wc.resize_inputs(c)
        out = ops.resize_cubic(dev(img), c.Hd, c.Wd).cpu().numpy()
        r, bound = wc.resize_reference(img, c.Hd, c.Wd)
        worst = max(worst, wc.check_float(out, r, bound, c.name))
        if (c.Hs, c.Ws) == (c.Hd, c.Wd):
            wc.same_bytes(out, img, c.name + ": t = 0 copies the input")
    c = wc.STRIDE_RESIZE
    assert c.B * c.Hd * c.Wd * c.C > 256 * 8192
    print(f"\nresize_cubic: worst |error| / bound {worst:.3f}")


def test_fb_confidence_against_float64(cuda):
    ops, worst = _ops(), [0.0, 0.0]
    for c in wc.FB_CASES:
        fw, bw, planted = wc.fb_inputs(c)
        conf, logc = ops.fb_confidence(dev(fw), dev(bw), c.sigma)
        conf, logc = conf.cpu().numpy(), logc.cpu().numpy()
        rc, rl = wc.check_fb(conf, logc, wc.fb_reference(fw, bw, c.sigma), c.name)
        worst = [max(worst[0], rc), max(worst[1], rl)]
        assert conf[planted["zero"]] == 1.0 and logc[planted["zero"]] == 0, c.name
        for k in ("1e6", "1e30"):
            assert conf[planted[k]] == 0 and logc[planted[k]] < -1e9, (c.name, k)
    print(f"\nfb_confidence: worst |error| / bound: conf {worst[0]:.3f}, logc {worst[1]:.3f}")


def test_travel_mask_batched(cuda):
    ops = _ops()
    for c in wc.TRAVEL_CASES:
        conf, flow, dist, travel = wc.travel_inputs(c)
        raw, tout = ops.travel_mask(dev(conf), dev(flow), dev(dist), dev(travel), c.thres, c.mode)
        raw, tout = raw.cpu().numpy(), tout.cpu().numpy()
        if c.mode == "cv2_cubic":
            want_raw, want_t = wc.travel_oracle(conf, flow, dist, travel, c.thres, c.mode)
            wc.same_bytes(raw, want_raw, c.name + " raw")
            wc.same_bytes(tout, want_t, c.name + " travel")
            dil = ops.dilate(dev(raw), 15).cpu().numpy()
            for b in range(c.B):                                # the oracle's own function, dilation included
                m, t = MO.confidence_to_mask(conf[b], flow[b], dist[b], travel[b], c.thres, c.mode)
                wc.same_bytes(tout[b], t, f"{c.name} travel of item {b}")
                wc.same_bytes(dil[b], m, f"{c.name} mask of item {b}")
        else:
            ratio, n, cap = wc.check_travel(raw, tout, wc.travel_reference(conf, flow, dist, travel, c.thres, c.mode), c.name)
            print(f"\ntravel_mask {c.name}: worst |error| / bound {ratio:.3f}, {n} exempt pixels (cap {cap})")


@pytest.mark.parametrize("H,W,B", wc.DILATE_CASES)
def test_dilate_batched(cuda, H, W, B):
    ops = _ops()
    m = wc.dilate_inputs(H, W, B)
    assert all(m[b].any() for b in range(B)) and not np.array_equal(m[0], m[1])
    for k in wc.DILATE_KSIZES:
        out = ops.dilate(dev(m), k).cpu().numpy()
        kern = MO.ellipse_kernel(k)
        wc.same_bytes(out, np.stack([MO.dilate(m[b], kern) for b in range(B)]), f"dilate {H}x{W} k{k}")
