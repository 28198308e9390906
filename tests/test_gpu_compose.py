"""-m gpu: `ops.compose_refs` (`ofx_compose_refs`, two launches) against the reference's round loop through the oracle, the float64
warp of the selected reference for the float modes, and the two device wrappers built on it against the host-side functions
they replace.  The restatement, the cases and their seeds are tests/compose_check.py's; tests/test_compose_host.py holds the
restatement against the oracle on the CPU."""
import numpy as np
import pytest
import torch

import compose_check as CC
import warp_check as WC

pytestmark = pytest.mark.gpu


def _run(c, mode, first_only=False):
    from sd_animation_optical_flow_amd import ops
    flow, conf, frames = CC.make_inputs(c)
    dev = lambda a: torch.from_numpy(a).cuda()
    out = ops.compose_refs(dev(flow), dev(conf), dev(frames), c.thres, mode, first_only)
    assert all(t.is_cuda for t in out)
    ret, mask, select, order, counts = (t.cpu().numpy() for t in out)
    assert ret.shape == (c.H, c.W, 3) and mask.shape == select.shape == (c.H, c.W) and order.shape == counts.shape == (c.N,)
    assert order.dtype == counts.dtype == np.int32
    return (flow, conf, frames), (ret, mask, select, order, counts)


def _exact_part(c, got, want):
    _, mask, select, order, counts = got
    assert order.tolist() == want["order"], c.name
    assert counts.tolist() == want["counts"], c.name
    WC.same_bytes(mask, want["mask"], f"{c.name} mask")
    WC.same_bytes(select, want["select"], f"{c.name} select")


@pytest.mark.parametrize("c", CC.GPU_CASES, ids=lambda c: c.name)
def test_cv2_cubic_is_bit_identical_to_the_reference_loop(cuda, c):
    (flow, conf, frames), got = _run(c, "cv2_cubic")
    want = CC.histogram_compose(conf, c.thres)
    _exact_part(c, got, want)
    ret, mask, order = CC.oracle_compose(flow, conf, frames, c.thres)                       # the reference's N rounds
    assert got[3].tolist() == order
    WC.same_bytes(got[0], ret, f"{c.name} ret")
    WC.same_bytes(got[1], mask, f"{c.name} mask vs the loop")
    # first_only: the first draw's warp, whole (generate_ai_frame_with_ref_both); the mask still covers every reference
    _, first = _run(c, "cv2_cubic", first_only=True)
    want1 = CC.histogram_compose(conf, c.thres, first_only=True)
    _exact_part(c, first, want1)
    assert (first[2] == order[0]).all()
    WC.same_bytes(first[0], WC.oracle_warp(frames[order[0]], flow[order[0]][None], 1.0, "cv2_cubic")[0], f"{c.name} first_only ret")


@pytest.mark.parametrize("first_only", [False, True], ids=["greedy", "first_only"])
@pytest.mark.parametrize("mode,c", CC.FLOAT_PARAMS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_float_modes_sample_the_selected_reference(cuda, mode, c, first_only):
    (flow, conf, frames), got = _run(c, mode, first_only)
    want = CC.histogram_compose(conf, c.thres, first_only)
    _exact_part(c, got, want)
    r, bound, exact = CC.float64_selected(flow, frames, want["select"], mode)
    n, cap = WC.check_u8(got[0][None], r, bound, exact, f"{c.name} {mode} ret")
    assert n <= cap


def test_counts_equal_the_conf_sum_route(cuda):
    """The integer histogram counts against the existing route: f64 `ops.conf_sum` of the binarised planes, round by round."""
    from sd_animation_optical_flow_amd import ops
    c = CC.GPU_CASES[3]
    (_, conf, _), got = _run(c, "cv2_cubic")
    planes = (torch.from_numpy(conf).cuda() > c.thres).float()
    for r in range(c.N):
        sums = ops.conf_sum(planes[..., None].contiguous(), 0)
        s = int(torch.argmax(sums))
        assert s == int(got[3][r]) and float(sums[s]) == float(got[4][r])
        planes = (planes - planes[s][None]).clamp_(0, 1)


def test_compose_warp_and_mask_device_equals_the_host_function(cuda):
    """The case of test_gpu_surface.test_compose_greedy_multi_reference, through both."""
    from sd_animation_optical_flow_amd import ofgen
    rng = np.random.default_rng(7)
    H, W, N = 48, 40, 3
    fm = np.zeros((N, 1, H, W, 3), np.float32)
    fm[..., 0:2] = rng.standard_normal((N, 1, H, W, 2)) * 2
    fm[..., 2] = rng.random((N, 1, H, W))
    fm[1, 0, 10:30, 5:35, 2] = 0.99
    ai = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
    orig = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    flow, conf = np.ascontiguousarray(fm[:, 0, :, :, 0:2]), np.ascontiguousarray(fm[:, 0, :, :, 2])
    for expand in (True, False):
        frame, mask2, order = ofgen.compose_warp_and_mask(fm.copy(), ai, orig, thres=0.6, expand=expand)
        got = ofgen.compose_warp_and_mask_device(flow, conf, ai, orig, thres=0.6, expand=expand)                    # arrays
        dev = ofgen.compose_warp_and_mask_device(torch.from_numpy(flow).cuda(), torch.from_numpy(conf).cuda(),
                                                 torch.from_numpy(np.stack(ai)).cuda(), torch.from_numpy(orig).cuda(), thres=0.6, expand=expand)
        for ret_d, mask_d, order_d in (got, dev):
            assert ret_d.is_cuda and mask_d.is_cuda and order_d.is_cuda and order_d.dtype == torch.int32
            assert order_d.tolist() == order
            WC.same_bytes(ret_d.cpu().numpy(), frame, "ret_frame")
            WC.same_bytes(mask_d.cpu().numpy(), mask2, "mask2")
    first = ofgen.compose_warp_and_mask_device(flow, conf, ai, orig, thres=0.6, expand=False, first_only=True)
    WC.same_bytes(first[0].cpu().numpy(), ofgen._pd.warp_frame(ai[order[0]], flow[order[0]]), "first_only ret")
    WC.same_bytes(first[1].cpu().numpy(), mask2, "first_only mask2")


class _Video:
    def __init__(self, frames):
        self.frames = frames
        self.size_hw = frames[0].shape[:2]

    def get_raw_frame(self, i):
        return self.frames[i]


class _Idx:
    def __init__(self, idx):
        self.indices = list(idx)

    def __len__(self):
        return len(self.indices)


def _frames64(n):
    g = torch.Generator().manual_seed(21)
    base = torch.nn.functional.avg_pool2d(torch.rand((1, 3, 80, 80), generator=g), 5, 1, 2)
    base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)
    return [base[0, :, 8 + 2 * i:72 + 2 * i, 8 - i:72 - i].permute(1, 2, 0).contiguous().numpy() for i in range(n)]


def test_multiple_to_one_device_equals_calculate_multiple_to_one(cuda, raft_sd, tmp_path):
    import os

    from sd_animation_optical_flow_amd import ofgen, pdcnet_of
    algo = pdcnet_of.create_of_algo(raft_sd)
    video = _Video(_frames64(3))
    host = ofgen.PDCNetAux(algo, str(tmp_path / "host"), batch_size=2)
    mat = host.calculate_multiple_to_one(video, _Idx([0, 2, 1]), 1)                          # [3,1,64,64,3], index 2 the identity pair
    aux = ofgen.PDCNetAux(algo, str(tmp_path / "dev"), batch_size=2)
    flow, conf = aux.multiple_to_one_device(video, _Idx([0, 2, 1]), 1)
    assert flow.is_cuda and conf.is_cuda and tuple(flow.shape) == (3, 64, 64, 2) and tuple(conf.shape) == (3, 64, 64)
    WC.same_bytes(flow.cpu().numpy(), np.ascontiguousarray(mat[:, 0, :, :, 0:2]), "flow")
    WC.same_bytes(conf.cpu().numpy(), np.ascontiguousarray(mat[:, 0, :, :, 2]), "conf")
    assert float(flow[2].abs().max()) == 0.0 and float(conf[2].min()) == 1.0                 # identity pair
    # fresh pairs were saved as calculate_given_pairs saves them
    assert sorted(os.listdir(tmp_path / "dev" / "pdcnet")) == ["00000-00001.npy", "00002-00001.npy"] and aux.cached_pair == {(0, 1), (2, 1)}
    WC.same_bytes(np.load(tmp_path / "dev" / "pdcnet" / "00002-00001.npy"), mat[1, 0], "cached pair")
    # a second call uploads from the cache: a new instance without a model proves it
    aux2 = ofgen.PDCNetAux(algo, str(tmp_path / "dev"), batch_size=2)
    aux2.pair_fields = None
    flow2, conf2 = aux2.multiple_to_one_device(video, [0, 2, 1], 1)
    assert torch.equal(flow2, flow) and torch.equal(conf2, conf)
