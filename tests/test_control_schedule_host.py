"""No device: `controlnet.ControlSchedule` over nets with cached results (plain torch mixing, CPU tensors here), and the host-side
refusals of `sampler.img2img` and `controlnet.canny_condition` that come before anything touches a device."""
import numpy as np
import pytest
import torch


def _nets(end=0.5):
    from sd_animation_optical_flow_amd.controlnet import SingleControlNet
    g = torch.Generator().manual_seed(5)
    a = [torch.randn((2, 3, 4, 5), generator=g) for _ in range(3)]
    b = [torch.randn((2, 3, 4, 5), generator=g) for _ in range(3)]
    return [SingleControlNet(1.0, "canny", {}, None, result=a), SingleControlNet(0.75, "hed", {}, None, guidance_end=end, result=b)], a, b


def test_schedule_mixes_once_per_weight_tuple():
    from sd_animation_optical_flow_amd.controlnet import ControlSchedule, apply_multi_controlnet
    nets, a, b = _nets()
    cs = ControlSchedule(nets)
    v1 = cs(0, 0.25)
    assert cs(1, 0.5) is v1 and cs.mixes == 1                     # both ends of a window are inclusive
    want = apply_multi_controlnet(None, None, None, 0.25, nets)
    assert all(torch.equal(x, y) for x, y in zip(v1, want))
    assert all(torch.allclose(x, ra + 0.75 * rb, rtol=0.0, atol=1e-6) for x, ra, rb in zip(v1, a, b))     # add_(alpha=) may fuse
    v2 = cs(2, 0.75)
    assert v2 is not v1 and cs(3, 1.0) is v2 and cs.mixes == 2
    assert all(torch.equal(x, ra) for x, ra in zip(v2, a)) and all(x is not ra for x, ra in zip(v2, a))     # fresh tensors, not the cache
    assert cs(0, 0.25) is not v1 and cs.mixes == 3                # a window that reopens is a new tuple: one more mix


def test_schedule_is_none_when_every_window_is_shut():
    from sd_animation_optical_flow_amd.controlnet import ControlSchedule
    nets, _, _ = _nets()
    nets[0].guidance_start, nets[1].guidance_start = 0.3, 0.3
    cs = ControlSchedule(nets)
    assert cs(0, 0.25) is None and cs.mixes == 0
    assert cs(1, 0.5) is not None and cs.mixes == 1


def test_schedule_refuses_nets_without_results():
    from sd_animation_optical_flow_amd.controlnet import ControlSchedule, SingleControlNet
    with pytest.raises(ValueError):
        ControlSchedule([])
    nets, _, _ = _nets()
    with pytest.raises(ValueError):
        ControlSchedule(nets + [SingleControlNet(1.0, "canny", {}, np.zeros((8, 8), np.uint8))])


def test_img2img_and_canny_condition_refuse_on_the_host():
    from sd_animation_optical_flow_amd import sampler as S
    from sd_animation_optical_flow_amd.controlnet import canny_condition

    class FakeUNet:
        in_channels, device = 9, "cpu"

    img = np.zeros((64, 96, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="t_enc = 0"):
        S.img2img(FakeUNet(), None, None, img, None, None, denoising_strength=0.05, ddim_steps=10)
    with pytest.raises(ValueError, match="in_channels must be 4"):
        S.img2img(FakeUNet(), None, None, img, None, None, denoising_strength=0.4, ddim_steps=10)
    with pytest.raises(ValueError):
        canny_condition(img.astype(np.float32), 100, 200)
    with pytest.raises(ValueError):
        canny_condition(np.zeros((2, 8, 8, 3), dtype=np.uint8), 100, 200)
