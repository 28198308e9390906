"""-m gpu: `VaeDecoder(precision="fp16")` and `VaeEncoder(precision="fp16")` against float64, held to the reference's own arithmetic for
this stage: its `Decoder` / `Encoder` under torch.autocast, measured on the CPU by tests/golden/make_golden_vae_autocast.py.

    bar     distance to float64 <= 2 x autocast_vs_f64: the device performs a subset of autocast's roundings (the operands of the
            convolutions only; GroupNorm, SiLU, attention, every activation and every result stay fp32), the bar of
            tests/test_gpu_unet_precision.py.  The golden asserts emulated_vs_f64 <= 1.5 x autocast_vs_f64, so the bar has margin
            from the reference alone.
    floor   distance to float64 >= 0.25 x emulated_vs_f64 (the same network in fp32 on the CPU with the convolutions' operands
            rounded to half): the half arithmetic actually ran -- the fp32 path sits three orders of magnitude below
            (tests/test_gpu_raft_f16.py).

The bars are read from the golden, case by case; the float64 references are computed once per module and shared."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import vae_decoder_check as VC   # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
DEC_CASES = ("dec_8x6", "dec_b2_6x10")
ENC_CASES = ("enc_64x48", "enc_b2_40x56")


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(GOLDEN, "vae_ref_autocast.npz"))
    names = list(g["cases"])
    assert names == list(DEC_CASES + ENC_CASES)                              # every case of the golden is run
    yard = {n: (float(g["autocast_vs_f64"][i]), float(g["emulated_vs_f64"][i])) for i, n in enumerate(names)}
    inputs = {"dec_8x6": np.load(os.path.join(GOLDEN, "vae_dec_ref_8x6.npz"))["z"], "dec_b2_6x10": g["z_b2_6x10"],
              "enc_64x48": np.load(os.path.join(GOLDEN, "vae_ref_64x48.npz"))["image"], "enc_b2_40x56": g["image_b2_40x56"]}
    return yard, {k: torch.from_numpy(v) for k, v in inputs.items()}


@pytest.fixture(scope="module")
def dec_sd():
    from sd_animation_optical_flow_amd.vae import random_vae_decoder_state_dict
    return random_vae_decoder_state_dict(0)


@pytest.fixture(scope="module")
def enc_sd():
    from oracle import vae_oracle as VO
    return VO.init_vae_state_dict(0)


@pytest.fixture(scope="module")
def ref64(gold, dec_sd, enc_sd):
    """Float64 truth of every case, computed once and left unchanged."""
    from oracle import vae_oracle as VO
    _, inputs = gold
    d64, e64 = VC.to64(dec_sd), {k: v.double() for k, v in enc_sd.items()}
    out = {n: VC.decode64(d64, inputs[n]) for n in DEC_CASES}
    out.update({n: VO.encode_moments(e64, inputs[n].double()) for n in ENC_CASES})
    return out


@pytest.fixture(scope="module")
def dec16(cuda, dec_sd):
    from sd_animation_optical_flow_amd.vae import VaeDecoder
    dec = VaeDecoder(dec_sd, precision="fp16")
    assert dec.precision == "fp16" and all(dec.fused_upsample.values())
    return dec


@pytest.fixture(scope="module")
def dec32(cuda, dec_sd):
    from sd_animation_optical_flow_amd.vae import VaeDecoder
    return VaeDecoder(dec_sd)


@pytest.fixture(scope="module")
def enc16(cuda, enc_sd):
    from sd_animation_optical_flow_amd.vae import VaeEncoder
    return VaeEncoder(enc_sd, precision="fp16")


def _held(what, name, got, ref, yard):
    auto, emu = yard[name]
    assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32
    d = float((got.double().cpu() - ref).abs().max())
    print(f"{what} [{name}]: vs float64 {d:.3e}; autocast {auto:.3e}, emulation {emu:.3e}; bar {2 * auto:.3e}, floor {0.25 * emu:.3e}")
    assert d <= 2.0 * auto, (what, name, d, auto)
    assert d >= 0.25 * emu, (what, name, d, emu)
    return d


@pytest.mark.parametrize("name", DEC_CASES)
def test_fp16_decoder_is_held_to_twice_the_reference_under_autocast(gold, ref64, dec16, dec32, name):
    yard, inputs = gold
    z = inputs[name].cuda()
    fused = dec16.decode(z)
    _held("VaeDecoder fp16, fused Upsample", name, fused, ref64[name], yard)
    keep = dict(dec16.fused_upsample)
    dec16.fused_upsample = {lvl: False for lvl in keep}                      # the unfused pair, its convolution in fp16
    try:
        unfused = dec16.decode(z)
    finally:
        dec16.fused_upsample = keep
    _held("VaeDecoder fp16, unfused Upsample", name, unfused, ref64[name], yard)
    plain = dec32.decode(z)
    assert not torch.equal(fused, plain) and not torch.equal(unfused, plain)
    # the fp32 decoder on the same latent, for scale: three orders of magnitude below the floor's yardstick
    d32 = float((plain.double().cpu() - ref64[name]).abs().max())
    print(f"VaeDecoder fp32 [{name}]: vs float64 {d32:.3e}")
    assert d32 < 0.25 * yard[name][1]


@pytest.mark.parametrize("name", ENC_CASES)
def test_fp16_encoder_is_held_to_twice_the_reference_under_autocast(gold, ref64, enc16, name):
    yard, inputs = gold
    _held("VaeEncoder fp16", name, enc16.encode_moments(inputs[name].cuda()), ref64[name], yard)


def test_precision_fp32_and_the_default_constructor_give_identical_bits(gold, cuda, dec_sd, enc_sd, dec32):
    from sd_animation_optical_flow_amd.vae import VaeDecoder, VaeEncoder
    _, inputs = gold
    explicit = VaeDecoder(dec_sd, precision="fp32")
    assert explicit.precision == dec32.precision == "fp32"
    for name in DEC_CASES:
        z = inputs[name].cuda()
        assert torch.equal(explicit.decode(z), dec32.decode(z)), name
        assert torch.equal(explicit.decode_latent(z), dec32.decode_latent(z)), name
    del explicit
    e_default, e_explicit = VaeEncoder(enc_sd), VaeEncoder(enc_sd, precision="fp32")
    assert e_default.precision == e_explicit.precision == "fp32"
    for name in ENC_CASES:
        image = inputs[name].cuda()
        assert torch.equal(e_default.encode_moments(image), e_explicit.encode_moments(image)), name


@pytest.mark.parametrize("name", DEC_CASES)
def test_decode_latent_bytes_in_fp16(gold, ref64, dec16, name):
    """Against `to_u8_bgr` of the float64 image.  With d the float distance of this run, clip is 1-Lipschitz and the byte is the
    floor of v * 127.5 + 127.5, so every byte is within floor(127.5 d) + 1 levels of the float64 image's.  The scale factor is 1 for
    this call (1 / 1 * z = z exactly), so that the latent decoded is the golden's."""
    _, inputs = gold
    z = inputs[name].cuda()
    keep = dec16.scale_factor
    dec16.scale_factor = 1.0
    try:
        frames = dec16.decode_latent(z)
        image = dec16.decode(z)
    finally:
        dec16.scale_factor = keep
    B, _, H, W = ref64[name].shape
    assert frames.is_cuda and frames.dtype == torch.uint8 and tuple(frames.shape) == (B, H, W, 3)
    d = float((image.double().cpu() - ref64[name]).abs().max())
    levels = int(np.floor(127.5 * d)) + 1
    frames = frames.cpu().numpy().astype(np.int32)
    worst = 0
    for b in range(B):
        want = VC.to_u8_bgr(ref64[name][b:b + 1]).astype(np.int32)
        worst = max(worst, int(np.abs(frames[b] - want).max()))
    print(f"decode_latent fp16 [{name}]: float distance {d:.3e}, bytes within {worst} levels (allowed {levels})")
    assert worst <= levels


def test_batch_slicing_is_bit_identical_in_fp16(gold, dec16):
    _, inputs = gold
    z = inputs["dec_b2_6x10"].cuda()
    assert z.shape[0] == 2
    whole = dec16.decode(z)
    assert torch.equal(dec16.decode(z, max_batch=1), whole)
    assert torch.equal(dec16.decode_latent(z, max_batch=1), dec16.decode_latent(z))


def test_ofgen_decode_latent_takes_the_fp16_decoder(gold, dec16):
    """`ofgen.decode_latent` takes a constructed decoder: nothing downstream knows about the precision."""
    from sd_animation_optical_flow_amd import ofgen
    _, inputs = gold
    z = inputs["dec_8x6"] * dec16.scale_factor
    frame = ofgen.decode_latent(dec16, z)
    assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.shape == (64, 48, 3)
    assert np.array_equal(frame, dec16.decode_latent(z.cuda())[0].cpu().numpy())
