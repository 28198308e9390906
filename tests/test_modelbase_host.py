"""Host side of `modelbase` (no GPU): what the five SD-stage models rely on in `load_tensors`, `env_flag`, `pad_channels4` and the
small checks, and the order of the VAE's constructor checks: checkpoint before device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_bits_cases as mb  # noqa: E402
from sd_animation_optical_flow_amd import modelbase as MB  # noqa: E402

WANT = [("a.weight", (2, 3)), ("a.bias", (2,)), ("b.weight", (4, 2, 1, 1))]


def _sd(prefix="", dtype=torch.float64):
    g = torch.Generator().manual_seed(1)
    return {prefix + k: torch.randn(s, generator=g).to(dtype) for k, s in WANT}


@pytest.mark.parametrize("prefix", ["", "model.diffusion_model.", "first."])
def test_load_tensors_reads_under_the_prefix_as_fp32_cpu(prefix):
    sd = _sd(prefix)
    sd["other.key"] = torch.zeros(3)                               # what `want` does not list is ignored
    sd["a.weight" if prefix else "x.a.weight"] = sd[prefix + "a.weight"]   # a key under another prefix changes nothing
    got = MB.load_tensors(sd, WANT, prefix, "Thing")
    assert list(got) == [k for k, _ in WANT]                       # un-prefixed keys, in the order of `want`
    for k, s in WANT:
        assert got[k].dtype == torch.float32 and got[k].device.type == "cpu" and tuple(got[k].shape) == s
        assert torch.equal(got[k], sd[prefix + k].float())


@pytest.mark.parametrize("prefix", ["", "p."])
def test_load_tensors_names_what_is_wrong(prefix):
    sd = _sd(prefix)
    lacking = {k: v for k, v in sd.items() if k != prefix + "a.bias"}
    with pytest.raises(KeyError, match=f"Thing checkpoint lacks {prefix}a.bias"):
        MB.load_tensors(lacking, WANT, prefix, "Thing")
    with pytest.raises(KeyError, match="Thing checkpoint lacks q.a.weight"):
        MB.load_tensors(sd, WANT, "q.", "Thing")                   # nothing under that prefix: the first key is named
    bad = dict(sd, **{prefix + "b.weight": torch.zeros((4, 2))})
    with pytest.raises(ValueError, match=rf"{prefix}b.weight: shape \(4, 2\) != \(4, 2, 1, 1\)"):
        MB.load_tensors(bad, WANT, prefix, "Thing")
    both = {k: v for k, v in bad.items() if k != prefix + "a.bias"}
    with pytest.raises(KeyError):                                  # the order of `want`: a.bias comes before b.weight
        MB.load_tensors(both, WANT, prefix, "Thing")


@pytest.mark.parametrize("value,want", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True), ("00", True)])
def test_env_flag_values_and_the_once_per_process_read(monkeypatch, value, want):
    name = "OFX_TEST_MODELBASE_FLAG"
    MB.env_flag.cache_clear()
    try:
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
        assert MB.env_flag(name) is want
        monkeypatch.setenv(name, "0" if want else "1")             # read once per process per name: a later change is not seen
        assert MB.env_flag(name) is want
        assert MB.env_flag(name + "_OTHER") is False               # per name
    finally:
        MB.env_flag.cache_clear()


def test_the_module_switches_read_their_own_variables(monkeypatch):
    from sd_animation_optical_flow_amd import controlnet, text_encoder, transformer, unet, vae
    switches = {"OFX_UNET_TORCH_GLUE": unet._torch_glue, "OFX_CNET_TORCH_GLUE": controlnet._torch_glue, "OFX_ST_TORCH_GLUE": transformer._torch_glue,
                "OFX_CLIP_TORCH_GLUE": text_encoder._torch_glue, "OFX_VAE_NO_UPCONV": vae._no_upconv}
    try:
        for on in switches:
            MB.env_flag.cache_clear()
            for name in switches:
                monkeypatch.setenv(name, "1" if name == on else "0")
            assert {name: fn() for name, fn in switches.items()} == {name: name == on for name in switches}
    finally:
        MB.env_flag.cache_clear()


@pytest.mark.parametrize("c", [1, 3, 5, 9])
def test_pad_channels4_zero_tail_and_unchanged_data(c):
    g = torch.Generator().manual_seed(c)
    nchw = torch.randn((2, c, 3, 5), generator=g)
    x = nchw.permute(0, 2, 3, 1)                                   # the callers' operand: an NHWC view of an NCHW tensor
    out = MB.pad_channels4(x, c)
    cp = (c + 3) // 4 * 4
    assert tuple(out.shape) == (2, 3, 5, cp) and out.is_contiguous() and out.dtype == torch.float32
    assert torch.equal(out[..., :c], x) and bool((out[..., c:] == 0).all())
    assert torch.equal(nchw.permute(0, 2, 3, 1), x)                # the input is not written to


@pytest.mark.parametrize("c", [4, 8])
def test_pad_channels4_without_a_tail_is_contiguous_and_no_copy(c):
    x = torch.randn((2, 3, 5, c))
    same = MB.pad_channels4(x, c)
    assert same.data_ptr() == x.data_ptr() and same.is_contiguous()            # already contiguous: the same storage
    view = torch.randn((2, c, 3, 5)).permute(0, 2, 3, 1)
    out = MB.pad_channels4(view, c)
    assert out.is_contiguous() and tuple(out.shape) == (2, 3, 5, c) and torch.equal(out, view)


def test_small_checks():
    t = torch.zeros((2, 3, 4))
    assert not MB.is_f32_cuda(t, 3)                                # a host tensor
    assert not MB.is_f32_cuda(None, 3) and not MB.is_f32_cuda([1.0], 1)
    MB.check_activation_bytes((1 << 31) - 1, "too big")
    with pytest.raises(RuntimeError, match="too big"):
        MB.check_activation_bytes(1 << 31, "too big")
    out = []
    MB.wb(out, "conv", 8, 4, 3, 3)
    MB.wb(out, "norm", 8)
    assert out == [("conv.weight", (8, 4, 3, 3)), ("conv.bias", (8,)), ("norm.weight", (8,)), ("norm.bias", (8,))]


@pytest.mark.parametrize("which", ["encoder", "decoder"])
def test_vae_checks_the_checkpoint_before_it_asks_for_a_device(which):
    """A missing key is a KeyError and a wrong shape a ValueError on every machine, one without a device included (there the
    constructors used to raise the RuntimeError about the device first)."""
    from sd_animation_optical_flow_amd import vae
    cls, rand = (vae.VaeEncoder, vae.random_vae_state_dict) if which == "encoder" else (vae.VaeDecoder, vae.random_vae_decoder_state_dict)
    sd = rand(0, mb.VAE_SMALL)
    key = f"{which}.mid.attn_1.q.weight"
    with pytest.raises(KeyError, match=f"VAE checkpoint lacks {which}.mid.attn_1.q.weight"):
        cls({k: v for k, v in sd.items() if k != key}, cfg=mb.VAE_SMALL)
    with pytest.raises(KeyError, match=f"VAE checkpoint lacks {which}.conv_in.weight"):
        cls({}, cfg=mb.VAE_SMALL)
    with pytest.raises(ValueError, match=f"{which}.mid.attn_1.q.weight: shape"):
        cls({"first_stage_model." + k: (v[:1] if k == key else v) for k, v in sd.items()}, cfg=mb.VAE_SMALL)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a HIP device"):          # a good checkpoint: the device is what is missing
            cls(sd, cfg=mb.VAE_SMALL)
