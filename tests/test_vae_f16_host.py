"""`precision=` of the first-stage models (VaeEncoder / VaeDecoder) and of `ops.upconv2x` (ofx_upconv2x_prec) as far as the host can
tell: the argument checks that need no device, the prototypes, the launcher's tile choice, and the golden of the reference under
autocast (tests/golden/make_golden_vae_autocast.py).  No test here needs a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "vae_ref_autocast.npz")
EINVAL, EALIGN = -1, -2                      # include/ofx.h
PREC_FP32, PREC_F16 = 0, 5
BAD = ("fp64", "bf16x3", "FP16", "fp16_epi", None, 5)


def test_bad_precisions_are_value_errors_before_the_checkpoint_or_a_device():
    from sd_animation_optical_flow_amd import ops, vae
    x = torch.zeros((1, 2, 2, 8))                                           # CPU tensors: a device check would be a RuntimeError
    w = torch.zeros((4, 8, 4, 8))
    for bad in BAD:
        with pytest.raises(ValueError, match="precision"):
            ops.upconv2x(x, w, precision=bad)
        for cls in (vae.VaeEncoder, vae.VaeDecoder):
            with pytest.raises(ValueError, match="fp32.*fp16"):             # names the two values
                cls({}, precision=bad)                                      # before the (empty) checkpoint is read
    assert vae.VAE_PRECISIONS == ("fp32", "fp16") and ops.UPCONV_PRECISIONS == {"fp32": PREC_FP32, "fp16": PREC_F16}
    # the accepted values reach the old checks: the empty checkpoint is what is wrong, on a machine without a device too
    for good in ("fp32", "fp16"):
        for cls in (vae.VaeEncoder, vae.VaeDecoder):
            with pytest.raises(KeyError):
                cls({}, precision=good)
    with pytest.raises(RuntimeError):
        ops.upconv2x(x, w, precision="fp16")                                # a CPU tensor, not the precision


def test_the_default_is_fp32_everywhere():
    from sd_animation_optical_flow_amd import ops, vae
    for fn in (vae.VaeEncoder.__init__, vae.VaeDecoder.__init__, ops.upconv2x):
        assert inspect.signature(fn).parameters["precision"].default == "fp32"


def _proto(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_ctypes_table_and_the_header_agree_on_the_new_prototypes():
    from sd_animation_optical_flow_amd import _lib
    header = open(os.path.join(ROOT, "include", "ofx.h")).read()
    kind = lambda a: "p" if "*" in a else {"int": "i", "long": "l", "float": "f", "size_t": "z"}[a.rsplit(" ", 1)[0].replace("const ", "")]
    ctype = {C.c_void_p: "p", C.c_int: "i", C.c_long: "l", C.c_float: "f", C.c_size_t: "z"}
    args, base = _proto(header, "ofx_upconv2x_prec"), _proto(header, "ofx_upconv2x")
    res, table = _lib.SIGNATURES["ofx_upconv2x_prec"]
    assert res is C.c_int and [ctype[t] for t in table] == [kind(a) for a in args]
    assert len(table) == len(_lib.SIGNATURES["ofx_upconv2x"][1]) + 1
    i = args.index("int precision")
    assert args[:i] + args[i + 1:] == base and args[i + 1] == "void* stream"       # the old prototype with `precision` before the stream
    res, table = _lib.SIGNATURES["ofx_upconv2x_bn"]
    assert res is C.c_int and [ctype[t] for t in table] == [kind(a) for a in _proto(header, "ofx_upconv2x_bn")] == ["i", "i"]
    flat = re.sub(r" +", " ", header)
    assert "#define OFX_PREC_FP32 0" in flat and "#define OFX_PREC_F16 5" in flat


def test_argument_validation_precedes_every_hip_call():
    """Testable without a device: a bad precision is OFX_EINVAL whatever else is passed, and the checks of ofx_upconv2x apply to the
    fp16 entry unchanged."""
    from sd_animation_optical_flow_amd import _lib
    lib = _lib.lib()
    buf = (C.c_float * 4096)()
    p = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)
    off = C.c_void_p(p.value + 4)
    for prec in (1, 2, 3, 4, 6, 261, -1):
        assert lib.ofx_upconv2x_prec(p, p, None, p, 8, 1, 2, 2, 8, 8, prec, None) == EINVAL
        assert lib.ofx_upconv2x_prec(p, p, None, p, 8, 1, 2, 2, 6, 8, prec, None) == EINVAL          # not OFX_EALIGN: the precision first
    for prec in (PREC_FP32, PREC_F16):
        assert lib.ofx_upconv2x_prec(None, p, None, p, 8, 1, 2, 2, 8, 8, prec, None) == EINVAL       # null pointer
        assert lib.ofx_upconv2x_prec(p, p, None, p, 7, 1, 2, 2, 8, 8, prec, None) == EINVAL          # ldo < Cout
        assert lib.ofx_upconv2x_prec(p, p, None, p, 8, 0, 2, 2, 8, 8, prec, None) == EINVAL          # empty batch
        assert lib.ofx_upconv2x_prec(p, p, None, p, 8, 1, 32768, 32768, 8, 8, prec, None) == EINVAL  # 2^32 output pixels
        assert lib.ofx_upconv2x_prec(p, p, None, p, 8, 1, 2, 2, 6, 8, prec, None) == EALIGN          # Cin % 4
        assert lib.ofx_upconv2x_prec(off, p, None, p, 8, 1, 2, 2, 8, 8, prec, None) == EALIGN        # x not 16-byte aligned
        assert lib.ofx_upconv2x_prec(p, off, None, p, 8, 1, 2, 2, 8, 8, prec, None) == EALIGN        # w not 16-byte aligned


def test_the_launcher_picks_the_same_tile_in_both_precisions():
    from sd_animation_optical_flow_amd import _lib, ops
    lib = _lib.lib()
    for prec in ("fp32", "fp16"):
        assert [ops.upconv2x_bn(c, prec) for c in (1, 4, 40, 64, 65, 128, 136, 256, 512)] == [64, 64, 64, 64, 128, 128, 128, 128, 128]
    assert lib.ofx_upconv2x_bn(0, PREC_F16) == EINVAL and lib.ofx_upconv2x_bn(64, 1) == EINVAL
    with pytest.raises(ValueError, match="precision"):
        ops.upconv2x_bn(64, "bf16x3")


def test_the_golden_holds_every_case_and_its_ratios_are_within_the_cap():
    g = np.load(GOLD)
    assert list(g["cases"]) == ["dec_8x6", "dec_b2_6x10", "enc_64x48", "enc_b2_40x56"]
    auto, emu, f32 = g["autocast_vs_f64"], g["emulated_vs_f64"], g["fp32_vs_f64"]
    assert auto.shape == emu.shape == f32.shape == (4,)
    assert float(g["ratio_cap"][0]) == 1.5
    for name, a, e, f in zip(g["cases"], auto, emu, f32):
        print(f"{name}: autocast {a:.3e} emulated {e:.3e} ratio {e / a:.2f} fp32 {f:.3e}")
        assert 0.0 < e <= 1.5 * a and 0.0 < f < 0.05 * e, name                # the device's bar (2 a) and floor (e / 4) are ordered: e / 4 < 2 a
    assert g["z_b2_6x10"].shape == (2, 4, 6, 10) and g["z_b2_6x10"].dtype == np.float32
    assert g["image_b2_40x56"].shape == (2, 3, 40, 56) and float(np.abs(g["image_b2_40x56"]).max()) <= 1.0
    # the first case of each module is the stored input of the fp32 goldens
    assert np.load(os.path.join(HERE, "golden", "vae_dec_ref_8x6.npz"))["z"].shape == (1, 4, 8, 6)
    assert np.load(os.path.join(HERE, "golden", "vae_ref_64x48.npz"))["image"].shape == (1, 3, 64, 48)
