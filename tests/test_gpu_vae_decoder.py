"""-m gpu: the first-stage (VAE) decoder on the HIP kernels -- the fused nearest-2x upsample convolution and its unfused pair against
float64, the byte exit against the torch / numpy expression bit for bit, and `VaeDecoder` against the vectors of the real reference
`Decoder` and against the float64 restatement (tests/vae_decoder_check.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vae_decoder_check as VC   # noqa: E402

GOLD = os.path.join(HERE, "golden", "vae_dec_ref_8x6.npz")
EPS = 2.0 ** -24
UPCONV_SHAPES = [(1, 1, 1, 32, 32), (2, 3, 5, 64, 48), (1, 8, 16, 128, 128), (1, 9, 17, 32, 64), (1, 16, 12, 512, 512), (1, 7, 33, 256, 256)]


def bar_of(ref):
    """The encoder's own bar (tests/test_gpu_vae.py)."""
    return 2e-4 * max(1.0, float(ref.abs().max()))


# ---------------------------------------------------------------------------------------------- upsample convolution
@pytest.fixture(scope="module")
def upconv_cases():
    """Per shape: inputs and the float64 reference with its operand magnitude S = conv(|x|, |w|) over the original nine taps,
    computed once and shared by the fused and the unfused test."""
    cases = {}
    for shp in UPCONV_SHAPES:
        B, H, W, ci, co = shp
        g = torch.Generator().manual_seed(1000 + H * 37 + W)
        x = torch.randn((B, ci, H, W), generator=g)
        w = torch.randn((co, ci, 3, 3), generator=g) / (9 * ci) ** 0.5
        b = 0.1 * torch.randn((co,), generator=g)
        ref = VC.upconv64(x, w) + b.double().view(1, -1, 1, 1)
        S = VC.upconv64(x.abs(), w.abs())
        cases[shp] = dict(x=x, w=w, b=b, ref=ref, S=S)
    return cases


def _check_upconv(out_nhwc, case, ci, label):
    out = out_nhwc.permute(0, 3, 1, 2).double().cpu()
    err = (out - case["ref"]).abs()
    bound = (9 * ci + 4) * EPS * case["S"]
    worst = float((err / bound).max())
    print(f"{label}: max |err| {float(err.max()):.3e}, max err / bound {worst:.4f}")
    assert tuple(out.shape) == tuple(case["ref"].shape)
    assert bool((err <= bound).all()), (label, worst)


@pytest.mark.parametrize("shp", UPCONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upconv2x_against_float64(cuda, upconv_cases, shp):
    """|out - ref64| <= (9 Cin + 4) 2^-24 S per output: an fp32 dot product of 4 Cin folded terms accumulates at most 4 Cin roundings
    of partial sums bounded by S (|w1 + w2| <= |w1| + |w2|), the folded weights carry one rounding each, the bias one more.  Plain
    output, then a strided row (ldo > Cout at a channel offset) whose other channels must stay untouched."""
    from sd_animation_optical_flow_amd import ops
    B, H, W, ci, co = shp
    c = upconv_cases[shp]
    x = c["x"].permute(0, 2, 3, 1).contiguous().cuda()
    wf = ops.upconv2x_weight(c["w"]).cuda()
    out = ops.upconv2x(x, wf, c["b"].cuda())
    assert tuple(out.shape) == (B, 2 * H, 2 * W, co)
    _check_upconv(out, c, ci, f"fused {shp}")
    wide = torch.full((B, 2 * H, 2 * W, co + 12), 7.0, device="cuda")
    ops.upconv2x(x, wf, c["b"].cuda(), out=wide, out_off=4)
    _check_upconv(wide[..., 4:4 + co], c, ci, f"fused, strided {shp}")
    assert bool((wide[..., :4] == 7.0).all()) and bool((wide[..., 4 + co:] == 7.0).all())
    # without bias: the same minus the bias, to one rounding of the sum
    nb = ops.upconv2x(x, wf, None).permute(0, 3, 1, 2).double().cpu()
    assert bool(((nb + c["b"].double().view(1, -1, 1, 1) - c["ref"]).abs() <= (9 * ci + 4) * EPS * c["S"]).all())


@pytest.mark.parametrize("shp", UPCONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unfused_upsample_then_conv_against_float64(cuda, upconv_cases, shp):
    """The A/B baseline, `upsample2x_nearest` + the 3x3 `ofx_conv2d`, under the same bound; the upsample itself is bit-exact."""
    from sd_animation_optical_flow_amd import ops
    B, H, W, ci, co = shp
    c = upconv_cases[shp]
    x = c["x"].permute(0, 2, 3, 1).contiguous().cuda()
    up = ops.upsample2x_nearest(x)
    assert torch.equal(up.cpu(), F.interpolate(c["x"], scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1))
    out = ops.conv2d_nhwc(up, ops.pack_conv_weight(c["w"]).cuda(), 3, 3, co, shift=c["b"].cuda())
    _check_upconv(out, c, ci, f"unfused {shp}")


def test_upconv2x_rejects_bad_arguments_without_launching(cuda):
    from sd_animation_optical_flow_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros((1, 2, 2, 8), device="cuda")
    w = torch.zeros((4, 8, 4, 8), device="cuda")
    o = torch.zeros((1, 4, 4, 8), device="cuda")
    s = ops._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.ofx_upconv2x(p(x), p(w), None, p(o), 8, 1, 2, 2, 8, 8, s) == 0
    assert L.ofx_upconv2x(None, p(w), None, p(o), 8, 1, 2, 2, 8, 8, s) == -1                  # OFX_EINVAL: null pointer
    assert L.ofx_upconv2x(p(x), p(w), None, p(o), 7, 1, 2, 2, 8, 8, s) == -1                  # ldo < Cout
    assert L.ofx_upconv2x(p(x), p(w), None, p(o), 8, 0, 2, 2, 8, 8, s) == -1                  # empty batch
    assert L.ofx_upconv2x(p(x), p(w), None, p(o), 8, 1, 32768, 32768, 8, 8, s) == -1          # 2^32 output pixels: 32-bit rows
    assert L.ofx_upconv2x(p(x), p(w), None, p(o), 8, 1, 2, 2, 6, 8, s) == -2                  # OFX_EALIGN: Cin % 4
    assert L.ofx_upconv2x(C.c_void_p(x.data_ptr() + 4), p(w), None, p(o), 8, 1, 2, 2, 8, 8, s) == -2   # x not 16-byte aligned
    assert L.ofx_upsample2x_nearest_f32(p(x), p(o), 1, 2, 2, 6, s) == -2
    assert L.ofx_upsample2x_nearest_f32(None, p(o), 1, 2, 2, 8, s) == -1
    assert L.ofx_decode_to_u8(p(x), 2, p(o), 1, 2, 2, s) == -1                                # fewer than three channels per pixel
    torch.cuda.synchronize()
    assert bool((o == 0).all())
    with pytest.raises(RuntimeError):
        ops.upconv2x(x, torch.zeros((4, 8, 4, 12), device="cuda"))                            # Cin of the weights != Cin of x
    with pytest.raises(RuntimeError):
        ops.upconv2x(x.cpu(), w)
    with pytest.raises(RuntimeError):
        ops.upconv2x_weight(torch.zeros((4, 4, 1, 1)))


# ---------------------------------------------------------------------------------------------- byte exit
def _u8_ref(x_nhwc):
    a = x_nhwc[..., :3].clip(-1, 1).numpy()
    return np.ascontiguousarray((a * 127.5 + 127.5).astype(np.uint8)[..., ::-1])


def test_decode_to_u8_is_bit_exact(cuda):
    """Against the torch / numpy expression of decode_latent on the CPU: random values, values beyond +-1 (far beyond, and
    infinite), and every value within 3 ulps of each byte boundary (k - 127.5) / 127.5, where a fused multiply-add or a rounding
    cast would land on the other byte.  Rows of 3 and of 4 floats, pixel counts that are not a multiple of the 4 a thread takes."""
    from sd_animation_optical_flow_amd import ops
    g = torch.Generator().manual_seed(3)
    edges = []
    for k in range(0, 257):
        v = np.float32((k - 127.5) / 127.5)
        lo = hi = v
        edges.append(v)
        for _ in range(3):
            lo, hi = np.nextafter(lo, np.float32(-4)), np.nextafter(hi, np.float32(4))
            edges += [lo, hi]
    edges = torch.from_numpy(np.array(edges, dtype=np.float32))
    far = torch.tensor([-1.0, 1.0, -1.0000001, 1.0000001, -3.0, 3.0, -1e30, 1e30, float("inf"), float("-inf"), 0.0, -0.0])
    vals = torch.cat([edges, far, torch.rand((5000,), generator=g) * 3 - 1.5])
    for ld, (B, H, W) in ((3, (1, 7, 9)), (4, (2, 5, 13)), (4, (1, 1, 1)), (3, (1, 64, 37))):
        n = B * H * W * ld
        idx = torch.randperm(vals.numel(), generator=g)
        x = vals[idx].repeat((n + vals.numel() - 1) // vals.numel())[:n].reshape(B, H, W, ld).contiguous()
        out = ops.decode_to_u8(x.cuda()).cpu().numpy()
        assert out.dtype == np.uint8 and out.shape == (B, H, W, 3)
        assert np.array_equal(out, _u8_ref(x)), (ld, B, H, W)
    # every edge value in each of the three channel positions
    m = edges.numel() + far.numel()
    col = torch.cat([edges, far])
    x = torch.stack([col, col.roll(1), col.roll(2)], dim=1).reshape(1, 1, m, 3).contiguous()
    assert np.array_equal(ops.decode_to_u8(x.cuda()).cpu().numpy(), _u8_ref(x))


# ---------------------------------------------------------------------------------------------- the decoder
@pytest.fixture(scope="module")
def dec_sd():
    from sd_animation_optical_flow_amd.vae import random_vae_decoder_state_dict
    return random_vae_decoder_state_dict(0)


@pytest.fixture(scope="module")
def vae_dec(cuda, dec_sd):
    from sd_animation_optical_flow_amd.vae import VaeDecoder
    return VaeDecoder({"first_stage_model." + k: v for k, v in dec_sd.items()})      # the prefix of full SD checkpoints


@pytest.fixture(scope="module")
def sd64(dec_sd):
    return VC.to64(dec_sd)


def test_decoder_against_the_reference_vectors_directly(vae_dec):
    """One hop: the HIP decoder on the golden latent against what the REAL reference `Decoder` after `post_quant_conv` produced."""
    g = np.load(GOLD)
    ref = torch.from_numpy(g["image"])
    assert all(vae_dec.fused_upsample.values())
    out = vae_dec.decode(torch.from_numpy(g["z"]).cuda()).cpu()
    assert tuple(out.shape) == tuple(ref.shape) == (1, 3, 64, 48)
    err = float((out - ref).abs().max())
    print(f"decode vs reference: max |err| {err:.3e}, bar {bar_of(ref):.3e}")
    assert err <= bar_of(ref)


_CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd.vae import VaeDecoder, random_vae_decoder_state_dict
g = np.load(sys.argv[2])
dec = VaeDecoder(random_vae_decoder_state_dict(0))
assert not any(dec.fused_upsample.values())
out = dec.decode(torch.from_numpy(g["z"]).cuda()).cpu()
ref = torch.from_numpy(g["image"])
print("ERR %.9e %.9e" % (float((out - ref).abs().max()), float(ref.abs().max())))
"""


def test_decoder_unfused_in_a_fresh_process(cuda):
    """OFX_VAE_NO_UPCONV=1 is read once per process, so the unfused decoder runs in a child: same golden, same bar."""
    env = dict(os.environ, OFX_VAE_NO_UPCONV="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(HERE), GOLD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ERR ")][-1].split()
    err, mx = float(line[1]), float(line[2])
    print(f"unfused decode vs reference: max |err| {err:.3e}")
    assert err <= 2e-4 * max(1.0, mx)


@pytest.mark.parametrize("B,h,w", [(1, 1, 1), (2, 5, 9), (1, 16, 12)])
def test_decoder_against_the_float64_restatement(vae_dec, sd64, B, h, w):
    z = torch.randn((B, 4, h, w), generator=torch.Generator().manual_seed(100 + h))
    ref = VC.decode64(sd64, z)
    out = vae_dec.decode(z.cuda()).double().cpu()
    assert tuple(out.shape) == (B, 3, 8 * h, 8 * w)
    err = float((out - ref).abs().max())
    print(f"decode {B}x{h}x{w} vs float64: max |err| {err:.3e}, bar {bar_of(ref):.3e}")
    assert err <= bar_of(ref)
    # decode_first_stage divides by the scale factor first (ddpm.py:820-828)
    out2 = vae_dec.decode_first_stage(z.cuda()).double().cpu()
    ref2 = VC.decode64(sd64, 1.0 / VC.SCALE_FACTOR * z)
    assert float((out2 - ref2).abs().max()) <= bar_of(ref2)


def test_decode_latent_bytes_against_the_reference_frame(vae_dec):
    """The byte frame against the reference's: a differing byte differs by exactly 1, and only where the reference's float before
    truncation lies within 127.5 * bar of an integer (the decoder may sit on the other side of it).  The golden frame came from
    the latent itself, so the scale factor is 1 for this call (1 / 1 * z = z exactly)."""
    g = np.load(GOLD)
    ref_img = torch.from_numpy(g["image"])
    keep = vae_dec.scale_factor
    vae_dec.scale_factor = 1.0
    try:
        out = vae_dec.decode_latent(torch.from_numpy(g["z"]).cuda())
    finally:
        vae_dec.scale_factor = keep
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (1, 64, 48, 3)
    out = out[0].cpu().numpy().astype(np.int32)
    ref = g["frame_bgr"].astype(np.int32)
    v = (ref_img.clip(-1, 1)[0].permute(1, 2, 0).numpy() * 127.5 + 127.5)[:, :, ::-1]       # the float each reference byte truncates
    diff = out != ref
    print(f"decode_latent: {int(diff.sum())} of {diff.size} bytes differ")
    assert bool((np.abs(out - ref)[diff] == 1).all())
    near = np.abs(v - np.round(v)) <= 127.5 * bar_of(ref_img)
    assert bool(near[diff].all())
    assert np.array_equal(VC.to_u8_bgr(ref_img).astype(np.int32), ref)                       # the reference alone: zero differing bytes


def test_decoder_batch_limits_and_slicing(vae_dec):
    assert vae_dec.max_batch(768, 512) == 5 and vae_dec.max_batch(1024, 1024) == 1
    z = torch.randn((3, 4, 3, 4), generator=torch.Generator().manual_seed(8)).cuda()
    sliced = vae_dec.decode(z, max_batch=2)
    assert tuple(sliced.shape) == (3, 3, 24, 32)
    for b in range(3):
        one = vae_dec.decode(z[b:b + 1])
        # another batch size may take another tile and summation order: fp32 rounding, far inside the bar
        assert float((sliced[b:b + 1] - one).abs().max()) <= 1e-4 * max(1.0, float(one.abs().max()))
    assert torch.equal(vae_dec.decode(z, max_batch=1), torch.cat([vae_dec.decode(z[b:b + 1]) for b in range(3)]))


def test_decoder_rejects_bad_latents(vae_dec):
    with pytest.raises(RuntimeError):
        vae_dec.decode(torch.zeros((1, 4, 4, 4)))                         # CPU tensor
    with pytest.raises(RuntimeError):
        vae_dec.decode(torch.zeros((1, 3, 4, 4), device="cuda"))          # wrong channel count
    with pytest.raises(RuntimeError):
        vae_dec.decode(torch.zeros((4, 4, 4), device="cuda"))             # wrong rank
    with pytest.raises(RuntimeError):
        vae_dec.decode_latent(torch.zeros((1, 4, 4, 4)))
    from sd_animation_optical_flow_amd.vae import VaeDecoder
    with pytest.raises(KeyError):
        VaeDecoder({})
    sd = dict(vae_dec_sd_small())
    with pytest.raises(ValueError):
        VaeDecoder(sd)


def vae_dec_sd_small():
    """A state dict with one tensor of the wrong shape."""
    from sd_animation_optical_flow_amd.vae import decoder_tensors
    sd = {k: torch.zeros(s) for k, s in decoder_tensors()}
    sd["decoder.conv_in.weight"] = torch.zeros((512, 4, 1, 1))
    return sd


def test_ofgen_decode_latent_returns_a_bgr_frame(vae_dec):
    from sd_animation_optical_flow_amd import ofgen
    z = torch.randn((1, 4, 2, 3), generator=torch.Generator().manual_seed(4)) * 0.18215
    frame = ofgen.decode_latent(vae_dec, z)
    assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.shape == (16, 24, 3)
    assert np.array_equal(frame, vae_dec.decode_latent(z.cuda())[0].cpu().numpy())
