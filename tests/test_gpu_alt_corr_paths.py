"""-m gpu: volume-free correlation (`alternate_corr=True`, OFX_RAFT_ALT_CORR) on every engine path and through the Python surface,
for the basic and the small network.

Bar (BASELINE.json north_star): mean flow EPE < 1e-3 px -- from the float64-capable oracles run with alternate_corr=True
(`oracle.raft_oracle.raft_forward`; tests/small_raft_check.py for the small network, whose lookup is one function for both modes)
and from the engine's own volume mode on the same pairs.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import small_raft_check as SR
from oracle import raft_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# T = 4 frames: `ops.warp` samples batches of >= 4 frames with the function the fused upsample-and-warp kernels call, so the warped
# frames can be compared bit for bit (smaller batches take the generic bilinear kernel: 1 LSB apart on rounding ties, test_gpu_raft_small)
H, W, T, ITERS = 128, 160, 4, 6
# image T is the key frame: frames -> key (the shared-image2 batch), key -> frames (the shared-image1 batch); images repeat
PAIRS = [(t, T) for t in range(T)] + [(T, t) for t in range(T)]
ALT, SH2 = 8, 2


def _frames(seed, B, H, W):
    g = torch.Generator().manual_seed(seed)
    base = F.avg_pool2d(torch.rand((1, 3, H + 32, W + 32), generator=g), 5, 1, 2)
    base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)
    key = base[0, :, 16:16 + H, 16:16 + W].permute(1, 2, 0).contiguous()
    frames = []
    for b in range(B):
        dx, dy = (3 * b + 2) % 7 - 3, (5 * b + 1) % 5 - 2
        frames.append(base[0, :, 16 + dy:16 + dy + H, 16 + dx:16 + dx + W].permute(1, 2, 0).contiguous())
    return key, torch.stack(frames)


def _epe(a, b):
    return (a.double().cpu() - b.double().cpu()).pow(2).sum(-1).sqrt().mean().item()


class Net:
    """One network: its weights, an engine per correlation mode, the test images and the oracle's alt-corr flows of PAIRS."""

    def __init__(self, name, sd):
        from sd_animation_optical_flow_amd.raft import RaftEngine
        self.name, self.sd = name, sd
        self.eng = RaftEngine(sd)
        key, frames = _frames(21, T, H, W)
        self.key, self.frames = key.cuda(), frames.cuda()
        self.images = torch.cat([frames, key[None]]).contiguous()
        i1 = self.images[[a for a, _ in PAIRS]].permute(0, 3, 1, 2)
        i2 = self.images[[b for _, b in PAIRS]].permute(0, 3, 1, 2)
        if name == "basic":
            _, up = RO.raft_forward(sd, i1.float(), i2.float(), iters=ITERS, alternate_corr=True)
        else:
            _, up = SR.raft_small_forward(sd, i1, i2, ITERS)
        self.ref = up.permute(0, 2, 3, 1).contiguous()
        self.images = self.images.cuda()


@pytest.fixture(scope="module", params=["basic", "small"])
def net(request, cuda, raft_sd):
    if request.param == "basic":
        return Net("basic", raft_sd)
    from sd_animation_optical_flow_amd.weights import random_state_dict
    return Net("small", random_state_dict(0, small=True))


def _bar(tag, got, *refs):
    for nm, ref in refs:
        e = _epe(got, ref)
        print(f"{tag}: EPE {e:.3e} px from {nm}")
        assert e < 1e-3, (tag, nm)


def test_shared_key_frame_takes_alternate_corr(net):
    e = net.eng
    alt = e.forward(net.frames, net.key, iters=ITERS, alternate_corr=True)                  # OFX_RAFT_SHARED_IMG2
    vol = e.forward(net.frames, net.key, iters=ITERS)
    _bar(f"{net.name} shared image2", alt, ("the oracle", net.ref[:T]), ("the volume mode", vol))
    rep = e.forward(net.frames, net.key[None].repeat(T, 1, 1, 1).contiguous(), iters=ITERS, alternate_corr=True)
    _bar(f"{net.name} repeated image2", rep, ("the shared call", alt))
    alt1 = e.forward(net.key, net.frames, iters=ITERS, alternate_corr=True)                 # OFX_RAFT_SHARED_IMG1
    _bar(f"{net.name} shared image1", alt1, ("the oracle", net.ref[T:]), ("the volume mode", e.forward(net.key, net.frames, iters=ITERS)))


def test_forward_pairs_takes_alternate_corr(net):
    e = net.eng
    i1, i2 = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    alt = e.forward_pairs(net.images, i1, i2, iters=ITERS, alternate_corr=True)
    vol = e.forward_pairs(net.images, i1, i2, iters=ITERS)
    _bar(f"{net.name} forward_pairs", alt, ("the oracle", net.ref), ("the volume mode", vol))
    _bar(f"{net.name} forward_pairs", alt[:T], ("the shared-key call", e.forward(net.frames, net.key, iters=ITERS, alternate_corr=True)))


def test_warp_inside_the_upsample_and_warm_start(net):
    from sd_animation_optical_flow_amd import ops
    e = net.eng
    key_ai = (255 - net.key).contiguous()
    flow = e.forward(net.frames, net.key, iters=ITERS, alternate_corr=True)
    wflow, warped = e.forward(net.frames, net.key, iters=ITERS, alternate_corr=True, warp_frame=key_ai)
    assert torch.equal(wflow, flow)
    assert torch.equal(warped, ops.warp(key_ai, wflow.contiguous(), mode="bilinear", sign=1.0))
    i1, i2 = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    pflow, pwarped = e.forward_pairs(net.images, i1, i2, iters=ITERS, alternate_corr=True, warp_frame=key_ai, n_warp=T)
    assert torch.equal(pflow, e.forward_pairs(net.images, i1, i2, iters=ITERS, alternate_corr=True))
    assert torch.equal(pwarped, ops.warp(key_ai, pflow[:T].contiguous(), mode="bilinear", sign=1.0))
    zero = torch.zeros((T, H // 8, W // 8, 2), device="cuda")
    assert torch.equal(e.forward(net.frames, net.key, iters=ITERS, alternate_corr=True, flow_init=zero), flow)
    zero_p = torch.zeros((len(PAIRS), H // 8, W // 8, 2), device="cuda")
    assert torch.equal(e.forward_pairs(net.images, i1, i2, iters=ITERS, alternate_corr=True, flow_init=zero_p), pflow)
    # a real warm start: the refinement continues from the previous flow and stays on the oracle's answer
    up, low = e.forward(net.frames, net.key, iters=ITERS, alternate_corr=True, want_low=True)
    warm, _ = e.forward(net.frames, net.key, iters=ITERS, alternate_corr=True, want_low=True, flow_init=low)
    assert _epe(warm, e.forward(net.frames, net.key, iters=ITERS, flow_init=low)) < 1e-3


def test_a_workspace_of_exactly_the_mode_size_is_enough(net):
    from sd_animation_optical_flow_amd import _lib
    e, L = net.eng, _lib.lib()
    want = e.forward(net.frames, net.key, iters=ITERS, alternate_corr=True)
    need = L.ofx_raft_workspace_bytes_mode(e._h, 0, T, H, W, ALT | SH2)
    assert 0 < need < L.ofx_raft_workspace_bytes_mode(e._h, 0, T, H, W, 0) == L.ofx_raft_workspace_bytes(e._h, T, H, W)
    e._ws = None
    e._ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    assert torch.equal(e.forward(net.frames, net.key, iters=ITERS, alternate_corr=True), want)
    assert e._ws.numel() == need
    i1, i2 = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    wantp = e.forward_pairs(net.images, i1, i2, iters=ITERS, alternate_corr=True)
    needp = L.ofx_raft_workspace_bytes_mode(e._h, T + 1, len(PAIRS), H, W, ALT)
    assert 0 < needp < L.ofx_raft_workspace_bytes_pairs(e._h, T + 1, len(PAIRS), H, W)
    e._ws = None
    e._ws = torch.empty((needp,), dtype=torch.uint8, device="cuda")
    assert torch.equal(e.forward_pairs(net.images, i1, i2, iters=ITERS, alternate_corr=True), wantp)
    assert e._ws.numel() == needp
    e._ws = torch.empty((needp - 256,), dtype=torch.uint8, device="cuda")                    # one allocation unit short: refused by the C side
    with pytest.raises(_lib.OfxError, match="workspace"):
        import ctypes as C
        out = torch.empty((len(PAIRS), H, W, 2), device="cuda")
        a1, a2 = (C.c_int * len(PAIRS))(*i1), (C.c_int * len(PAIRS))(*i2)
        _lib.check(L.ofx_raft_forward_pairs(e._h, C.c_void_p(net.images.data_ptr()), T + 1, a1, a2, len(PAIRS), H, W, ITERS, ALT,
                                            C.c_void_p(out.data_ptr()), None, C.c_void_p(e._ws.data_ptr()), e._ws.numel(), None), "pairs")
    e._ws = None


def test_auto_mode_runs_unsliced_what_the_volume_layout_would_slice(net):
    from sd_animation_optical_flow_amd import _lib
    from sd_animation_optical_flow_amd.raft import RaftEngine
    L = _lib.lib()
    auto = RaftEngine(net.sd, corr="auto")
    auto.ws_budget_bytes = int(L.ofx_raft_workspace_bytes(auto._h, T, H, W)) - 1            # one byte short of the volume layout of T pairs
    assert auto.pairs_that_fit(T, H, W) < T
    assert auto.pairs_that_fit(T, H, W, alternate_corr=True) == T
    assert auto.max_pairs_now(H, W, T, alternate_corr=None) == auto.max_pairs_now(H, W, T, alternate_corr=True) >= auto.max_pairs_now(H, W, T)
    flow = auto.forward(net.frames, net.key, iters=ITERS)
    assert auto._ws.numel() == L.ofx_raft_workspace_bytes_mode(auto._h, 0, T, H, W, ALT | SH2)      # one call, the volume-free layout
    assert torch.equal(flow, net.eng.forward(net.frames, net.key, iters=ITERS, alternate_corr=True))
    _bar(f"{net.name} auto", flow, ("the oracle", net.ref[:T]))
    i1, i2 = [a for a, _ in PAIRS], [b for _, b in PAIRS]
    auto.ws_budget_bytes = int(L.ofx_raft_workspace_bytes_pairs(auto._h, T + 1, len(PAIRS), H, W)) - 1
    assert torch.equal(auto.forward_pairs(net.images, i1, i2, iters=ITERS), net.eng.forward_pairs(net.images, i1, i2, iters=ITERS, alternate_corr=True))
    # the per-call argument wins over the default, and a batch the volume layout holds stays on the volume
    assert torch.equal(auto.forward(net.frames[:1], net.key, iters=ITERS, alternate_corr=False), net.eng.forward(net.frames[:1], net.key, iters=ITERS))
    auto.ws_budget_bytes = None
    assert torch.equal(auto.forward(net.frames, net.key, iters=ITERS), net.eng.forward(net.frames, net.key, iters=ITERS))
    local = RaftEngine(net.sd, corr="local")
    assert torch.equal(local.forward(net.frames, net.key, iters=ITERS), net.eng.forward(net.frames, net.key, iters=ITERS, alternate_corr=True))
    assert torch.equal(local.forward(net.frames, net.key, iters=ITERS, alternate_corr=False), net.eng.forward(net.frames, net.key, iters=ITERS))
    with pytest.raises(ValueError):
        RaftEngine(net.sd, corr="fast")


def test_the_product_surface_inherits_the_mode(net):
    from sd_animation_optical_flow_amd import clip, pdcnet_of
    vol = pdcnet_of.create_of_algo(net.sd)
    loc = pdcnet_of.create_of_algo(net.sd, corr="local")
    assert loc.network.corr == "local" and vol.network.corr == "volume"
    loc.iters = vol.iters = ITERS                                                            # the oracle's flows are ITERS iterations
    key_ai = (255 - net.key).contiguous()
    a = loc.calc_batch_device(net.key, net.frames, warp_frame=key_ai)
    b = vol.calc_batch_device(net.key, net.frames, warp_frame=key_ai)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
    _bar(f"{net.name} calc_batch_device", a[0], ("the volume mode", b[0]), ("the oracle", net.ref[:T]))
    assert (a[1] - b[1]).abs().max().item() < 1e-2                                           # confidence of flows 1e-3 px apart
    pf, pc = loc.calc_pairs(net.images, [(T, 0), (T, 1)])
    qf, qc = vol.calc_pairs(net.images, [(T, 0), (T, 1)])
    assert pf.shape == qf.shape and pc.shape == qc.shape and pf.dtype == qf.dtype
    _bar(f"{net.name} calc_pairs", pf, ("the volume mode", qf), ("the oracle", net.ref[:2]))
    sl = clip.FrameSynthesizer(loc, warp_mode="bilinear", thres=0.9, ksize=7).synthesize(net.frames, net.key, key_ai)
    sv = clip.FrameSynthesizer(vol, warp_mode="bilinear", thres=0.9, ksize=7).synthesize(net.frames, net.key, key_ai)
    for x, y in zip(sl, sv):
        assert x.shape == y.shape and x.dtype == y.dtype
    _bar(f"{net.name} FrameSynthesizer", sl[0], ("the volume mode", sv[0]))


CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from sd_animation_optical_flow_amd.raft import RaftEngine
from sd_animation_optical_flow_amd.weights import random_state_dict
from sd_animation_optical_flow_amd import ops
ops.prof_enable(True)
g = torch.Generator().manual_seed(5)
base = torch.nn.functional.avg_pool2d(torch.rand((1, 3, 160, 192), generator=g), 5, 1, 2)
base = ((base - base.min()) / (base.max() - base.min()) * 255).round().to(torch.uint8)[0].permute(1, 2, 0)
key = base[16:144, 16:176].contiguous().cuda()
frames = torch.stack([base[16 + d:144 + d, 18 - d:178 - d] for d in (1, 2)]).contiguous().cuda()
images = torch.cat([frames, key[None]]).contiguous()
epe = lambda a, b: (a - b).pow(2).sum(-1).sqrt().mean().item()
for small in (False, True):
    e = RaftEngine(random_state_dict(0, small=small))
    a = epe(e.forward(frames, key, iters=6, alternate_corr=True), e.forward(frames, key, iters=6))
    b = epe(e.forward_pairs(images, [0, 1, 2], [2, 2, 0], iters=6, alternate_corr=True), e.forward_pairs(images, [0, 1, 2], [2, 2, 0], iters=6))
    print("EPE", small, a, b)
    assert a < 1e-3 and b < 1e-3
torch.cuda.synchronize()
print("KERNELS", sorted(n for n in ops.prof_collect() if "local_corr" in n))
"""


@pytest.mark.parametrize("switch", ["1", None])
def test_the_switch_puts_every_path_back_on_the_per_pixel_kernel(cuda, tmp_path, switch):
    """OFX_LOCAL_CORR_NO_TILED=1 in a fresh process: shared-key and indexed-pairs alternate_corr calls of both networks still meet the
    bar against the volume mode, and the launches are the per-pixel kernel's; without it they are the tiled kernel's."""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ)
    env.pop("OFX_LOCAL_CORR_NO_TILED", None)
    if switch:
        env["OFX_LOCAL_CORR_NO_TILED"] = switch
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=600)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0
    want = "['local_corr']" if switch else "['local_corr_tiled']"
    assert f"KERNELS {want}" in p.stdout
