"""Float64 restatement of the SMALL RAFT network (raft-small.pth; RAFT/core/raft.py:29-33, :48-56) in plain torch ops.

The yardstick for the native small-network schedule at sizes the committed fixture (tests/golden/raft_small_ref_128x160.npz) does
not cover, in the manner of recurrence_check.py / wino_check.py.  Written from the network's description, not from the reference's
code: SmallEncoder (7x7/s2 stem, three stages of two bottleneck blocks, 1x1 head; InstanceNorm2d without affine for the feature
network, no norm for the context network), all-pairs correlation with D = 128 and a 4-level pyramid, radius-3 lookups, the
SmallUpdateBlock (motion encoder, 3x3 ConvGRU, FlowHead(96, 128)) and upflow8.  Everything runs in float64 on the CPU.

The lookup samples the pyramid with `F.grid_sample(align_corners=True, padding_mode='zeros')`; the alternate (volume-free)
correlation of the reference is the same quantity (a dot product with bilinearly sampled, average-pooled image-2 features equals the
bilinear sample of the pooled volume), so `raft_small_forward(alternate_corr=True)` and the default one are one function here.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
HD, CD, RADIUS, LEVELS = 96, 64, 3, 4


def to64(sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    return {(k[7:] if k.startswith("module.") else k): v.detach().to(torch.float64).cpu()
            for k, v in sd.items() if torch.is_tensor(v) and v.dtype.is_floating_point}


def _conv(sd, key: str, x: Tensor, stride: int = 1) -> Tensor:
    w = sd[key + ".weight"]
    return F.conv2d(x, w, sd[key + ".bias"], stride=stride, padding=(w.shape[2] // 2, w.shape[3] // 2))


def encoder(sd, enc: str, x: Tensor) -> Tensor:
    """SmallEncoder: 'fnet' with instance norm (no affine, eps 1e-5), 'cnet' without any norm.  x: images in [-1, 1]."""
    norm = (lambda t: F.instance_norm(t, eps=1e-5)) if enc == "fnet" else (lambda t: t)
    x = torch.relu(norm(_conv(sd, enc + ".conv1", x, 2)))
    for li, stride in ((1, 1), (2, 2), (3, 2)):
        for bi in (0, 1):
            p = f"{enc}.layer{li}.{bi}"
            s = stride if bi == 0 else 1
            y = torch.relu(norm(_conv(sd, p + ".conv1", x)))
            y = torch.relu(norm(_conv(sd, p + ".conv2", y, s)))
            y = torch.relu(norm(_conv(sd, p + ".conv3", y)))
            if s != 1:
                x = norm(_conv(sd, p + ".downsample.0", x, s))
            x = torch.relu(x + y)
    return _conv(sd, enc + ".conv2", x)


def corr_pyramid(fmap1: Tensor, fmap2: Tensor, levels: int = LEVELS) -> List[Tensor]:
    b, d, h, w = fmap1.shape
    vol = torch.einsum("bdn,bdm->bnm", fmap1.reshape(b, d, h * w), fmap2.reshape(b, d, h * w)) / math.sqrt(d)
    pyr = [vol.reshape(b * h * w, 1, h, w)]
    for _ in range(levels - 1):
        pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
    return pyr


def corr_lookup(pyr: List[Tensor], coords: Tensor, radius: int = RADIUS) -> Tensor:
    """coords [B,2,h,w] (x, y) -> [B, L*(2r+1)^2, h, w]; channel l*(2r+1)^2 + i*(2r+1) + j samples level l at
    (x / 2^l + i - r, y / 2^l + j - r)."""
    b, _, h, w = coords.shape
    n, rd = b * h * w, 2 * radius + 1
    c = coords.permute(0, 2, 3, 1).reshape(n, 1, 1, 2)
    off = torch.arange(-radius, radius + 1, dtype=coords.dtype)
    delta = torch.stack([off.reshape(rd, 1).expand(rd, rd), off.reshape(1, rd).expand(rd, rd)], -1)   # [i, j] = (i - r, j - r)
    outs = []
    for lvl, vol in enumerate(pyr):
        hl, wl = vol.shape[-2:]
        pts = c / 2 ** lvl + delta[None]
        grid = torch.stack([2 * pts[..., 0] / (wl - 1) - 1, 2 * pts[..., 1] / (hl - 1) - 1], -1)
        outs.append(F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(b, h, w, rd * rd))
    return torch.cat(outs, -1).permute(0, 3, 1, 2).contiguous()


def update_block(sd, net: Tensor, inp: Tensor, corr: Tensor, flow: Tensor) -> Tuple[Tensor, Tensor]:
    """SmallUpdateBlock: (net', delta_flow).  No mask head."""
    p = "update_block."
    cor = torch.relu(_conv(sd, p + "encoder.convc1", corr))
    flo = torch.relu(_conv(sd, p + "encoder.convf2", torch.relu(_conv(sd, p + "encoder.convf1", flow))))
    motion = torch.cat([torch.relu(_conv(sd, p + "encoder.conv", torch.cat([cor, flo], 1))), flow], 1)
    x = torch.cat([inp, motion], 1)
    hx = torch.cat([net, x], 1)
    z = torch.sigmoid(_conv(sd, p + "gru.convz", hx))
    r = torch.sigmoid(_conv(sd, p + "gru.convr", hx))
    q = torch.tanh(_conv(sd, p + "gru.convq", torch.cat([r * net, x], 1)))
    net = (1 - z) * net + z * q
    delta = _conv(sd, p + "flow_head.conv2", torch.relu(_conv(sd, p + "flow_head.conv1", net)))
    return net, delta


def coords_grid(b: int, h: int, w: int, dtype=torch.float64) -> Tensor:
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    return torch.stack([xs, ys], 0)[None].repeat(b, 1, 1, 1)


def upflow8(flow: Tensor) -> Tensor:
    return 8 * F.interpolate(flow, size=(8 * flow.shape[2], 8 * flow.shape[3]), mode="bilinear", align_corners=True)


def raft_small_forward(sd, image1: Tensor, image2: Tensor, iters: int = 20, trace: dict = None) -> Tuple[Tensor, Tensor]:
    """RAFT(small).forward(test_mode=True) in float64: images [B,3,H,W] with values 0..255 (RGB) -> (flow_low, flow_up), NCHW."""
    sd = to64(sd)
    i1 = 2 * (image1.to(torch.float64) / 255.0) - 1.0
    i2 = 2 * (image2.to(torch.float64) / 255.0) - 1.0
    fmap1, fmap2 = encoder(sd, "fnet", i1), encoder(sd, "fnet", i2)
    pyr = corr_pyramid(fmap1, fmap2)
    cnet = encoder(sd, "cnet", i1)
    net, inp = torch.tanh(cnet[:, :HD]), torch.relu(cnet[:, HD:HD + CD])
    b, _, h, w = fmap1.shape
    coords0 = coords_grid(b, h, w)
    coords1 = coords0.clone()
    if trace is not None:
        trace.update(fmap1=fmap1, fmap2=fmap2, net=net, inp=inp, pyramid=pyr)
    for _ in range(iters):
        corr = corr_lookup(pyr, coords1)
        net, delta = update_block(sd, net, inp, corr, coords1 - coords0)
        coords1 = coords1 + delta
    flow_low = coords1 - coords0
    return flow_low, upflow8(flow_low)


def nhwc(t: Tensor) -> Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def epe(a: Tensor, b: Tensor, dim: int = -1) -> float:
    return float((a.double() - b.double()).pow(2).sum(dim).sqrt().mean())
