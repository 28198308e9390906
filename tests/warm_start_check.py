"""Float64 restatement of the WARM-STARTED RAFT forward (RAFT.forward(flow_init=...), RAFT/core/raft.py:86-144 with :118-119) for both
networks, and a brute-force restatement of forward_interpolate (RAFT/core/utils/utils.py:26-53).

Composed from the existing restatements -- oracle/raft_oracle.py (basic network) and tests/small_raft_check.py (small network) --
without editing either: the encoders, correlation pyramid, lookup and update blocks are theirs; only the state initialisation
differs (coords1 = coords0 + flow_init instead of coords0).  Everything runs in float64 on the CPU.

`forward_interpolate_brute` is the nearest-source search written out in numpy, chunked over output pixels: every pixel (x0, y0) is a
source at (x0 + dx, y0 + dy) in float64, valid iff 0 < x1 < w and 0 < y1 < h; every output pixel takes the flow of the valid source
at the smallest squared distance (dx^2 + dy^2: two products and one add, each rounded once, as numpy evaluates it), ties to the
lowest source index; a field without a valid source is NaN.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

import small_raft_check as SR
from oracle import raft_oracle as RO

Tensor = torch.Tensor


def raft_forward_warm(sd, image1: Tensor, image2: Tensor, flow_init: Tensor, iters: int = 20) -> Tuple[Tensor, Tensor]:
    """The basic network (eval-mode BatchNorm), warm-started: images [B,3,H,W] 0..255 RGB, flow_init [B,2,H/8,W/8] ->
    (flow_low, flow_up) NCHW, float64."""
    sd = RO.to_float64(sd)
    i1 = 2 * (image1.to(torch.float64) / 255.0) - 1.0
    i2 = 2 * (image2.to(torch.float64) / 255.0) - 1.0
    b = i1.shape[0]
    fm = RO.encoder(sd, "fnet", torch.cat([i1, i2], 0), "instance")
    fmap1, fmap2 = fm[:b], fm[b:]
    cn = RO.encoder(sd, "cnet", i1, "batch")
    net, inp = torch.tanh(cn[:, :RO.HDIM]), torch.relu(cn[:, RO.HDIM:RO.HDIM + RO.CDIM])
    _, _, h, w = fmap1.shape
    pyr = RO.corr_pyramid(fmap1, fmap2)
    coords0 = RO.coords_grid(b, h, w, torch.float64)
    coords1 = coords0 + flow_init.to(torch.float64)
    mask = None
    for it in range(iters):
        corr = RO.corr_lookup(pyr, coords1)
        net, mask, delta = RO.update_block(sd, net, inp, corr, coords1 - coords0, want_mask=(it == iters - 1))
        coords1 = coords1 + delta
    flow_low = coords1 - coords0
    return flow_low, RO.upsample_flow(flow_low, mask)


def raft_small_forward_warm(sd, image1: Tensor, image2: Tensor, flow_init: Tensor, iters: int = 20) -> Tuple[Tensor, Tensor]:
    """The small network, warm-started: as `raft_forward_warm`, upflow8 at the end."""
    sd = SR.to64(sd)
    i1 = 2 * (image1.to(torch.float64) / 255.0) - 1.0
    i2 = 2 * (image2.to(torch.float64) / 255.0) - 1.0
    fmap1, fmap2 = SR.encoder(sd, "fnet", i1), SR.encoder(sd, "fnet", i2)
    pyr = SR.corr_pyramid(fmap1, fmap2)
    cnet = SR.encoder(sd, "cnet", i1)
    net, inp = torch.tanh(cnet[:, :SR.HD]), torch.relu(cnet[:, SR.HD:SR.HD + SR.CD])
    b, _, h, w = fmap1.shape
    coords0 = SR.coords_grid(b, h, w)
    coords1 = coords0 + flow_init.to(torch.float64)
    for _ in range(iters):
        corr = SR.corr_lookup(pyr, coords1)
        net, delta = SR.update_block(sd, net, inp, corr, coords1 - coords0)
        coords1 = coords1 + delta
    flow_low = coords1 - coords0
    return flow_low, SR.upflow8(flow_low)


def forward_interpolate_brute(flow: np.ndarray, chunk: int = 512, return_index: bool = False):
    """flow f32 [2,h,w] (the reference's layout) -> f32 [2,h,w]; with return_index also the chosen source index per pixel
    ([h*w] int64, -1 where the field has no valid source)."""
    dx, dy = np.asarray(flow[0], np.float32), np.asarray(flow[1], np.float32)
    h, w = dx.shape
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1 = (x0 + dx).reshape(-1)            # int64 + float32 -> float64, exact
    y1 = (y0 + dy).reshape(-1)
    valid = np.nonzero((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h))[0]
    out = np.full((2, h * w), np.nan, np.float32)
    pick = np.full(h * w, -1, np.int64)
    if valid.size:
        sx, sy = x1[valid], y1[valid]
        qx, qy = x0.reshape(-1).astype(np.float64), y0.reshape(-1).astype(np.float64)
        for p0 in range(0, h * w, chunk):
            ddx = sx[None, :] - qx[p0:p0 + chunk, None]
            ddy = sy[None, :] - qy[p0:p0 + chunk, None]
            d2 = ddx * ddx + ddy * ddy
            pick[p0:p0 + chunk] = valid[np.argmin(d2, axis=1)]        # argmin: the first (lowest-index) minimum
        out[0], out[1] = dx.reshape(-1)[pick], dy.reshape(-1)[pick]
    out = out.reshape(2, h, w)
    return (out, pick) if return_index else out


def nearest_d2(flow: np.ndarray, pick: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """For a chosen source per pixel (index array [h*w]): (d2 of that source, the minimal d2 over valid sources), float64."""
    dx, dy = np.asarray(flow[0], np.float32), np.asarray(flow[1], np.float32)
    h, w = dx.shape
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1, y1 = (x0 + dx).reshape(-1), (y0 + dy).reshape(-1)
    qx, qy = x0.reshape(-1).astype(np.float64), y0.reshape(-1).astype(np.float64)
    valid = np.nonzero((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h))[0]
    dmin = np.empty(h * w)
    for p0 in range(0, h * w, 512):
        ddx = x1[valid][None, :] - qx[p0:p0 + 512, None]
        ddy = y1[valid][None, :] - qy[p0:p0 + 512, None]
        dmin[p0:p0 + 512] = (ddx * ddx + ddy * ddy).min(axis=1)
    cx, cy = x1[pick] - qx, y1[pick] - qy
    return cx * cx + cy * cy, dmin
