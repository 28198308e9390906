"""The oracle, the case table and the simulated bugs of the direct kernels' GRU gate epilogues (igemm_kernel in csrc/conv.hip with
OFX_EPI_GRU_ZR / OFX_EPI_GRU_Q).  Not a conftest: imported by name, and importable without a device.

Launches under test.  Every case is a descriptor the engine makes (raft_engine.cpp), on the smallest maps that have each mask and
seam, with the plan (tile, chunk length, arithmetic, pipelines, split-K, A-side schedule) it must reach written next to it:

    basic   hd 128, hx rows of 384 [h | motion | inp], gadd rows of 768 [zr1 | q1 | zr2 | q2]; 1x5 (pass 1) and 5x1 (pass 2)
            ZR: in0 = hx, c0 256, Cout 256.  Q: in0 = rh (ld 128), in1 = hx + 128 (ld 384, c1 128), Cout 128
    small   hd 96, hx rows of 256, no addend, 3x3.  ZR: c0 256, Cout 192.  Q: in0 = rh (ld 96), in1 = hx + 96 (c1 160), Cout 96
    tiny    one segment of 72 channels (hd 32 plus 40), 3x3, with an addend: the general gather (cin % 16 != 0).
            ZR: Cout 64.  Q: Cout 32, in0 = [r * h | x] rows of 72, aux_h a buffer of its own with rows of 40

    W = 1x8x16   one 8x16 patch, two 8x8 patches, M = 128: every tile whole
    R = 1x9x17   M = 153: a ragged last M tile on the general / scalar schedules, four overhanging patches on the halo patch
    D = 2x16x16  whole 16x16 patches and a batch seam for the vertical halo

Inputs (those of test_gpu_conv_winograd_sweep.run_gru_case): h = tanh(N), motion = 2 relu(N), inp = N, weights
N * 1.5 / sqrt(cin KH KW), gadd = 0.3 N, z ~ U(0, 1), r * h = 0.5 tanh(N).  A saturated gate hides a wrong pre-activation, so
`reference` asserts of every case that at least 3/4 of the pre-activations have |v| < 2 and none reaches 8.

Oracle.  The float64 pre-activation v = conv(x, w) + addend and its magnitude M = conv(|x|, |w|) + |addend|, carried through the
gates by their Lipschitz constants as in run_gru_case: |z - ref| <= K 2^-24 M / 4 + ACT_ULP, |r h - ref| <= K 2^-24 M |h| / 4 +
ACT_ULP max(|h|, 1), |h' - ref| <= K 2^-24 M z + ACT_ULP.  fp32: K = wino_check.K_DIRECT.  Split-bf16 arithmetics (the f16_check.py
pattern: the oracle absorbs the operand arithmetic): both operands are split on the CPU with torch's round-to-nearest-even bfloat16
cast, hi = bf16(x), lo = bf16(x - hi); the bf16x3 reference is the float64 sum of the three products the kernel forms,
hi hi + hi lo + lo hi, the bf16x6 reference the float64 convolution of the exact operands (its three pieces are exact).  What is
left, the fp32 accumulation on the bf16 matrix cores, is measured: wino_check.K_DIRECT_BF16X3 / K_DIRECT_BF16X6.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import wino_check as wc

EPI_ZR, EPI_Q = 1, 2
EPI_NAME = {EPI_ZR: "zr", EPI_Q: "q"}
FILTERS = {"3x3": (3, 3), "1x5": (1, 5), "5x1": (5, 1)}
MAPS = {"W": (1, 8, 16), "R": (1, 9, 17), "D": (2, 16, 16)}
GUARD = 16                                       # rows before and after every [M][ld] buffer
WS_BYTES = 4 << 20                               # split-K workspace: 64 KiB of counters + 32 tiles x 4 splits x 16 KiB at most
PREC_X3, PREC_X6 = (1, 2), (3, 4)                # OFX_PREC_BF16X3 / _W, OFX_PREC_BF16X6 / _W


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers shared with test_gpu_conv_winograd_sweep.py

def _conv_rows(x, w, kh, kw, rows):
    """x NCHW -> the 'same' correlation at output rows `rows` only, float64, [B, Cout, len(rows), W]."""
    ph, pw = kh // 2, kw // 2
    xp = F.pad(x.double(), (0, 0, ph, ph))
    sl = torch.stack([xp[:, :, y:y + kh] for y in rows], 1)             # [B, R, C, kh, W]
    B, R = sl.shape[:2]
    out = F.conv2d(sl.reshape(B * R, *sl.shape[2:]), w.double(), padding=(0, pw))   # [B R, Cout, 1, W]
    return out.reshape(B, R, -1, x.shape[3]).permute(0, 2, 1, 3)


def _guarded(rows, ld, g, fill=None):
    """[GUARD + rows + GUARD, ld] with NaN guard rows; the body is `fill` or uniform noise."""
    buf = torch.full((rows + 2 * GUARD, ld), float("nan"))
    buf[GUARD:GUARD + rows] = torch.rand((rows, ld), generator=g) if fill is None else fill
    return buf


def _at(buf, ld):   # device pointer of row 0 of a guarded buffer
    return buf.data_ptr() + 4 * GUARD * ld


def _rows_of(t, B, H, W, rows):   # [M][C] -> [B, C, len(rows), W]
    return t.view(B, H, W, -1)[:, rows].permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts: the descriptor of a (layout, epilogue, filter) as numbers and (buffer, column offset) pairs

LAYOUTS = {"basic": dict(hd=128, hx_ld=384, gadd_ld=768), "small": dict(hd=96, hx_ld=256, gadd_ld=0),
           "tiny": dict(hd=32, hx_ld=72, gadd_ld=96)}
GOFF = {"zr1": 0, "q1": 256, "zr2": 384, "q2": 640}


def spec(layout, epi, filt):
    """-> dict: hd, cout, in0 / in1 / add / aux_h as (buffer name, column offset) or None, their row strides, c0, c1."""
    L = LAYOUTS[layout]
    hd, ld = L["hd"], L["hx_ld"]
    s = dict(hd=hd, cout=2 * hd if epi == EPI_ZR else hd, in1=None, ld1=0, c1=0, add=None, ldadd=0, aux_h=("hx", 0), ldh=ld)
    if layout == "basic":
        pass_ = "1" if filt == "1x5" else "2"
        s.update(add=("gadd", GOFF[EPI_NAME[epi] + pass_]), ldadd=L["gadd_ld"])
    if layout == "tiny":
        s.update(add=("gadd", 0 if epi == EPI_ZR else 64), ldadd=L["gadd_ld"])
    if epi == EPI_ZR:
        s.update(in0=("hx", 0), ld0=ld, c0=ld if layout != "basic" else 2 * hd)
    elif layout == "tiny":
        s.update(in0=("xq", 0), ld0=ld, c0=ld, aux_h=("hq", 0), ldh=40)
    else:
        s.update(in0=("rh", 0), ld0=hd, c0=hd, in1=("hx", hd), ld1=ld, c1=(2 * hd if layout == "basic" else ld) - hd)
    s["cin"] = s["c0"] + s["c1"]
    return s


@functools.lru_cache(maxsize=None)
def inputs(layout, epi, filt, mp):
    """-> (bufs, w): the CPU float32 buffers [M, ld] the descriptor names (z / rh of GRU_ZR, its outputs: NaN) and w OIHW."""
    B, H, W = MAPS[mp]
    M = B * H * W
    L, s = LAYOUTS[layout], spec(layout, epi, filt)
    hd, ld = L["hd"], L["hx_ld"]
    seed = 1000 * list(LAYOUTS).index(layout) + 100 * epi + 10 * list(FILTERS).index(filt) + list(MAPS).index(mp)
    g = torch.Generator().manual_seed(seed)
    n = lambda c: torch.randn((M, c), generator=g)
    rest = ld - hd                                                       # [h | motion | inp], motion the first half of the rest
    hx = torch.cat([torch.tanh(n(hd)), torch.relu(n(rest // 2)) * 2.0, n(rest - rest // 2)], 1)
    bufs = {"hx": hx}
    if L["gadd_ld"]:
        bufs["gadd"] = n(L["gadd_ld"]) * 0.3
    kh, kw = FILTERS[filt]
    w = torch.randn((s["cout"], s["cin"], kh, kw), generator=g) * (1.5 / np.sqrt(s["cin"] * kh * kw))
    if epi == EPI_ZR:
        bufs["z"] = torch.full((M, hd), float("nan"))
        bufs["rh"] = torch.full((M, hd), float("nan"))
    else:
        bufs["z"] = torch.rand((M, hd), generator=g)
        rh = torch.tanh(n(hd)) * 0.5
        if layout == "tiny":
            bufs["xq"] = torch.cat([rh, hx[:, hd:]], 1)
            bufs["hq"] = torch.cat([hx[:, :hd], 100.0 + torch.rand((M, 40 - hd), generator=g)], 1)
            del bufs["hx"]
        else:
            bufs["rh"] = rh
    return bufs, w


def _seg(bufs, ref, c):
    return bufs[ref[0]][:, ref[1]:ref[1] + c]


def _nchw(t, mp):
    B, H, W = MAPS[mp]
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _conv(x_mc, w, filt, mp):
    """[M, cin] (any float dtype) x OIHW -> float64 [M, cout]."""
    kh, kw = FILTERS[filt]
    out = _conv_rows(_nchw(x_mc, mp), w, kh, kw, range(MAPS[mp][1]))
    return out.permute(0, 2, 3, 1).reshape(x_mc.shape[0], -1)


def split2(t):
    """fp32 -> (hi, lo) float32 tensors holding bf16 values: hi = bf16(x), lo = bf16(x - hi), round-to-nearest-even both times."""
    hi = t.float().bfloat16().float()
    return hi, (t.float() - hi).bfloat16().float()


def split3(t):
    hi, _ = split2(t)
    r1 = t.float() - hi
    mid = r1.bfloat16().float()
    return hi, mid, (r1 - mid).bfloat16().float()


def split_weight_bits(packed):
    """The format of ops.split_conv_weight, restated: int16 [n / 4, 8], four hi then four lo per group of four consecutive k."""
    hi, lo = split2(packed.reshape(-1, 4))
    return torch.cat([hi.bfloat16().view(torch.int16), lo.bfloat16().view(torch.int16)], 1)


def split_weight3_bits(packed):
    """The format of ops.split_conv_weight3: n floats of [hi x4 | mid x4] groups, then n / 2 floats of [lo x4] groups (as int16)."""
    hi, mid, lo = (p.bfloat16().view(torch.int16) for p in split3(packed.reshape(-1, 4)))
    return torch.cat([torch.cat([hi, mid], 1).reshape(-1), lo.reshape(-1)])


class Ref:
    """The float64 side of one (layout, epilogue, filter, map, arithmetic class): x [M, cin], w, addend, v, mag, h, z_in."""

    def gates(self, v):
        """The epilogue in float64 on a pre-activation v [M, cout] -> {output name: [M, hd]}."""
        hd = self.hd
        if self.epi == EPI_ZR:
            s = torch.sigmoid(v)
            return {"z": s[:, :hd], "rh": s[:, hd:] * self.h}
        return {"h": (1 - self.z_in) * self.h + self.z_in * torch.tanh(v)}

    def bounds(self):
        """{output name: (magnitude, slope, extra)} of wino_check.check."""
        hd, h = self.hd, self.h
        if self.epi == EPI_ZR:   # sigmoid' <= 1/4 carries the pre-activation bound to z and, times |h|, to r * h
            return {"z": (self.mag[:, :hd], 0.25, wc.ACT_ULP), "rh": (self.mag[:, hd:], 0.25 * h.abs(), wc.ACT_ULP * h.abs().clamp_min(1.0))}
        return {"h": (self.mag, self.z_in, wc.ACT_ULP)}                  # tanh' <= 1, weighted by z


def pre_activation(r, x=None, w=None, add=None, terms=("hh", "hl", "lh")):
    """v of Ref r in float64 with some of its operands replaced (the simulated bugs); terms: the bf16x3 products kept."""
    x = r.x if x is None else x
    w = r.w if w is None else w
    add = r.add if add is None else add
    if r.x3:
        (xh, xl), (wh, wl) = split2(x), split2(w)
        pairs = {"hh": (xh, wh), "hl": (xh, wl), "lh": (xl, wh)}
        acc = sum(_conv(*pairs[t], r.filt, r.mp) for t in terms)
    else:
        acc = _conv(x, w, r.filt, r.mp)
    return acc + add


@functools.lru_cache(maxsize=None)
def reference(layout, epi, filt, mp, x3=False):
    bufs, w = inputs(layout, epi, filt, mp)
    s = spec(layout, epi, filt)
    r = Ref()
    r.layout, r.epi, r.filt, r.mp, r.x3, r.hd, r.spec = layout, epi, filt, mp, x3, s["hd"], s
    r.x = torch.cat([_seg(bufs, s["in0"], s["c0"])] + ([_seg(bufs, s["in1"], s["c1"])] if s["in1"] else []), 1)
    r.w = w
    M = r.x.shape[0]
    r.add = _seg(bufs, s["add"], s["cout"]).double() if s["add"] else torch.zeros((M, s["cout"]), dtype=torch.float64)
    r.h = _seg(bufs, s["aux_h"], s["hd"]).double()
    r.z_in = bufs["z"].double() if epi == EPI_Q else None
    r.v = pre_activation(r)
    r.mag = _conv(r.x.abs(), w.abs(), filt, mp) + r.add.abs()
    # a saturated gate hides a wrong pre-activation: a condition of every case, not a tolerance
    r.unsaturated, r.vmax = float((r.v.abs() < 2).double().mean()), float(r.v.abs().max())
    assert r.unsaturated >= 0.75 and r.vmax < 8, (layout, epi, filt, mp, r.unsaturated, r.vmax)
    r.out = r.gates(r.v)
    return r


def K_of(prec):
    return wc.K_DIRECT if prec == 0 else wc.K_DIRECT_BF16X3 if prec in PREC_X3 else wc.K_DIRECT_BF16X6


def violates(r, got, K):
    """Any element of any output of `got` ({name: [M, hd]}) outside the bound."""
    b = r.bounds()
    return any(bool(wc.violations(got[k], r.out[k], b[k][0], K, b[k][1], b[k][2]).any()) for k in r.out)


def check(r, got, K, what):
    """Assert the bound of every output and return the worst ratio."""
    b = r.bounds()
    return max(wc.check(got[k], r.out[k], b[k][0], K, f"{what} {k}", b[k][1], b[k][2]) for k in r.out)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table

def _plan(bm, bn, bk, ks=1, ksplit=1):
    return dict(bm=bm, bn=bn, bk=bk, ks=ks, ksplit=ksplit)


CASES = []


def _rows(layout, epis, prec, tile, ws, plan, modes, maps=None):
    """One row of the table: every (epilogue, filter, map) of it.  modes: the A-side schedule per map (or one for all)."""
    filts = ("1x5", "5x1") if layout == "basic" else ("3x3",)
    for epi in epis:
        for filt in filts:
            for mp in (maps or (modes if isinstance(modes, dict) else "WR")):
                mode = modes[mp] if isinstance(modes, dict) else modes
                name = f"{layout}-{EPI_NAME[epi]}-{filt}-p{prec}-" + (f"t{tile}" if tile else "auto") + ("-ws" if ws else "") + f"-{mp}"
                CASES.append(dict(name=name, layout=layout, epi=epi, filt=filt, map=mp, prec=prec, tile=tile, ws=ws,
                                  plan=dict(plan, prec=prec, mode=mode)))


ZRQ = (EPI_ZR, EPI_Q)
_rows("basic", ZRQ, 0, 0, False, _plan(64, 64, 32, ks=2), 1, "WRD")
_rows("basic", ZRQ, 0, 0, True, _plan(64, 64, 32, ksplit=4), {"W": 2, "R": 1, "D": 2})
_rows("basic", ZRQ, 0, 32064064, False, _plan(64, 64, 32), {"W": 2, "R": 1, "D": 2})
_rows("basic", ZRQ, 0, 2032064064, False, _plan(64, 64, 32, ks=2), 1, "WRD")
_rows("basic", ZRQ, 0, 16064064, False, _plan(64, 64, 16), 1, "WRD")
_rows("basic", ZRQ, 0, 16128128, False, _plan(128, 128, 16), 2, "WRD")
_rows("basic", ZRQ, 0, 16128064, False, _plan(128, 64, 16), 2, "WRD")
_rows("basic", ZRQ, 0, 16256064, False, _plan(256, 64, 16), 2, "DR")
_rows("basic", ZRQ, 0, 32128128, False, _plan(128, 128, 32), 1, "RD")
_rows("basic", ZRQ, 0, 32128064, False, _plan(128, 64, 32), 1, "RW")
_rows("small", (EPI_ZR,), 0, 0, False, _plan(64, 64, 32, ks=2), 1)           # 3 N tiles, the z | r boundary inside tile 1
_rows("small", (EPI_ZR,), 0, 0, True, _plan(64, 64, 32, ksplit=4), {"W": 2, "R": 1})
_rows("small", (EPI_ZR,), 0, 16128192, False, _plan(128, 192, 16), 2)        # one N tile
_rows("small", (EPI_ZR,), 0, 16128096, False, _plan(128, 96, 16), 2)         # a z tile and an r tile
_rows("small", (EPI_ZR,), 0, 16128064, False, _plan(128, 64, 16), 2)
_rows("small", (EPI_ZR,), 0, 32128032, False, _plan(128, 32, 32), 1)
_rows("small", (EPI_Q,), 0, 0, False, _plan(128, 32, 32), 1)
_rows("small", (EPI_Q,), 0, 0, True, _plan(128, 32, 32), 1)                  # whatever the workspace
_rows("small", (EPI_Q,), 0, 16128064, False, _plan(128, 64, 16), 2)
_rows("small", (EPI_Q,), 0, 32064064, False, _plan(64, 64, 32), {"W": 2, "R": 1})
_rows("tiny", (EPI_ZR,), 0, 0, False, _plan(64, 64, 32, ks=2), 0)
_rows("tiny", (EPI_ZR,), 0, 0, True, _plan(64, 64, 32, ksplit=3), 0)
_rows("tiny", (EPI_ZR,), 0, 16128064, False, _plan(128, 64, 16), 0)
_rows("tiny", (EPI_Q,), 0, 0, False, _plan(128, 32, 32), 0)
for _p in (1, 2, 3, 4):
    _rows("basic", ZRQ, _p, 0, False, _plan(64, 64, 16), 0)
    _rows("basic", ZRQ, _p, 16128128, False, _plan(128, 128, 16), 2)
    _rows("basic", ZRQ, _p, 16128064, False, _plan(128, 64, 16), 2)
_rows("small", (EPI_Q,), 1, 0, False, _plan(128, 128, 16), {"W": 2, "R": 0})   # 96 of 128 columns
IDS = [c["name"] for c in CASES]


def masked(c):
    """Whether some tile of the case runs the FULL == false epilogue: a ragged last M tile, or (halo patch) overhanging patches."""
    B, H, W = MAPS[c["map"]]
    p = c["plan"]
    if p["mode"] == 2:
        ph, pw = (16, 16) if p["bm"] == 256 else (8, 16) if p["bm"] == 128 else (8, 8)
        return bool(H % ph or W % pw)
    return bool((B * H * W) % p["bm"])


def signature(c):
    p = c["plan"]
    return (c["epi"], p["bm"], p["bn"], p["bk"], p["prec"], p["ks"], p["ksplit"] > 1, p["mode"], masked(c))


def covered():
    """The set of (epi, bm, bn, bk, prec, ks, ksplit > 1, mode, masked) the table reaches."""
    return {signature(c) for c in CASES}


def order_class(c):
    """What fixes the order in which a case's kernel sums K (fp32 MFMA: an fmaf chain in that order).  Two cases of one reference
    whose classes differ cannot give the same bits by construction; two of one class may."""
    p = c["plan"]
    return (p["prec"], p["ks"], p["ksplit"], p["mode"] == 2, p["bk"] if p["mode"] == 2 else 0)


def ref_of(c):
    return reference(c["layout"], c["epi"], c["filt"], c["map"], c["prec"] in PREC_X3)


def descriptor(c, ptr, ws=0):
    """The case's ConvDesc.  ptr(buffer name) -> the address of its row 0; ws: the address of WS_BYTES of split-K workspace."""
    from sd_animation_optical_flow_amd import _lib
    s = spec(c["layout"], c["epi"], c["filt"])
    B, H, W = MAPS[c["map"]]
    kh, kw = FILTERS[c["filt"]]
    at = lambda ref: ptr(ref[0]) + 4 * ref[1]
    d = _lib.ConvDesc()
    d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, H, W, H, W, s["cout"]
    d.KH, d.KW, d.stride, d.padH, d.padW = kh, kw, 1, kh // 2, kw // 2
    d.in0, d.ld0, d.c0 = at(s["in0"]), s["ld0"], s["c0"]
    if s["in1"]:
        d.in1, d.ld1, d.c1 = at(s["in1"]), s["ld1"], s["c1"]
    if s["add"]:
        d.addend, d.ldadd = at(s["add"]), s["ldadd"]
    d.aux_h, d.ldh = at(s["aux_h"]), s["ldh"]
    d.aux_z = ptr("z")
    if c["epi"] == EPI_ZR:
        d.aux_rh = ptr("rh")
    d.w = ptr("w")
    d.act, d.epi, d.tile, d.precision = 0, c["epi"], c["tile"], c["prec"]
    if c["ws"]:
        d.splitk_ws, d.splitk_ws_bytes = ws, WS_BYTES
    return d


def packed_weight(c):
    """The weight operand of the case's arithmetic (CPU): packed fp32, or the pre-split formats of the _W precisions."""
    from sd_animation_optical_flow_amd import ops
    wp = ops.pack_conv_weight(inputs(c["layout"], c["epi"], c["filt"], c["map"])[1])
    return ops.split_conv_weight(wp) if c["prec"] == 2 else ops.split_conv_weight3(wp) if c["prec"] == 4 else wp


# ---------------------------------------------------------------------------------------------------------------------------------
# simulated kernel bugs, each applied to the float64 result

def _k_masked(r, keep):
    """w with the taps of packed index k = (ky KW + kx) cin + c dropped where not keep(k)."""
    co, ci, kh, kw = r.w.shape
    wk = r.w.permute(0, 2, 3, 1).reshape(co, -1).clone()
    k = torch.arange(wk.shape[1])
    wk[:, ~keep(k)] = 0
    return wk.reshape(co, kh, kw, ci).permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def _v_bug(key, kind, param):
    r = reference(*key)
    if kind == "k_range":       # the last of `param` splits' K range (whole 32-wide chunks) missing
        nk = -(-(r.w[0].numel()) // 32)
        k0 = 32 * (-(-nk // param)) * (param - 1)
        return pre_activation(r, w=_k_masked(r, lambda k: k < k0))
    if kind == "odd_chunks":    # the second pipeline's half: the odd 32-wide chunks
        return pre_activation(r, w=_k_masked(r, lambda k: (k // 32) % 2 == 0))
    if kind == "addend":        # the addend from another gadd offset
        bufs, _ = inputs(*key[:4])
        name, off = r.spec["add"]
        other = {0: 384, 384: 0, 256: 640, 640: 256}[off] if r.layout == "basic" else (32 if off == 0 else 0)
        return pre_activation(r, add=bufs[name][:, other:other + r.spec["cout"]].double())
    if kind == "terms":
        return pre_activation(r, terms=param)
    raise KeyError(kind)


def simulated_bugs(c):
    """{bug name: outputs} for every simulated bug that applies to case c."""
    r = ref_of(c)
    key = (c["layout"], c["epi"], c["filt"], c["map"], r.x3)
    p, hd = c["plan"], r.hd
    B, H, W = MAPS[c["map"]]
    M = B * H * W
    bugs = {}
    if c["epi"] == EPI_ZR:
        t0 = (hd // p["bn"]) * p["bn"]
        if hd % p["bn"]:        # z and r halves exchanged inside the N tile [t0, t0 + bn) that straddles them
            n = min(hd - t0, t0 + p["bn"] - hd, hd)
            s = torch.sigmoid(r.v)
            z, rh = r.out["z"].clone(), r.out["rh"].clone()
            z[:, hd - n:] = s[:, hd:hd + n]
            rh[:, :n] = s[:, hd - n:hd] * r.h[:, :n]
            bugs["zr_exchanged_in_the_straddling_tile"] = {"z": z, "rh": rh}
        bufs, _ = inputs(*key[:4])
        name, off = r.spec["aux_h"]                                     # r * h formed with h[n] instead of h[n - hd]
        bugs["rh_with_h_of_column_n"] = {"z": r.out["z"], "rh": torch.sigmoid(r.v[:, hd:]) * bufs[name][:, off + hd:off + 2 * hd].double()}
    else:
        zn = torch.roll(r.z_in, -1, 0)                                   # z of the next row
        bugs["z_of_the_next_row"] = {"h": (1 - zn) * r.h + zn * torch.tanh(r.v)}
    if p["ksplit"] > 1:
        bugs["splitk_partial_dropped"] = r.gates(_v_bug(key, "k_range", p["ksplit"]))
    if p["ks"] == 2:
        bugs["odd_k_chunks_dropped"] = r.gates(_v_bug(key, "odd_chunks", 0))
    if r.spec["add"]:
        bugs["addend_at_the_wrong_offset"] = r.gates(_v_bug(key, "addend", 0))
    if masked(c):               # nothing written on the rows of the ragged tile / on the pixels of the overhanging patches
        rows = torch.zeros((B, H, W), dtype=torch.bool)
        if p["mode"] == 2:
            ph, pw = (16, 16) if p["bm"] == 256 else (8, 16)
            rows[:, (H // ph) * ph:], rows[:, :, (W // pw) * pw:] = True, True
        else:
            rows.view(-1)[(M // p["bm"]) * p["bm"]:] = True
        rows = rows.view(-1, 1)
        old = {"h": r.h} if c["epi"] == EPI_Q else {"z": torch.full_like(r.h, float("nan")), "rh": torch.full_like(r.h, float("nan"))}
        bugs["unwritten_on_the_masked_rows"] = {k: torch.where(rows, old[k], v) for k, v in r.out.items()}
    if r.x3:
        bugs["hi_lo_dropped"] = r.gates(_v_bug(key, "terms", ("hh", "lh")))
        bugs["lo_hi_dropped"] = r.gates(_v_bug(key, "terms", ("hh", "hl")))
    return bugs
