"""The oracle and the case table of the GRU gate epilogues in the fp16 arithmetic (igemm_kernel in csrc/conv.hip with OFX_PREC_F16 and
OFX_EPI_GRU_ZR / OFX_EPI_GRU_Q: what `RaftEngine(precision="fp16")` runs its SepConvGRU on; a descriptor asks for them with
OFX_PREC_F16_EPI -- OFX_PREC_F16 itself keeps rejecting every gate epilogue, as it documents).  Not a conftest: imported by name, and
importable without a device.  Layouts, maps, inputs, descriptors and the gates' Lipschitz constants are gru_check.py's, imported.

Cases.  The `basic` rows of gru_check's table -- ZR: in0 = hx, c0 256, Cout 256, an addend, aux_z / aux_rh / aux_h; Q: in0 = rh (ld
128), in1 = hx + 128 (ld 384, c1 128), Cout 128 -- with the 1x5 and the 5x1 filter, on the maps gru_check names as the smallest with
every mask and seam (W = 1x8x16 whole tiles, R = 1x9x17 ragged M and overhanging patches, D = 2x16x16 the batch seam of the vertical
halo), and its `tiny` 72-channel layout (cin % 16 != 0: the general gather).  Every case states the plan it must reach; the plan of
this arithmetic differs from the fp32 one: the automatic choice on these small grids is the 64x64 tile on 8x8 halo patches (BK 16)
where the map is whole patches and the scalar-coordinate schedule at BK 32 where it is not (R: a cover of 2.5), never split-K or the
paired pipelines; a forced BK 16 tile takes the halo patch (overhanging on R), a forced BK 32 tile the scalar-coordinate schedule.

Oracle (the f16_check.py pattern: the oracle absorbs the operand rounding).  The float64 pre-activation of the half-rounded
operands, v = conv(x.half().double(), w.half().double()) + addend, and its magnitude M = conv(|x_h|, |w_h|) + |addend|.  A product of
two fp16 values is exact in fp32, so what is left is the fp32 accumulation -- a term passes through at most K = KH KW Cin additions
-- and the epilogue's two roundings (scale / shift, addend): |v_device - v| <= (K + 2) u M with u = 2^-24, the derived bound of
f16_check.py; nothing in it is measured.  It is carried through the gates by gru_check's Lipschitz constants:
    |z - ref| <= (K + 2) u M / 4 + ACT_ULP,   |r h - ref| <= (K + 2) u M |h| / 4 + ACT_ULP max(|h|, 1),
    |h' - ref| <= (K + 2) u M z + ACT_ULP.
Inputs keep gru_check.reference's condition -- at least 3/4 of the pre-activations with |v| < 2, none reaching 8 -- before AND after
the rounding; `reference` asserts both."""
import functools

import torch

import gru_check as gc

PREC_F16 = 5                                     # include/ofx.h: the arithmetic (what a plan reports) ...
PREC_F16_EPI = PREC_F16 | 256                    # ... and the descriptor value that asks it for the gate epilogues (OFX_PREC_F16_EPI)
ZRQ = (gc.EPI_ZR, gc.EPI_Q)
CASES = []


def _rows(layout, epis, tile, plan, modes, maps):
    """gru_check._rows for this arithmetic, into this module's table.  plan: (bm, bn, bk); modes: per map, or one for all."""
    filts = ("1x5", "5x1") if layout == "basic" else ("3x3",)
    for epi in epis:
        for filt in filts:
            for mp in maps:
                mode = modes[mp] if isinstance(modes, dict) else modes
                bm, bn, bk = plan[mp] if isinstance(plan, dict) else plan
                name = f"{layout}-{gc.EPI_NAME[epi]}-{filt}-f16-" + (f"t{tile}" if tile else "auto") + f"-{mp}"
                CASES.append(dict(name=name, layout=layout, epi=epi, filt=filt, map=mp, prec=PREC_F16_EPI, tile=tile, ws=False,
                                  plan=dict(bm=bm, bn=bn, bk=bk, ks=1, ksplit=1, prec=PREC_F16, mode=mode)))


# automatic: grids far below the chip -> 64x64; 8x8 halo patches where the map is whole ones, else BK 32 and scalar coordinates
_rows("basic", ZRQ, 0, {"W": (64, 64, 16), "R": (64, 64, 32), "D": (64, 64, 16)}, {"W": 2, "R": 1, "D": 2}, "WRD")
# the tiles the plan picks on grids that fill the chip (128x128 for z|r, 128x64 ... for q), on the halo patch, overhanging on R
_rows("basic", ZRQ, 16128128, (128, 128, 16), 2, "WRD")
_rows("basic", ZRQ, 16128064, (128, 64, 16), 2, "WRD")
_rows("basic", ZRQ, 16064064, (64, 64, 16), 2, "WR")
# maps whose cover by patches is too wasteful keep the scalar-coordinate schedule at BK 32: every tile
_rows("basic", ZRQ, 32128128, (128, 128, 32), 1, "RD")
_rows("basic", ZRQ, 32128064, (128, 64, 32), 1, "RW")
_rows("basic", ZRQ, 32064064, (64, 64, 32), 1, "RW")
# 72 channels: the general gather, both chunk lengths
_rows("tiny", (gc.EPI_ZR,), 0, (64, 64, 32), 0, "WR")
_rows("tiny", (gc.EPI_ZR,), 16128064, (128, 64, 16), 0, "WR")
_rows("tiny", (gc.EPI_ZR,), 16064064, (64, 64, 16), 0, "WR")
_rows("tiny", (gc.EPI_Q,), 0, (128, 128, 32), 0, "WR")
_rows("tiny", (gc.EPI_Q,), 16128128, (128, 128, 16), 0, "WR")
IDS = [c["name"] for c in CASES]


def K_of(c):
    """(K + 2) of the derived bound: K = KH KW Cin."""
    kh, kw = gc.FILTERS[c["filt"]]
    return kh * kw * gc.spec(c["layout"], c["epi"], c["filt"])["cin"] + 2


def _unsaturated(v):
    return float((v.abs() < 2).double().mean()), float(v.abs().max())


@functools.lru_cache(maxsize=None)
def reference(layout, epi, filt, mp):
    """gru_check.reference with the operands rounded to half: a gru_check.Ref whose v, mag and out are those of x_h, w_h."""
    base = gc.reference(layout, epi, filt, mp)                           # asserts the input condition on the unrounded operands
    r = gc.Ref()
    r.__dict__.update(base.__dict__)
    r.x, r.w = base.x.half().float(), base.w.half().float()
    assert bool(torch.isfinite(r.x).all()) and bool(torch.isfinite(r.w).all())
    r.v = gc._conv(r.x, r.w, filt, mp) + r.add
    r.mag = gc._conv(r.x.abs(), r.w.abs(), filt, mp) + r.add.abs()
    r.unsaturated, r.vmax = _unsaturated(r.v)
    assert r.unsaturated >= 0.75 and r.vmax < 8, (layout, epi, filt, mp, r.unsaturated, r.vmax)   # ... and on the rounded ones
    r.out = r.gates(r.v)
    return r


def ref_of(c):
    return reference(c["layout"], c["epi"], c["filt"], c["map"])
