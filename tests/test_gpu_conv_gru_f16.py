"""The GRU gate epilogues in the fp16 arithmetic (OFX_PREC_F16_EPI with OFX_EPI_GRU_ZR / OFX_EPI_GRU_Q) against float64, instantiation by
instantiation: raw ConvDesc launches through ofx_conv2d in the engine's layouts.  The case table, the plan every case must reach
and the oracle -- the float64 gates of the half-rounded operands under the derived bound (K + 2) 2^-24 M, nothing measured -- are
gru_f16_check.py's; buffers, descriptors and the gates' Lipschitz constants are gru_check.py's.

Per case: the plan asserted through ofx_conv2d_plan; the input condition (3/4 of the pre-activations unsaturated, before and after
the rounding); the result inside the bound (the worst |error| / bound is printed); every byte outside the destination untouched
(NaN guard rows around every buffer stay NaN; hx bit-identical after ZR, only columns [0, hd) of rows [0, M) changed after Q); a
second launch bit for bit; and the fp16 arithmetic ran, not the fp32 kernel (some bit differs from the fp32 launch).

Worst |error| / bound per row of the table, measured on MI355X (ZR / Q; all 78 cases pass; profiles/r36_raft_f16_rate.txt, section 2):
    basic  auto 0.0004 / 0.0008    16128128 0.0004 / 0.0006    16128064 0.0004 / 0.0006    16064064 0.0003 / 0.0006
           BK 32 tiles (scalar coordinates) 0.0005 / 0.0008
    tiny   ZR 0.0001, Q 0.0004
(the bound is a worst case over summation orders, K 2^-24 times the sum of magnitudes; a random-sign accumulation sits far inside)"""
import ctypes as C

import pytest
import torch

import gru_check as gc
import gru_f16_check as gf
import wino_check as wc

G = gc.GUARD
bits = lambda t: t.view(torch.int32)


def _guard(body):
    buf = torch.full((body.shape[0] + 2 * G, body.shape[1]), float("nan"))
    buf[G:G + body.shape[0]] = body
    return buf


def _host(c):
    bufs, _ = gc.inputs(c["layout"], c["epi"], c["filt"], c["map"])
    return {k: _guard(v) for k, v in bufs.items()}


def _descriptor(c, ptr, precision):
    d = gc.descriptor(c, ptr)
    d.precision = precision
    return d


def _launch(c, host, wdev, precision=gf.PREC_F16_EPI):
    """One ofx_conv2d of case c on fresh device copies of the guarded host buffers -> {name: the buffer afterwards, on the CPU}."""
    from sd_animation_optical_flow_amd import _lib
    dev = {k: v.cuda() for k, v in host.items()}
    ptr = lambda name: wdev.data_ptr() if name == "w" else dev[name].data_ptr() + 4 * G * dev[name].shape[1]
    d = _descriptor(c, ptr, precision)
    st = _lib.lib().ofx_conv2d(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0, (c["name"], st)
    return {k: v.cpu() for k, v in dev.items()}


def _outputs(c, host, after):
    """The untouched-memory checks, then {output name: [M, hd]} of the launch."""
    s = gc.spec(c["layout"], c["epi"], c["filt"])
    hd = s["hd"]
    M = next(iter(host.values())).shape[0] - 2 * G
    written = {"z": (0, hd), "rh": (0, hd)} if c["epi"] == gc.EPI_ZR else {s["aux_h"][0]: (s["aux_h"][1], s["aux_h"][1] + hd)}
    for name, before in host.items():
        a, b = bits(after[name]).clone(), bits(before)
        if name in written:                                              # only these columns of rows [0, M) may change
            lo, hi = written[name]
            a[G:G + M, lo:hi] = b[G:G + M, lo:hi]
        assert torch.equal(a, b), f"{c['name']}: {name} changed outside the destination (guard rows included)"
    if c["epi"] == gc.EPI_ZR:
        return {"z": after["z"][G:G + M], "rh": after["rh"][G:G + M]}
    name, off = s["aux_h"]
    return {"h": after[name][G:G + M, off:off + hd]}


@pytest.mark.gpu
@pytest.mark.parametrize("c", gf.CASES, ids=gf.IDS)
def test_fp16_gru_epilogue_against_float64(cuda, c):
    from sd_animation_optical_flow_amd import _lib, ops
    # the plan the case is there for (dummy aligned pointers: nothing is read)
    plan = _lib.ConvPlan()
    assert _lib.lib().ofx_conv2d_plan(C.byref(_descriptor(c, lambda name: 0x10000, gf.PREC_F16_EPI)), 0, 0, C.byref(plan)) == 0
    got_plan = dict(bm=plan.bm, bn=plan.bn, bk=plan.bk, ks=plan.ks, ksplit=plan.ksplit, prec=plan.prec, mode=plan.mode)
    assert plan.path == 0 and got_plan == c["plan"], (c["name"], got_plan)

    r = gf.ref_of(c)                                                     # asserts the input condition, before and after rounding
    host = _host(c)
    wdev = ops.pack_conv_weight(gc.inputs(c["layout"], c["epi"], c["filt"], c["map"])[1]).cuda()
    after = _launch(c, host, wdev)
    got = _outputs(c, host, after)
    K, b = gf.K_of(c), r.bounds()
    ratio = max(wc.worst_ratio(got[k], r.out[k], *b[k]) for k in got) / K
    print(f"RATIO {c['name']} {gc.signature(c)} unsaturated {r.unsaturated:.3f} worst |error| / bound {ratio:.4f}")
    gc.check(r, got, K, c["name"])
    again = _launch(c, host, wdev)
    assert all(torch.equal(bits(after[k]), bits(again[k])) for k in after), f"{c['name']}: a repeat differs"
    exact = _outputs(c, host, _launch(c, host, wdev, precision=0))
    assert not all(torch.equal(bits(got[k]), bits(exact[k])) for k in got), f"{c['name']}: the bits of the fp32 kernel"
