"""The direct kernels' GRU gate epilogues (igemm_kernel with OFX_EPI_GRU_ZR / OFX_EPI_GRU_Q) against float64, instantiation by
instantiation: raw ConvDesc launches through ofx_conv2d in the engine's layouts, no wino_w, so nothing routes to Winograd.  The
oracle, the case table (with the plan every case reaches, held on the CPU by test_conv_gru_host.py) and the bound are gru_check.py's.

Per case: the result inside the bound (the worst ratio is printed), every byte outside the destination untouched (NaN guard rows
around every buffer; hx bit-identical after ZR, only columns [0, hd) of rows [0, M) changed after Q; z, r * h and the addend only
read), a second launch bit for bit, and for split-K the workspace's counters back at zero and a third launch on the workspace as
the kernel left it.  A forced tile whose kernel sums K in another order than the automatic one (gru_check.order_class) must differ
from it in some bit: the intended kernel ran.

Worst |err| / (slope 2^-24 M) per row of the table, measured on MI355X over the row's maps and filters (ZR / Q); the bound is
K_DIRECT = 11 for fp32, K_DIRECT_BF16X3 = 3.8 and K_DIRECT_BF16X6 = 7.3 (wino_check.py; 4.6 when these cases were measured).  All 234 cases pass; no kernel bug found.

    basic fp32   auto (64x64 BK 32, paired) 1.98 / 2.10     + workspace (split-K 4) 1.06 / 1.44     32064064 2.03 / 2.08
                 2032064064 1.98 / 2.10     16064064 2.06 / 2.45     16128128, 16128064, 16256064 (halo patch) 1.65 / 1.59
                 32128128 2.06 / 2.45       32128064 2.03 / 2.08
    small fp32   ZR: auto 1.56, + workspace 0.85, 16128192 / 16128096 / 16128064 1.30, 32128032 1.52
                 Q: auto (128x32), with and without a workspace, 2.85; 16128064 1.48; 32064064 2.85
    tiny fp32    ZR: auto 1.08, + workspace (split-K 3) 1.14, 16128064 1.95.  Q: auto 1.25
    bf16x3 / _w  basic auto (64x64 BK 16, general gather) 1.10 / 1.94; 16128128, 16128064 1.26 / 0.92; small Q auto 1.66
    bf16x6 / _w  basic auto 1.95 / 2.31; 16128128, 16128064 1.54 / 1.62
    (the on-the-fly and the pre-split weight formats gave the same ratios, as did tiles that sum K in the same order)"""
import ctypes as C
import functools

import pytest
import torch

import gru_check as gc
import wino_check as wc

G = gc.GUARD
EINVAL = -1
bits = lambda t: t.view(torch.int32)


def _guard(body, fill=float("nan")):
    buf = torch.full((body.shape[0] + 2 * G, body.shape[1]), fill)
    buf[G:G + body.shape[0]] = body
    return buf


def _launch(c, host, wdev, ws=None, expect=0, **override):
    """One ofx_conv2d of case c on fresh device copies of the guarded host buffers -> {name: the buffer afterwards, on the CPU}."""
    from sd_animation_optical_flow_amd import _lib
    dev = {k: v.cuda() for k, v in host.items()}
    ptr = lambda name: wdev.data_ptr() if name == "w" else dev[name].data_ptr() + 4 * G * dev[name].shape[1]
    d = gc.descriptor(c, ptr, ws.data_ptr() if ws is not None else 0)
    for k, v in override.items():
        setattr(d, k, v)
    st = _lib.lib().ofx_conv2d(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == expect, (c["name"], st)
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
        assert torch.equal(a, b), f"{c['name']}: {name} changed outside the destination"
    if c["epi"] == gc.EPI_ZR:
        return {"z": after["z"][G:G + M], "rh": after["rh"][G:G + M]}
    name, off = s["aux_h"]
    return {"h": after[name][G:G + M, off:off + hd]}


def _host(c):
    bufs, _ = gc.inputs(c["layout"], c["epi"], c["filt"], c["map"])
    return {k: _guard(v) for k, v in bufs.items()}


def _run(c):
    """Launch c, check it against float64 and the memory around it, repeat it -> (outputs, worst ratio)."""
    r, K = gc.ref_of(c), gc.K_of(c["prec"])
    host = _host(c)
    wdev = gc.packed_weight(c).cuda()
    ws = torch.zeros((gc.WS_BYTES,), dtype=torch.uint8, device="cuda") if c["ws"] else None
    after = _launch(c, host, wdev, ws)
    got = _outputs(c, host, after)
    b = r.bounds()
    ratio = max(wc.worst_ratio(got[k], r.out[k], *b[k]) for k in got)
    print(f"RATIO {c['name']} {gc.signature(c)} {ratio:.3f}")
    gc.check(r, got, K, c["name"])
    again = _launch(c, host, wdev, ws)
    assert all(torch.equal(bits(after[k]), bits(again[k])) for k in after), f"{c['name']}: a repeat differs"
    if c["plan"]["ksplit"] > 1:
        assert not bool(ws[:65536].any()), f"{c['name']}: arrival counters not back at zero"
        third = _launch(c, host, wdev, ws)                               # on the workspace as the kernel left it
        assert all(torch.equal(bits(after[k]), bits(third[k])) for k in after), f"{c['name']}: differs on a used workspace"
        assert not bool(ws[:65536].any())
    return got, ratio


def _auto_of(c):
    return next(a for a in gc.CASES if a["tile"] == 0 and not a["ws"] and
                all(a[k] == c[k] for k in ("layout", "epi", "filt", "map", "prec")))


@functools.lru_cache(maxsize=None)
def _auto_outputs(name):
    c = gc.CASES[gc.IDS.index(name)]
    return _launch(c, _host(c), gc.packed_weight(c).cuda())


@pytest.mark.gpu
@pytest.mark.parametrize("c", gc.CASES, ids=gc.IDS)
def test_direct_gru_epilogue_against_float64(cuda, c):
    got, _ = _run(c)
    auto = _auto_of(c)
    if auto is not c and gc.order_class(auto) != gc.order_class(c):      # another summation order: the intended kernel ran
        ref = _outputs(auto, _host(auto), _auto_outputs(auto["name"]))
        assert not all(torch.equal(bits(got[k]), bits(ref[k])) for k in got), c["name"]


@pytest.mark.gpu
def test_a_zr_split_inside_a_sub_tile_is_rejected_before_any_launch(cuda):
    """hd = 48 (Cout 96) is OFX_EINVAL with nothing launched: poisoned aux_z / aux_rh / aux_h stay poisoned.  The same buffers with
    Cout 64 run and pass."""
    POISON = 7.25
    c = gc.CASES[gc.IDS.index("tiny-zr-3x3-p0-auto-W")]
    r = gc.ref_of(c)
    M, hd = r.h.shape[0], r.hd
    host = _host(c)
    for name in ("z", "rh"):                                             # room for the rows of 48 floats a launch would write
        host[name] = torch.full((M + 2 * G, 48), POISON)
    host["hx"][:G], host["hx"][G + M:] = POISON, POISON
    w96 = torch.zeros((96, 9 * 72 + 24), device="cuda")
    after = _launch(c, host, w96, expect=EINVAL, Cout=96)
    assert all(torch.equal(bits(after[k]), bits(host[k])) for k in host)
    # Cout 64: dense rows of hd = 32 floats from the same addresses
    from sd_animation_optical_flow_amd import _lib
    dev = {k: v.cuda() for k, v in host.items()}
    wdev = gc.packed_weight(c).cuda()
    ptr = lambda name: wdev.data_ptr() if name == "w" else dev[name].data_ptr() + (4 * G * dev[name].shape[1] if name not in ("z", "rh") else 0)
    d = gc.descriptor(c, ptr)
    assert _lib.lib().ofx_conv2d(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    flat = {k: dev[k].cpu().reshape(-1) for k in ("z", "rh")}
    got = {k: v[:M * hd].view(M, hd) for k, v in flat.items()}
    gc.check(r, got, wc.K_DIRECT, "hd 32 in the poisoned buffers")
    assert all(bool((v[M * hd:] == POISON).all()) for v in flat.values())  # nothing past row M of the dense [M][32] array
    assert torch.equal(bits(dev["hx"].cpu()), bits(host["hx"])) and torch.equal(bits(dev["gadd"].cpu()), bits(host["gadd"]))
