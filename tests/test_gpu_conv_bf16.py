"""The split-bf16 direct convolutions with the plain epilogue on the device: every case of tests/bf16_check.py under bf16x3, bf16x3_w,
bf16x6 and bf16x6_w, raw ConvDesc launches through ofx_conv2d (no Winograd operand: nothing leaves the direct kernels).  The oracle,
the case table (with the plan every case reaches, held on the CPU by test_bf16_check_host.py) and the bound are bf16_check.py's.

Per case and precision: every element inside the bound (the worst ratio is printed; the maxima are recorded in the header of
wino_check.py), the NaN guard rows before and after the output and the NaN columns right of an out-slice untouched, a second launch
bit for bit, the pre-split weight format bit-identical to the on-the-fly split wherever the two reach one plan (everywhere but on
the bf16x3 BK = 32 tile, which has no pre-split twin), and a descriptor with a split-K workspace bit-identical to the one without
and the workspace left zero.

Measured on MI355X: all 128 runs pass; the worst |err| / (slope 2^-24 M) is 3.24 for bf16x3 / bf16x3_w (1x1, K = 324, on the BK = 32
tile) against K_DIRECT_BF16X3 = 3.8, and 4.85 for bf16x6 / bf16x6_w (1x5 over two segments on the 128x128 halo patch, one element of
65536; every other case at most 3.69) against K_DIRECT_BF16X6 = 7.3 -- the gate cases' 4.6 did not hold it, wino_check.py has the
table per group and the reason for 1.5 x.  No kernel defect found: a missing lower piece or product would stand at 10 ... 10^4."""
import pytest
import torch

import bf16_check as bc

pytestmark = pytest.mark.gpu

G = bc.GUARD
bits = lambda t: t.contiguous().view(torch.int32)
_results = {}                       # (case name, precision number) -> the output rows of the first launch, on the CPU


def _note(name, ratio):
    """Print a measured ratio (pytest -s shows them; the worst ones are recorded in the header of wino_check.py)."""
    print(f"ratio {name} {float(ratio):.4g}")


def _launch(c, prec, host, ws=True):
    """One ofx_conv2d of case c on fresh device copies of the host buffers -> {name: the buffer afterwards, on the CPU}."""
    from sd_animation_optical_flow_amd import ops
    dev = {k: v.cuda() for k, v in host.items()}
    d = bc.descriptor(c, prec, lambda name: dev[name].data_ptr())
    if not ws:
        d.splitk_ws, d.splitk_ws_bytes = 0, 0
    ops.conv2d_desc(d)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dev.items()}


def _output(c, host, after):
    """Everything but rows [G, G + M) x columns [0, cout) of `out` unchanged -> those rows and columns, [B, Ho, Wo, cout]."""
    Ho, Wo = bc.out_hw(c)
    M, co = c["B"] * Ho * Wo, c["cout"]
    for name, before in host.items():
        a, b = bits(after[name]).clone(), bits(before)
        if name == "out":
            a[G:G + M, :co] = b[G:G + M, :co]
        assert torch.equal(a, b), f"{c['name']}: {name} changed outside the destination"
    return after["out"][G:G + M, :co].reshape(c["B"], Ho, Wo, co)


def _run(c, prec):
    if (c["name"], prec) not in _results:
        host = bc.buffers(c, prec)
        after = _launch(c, prec, host)
        got = _output(c, host, after)
        again = _launch(c, prec, host)
        assert all(torch.equal(bits(after[k]), bits(again[k])) for k in after), f"{c['name']}: a repeat differs"
        if c["extra"].get("ws"):                                         # nothing to split in these arithmetics: the workspace stays out of it
            assert not bool(after["ws"].any())
            bare = _launch(c, prec, host, ws=False)
            assert torch.equal(bits(bare["out"]), bits(after["out"])), f"{c['name']}: differs without the workspace"
        _results[(c["name"], prec)] = got
    return _results[(c["name"], prec)]


@pytest.mark.parametrize("precision", list(bc.PRECISIONS))
@pytest.mark.parametrize("c", bc.CASES, ids=bc.IDS)
def test_split_bf16_convolution_against_the_products_it_forms(cuda, c, precision):
    prec = bc.PRECISIONS[precision]
    r = bc.reference(c["name"], bc.FAMILY[prec])
    got = _run(c, prec)
    assert tuple(got.shape) == tuple(r.out.shape)
    _note(f"{c['name']} {precision} {bc.signature(c, prec)}", bc.ratio(r, got))
    bc.check(r, got, bc.K_of(prec), f"{c['name']} {precision}")
    if precision.endswith("_w") and bc.same_plan(c):                     # the pre-split format: the same bits as the on-the-fly split
        assert torch.equal(bits(got), bits(_run(c, prec - 1))), f"{c['name']}: {precision} differs from {precision[:-2]}"
