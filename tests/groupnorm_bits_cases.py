"""The GroupNorm runs whose output bits are recorded (tools/groupnorm_bits.py, tests/test_gpu_groupnorm_bits.py): `ops.groupnorm` on
every sd_ops_check.GN_CASES entry and on GN_LARGE without and with SiLU, `ops.groupnorm_cat` on every unet_check.GNC_CASES entry.
The shapes and inputs are the ones of tests/test_gpu_sd_ops.py and tests/test_gpu_unet.py; nothing is added here.  Plain data and
input construction: importing this module needs no GPU."""
import hashlib
import os

import numpy as np
import torch

import sd_ops_check as sc
import unet_check as UC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "groupnorm_bits", "sha256.json")


def sha256(t):
    """SHA-256 of a float32 cpu tensor's bytes (C order)."""
    a = np.ascontiguousarray(t.numpy())
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


def _gn(c, inputs, silu):
    def make():
        x, gamma, beta = inputs()
        B, HW, Cn = x.shape
        dev = lambda t: None if t is None else t.cuda()

        def launch(ops):
            xd = x.cuda().view(B, HW, 1, Cn)
            return ops.groupnorm(xd, dev(gamma), dev(beta), c["groups"], sc.GN_EPS, silu, out=xd if c["alias"] else None)
        return launch
    return make


def _large_input():
    """The input of test_groupnorm_apply_takes_its_grid_stride_trip (tests/test_gpu_sd_ops.py)."""
    c = sc.GN_LARGE
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn((1, c["HW"], c["C"]), generator=g) * 2.0 + 0.5
    x = torch.cat([x0, x0.flip(1) * 1.25 - 0.75])
    gamma = torch.randn((c["C"],), generator=g) * 0.5 + 1.0
    beta = torch.randn((c["C"],), generator=g)
    return x, gamma, beta


def _wide(t, pad):
    """t [B,HW,C] -> the same values as a channel slice of a wider device tensor whose other columns hold NaN."""
    B, HW, Cn = t.shape
    w = torch.full((B, 1, HW, Cn + 2 * pad), float("nan"), device="cuda")
    w[..., pad:pad + Cn] = t.cuda().view(B, 1, HW, Cn)
    return w[..., pad:pad + Cn]


def _gnc(c):
    def make():
        x0, x1, e, gamma, beta = UC.gnc_input(c)
        B, HW, C0 = x0.shape

        def launch(ops):
            if c["kind"] == "nan_slices":
                Cn = C0 + x1.shape[2]
                d0, d1 = _wide(x0, 4), _wide(x1, 8)
                de = torch.full((B, Cn + 12), float("nan"), device="cuda")
                de[:, 8:8 + Cn] = e.cuda()
                de = de[:, 8:8 + Cn]
            else:
                d0 = x0.cuda().view(B, 1, HW, C0)
                d1 = None if x1 is None else x1.cuda().view(B, 1, HW, -1)
                de = None if e is None else e.cuda()
            return ops.groupnorm_cat(d0, d1, gamma.cuda(), beta.cuda(), e=de, groups=c["groups"], eps=UC.GN_EPS, silu=c["silu"],
                                     out=d0 if c["kind"] == "alias" else None)
        return launch
    return make


def runs():
    """[(name, make)]: make() builds the case's inputs on the CPU and returns launch(ops), which runs the case once on fresh device
    copies of them (an in-place case overwrites its copy) and returns the output, on the device."""
    out = [("groupnorm/" + c["name"], _gn(c, lambda c=c: sc.gn_input(c), c["silu"])) for c in sc.GN_CASES]
    out += [(f"groupnorm/{sc.GN_LARGE['name']}-silu{int(silu)}", _gn(sc.GN_LARGE, _large_input, silu)) for silu in (False, True)]
    out += [("groupnorm_cat/" + c["name"], _gnc(c)) for c in UC.GNC_CASES]
    return out
