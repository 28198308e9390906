"""The convolution launcher's plan as a recorded function: ofx_conv2d_plan (pure, no device) swept over a product of descriptors
around every gate of the Winograd routes, one SHA-256 per (kernel shape, forced tile, knob setting) slice over the status and every
field of ofx_conv_plan, against tests/golden/conv_plan/sha256.json.  A change to the launcher that is meant to keep the plan
(a refactor of the route choice) shows here exactly; one that is meant to change it re-records the slices it moves:

    python tests/test_conv_plan_golden.py write [DIR]     on the build whose plan is the reference
    python tests/test_conv_plan_golden.py compare [DIR]   on the new one (exit status 1 on a difference)

The OFX_CONV_NO_WINOGRAD* switches are read once per process: each is swept, over a reduced product, in a child of its own.
No GPU: the descriptors carry dummy, aligned, never-dereferenced pointers."""
import ctypes as C
import hashlib
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan")
PTR = 0x10000                       # non-null, 16-byte aligned, never dereferenced
BIG = 1 << 40
EINVAL = -1

KERNELS = {"3x3": (3, 3), "1x5": (1, 5), "5x1": (5, 1), "1x1": (1, 1)}
TILES = (0, 1, 2)                   # the rule, OFX_CONV_TILE_WINOGRAD, OFX_CONV_TILE_WINOGRAD4
KNOBS = ("OFX_CONV_NO_WINOGRAD", "OFX_CONV_NO_WINOGRAD15", "OFX_CONV_NO_WINOGRAD4")
# both sides of each grid gate (1024 / 768 patch x channel-block groups, 256 patches), maps of whole and of ragged patches
BHW = ((1, 16, 32), (4, 64, 96), (16, 64, 96), (63, 64, 96), (64, 64, 96), (256, 16, 32), (8, 64, 128), (16, 68, 120), (2048, 8, 32))
SEGS = ((16, 0), (64, 0), (128, 128), (24, 0), (1760, 0))      # (c0, c1): slabs, two segments, no whole slab, past the fused norm's 1744
COUT = (64, 96, 256)
NORMS = ("none", "both", "mean", "rstd")
EPIS = (0, 1, 2)                    # plain, GRU_ZR, GRU_Q


def _variants(reduced):
    """(stride, act, epi, norm, res, addend, precision, pool): the full product at stride 1 in fp32; the strided, split-bf16 and
    pooled-volume launches, which no Winograd route takes whatever else is set, over the plain epilogue with and without a norm.
    reduced (the knob sweeps): identity activation, norm both or none, no addend."""
    out = []
    for act, epi, norm, res, addend in itertools.product((0, 1), EPIS, NORMS, (0, 1), (0, 1)):
        if reduced and (act or addend or norm in ("mean", "rstd")):
            continue
        out.append((1, act, epi, norm, res, addend, 0, 0))
    if not reduced:
        for act, norm in itertools.product((0, 1), ("none", "both")):
            out.append((2, act, 0, norm, 0, 0, 0, 0))
            out.append((1, act, 0, norm, 0, 0, 1, 0))          # OFX_PREC_BF16X3
        out.append((1, 0, 0, "none", 0, 0, 0, 1))
    return out


def sweep(reduced=False):
    """{slice name: (digest, Counter-like dict of path / status occurrences)} of this process's library and knobs."""
    from sd_animation_optical_flow_amd import _lib
    plan_fn = _lib.lib().ofx_conv2d_plan
    d, p = _lib.ConvDesc(), _lib.ConvPlan()
    dref, pref = C.byref(d), C.byref(p)
    d.in0 = d.w = d.out = d.aux_z = d.aux_rh = d.aux_h = PTR
    variants = _variants(reduced)
    result = {}
    for (kname, (kh, kw)), tile in itertools.product(KERNELS.items(), TILES):
        h = hashlib.sha256()
        seen = {}
        d.KH, d.KW, d.padH, d.padW, d.tile = kh, kw, kh // 2, kw // 2, tile
        for stride, act, epi, norm, res, addend, prec, pool in variants:
            d.stride, d.act, d.epi, d.precision = stride, act, epi, prec
            d.nmean = PTR if norm in ("both", "mean") else None
            d.nrstd = PTR if norm in ("both", "rstd") else None
            d.res = PTR if res else None
            d.addend = PTR if addend else None
            for (B, H, W), (c0, c1), cout in itertools.product(BHW, SEGS, COUT):
                d.B, d.Hin, d.Win = B, H, W
                d.Hout, d.Wout = (H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1
                d.ld0, d.c0, d.ld1, d.c1 = c0, c0, c1, c1
                d.in1 = PTR if c1 else None
                d.Cout = d.ldo = d.ldres = d.ldadd = d.ldh = cout
                # statistics room: none wanted, ample, one float short of what F(4x4,3x3) leaves (one row per 16x32 patch) and
                # of what F(2x2,3x3) leaves (per 8x16 patch; ample for the first)
                short4 = B * (H // 16) * (W // 32) * cout * 2 - 1
                short2 = B * (H // 8) * (W // 16) * cout * 2 - 1
                for cap in ((0,) if pool else (0, BIG, max(short4, 1), max(short2, 1))):
                    for w2, w4 in ((0, 0), (1, 0), (0, 1), (1, 1)):
                        d.wino_w = PTR if w2 else None
                        d.wino4_w = PTR if w4 else None
                        st = plan_fn(dref, cap, pool, pref)
                        if st:
                            h.update(b"%d;" % st)
                            key = "rejected"
                        else:
                            h.update(bytes(p))
                            key = p.path
                        seen[key] = seen.get(key, 0) + 1
        result[f"{kname}/tile{tile}"] = (h.hexdigest(), seen)
    return result


def _child(knob):
    """The reduced sweep in a fresh process with `knob` set (and the other two unset)."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env[knob] = "1"
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), "child"], env=env, stdout=subprocess.PIPE, text=True)


def digests():
    """Every slice: the full sweep under the default knobs here, the reduced one under each switch in a child."""
    assert not any(k in os.environ for k in KNOBS), "the default sweep needs the switches unset"
    children = {knob: _child(knob) for knob in KNOBS}
    out = {f"{name}/default": v for name, v in sweep().items()}
    for knob, proc in children.items():
        text, _ = proc.communicate()
        assert proc.returncode == 0, knob
        out.update({f"{name}/{knob}": tuple(v) for name, v in json.loads(text).items()})
    return out


def test_plan_matches_the_recorded_digests():
    got = digests()
    want = json.load(open(os.path.join(GOLDEN, "sha256.json")))
    assert sorted(got) == sorted(want)
    bad = [name for name in sorted(got) if got[name][0] != want[name]]
    assert not bad, bad
    # the sweep reaches what it is there to hold: every Winograd path often, forced tiles that run and that are rejected, and
    # each switch turning its route off
    total = {}
    for name, (_, seen) in got.items():
        if name.endswith("/default"):
            for k, n in seen.items():
                total[str(k)] = total.get(str(k), 0) + n
    assert all(total.get(str(path), 0) >= 100 for path in (1, 2, 3, 4)), total
    for name in ("3x3/tile1/default", "3x3/tile2/default", "1x5/tile1/default", "5x1/tile1/default"):
        seen = {str(k): n for k, n in got[name][1].items()}
        assert seen.get("rejected", 0) > 0 and set(seen) - {"rejected"}, (name, seen)
    paths = lambda name: {str(k) for k in got[name][1]} - {"rejected"}
    assert paths("3x3/tile0/OFX_CONV_NO_WINOGRAD") == {"0"} and paths("1x5/tile0/OFX_CONV_NO_WINOGRAD") == {"0"}
    assert paths("1x5/tile0/OFX_CONV_NO_WINOGRAD15") == {"0"} and "1" in paths("3x3/tile0/OFX_CONV_NO_WINOGRAD15")
    assert paths("3x3/tile0/OFX_CONV_NO_WINOGRAD4") == {"0", "1"} and "3" in paths("3x3/tile2/OFX_CONV_NO_WINOGRAD4")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    mode = sys.argv[1]
    assert mode in ("write", "compare", "child")
    if mode == "child":
        json.dump(sweep(reduced=True), sys.stdout)
        sys.exit(0)
    golden = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    path = os.path.join(golden, "sha256.json")
    got = digests()
    if mode == "write":
        os.makedirs(golden, exist_ok=True)
        with open(path, "w") as f:
            json.dump({name: v[0] for name, v in sorted(got.items())}, f, indent=1)
            f.write("\n")
        print("wrote", len(got), "digests to", path)
    else:
        want = json.load(open(path))
        bad = [name for name in sorted(set(got) | set(want)) if name not in got or got[name][0] != want.get(name)]
        print(f"{len(got) - len(bad)} / {len(got)} slices identical", bad)
        sys.exit(1 if bad else 0)
