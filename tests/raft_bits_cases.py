"""The RAFT engine runs whose output bits are recorded (tools/raft_bits.py, tests/test_gpu_raft_bits.py): both networks on seeded
frames and seeded weights, through `RaftEngine`'s public names only, one run per schedule the executor can take -- side streams or
one stream, shared frames, both correlation modes, the split-bf16 modes, warp, warm start, the indexed-pairs call.  A change of how
the executor (csrc/raft_engine.cpp) describes or orders its launches keeps these bits; a change of a kernel's arithmetic, a tile
choice or a route records new ones.

A digest covers flow_up, flow_low and the warped frames where the run returns them, then `engine.buffer(name)` of every intermediate
the forward registers (none for the indexed-pairs call).  Every hashed tensor must be finite: a run asserts that, so a digest never
records NaNs.

The split-volume runs (SPLIT_SIZE: the smallest grid the A-stationary volume kernel takes, at batch sizes that just pass its fill
thresholds) digest their flows and pyramid levels only, and assert once, outside the digest, that the split kernel ran.

OFX_OVERLAP_MAX_M, OFX_NO_EPI_STATS, OFX_LOCAL_CORR_NO_TILED and OFX_VOL_GENERIC are read once per process: the runs of CHILD_GROUPS
go through `child_digests`, one child process per group.  Plain data and input construction: importing this module needs no GPU."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "raft_bits", "sha256.json")
ITERS = 3                            # the kernel-carried fork event needs a second iteration
SIZES = {"": (128, 160), "-72x88": (72, 88)}   # the goldens' size (1/8 grid 16x20); a 9x11 grid with odd tails
PAIRS = ([0, 1, 0, 2], [1, 0, 2, 1])
# The split-plane volume (corr_split.hip) needs w/8 % 16 == 0 and h/8 % 8 == 0: a 16x32 grid, N = 512 in two 256-row groups.  It is
# taken from a fill of 2 * pairs / 256 workgroups per CU of 0.84 (exact fp32 planes) / 0.52 (bf16x6) on: B = 108, B = 68, 96 pairs
SPLIT_SIZE = (128, 256)
SPLIT_PAIRS = ([0, 1, 2, 3, 0, 2] * 16, [1, 0, 3, 1, 3, 0] * 16)
# switch -> value of the child process; the runs of each group are the names under "<switch>=<value>/"
CHILD_GROUPS = {"OFX_OVERLAP_MAX_M=0": ("basic/forward-B2", "basic/shared-image2-B3", "basic/pairs-volume"),
                "OFX_NO_EPI_STATS=1": ("basic/forward-B2",),
                # the per-pixel lookup: it reads the pair map's host arrays and shared flags
                "OFX_LOCAL_CORR_NO_TILED=1": ("basic/alternate_corr-shared-image2-B3", "basic/pairs-local", "small/pairs-local"),
                # the generic GEMM at a shape where the split kernel would otherwise be taken
                "OFX_VOL_GENERIC=1": ("basic/split-volume-fp32-shared-image2-B108",)}


def sha256(tensors):
    """SHA-256 over dtype, shape and bytes (C order) of every tensor, in order; every floating-point tensor must be finite."""
    h = hashlib.sha256()
    for t in tensors:
        assert not t.is_floating_point() or bool(torch.isfinite(t).all()), "a hashed tensor is not finite"
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def frames(seed, n, H, W):
    """uint8 [n,H,W,3] from a CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g)


@functools.lru_cache(maxsize=None)
def _engine(small=False, **kw):
    from sd_animation_optical_flow_amd.raft import RaftEngine
    from sd_animation_optical_flow_amd.weights import random_state_dict
    return RaftEngine(random_state_dict(0, small=small), **kw)


def _buffers(eng, alt):
    """The intermediates a plain forward registers, in a fixed order."""
    names = ["fmap1", "fmap2", "hx", "coords1", "corr"] + (["mask"] if eng.variant == "basic" else [])
    if not alt:
        names += [f"pyr{l}" for l in range(4)]
    return [eng.buffer(n) for n in names]


def _split_ran(launch):
    """One launch under the per-family profile: the split-plane kernel ran -- or, in OFX_VOL_GENERIC's child, did not."""
    from sd_animation_optical_flow_amd import ops
    ops.prof_enable(1)
    try:
        launch()
        families = ops.prof_collect()
    finally:
        ops.prof_enable(0)
    assert ("corr_split_planes" in families) == ("OFX_VOL_GENERIC" not in os.environ), sorted(families)


def _forward(small=False, size="", B=2, shared=None, engine=(), warp=False, want_flow=True, warm=False, split=False, **kw):
    """engine: the RaftEngine's own keywords as (name, value) pairs; kw: `forward`'s.  shared: 'image1' / 'image2' = one frame for
    the whole batch on that side.  split: a split-volume run (see the module's text)."""
    def make():
        H, W = SPLIT_SIZE if split else SIZES[size]
        eng = _engine(small, **dict(engine))
        x = frames(11, 2 * B + 1, H, W).cuda()
        i1 = x[0] if shared == "image1" else x[:B].contiguous()
        i2 = x[B] if shared == "image2" else x[B:2 * B].contiguous()
        args = dict(kw, iters=ITERS, want_low=True)
        if warp:
            args.update(warp_frame=x[2 * B], want_flow=want_flow)
        if warm:                     # the previous run's flow_low through forward_interpolate, as a video chain does
            from sd_animation_optical_flow_amd import ops
            args["flow_init"] = ops.forward_interpolate(eng.forward(i1, i2, **args)[1])

        def launch():
            out = eng.forward(i1, i2, **args)
            if split:
                return list(out) + [eng.buffer(f"pyr{l}") for l in range(4)]
            return [t for t in out if t is not None] + _buffers(eng, bool(kw.get("alternate_corr")))
        if split:
            _split_ran(launch)
        return launch
    return make


def _pairs(small=False, alt=False, warp=False, engine=(), split=False):
    """split: the split-volume run over all four frames and SPLIT_PAIRS."""
    def make():
        H, W = SPLIT_SIZE if split else SIZES[""]
        eng = _engine(small, **dict(engine))
        x = frames(12, 4, H, W).cuda()
        args = dict(iters=ITERS, alternate_corr=alt)
        if warp:
            args.update(warp_frame=x[3], n_warp=2)

        def launch():
            out = eng.forward_pairs(x, *SPLIT_PAIRS, **args) if split else eng.forward_pairs(x[:3].contiguous(), *PAIRS, **args)
            return list(out) if isinstance(out, tuple) else [out]
        if split:
            _split_ran(launch)
        return launch
    return make


def _local_runs():
    """The runs of one process, switches aside: [(name, make)]."""
    out = [(f"basic/forward-B2{sz}", _forward(size=sz)) for sz in SIZES]
    out += [("basic/serial", _forward(serial=True)),
            ("basic/shared-image2-B3", _forward(B=3, shared="image2")),
            ("basic/shared-image1-B2", _forward(shared="image1")),
            ("basic/cnet_norm-batch", _forward(engine=(("cnet_norm", "batch"),))),
            ("basic/separate_stats", _forward(separate_stats=True)),
            ("basic/precision-bf16x3", _forward(engine=(("precision", "bf16x3"),))),
            ("basic/precision-bf16x6", _forward(engine=(("precision", "bf16x6"),))),
            ("basic/volume_precision-bf16x6", _forward(engine=(("volume_precision", "bf16x6"),))),
            ("basic/alternate_corr", _forward(alternate_corr=True)),
            ("basic/alternate_corr-shared-image2-B3", _forward(B=3, shared="image2", alternate_corr=True)),
            ("basic/alternate_corr-shared-image1-B2", _forward(shared="image1", alternate_corr=True)),
            ("basic/split-volume-fp32-shared-image2-B108", _forward(B=108, shared="image2", split=True)),
            ("basic/split-volume-bf16x6-B68", _forward(B=68, engine=(("volume_precision", "bf16x6"),), split=True)),
            ("basic/pairs-split-volume-bf16x6", _pairs(engine=(("volume_precision", "bf16x6"),), split=True)),
            ("basic/warp_frame-no-flow", _forward(warp=True, want_flow=False)),
            ("basic/flow_init", _forward(warm=True))]
    out += [(f"basic/pairs-{'local' if alt else 'volume'}{'-warp' if warp else ''}", _pairs(alt=alt, warp=warp))
            for alt in (False, True) for warp in (False, True)]
    out += [(f"small/forward-B2{sz}", _forward(small=True, size=sz)) for sz in SIZES]
    out += [("small/shared-image2-B3", _forward(small=True, B=3, shared="image2")),
            ("small/shared-image1-B2", _forward(small=True, shared="image1")),
            ("small/alternate_corr", _forward(small=True, alternate_corr=True)),
            ("small/alternate_corr-shared-image2-B3", _forward(small=True, B=3, shared="image2", alternate_corr=True)),
            ("small/warp_frame", _forward(small=True, warp=True)),
            ("small/flow_init", _forward(small=True, warm=True)),
            ("small/pairs-volume", _pairs(small=True)),
            ("small/pairs-local", _pairs(small=True, alt=True)),
            ("small/pairs-volume-warp", _pairs(small=True, warp=True)),
            ("small/pairs-local-warp", _pairs(small=True, alt=True, warp=True))]
    return out


def twice(make):
    """(digest of the first launch, digest of the second)."""
    launch = make()
    return sha256(launch()), sha256(launch())


@functools.lru_cache(maxsize=None)
def child_digests(group):
    """{run name: (first, second)} of one CHILD_GROUPS group, from one child process with the group's switch set."""
    key, value = group.split("=")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), group], env=dict(os.environ, **{key: value}), capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("DIGESTS ")][-1][8:])


def runs():
    """[(name, digests)]: digests() runs the case twice -- in this process, or in its group's child -- and returns the two digests."""
    local = _local_runs()
    out = [(name, functools.partial(twice, make)) for name, make in local]
    for group, names in CHILD_GROUPS.items():
        out += [(f"{group}/{name}", lambda g=group, n=name: tuple(child_digests(g)[n])) for name in names]
    return out


if __name__ == "__main__":           # the child of child_digests: the switch is already in the environment
    sys.path.insert(0, ROOT)
    makes = dict(_local_runs())
    print("DIGESTS " + json.dumps({name: twice(makes[name]) for name in CHILD_GROUPS[sys.argv[1]]}))
