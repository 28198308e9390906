"""Checkpoint loading for the flow network.

The reference loads `RAFT/models/raft-things.pth` into `DataParallel(RAFT)` (ofgen.py:63-68); that file
is not shipped with the reference, so besides `load_checkpoint` this module offers
`random_state_dict(seed)`: seeded weights with the reference's exact `state_dict()` key set, used by
bench.py and the demos when no checkpoint is available (timing is weight-independent).
`random_state_dict(seed, small=True)` does the same for the small network (`raft-small.pth`,
RAFT/core/raft.py:29-33), and `raft_variant(state_dict)` tells the two key sets apart.
"""
from __future__ import annotations

import math
import os
from typing import Dict

import torch

_ENC_CONVS = [("conv1", (64, 3, 7, 7))]
_cin = 64
for _li, (_dim, _stride) in enumerate([(64, 1), (96, 2), (128, 2)], start=1):
    _ENC_CONVS.append((f"layer{_li}.0.conv1", (_dim, _cin, 3, 3)))
    _ENC_CONVS.append((f"layer{_li}.0.conv2", (_dim, _dim, 3, 3)))
    if _stride != 1:
        _ENC_CONVS.append((f"layer{_li}.0.downsample.0", (_dim, _cin, 1, 1)))
    _ENC_CONVS.append((f"layer{_li}.1.conv1", (_dim, _dim, 3, 3)))
    _ENC_CONVS.append((f"layer{_li}.1.conv2", (_dim, _dim, 3, 3)))
    _cin = _dim

_BN = [("norm1", 64)]
for _li, (_dim, _stride) in enumerate([(64, 1), (96, 2), (128, 2)], start=1):
    for _bi in (0, 1):
        _BN += [(f"layer{_li}.{_bi}.norm1", _dim), (f"layer{_li}.{_bi}.norm2", _dim)]
    if _stride != 1:
        _BN.append((f"layer{_li}.0.norm3", _dim))

_UPDATE = [
    ("encoder.convc1", (256, 324, 1, 1)), ("encoder.convc2", (192, 256, 3, 3)),
    ("encoder.convf1", (128, 2, 7, 7)), ("encoder.convf2", (64, 128, 3, 3)),
    ("encoder.conv", (126, 256, 3, 3)),
    ("gru.convz1", (128, 384, 1, 5)), ("gru.convr1", (128, 384, 1, 5)), ("gru.convq1", (128, 384, 1, 5)),
    ("gru.convz2", (128, 384, 5, 1)), ("gru.convr2", (128, 384, 5, 1)), ("gru.convq2", (128, 384, 5, 1)),
    ("flow_head.conv1", (256, 128, 3, 3)), ("flow_head.conv2", (2, 256, 3, 3)),
    ("mask.0", (256, 128, 3, 3)), ("mask.2", (576, 256, 1, 1)),
]


# the small network (RAFT/core/raft.py:29-33, :48-51): SmallEncoder (extractor.py:195-267) with bottleneck blocks
# (extractor.py:60-116) and no norm parameters ('instance' without affine / 'none'), SmallUpdateBlock (update.py:62-112)
_SMALL_ENC_CONVS = [("conv1", (32, 3, 7, 7))]
_cin = 32
for _li, (_dim, _stride) in enumerate([(32, 1), (64, 2), (96, 2)], start=1):
    for _bi in (0, 1):
        _ci = _cin if _bi == 0 else _dim
        _SMALL_ENC_CONVS += [(f"layer{_li}.{_bi}.conv1", (_dim // 4, _ci, 1, 1)), (f"layer{_li}.{_bi}.conv2", (_dim // 4, _dim // 4, 3, 3)),
                             (f"layer{_li}.{_bi}.conv3", (_dim, _dim // 4, 1, 1))]
        if _bi == 0 and _stride != 1:
            _SMALL_ENC_CONVS.append((f"layer{_li}.0.downsample.0", (_dim, _cin, 1, 1)))
    _cin = _dim
_SMALL_OUT = {"fnet": 128, "cnet": 96 + 64}

_SMALL_UPDATE = [
    ("encoder.convc1", (96, 196, 1, 1)), ("encoder.convf1", (64, 2, 7, 7)), ("encoder.convf2", (32, 64, 3, 3)),
    ("encoder.conv", (80, 128, 3, 3)),
    ("gru.convz", (96, 242, 3, 3)), ("gru.convr", (96, 242, 3, 3)), ("gru.convq", (96, 242, 3, 3)),
    ("flow_head.conv1", (128, 96, 3, 3)), ("flow_head.conv2", (2, 128, 3, 3)),
]


def _param_shapes(small: bool) -> Dict[str, tuple]:
    """{key: shape} of the floating-point parameters of the network's `state_dict()` (no BatchNorm counters)."""
    out: Dict[str, tuple] = {}
    if small:
        for enc in ("fnet", "cnet"):
            for name, shp in _SMALL_ENC_CONVS + [("conv2", (_SMALL_OUT[enc], 96, 1, 1))]:
                out[f"{enc}.{name}.weight"], out[f"{enc}.{name}.bias"] = shp, shp[:1]
        for name, shp in _SMALL_UPDATE:
            out[f"update_block.{name}.weight"], out[f"update_block.{name}.bias"] = shp, shp[:1]
        return out
    for enc in ("fnet", "cnet"):
        for name, shp in _ENC_CONVS + [("conv2", (256, 128, 1, 1))]:
            out[f"{enc}.{name}.weight"], out[f"{enc}.{name}.bias"] = shp, shp[:1]
    for name, ch in _BN:
        keys = [f"cnet.{name}"] + ([f"cnet.{name[:-5]}downsample.1"] if name.endswith("norm3") else [])
        for k in keys:
            for f in ("weight", "bias", "running_mean", "running_var"):
                out[f"{k}.{f}"] = (ch,)
    for name, shp in _UPDATE:
        out[f"update_block.{name}.weight"], out[f"update_block.{name}.bias"] = shp, shp[:1]
    return out


def raft_variant(state_dict: Dict[str, torch.Tensor]) -> str:
    """'basic' (raft-things.pth) or 'small' (raft-small.pth) from the checkpoint's key set (`module.` prefixes and BatchNorm
    `num_batches_tracked` counters are accepted).  The reference picks the network with `args.small` (RAFT/core/raft.py:29-56); here
    the checkpoint itself says which one it holds.  A dict that is neither exactly -- keys of both networks, or keys missing -- raises
    ValueError naming the missing keys and the extra ones (keys of the other network)."""
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
    keys = {k for k in sd if not k.endswith("num_batches_tracked")}
    small = "update_block.gru.convz.weight" in keys and "fnet.layer1.0.conv3.weight" in keys
    shapes = _param_shapes(small)
    want, other = set(shapes), set(_param_shapes(not small))
    # (keys of neither network are ignored, as the engine ignores them)
    missing, extra = sorted(want - keys), sorted((keys & other) - want)
    shaped = sorted(k for k in want & keys if hasattr(sd[k], "shape") and tuple(sd[k].shape) != shapes[k])
    if missing or extra or shaped:
        def show(ks):
            return ", ".join(ks[:6]) + (f" (+{len(ks) - 6} more)" if len(ks) > 6 else "") if ks else "none"
        raise ValueError(f"not a RAFT {'small' if small else 'basic'} state_dict: missing keys: {show(missing)}; extra keys: {show(extra)}"
                         + (f"; keys of another shape: {show(shaped)}" if shaped else ""))
    return "small" if small else "basic"


def random_state_dict(seed: int = 0, small: bool = False) -> Dict[str, torch.Tensor]:
    """Seeded weights for the basic (non-small) RAFT: Kaiming-normal(fan_out) encoder convolutions
    (RAFT/core/extractor.py:150-152), uniform(+-1/sqrt(fan_in)) elsewhere, non-trivial BatchNorm
    running statistics for the context encoder.
    small=True: the small network's exact key set and shapes (106 keys, 990,162 floats; no norm parameters at all),
    Kaiming-normal(fan_out) encoder convolutions as extractor.py:240-242 initialises them, uniform(+-1/sqrt(fan_in)) elsewhere."""
    if small:
        return _random_small(int(seed))
    g = torch.Generator().manual_seed(int(seed))
    sd: Dict[str, torch.Tensor] = {}

    def uni(shape, bound):
        return (torch.rand(shape, generator=g) * 2.0 - 1.0) * bound

    for enc in ("fnet", "cnet"):
        for name, (co, ci, kh, kw) in _ENC_CONVS:
            sd[f"{enc}.{name}.weight"] = torch.randn((co, ci, kh, kw), generator=g) * math.sqrt(2.0 / (co * kh * kw))
            sd[f"{enc}.{name}.bias"] = uni((co,), 1.0 / math.sqrt(ci * kh * kw))
        sd[f"{enc}.conv2.weight"] = torch.randn((256, 128, 1, 1), generator=g) * math.sqrt(2.0 / 256)
        sd[f"{enc}.conv2.bias"] = uni((256,), 1.0 / math.sqrt(128))
    for name, ch in _BN:
        w = 0.8 + 0.4 * torch.rand((ch,), generator=g)
        b = 0.1 * torch.randn((ch,), generator=g)
        rm = 0.1 * torch.randn((ch,), generator=g)
        rv = 0.5 + torch.rand((ch,), generator=g)
        keys = [f"cnet.{name}"]
        if name.endswith("norm3"):
            keys.append(f"cnet.{name[:-5]}downsample.1")
        for k in keys:
            sd[k + ".weight"], sd[k + ".bias"] = w.clone(), b.clone()
            sd[k + ".running_mean"], sd[k + ".running_var"] = rm.clone(), rv.clone()
            sd[k + ".num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    for name, (co, ci, kh, kw) in _UPDATE:
        bound = 1.0 / math.sqrt(ci * kh * kw)
        sd[f"update_block.{name}.weight"] = uni((co, ci, kh, kw), bound)
        sd[f"update_block.{name}.bias"] = uni((co,), bound)
    return sd


def _random_small(seed: int) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}

    def uni(shape, bound):
        return (torch.rand(shape, generator=g) * 2.0 - 1.0) * bound

    for enc in ("fnet", "cnet"):
        for name, (co, ci, kh, kw) in _SMALL_ENC_CONVS + [("conv2", (_SMALL_OUT[enc], 96, 1, 1))]:
            sd[f"{enc}.{name}.weight"] = torch.randn((co, ci, kh, kw), generator=g) * math.sqrt(2.0 / (co * kh * kw))
            sd[f"{enc}.{name}.bias"] = uni((co,), 1.0 / math.sqrt(ci * kh * kw))
    for name, (co, ci, kh, kw) in _SMALL_UPDATE:
        bound = 1.0 / math.sqrt(ci * kh * kw)
        sd[f"update_block.{name}.weight"] = uni((co, ci, kh, kw), bound)
        sd[f"update_block.{name}.bias"] = uni((co,), bound)
    return sd


def load_checkpoint(ckpt) -> Dict[str, torch.Tensor]:
    """`ckpt`: a state_dict, a path to a `torch.save`d state_dict (optionally under a 'state_dict'
    key, optionally with `module.` prefixes), the string 'random:<seed>' (basic network) or
    'random-small:<seed>' (small network)."""
    if isinstance(ckpt, dict):
        sd = ckpt
    elif isinstance(ckpt, str) and ckpt.startswith("random-small:"):
        return random_state_dict(int(ckpt.split(":", 1)[1]), small=True)
    elif isinstance(ckpt, str) and ckpt.startswith("random:"):
        return random_state_dict(int(ckpt.split(":", 1)[1]))
    elif isinstance(ckpt, (str, os.PathLike)):
        if not os.path.exists(ckpt):
            raise FileNotFoundError(
                f"flow checkpoint {ckpt!r} not found (pass a RAFT state_dict path such as raft-things.pth, "
                "a state_dict, or 'random:<seed>')")
        # a state_dict of tensors needs nothing but tensors: never unpickle arbitrary objects from a user-supplied
        # path (OFX_UNSAFE_CHECKPOINT=1 opts back in for legacy .pth.tar files that pickle their args namespace)
        sd = torch.load(ckpt, map_location="cpu", weights_only=os.environ.get("OFX_UNSAFE_CHECKPOINT") != "1")
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
    else:
        raise TypeError(f"unsupported checkpoint spec {type(ckpt)}")
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
