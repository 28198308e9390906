"""CPU-only: the small RAFT network's weights, key-set detection and float64 restatement against the reference's own outputs
(tests/golden/raft_small_ref_128x160.npz, written by tests/golden/make_golden_small.py)."""
import hashlib
import os

import numpy as np
import pytest
import torch

import small_raft_check as SR
from sd_animation_optical_flow_amd.weights import load_checkpoint, raft_variant, random_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_small_ref_128x160.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def sd():
    return random_state_dict(0, small=True)


@pytest.fixture(scope="module")
def traced(gold, sd):
    tr = {}
    lo, up = SR.raft_small_forward(sd, torch.from_numpy(gold["image1"]), torch.from_numpy(gold["image2"]), 20, trace=tr)
    return tr, lo, up


def _digest(sd) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().numpy().tobytes())
    return h.hexdigest()


def test_seeded_small_weights_are_the_fixtures_and_have_the_reference_key_set(gold, sd):
    assert _digest(sd) == str(gold["state_dict_sha256"])
    keys = [str(k) for k in gold["state_dict_keys"]]
    assert list(sd) == keys and len(keys) == 106
    for k, shp in zip(keys, gold["state_dict_shapes"]):
        assert tuple(sd[k].shape) == tuple(int(d) for d in shp if d > 0), k
    assert sum(v.numel() for v in sd.values()) == 990162
    assert _digest(load_checkpoint("random-small:0")) == _digest(sd)


def test_restatement_reproduces_the_reference_stages(gold, sd, traced):
    tr, _, _ = traced
    rel = lambda a, b: float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
    for nm in ("fmap1", "fmap2", "net", "inp"):                     # (the fixture keeps these in float16)
        ref = torch.from_numpy(gold[nm + "_f16"].astype(np.float64))
        assert rel(tr[nm], ref) < 1e-3, nm
    stats = np.array([float(tr["fmap1"].sum()), float(tr["fmap1"].abs().sum()), float(tr["fmap2"].sum()), float(tr["fmap2"].abs().sum())])
    assert np.allclose(stats, gold["fmap_stats"], rtol=1e-5, atol=1e-3)
    h, w = tr["fmap1"].shape[-2:]
    c0 = SR.coords_grid(1, h, w)
    jit = torch.from_numpy(gold["lookup_jitter"]).double()
    for nm, c in (("int", c0), ("frac", c0 + jit * 5.0), ("far", c0 + jit * 60.0)):
        got = SR.corr_lookup(tr["pyramid"], c)[:, :, ::3, ::3]
        assert rel(got, torch.from_numpy(gold["lookup_" + nm]).double()) < 1e-5, nm
    lookup0 = SR.corr_lookup(tr["pyramid"], c0)
    net1, delta1 = SR.update_block(SR.to64(sd), tr["net"], tr["inp"], lookup0, c0 - c0)
    assert rel(net1, torch.from_numpy(gold["update_net1_f16"].astype(np.float64))) < 1e-3
    assert rel(delta1, torch.from_numpy(gold["update_delta1"]).double()) < 1e-5
    up = SR.upflow8(torch.from_numpy(gold["upflow8_in"]).double())
    assert rel(up, torch.from_numpy(gold["upflow8_out"]).double()) < 1e-6


def test_restatement_reproduces_the_reference_flows(gold, sd, traced):
    """The reference computes in float32: its 20-iteration flow sits 1.1e-5 px (mean EPE) from float64 at this size, which is the
    bar's scale here (2e-5 px)."""
    _, lo, up = traced
    e_up = SR.epe(up, torch.from_numpy(gold["flow_up"]), 1)
    e_lo = SR.epe(lo, torch.from_numpy(gold["flow_low"]), 1)
    e_alt = SR.epe(up[:, :, ::2, ::2], torch.from_numpy(gold["flow_up_alt"]), 1)
    assert e_up <= 2e-5 and e_alt <= 2e-5 and e_lo <= 2e-5 / 8 * 2, (e_up, e_alt, e_lo)
    # the RAFT_2-style pair: BGR frames, InputPadder (centred replicate padding to 136x160), the padded flow
    f1, f2 = gold["raft2_frame1"], gold["raft2_frame2"]
    t = lambda f: torch.from_numpy(np.ascontiguousarray(f[:, :, ::-1])).permute(2, 0, 1).double()[None]
    a, b = t(f1), t(f2)
    H, W = a.shape[-2:]
    ph, pw = (((H // 8) + 1) * 8 - H) % 8, (((W // 8) + 1) * 8 - W) % 8
    pad = lambda x: torch.nn.functional.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2), mode="replicate")
    _, q = SR.raft_small_forward(sd, pad(a), pad(b), 20)
    assert SR.epe(q[0].permute(1, 2, 0), torch.from_numpy(gold["raft2_flow"])) <= 2e-5


def test_raft_variant_names_the_network(sd):
    basic = random_state_dict(0)
    assert raft_variant(sd) == "small" and raft_variant(basic) == "basic"
    assert raft_variant({"module." + k: v for k, v in sd.items()}) == "small"
    assert raft_variant({"module." + k: v for k, v in basic.items()}) == "basic"
    from oracle import raft_oracle
    assert raft_variant(raft_oracle.init_state_dict(0)) == "basic"


def test_raft_variant_refuses_mixed_and_partial_dicts(sd):
    basic = random_state_dict(0)
    mixed = dict(sd)
    mixed["update_block.mask.0.weight"] = basic["update_block.mask.0.weight"]
    with pytest.raises(ValueError, match="update_block.mask.0.weight"):
        raft_variant(mixed)
    mixed2 = dict(basic)
    mixed2["update_block.gru.convz.weight"] = sd["update_block.gru.convz.weight"]
    with pytest.raises(ValueError, match="update_block.gru.convz.weight"):
        raft_variant(mixed2)
    partial = {k: v for k, v in sd.items() if k != "cnet.layer2.0.conv3.bias"}
    with pytest.raises(ValueError, match="cnet.layer2.0.conv3.bias"):
        raft_variant(partial)
    partial_b = {k: v for k, v in basic.items() if k != "update_block.gru.convq2.weight"}
    with pytest.raises(ValueError, match="update_block.gru.convq2.weight"):
        raft_variant(partial_b)
    swapped = dict(sd)
    swapped["fnet.conv1.weight"] = basic["fnet.conv1.weight"]                  # a key both networks have, with the other's shape
    with pytest.raises(ValueError, match="fnet.conv1.weight"):
        raft_variant(swapped)
