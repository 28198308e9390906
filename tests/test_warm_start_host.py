"""CPU: the warm-start fixture (tests/golden/raft_warm_ref_128x160.npz, tests/golden/make_golden_warm.py) against its float64
restatement (tests/warm_start_check.py), and forward_interpolate's nearest-source rule against a numpy brute force."""
import hashlib
import os

import numpy as np
import pytest
import torch

import warm_start_check as WS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_warm_ref_128x160.npz")
FLOAT_FIELDS = ("smooth", "random", "leaving")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _epe(a, b, dim=1):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).pow(2).sum(dim).sqrt().mean())


def _sd_digest(sd) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().numpy().tobytes())
    return h.hexdigest()


def test_fixture_is_small_and_pins_the_seeded_weights(gold):
    from oracle import raft_oracle as RO
    from sd_animation_optical_flow_amd.weights import random_state_dict
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert str(gold["state_dict_sha256"]) == _sd_digest(RO.init_state_dict(0))
    assert str(gold["small_state_dict_sha256"]) == _sd_digest(random_state_dict(0, small=True))


@pytest.mark.parametrize("case", ["basic", "basic_3", "basic_outside", "small"])
def test_float64_restatement_reproduces_the_reference(gold, case):
    from oracle import raft_oracle as RO
    from sd_animation_optical_flow_amd.weights import random_state_dict
    i1, i2 = torch.from_numpy(gold["image1"]).float(), torch.from_numpy(gold["image2"]).float()
    init = torch.from_numpy(gold["flow_init_outside" if case == "basic_outside" else "flow_init"])
    if case == "small":
        lo, up = WS.raft_small_forward_warm(random_state_dict(0, small=True), i1, i2, init, 20)
        ref_lo, ref_up = gold["small_flow_low"], gold["small_flow_up"]
    else:
        lo, up = WS.raft_forward_warm(RO.init_state_dict(0), i1, i2, init, 3 if case == "basic_3" else 20)
        sfx = {"basic": "", "basic_3": "_3", "basic_outside": "_outside"}[case]
        ref_lo, ref_up = gold["flow_low" + sfx], gold["flow_up" + sfx]
        if ref_up.shape[-1] != up.shape[-1]:
            up = up[:, :, ::2, ::2]
    assert float((lo - torch.from_numpy(ref_lo).double()).abs().max()) < 1e-4
    assert _epe(up, ref_up) < 2e-5


def test_warm_start_changes_the_flow(gold):
    """The init really enters the recurrence: 3 iterations from the smooth init are far from 3 iterations from zero."""
    from oracle import raft_oracle as RO
    i1, i2 = torch.from_numpy(gold["image1"]).float(), torch.from_numpy(gold["image2"]).float()
    cold_lo, _ = WS.raft_forward_warm(RO.init_state_dict(0), i1, i2, torch.zeros_like(torch.from_numpy(gold["flow_init"])), 3)
    assert float((cold_lo - torch.from_numpy(gold["flow_low_3"]).double()).abs().mean()) > 0.1


@pytest.mark.parametrize("name", FLOAT_FIELDS + ("invalid",))
def test_brute_force_reproduces_forward_interpolate_bit_for_bit(gold, name):
    out = WS.forward_interpolate_brute(gold["fi_in_" + name])
    assert np.array_equal(out, gold["fi_out_" + name], equal_nan=True)
    if name == "invalid":
        assert np.isnan(out).all()


def test_tie_field_reference_picks_a_nearest_source(gold):
    """Integer-valued fields tie everywhere: scipy's pick among ties is its tree's, so only the rule is checked -- every output value is
    the flow of some valid source at the minimal distance; the lowest-index rule picks such a source too."""
    f, ref = gold["fi_in_ties"], gold["fi_out_ties"]
    mine, pick = WS.forward_interpolate_brute(f, return_index=True)
    d2, dmin = WS.nearest_d2(f, pick)
    assert np.array_equal(d2, dmin)
    h, w = f.shape[1:]
    x0, y0 = np.meshgrid(np.arange(w), np.arange(h))
    x1, y1 = (x0 + f[0]).reshape(-1), (y0 + f[1]).reshape(-1)
    valid = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    flat = f.reshape(2, -1)
    for p in range(h * w):
        px, py = p % w, p // w
        d = (x1 - px) ** 2 + (y1 - py) ** 2
        at_min = valid & (d == dmin[p])
        vals = {(float(a), float(b)) for a, b in zip(flat[0][at_min], flat[1][at_min])}
        assert (float(ref[0].reshape(-1)[p]), float(ref[1].reshape(-1)[p])) in vals, p
    assert not np.array_equal(mine, ref)      # the fixture does hold ties the two rules break differently


def test_header_declares_the_warm_start_surface():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ofx.h")).read()
    assert "#define OFX_RAFT_FLOW_INIT  2048" in hdr
    for sym in ("ofx_forward_interpolate(", "ofx_forward_interpolate_scratch_bytes("):
        assert sym in hdr
    from sd_animation_optical_flow_amd import _lib
    assert "ofx_forward_interpolate" in _lib.SIGNATURES and "ofx_forward_interpolate_scratch_bytes" in _lib.SIGNATURES
    from sd_animation_optical_flow_amd import raft
    assert raft.FLAG_FLOW_INIT == 2048
