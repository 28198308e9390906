"""The fused attention kernel (csrc/attn_flash.hip) against float64, instantiation by instantiation: ofx_attention_f32 at the head
sizes 40 / 64 / 80 / 128 / 160, the head-strided entry ofx_attention_bnhd_f32 and ops.attention.

The reference, the bound derived for this kernel's arithmetic, the case table and the float32 emulation with its simulated bugs live
in flash_attn_check.py.  The table is plain data: CPU tests assert from a restatement of the kernel's geometry that every head size
meets every key / query residue, mask geometry, maximum schedule and non-finite input, that the measured v_exp_f32 yardstick is
where the header says, and that the checker catches each simulated bug at every head size.  GPU tests are marked -m gpu; the CPU
self-tests carry no marker.
"""
import ctypes as C_

import pytest
import torch

import flash_attn_check as fc
import sd_ops_check as sc

gpu = pytest.mark.gpu
GUARD = fc.FA_GUARD
IDS = [c["name"] for c in fc.FA_CASES]


def _note(name, value):
    """Print a measured ratio (pytest -s shows them; the worst ones are recorded in the header of flash_attn_check.py)."""
    print(f"ratio {name} {float(value):.4g}")


def _L():
    from sd_animation_optical_flow_amd import _lib
    return _lib.lib()


def _p(t):
    return C_.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return None if t is None else t.cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _flash_raw(q, k, v, bias, scale):
    """ofx_attention_f32 called directly, with no workspace at all (the fused kernel needs none) and `out` followed by GUARD
    sentinel floats.  Returns out [BH, Nq, D] on the CPU."""
    L = _L()
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    assert L.ofx_attention_workspace_bytes(BH, Nq, Nk, D) == 0
    qd, kd, vd, bd = q.cuda(), k.cuda(), v.cuda(), _dev(bias)
    obuf = torch.cat([torch.full((q.numel(),), float("nan")), torch.full((GUARD,), 12345.0)]).cuda()
    st = L.ofx_attention_f32(_p(qd), _p(kd), _p(vd), _p(bd), Nq * Nk if (bias is not None and bias.dim() == 3) else 0, _p(obuf), BH, Nq, Nk, D,
                             scale, None, 0, _stream())
    torch.cuda.synchronize()
    assert st == 0, st
    assert bool((obuf[q.numel():] == 12345.0).all()), "written past out"
    return obuf[:q.numel()].view(BH, Nq, D).cpu()


def _check(label, out, ref, bound):
    rep = fc.fa_compare(out, ref, bound)
    assert rep["ratio"] <= 1.0, (label, rep)
    assert rep["nan_missing"] == 0 and rep["nan_extra"] == 0, (label, rep)
    _note(label, rep["ratio"])
    return rep


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU tests

@gpu
@pytest.mark.parametrize("c", fc.FA_CASES, ids=IDS)
def test_flash_attention_against_float64(cuda, c):
    """Every element inside the bound, NaN exactly where the reference is NaN, nothing written behind `out`, no workspace."""
    q, k, v, bias, ref, bound = fc.fa_case_data(c)
    out = _flash_raw(q, k, v, bias, fc.fa_scale(c))
    _check(f"flash {c['name']}", out, ref, bound)


def _heads(BH):
    """(copies, B, H) with H >= 2: a single batch-head is run twice side by side."""
    return {1: (2, 1, 2), 3: (1, 1, 3), 8: (1, 2, 4), 16: (1, 2, 8)}[BH]


def _token_rows(t, B, H, pad, fill):
    """[B*H, N, D] on the CPU -> its [B, N, H*D] token-row form as a last-axis slice (at column 4) of a device buffer `pad` floats
    wider, the other columns holding `fill`."""
    BH, N, D = t.shape
    rows = t.view(B, H, N, D).permute(0, 2, 1, 3).reshape(B, N, H * D)
    wide = torch.full((B, N, H * D + pad), fill)
    wide[..., 4:4 + H * D] = rows
    wide = wide.cuda()
    return wide, wide[..., 4:4 + H * D]


@gpu
@pytest.mark.parametrize("c", fc.FA_CASES, ids=IDS)
def test_flash_attention_bnhd_against_float64(cuda, c):
    """The same cases through ofx_attention_bnhd_f32: q, k, v are last-axis slices of wider buffers with three different row
    strides (the columns beside them hold NaN: never to be read into a result), `out` is a slice of a wider buffer whose other
    columns keep their sentinel; H >= 2; bit for bit the contiguous entry, and inside the float64 bound."""
    q, k, v, bias, ref, bound = fc.fa_case_data(c)
    copies, B, H = _heads(c["BH"])
    if copies == 2:
        q, k, v, ref, bound = (torch.cat([t, t]) for t in (q, k, v, ref, bound))
        if bias is not None and bias.dim() == 3:
            bias = torch.cat([bias, bias])
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    assert B * H == BH and H >= 2
    scale = fc.fa_scale(c)
    (_, qs), (_, ks), (_, vs) = _token_rows(q, B, H, 8, float("nan")), _token_rows(k, B, H, 12, float("nan")), _token_rows(v, B, H, 16, float("nan"))
    ldq, ldk, ldv, ldo = H * D + 8, H * D + 12, H * D + 16, H * D + 20
    assert len({ldq, ldk, ldv}) == 3 and (qs.stride(1), ks.stride(1), vs.stride(1)) == (ldq, ldk, ldv)
    obuf = torch.cat([torch.full((B * Nq * ldo,), 7.0), torch.full((GUARD,), 12345.0)]).cuda()
    wide = obuf[:B * Nq * ldo].view(B, Nq, ldo)
    os_ = wide[..., 4:4 + H * D]
    bd = _dev(bias)
    st = _L().ofx_attention_bnhd_f32(_p(qs), ldq, _p(ks), ldk, _p(vs), ldv, _p(bd), Nq * Nk if (bias is not None and bias.dim() == 3) else 0,
                                     _p(os_), ldo, B, H, Nq, Nk, D, scale, _stream())
    torch.cuda.synchronize()
    assert st == 0, st
    assert bool((obuf[B * Nq * ldo:] == 12345.0).all()), "written past out"
    assert bool((wide[..., :4] == 7.0).all()) and bool((wide[..., 4 + H * D:] == 7.0).all()), "written beside the out slice"
    out = os_.cpu().view(B, Nq, H, D).permute(0, 2, 1, 3).reshape(BH, Nq, D)
    assert torch.equal(_bits(out), _bits(_flash_raw(q, k, v, bias, scale))), "the strided entry differs from the contiguous one"
    _check(f"flash_bnhd {c['name']}", out, ref, bound)


def _wrapper_cases(D):
    return [c for c in fc.FA_CASES if c["D"] == D and c["name"].endswith(("nk77-shared-lead32", "nk3tiles-per-leadBK-grouped"))]


@gpu
@pytest.mark.parametrize("D", fc.FLASH_D)
def test_ops_attention_against_float64(cuda, D):
    """Through the Python wrapper, with a shared and with a per-head bias."""
    from sd_animation_optical_flow_amd import ops
    cs = _wrapper_cases(D)
    assert {c["bias"] for c in cs} == {"shared", "per"}
    for c in cs:
        q, k, v, bias, ref, bound = fc.fa_case_data(c)
        out = ops.attention(q.cuda(), k.cuda(), v.cuda(), _dev(bias), scale=c["scale"]).cpu()
        _check(f"ops.attention {c['name']}", out, ref, bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU self-tests

def _blocks_masked(bias_rows, lo, hi):
    """bias_rows [rows, Nk]: whether every row has only -inf in the keys lo..hi-1."""
    return bool((bias_rows[:, lo:hi] == fc.NINF).all())


def _moves(c):
    """For each (batch-head, query) the list of 32-key blocks in which its float64 running maximum moves."""
    q, k, v, bias, _, _ = fc.fa_case_data(c)
    lg, _, _ = fc.fa_logits64(q, k, bias, fc.fa_scale(c))
    nb = sc._cdiv(c["Nk"], 32)
    bm = torch.stack([lg[..., 32 * b:32 * b + 32].max(-1).values for b in range(nb)], -1)      # [BH, Nq, nb]
    run = bm.cummax(-1).values
    return torch.cat([torch.ones_like(bm[..., :1], dtype=torch.bool), run[..., 1:] > run[..., :-1]], -1)


def test_the_table_covers_every_path_of_every_head_size():
    assert {c["D"] for c in fc.FA_CASES} == set(fc.FLASH_D) and len(set(IDS)) == len(IDS)
    for D in fc.FLASH_D:
        cs = [c for c in fc.FA_CASES if c["D"] == D]
        geo = {c["name"]: fc.fa_geometry(c) for c in cs}
        bk = fc.fa_bk(D)
        assert bk == (64 if D == 40 else 32) and all(g["BK"] == bk for g in geo.values())
        assert all(c["BH"] * c["Nq"] * c["Nk"] <= 2_500_000 for c in cs)
        # the workgroup mapping reaches every (batch-head, tile) once, in both forms
        for c in cs:
            g = geo[c["name"]]
            assert sorted(g["blocks"]) == [(z, t) for z in range(c["BH"]) for t in range(g["qtiles"])], c["name"]
        # key-count residues
        nks = {c["Nk"] for c in cs}
        assert nks >= {1, 31, 32, 33, bk, bk + 1, 77, 65 if bk == 32 else 129}, (D, nks)
        assert any(g["nt"] >= 3 for g in geo.values()) and any(g["nt"] == 1 and g["nb"] == bk // 32 for g in geo.values())
        # query-count residues: three tiles, and waves whose queries all lie past the end
        assert {c["Nq"] for c in cs} >= {1, 32, 33, 128, 129, 257}
        assert any(g["qtiles"] == 3 and g["dead_waves"] == 3 for g in geo.values())
        assert any(0 < w[3] < 32 for g in geo.values() for w in g["waves"])
        # batch-head counts; a grouped case with more than one tile and a bias per batch-head
        assert {c["BH"] for c in cs} >= {1, 3, 8, 16}
        assert {c["BH"] for c in cs if geo[c["name"]]["grouped"]} >= {8, 16} and {c["BH"] for c in cs if not geo[c["name"]]["grouped"]} >= {1, 3}
        assert any(geo[c["name"]]["grouped"] and geo[c["name"]]["qtiles"] > 1 and c["bias"] == "per" for c in cs)
        assert {c["bias"] for c in cs} == {None, "shared", "per"}
        # mask geometries, read off the generated bias wave by wave
        seen = set()
        for c in cs:
            if not c["bias"]:
                continue
            q, k, v, bias, ref, _ = fc.fa_case_data(c)
            g = geo[c["name"]]
            b3 = bias.expand(c["BH"], c["Nq"], c["Nk"])
            for z in range(c["BH"]):
                for (_, _, q0, n) in g["waves"]:
                    if n == 0:
                        continue
                    rows = b3[z, q0:q0 + n]
                    open_row = bool(torch.isfinite(rows).any(1).any())
                    if c["Nk"] > 32 and _blocks_masked(rows, 0, 32) and open_row:
                        seen.add("lead32")
                    if c["Nk"] > bk and _blocks_masked(rows, 0, bk) and open_row:
                        seen.add("leadBK")
                    if g["nb"] > 1 and _blocks_masked(rows, 32 * (g["nb"] - 1), c["Nk"]) and bool(torch.isfinite(rows[:, :32]).any(1).all()):
                        seen.add("trail")
            if c["mask"] == "rand30":
                frac = float((b3 == fc.NINF).float().mean())
                assert 0.2 < frac < 0.45, (c["name"], frac)
                seen.add("rand30")
            if c["mask"] == "fill1000":
                all_fill = (b3 == -1000.0).all(-1)
                assert bool(all_fill.any()) and bool((~all_fill).any()) and not bool(torch.isnan(ref).any())
                seen.add("fill1000")
            if c["mask"] == "fmax":
                assert bool(((b3 == -fc.FMAX).any(-1) & torch.isfinite(b3).all(-1)).all())
                seen.add("fmax")
        assert seen >= {"lead32", "leadBK", "trail", "rand30", "fill1000", "fmax"}, (D, seen)
        # fully masked rows: row 0, the wave edge, the tile edge, the last row of the last batch-head, each beside valid rows
        planted = [(z, r, c) for c in cs for z, r in c["planted"]]
        assert {r for _, r, _ in planted} >= {0, 31, 32, 127, 128}
        assert any(z == c["BH"] - 1 and r == c["Nq"] - 1 and c["bias"] == "per" for z, r, c in planted)
        for c in cs:
            rows = fc.fa_planted(c)
            if c["nonfinite"] == "inf_v":
                continue
            R = c["BH"] * c["Nq"]
            for r in rows:
                assert any(0 <= n < R and n not in rows for n in (r - 1, r + 1, r - 2, r + 2)), (c["name"], r)
        # maximum schedules, from the float64 logits block by block
        sched = {c["schedule"]: (c, _moves(c)) for c in cs if c["schedule"]}
        assert set(sched) == {"ascending", "descending", "one_lane"}
        for name, (c, mv) in sched.items():
            nb = geo[c["name"]]["nb"]
            assert nb >= 3
            wave0 = mv[0, :32]                                            # the first wave: 32 live queries
            if name == "ascending":
                assert bool(wave0.all())                                  # every query's maximum moves in every block
            elif name == "descending":
                assert not bool(wave0[:, 1:].any())                       # the rescale branch is never taken after block 0
            else:
                others = torch.ones(32, dtype=torch.bool)
                others[fc.ONE_LANE] = False
                assert bool(wave0[fc.ONE_LANE, nb - 1]) and not bool(wave0[others][:, 1:].any())
        # magnitudes
        assert {c["data"] for c in cs} == {"unit", "mag6", "big80", "scale0", "negscale"}
        assert any(c["scale"] == 0.0 and c["Nk"] > 1 for c in cs) and any(c["scale"] is not None and c["scale"] < 0 for c in cs)
        assert any(c["data"] == "mag6" and c["scale"] is not None for c in cs)
        big = next(c for c in cs if c["data"] == "big80")
        q, k, v, bias, _, _ = fc.fa_case_data(big)
        lg, _, _ = fc.fa_logits64(q, k, bias, fc.fa_scale(big))
        under = ((lg - lg.max(-1, keepdim=True).values) * fc.LOG2E_F32 < -126).float().mean()
        assert float(lg.abs().max()) > 80.0 and float(under) > 0.5, (D, float(under))
        # non-finite inputs
        assert {c["nonfinite"] for c in cs} == {None, "nan_bias", "nan_q", "inf_bias", "inf_v"}


def test_the_reference_is_nan_exactly_in_the_planted_rows():
    """A row is NaN in the float64 reference in all of its columns or in none; the NaN rows are the planted ones and those the
    non-finite inputs make (a +inf bias and 0 * inf at a masked key included); rows of -1000 only and rows with finite -FLT_MAX
    entries are numbers, and the -FLT_MAX keys weigh nothing."""
    for c in fc.FA_CASES:
        q, k, v, bias, ref, bound = fc.fa_case_data(c)
        flat = torch.isnan(ref.reshape(-1, c["D"]))
        assert not bool((flat.any(1) & ~flat.all(1)).any()), c["name"]
        assert flat.all(1).nonzero().flatten().tolist() == fc.fa_planted(c), c["name"]
        ok = ~torch.isnan(ref)
        assert bool(torch.isfinite(bound[ok]).all()) and bool((bound[ok] > 0).all()), c["name"]
        if c["mask"] == "fmax":
            open_only = torch.where(bias == -fc.FMAX, torch.full_like(bias, fc.NINF), bias)
            ref2, _ = fc.fa_reference(q, k, v, open_only, fc.fa_scale(c))
            assert torch.equal(ref, ref2), c["name"]


def test_the_exp2_yardstick_is_where_the_header_says():
    """torch's float32 exp2 against float64 over the shifted base-2 arguments of every case of the table."""
    worst = 0.0
    for c in fc.FA_CASES:
        q, k, v, bias, _, _ = fc.fa_case_data(c)
        s = fc.fa_base2_logits32(q, k, None if bias is None else bias.expand(c["BH"], c["Nq"], c["Nk"]), fc.fa_scale(c))
        mx = torch.where(torch.isfinite(s), s, torch.full_like(s, fc.NINF)).max(-1, keepdim=True).values
        worst = max(worst, fc.exp2_yardstick(s - mx))
    _note("yardstick exp2", worst)
    assert 0.0 < worst <= fc.Y_EXP2 and fc.E_EXP2 == 2.0 * fc.Y_EXP2, worst


def test_the_checker_catches_each_simulated_bug_at_every_head_size():
    """The unmodified float32 emulation is inside the bound at EVERY case (the bound can be met in fp32); every simulated bug is
    outside it -- a ratio above 1 or a wrong NaN set -- at one case or more of each head size."""
    caught = {(bug, D): [] for bug in fc.FA_BUGS for D in fc.FLASH_D}
    closest = {bug: float("inf") for bug in fc.FA_BUGS}
    worst_good = (0.0, "")
    for c in fc.FA_CASES:
        q, k, v, bias, ref, bound = fc.fa_case_data(c)
        scale = fc.fa_scale(c)
        good = fc.fa_emulate(q, k, v, bias, scale)
        rep = fc.fa_compare(good, ref, bound)
        assert rep["ok"], (c["name"], rep)
        worst_good = max(worst_good, (rep["ratio"], c["name"]))
        for bug in fc.FA_BUGS:
            bad = fc.fa_emulate(q, k, v, bias, scale, bug=bug)
            rep = fc.fa_compare(bad, ref, bound)
            if not rep["ok"]:
                caught[(bug, c["D"])].append((c["name"], rep["ratio"]))
    for (bug, D), hits in caught.items():
        assert hits, f"{bug} goes unnoticed at every case of head size {D}"
        closest[bug] = min(closest[bug], max(r for _, r in hits))
    _note(f"emulation, worst case {worst_good[1]}", worst_good[0])
    for bug in fc.FA_BUGS:
        print(f"bug {bug}: caught at {sum(len(caught[(bug, D)]) for D in fc.FLASH_D)} cases; the smallest over the head sizes of its largest ratio {closest[bug]:.4g}")
