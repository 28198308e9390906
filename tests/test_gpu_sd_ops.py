"""ofx_groupnorm, ofx_softmax_rows and the unfused branch of ofx_attention_f32 against float64, kernel by kernel.

Bounds, references and case tables live in sd_ops_check.py and are derived there (one term -- the device's expf and division -- is
measured against a CPU float32 yardstick, see its header).  The case tables are plain data: CPU tests assert that they contain every
thread layout and padding residue of the kernels and that the checker catches each simulated bug at every case.  GPU tests are
marked -m gpu; the CPU self-tests carry no marker.
"""
import ctypes as C_

import pytest
import torch

import sd_ops_check as sc

gpu = pytest.mark.gpu
GUARD = 64


def _note(name, value):
    """Print a measured ratio (pytest -s shows them; the worst ones are recorded in the header of sd_ops_check.py)."""
    print(f"ratio {name} {float(value):.4g}")


def _ops():
    from sd_animation_optical_flow_amd import ops
    return ops


def _L():
    from sd_animation_optical_flow_amd import _lib
    return _lib.lib()


def _p(t):
    return C_.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C_.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return None if t is None else t.cuda()


def _guarded(t, value=12345.0):
    """A device copy of the flat float tensor followed by GUARD sentinel floats."""
    return torch.cat([t.flatten(), torch.full((GUARD,), value)]).cuda()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. GroupNorm

def _run_groupnorm(c, x, gamma, beta):
    """The kernel's output [B, HW, C] on the CPU.  The scratch is exactly ofx_groupnorm_scratch_bytes(B, C) with sentinel bytes
    behind it, `out` is followed by sentinel floats (x itself when the case is in place), the input is read only otherwise."""
    ops = _ops()
    B, HW, Cn = x.shape
    need = _L().ofx_groupnorm_scratch_bytes(B, Cn)
    assert need == B * sc.gn_layout(B, HW, Cn, c["groups"])["slices"] * Cn * 16 + B * Cn * 8
    scratch = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    xbuf = _guarded(x)
    xd = xbuf[:x.numel()].view(B, HW, 1, Cn)
    obuf = xbuf if c["alias"] else _guarded(torch.full((x.numel(),), float("nan")))
    out = ops.groupnorm(xd, _dev(gamma), _dev(beta), c["groups"], sc.GN_EPS, c["silu"], out=obuf[:x.numel()], scratch=scratch[:need])
    assert out.data_ptr() == obuf.data_ptr()
    torch.cuda.synchronize()
    assert bool((obuf[x.numel():] == 12345.0).all()), "written past out"
    assert bool((scratch[need:] == 0xA5).all()), "written past the scratch"
    if not c["alias"]:
        assert bool((xbuf[x.numel():] == 12345.0).all()) and torch.equal(xbuf[:x.numel()].cpu(), x.flatten())
    return obuf[:x.numel()].view(B, HW, Cn).cpu()


@gpu
@pytest.mark.parametrize("c", sc.GN_CASES, ids=[c["name"] for c in sc.GN_CASES])
def test_groupnorm_against_float64(cuda, c):
    x, gamma, beta = sc.gn_input(c)
    out = _run_groupnorm(c, x, gamma, beta)
    ref = sc.gn_reference(x, gamma, beta, c["groups"])
    ratio, used = sc.gn_ratios(out, x, ref, c["silu"])
    _note(f"groupnorm {c['name']}", ratio)
    if c["silu"]:
        _note(f"groupnorm {c['name']} measured-term use", used)
    assert ratio <= 1.0, (c["name"], ratio)


@gpu
def test_groupnorm_apply_takes_its_grid_stride_trip(cuda):
    """B HW C / 4 > 65536 * 256: the last float4s are reached in a second trip of the apply kernel's loop.  Run like every other
    case (exact scratch, sentinels behind `out`, the input untouched), compared image by image (the reference of one image at a
    time), without and with SiLU."""
    c = sc.GN_LARGE
    B, HW, Cn = c["B"], c["HW"], c["C"]
    lay = sc.gn_layout(B, HW, Cn, c["groups"])
    assert lay["apply_trips"] == 2
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn((1, HW, Cn), generator=g) * 2.0 + 0.5
    x = torch.cat([x0, x0.flip(1) * 1.25 - 0.75])                     # the second image: other statistics, no second randn
    gamma = torch.randn((Cn,), generator=g) * 0.5 + 1.0
    beta = torch.randn((Cn,), generator=g)
    refs = [sc.gn_reference(x[b:b + 1], gamma, beta, c["groups"], layout=lay) for b in range(B)]
    for silu in (False, True):
        out = _run_groupnorm(dict(c, silu=silu), x, gamma, beta)
        for b in range(B):
            ratio, _ = sc.gn_ratios(out[b:b + 1], x[b:b + 1], refs[b], silu)
            _note(f"groupnorm large image {b} silu {int(silu)}", ratio)
            assert ratio <= 1.0, (b, silu, ratio)


@gpu
def test_groupnorm_refusals(cuda):
    """The documented code comes back before anything is launched: `out` stays NaN."""
    L = _L()

    def call(B, HW, Cn, groups, x_off=0, short=0):
        need = L.ofx_groupnorm_scratch_bytes(B, Cn)
        x = torch.zeros((B * HW * Cn + 8,), device="cuda")
        out = torch.full((B * HW * Cn + 8,), float("nan"), device="cuda")
        scratch = torch.zeros((need + 16,), dtype=torch.uint8, device="cuda")
        st = L.ofx_groupnorm(C_.c_void_p(x.data_ptr() + x_off), None, None, _p(out), _p(scratch), need - short, B, HW, Cn, groups, 1e-6, 0,
                             _stream())
        torch.cuda.synchronize()
        assert st == 0 or bool(torch.isnan(out).all())
        return st

    assert call(1, 4, 8, 2) == 0                          # the accepted twin of the calls below
    assert call(1, 4, 6, 3) == sc.EALIGN                 # C % 4 != 0
    assert call(1, 4, 8, 3) == sc.EINVAL                  # C % groups != 0
    assert call(65536, 1, 4, 1) == sc.EINVAL              # B beyond the grid's y extent
    assert call(1, 4, 8, 2, x_off=4) == sc.EALIGN         # x not 16-byte aligned
    assert call(1, 4, 8, 2, short=1) == sc.ENOMEM         # scratch one byte short


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. row softmax

@gpu
@pytest.mark.parametrize("c", sc.SM_CASES, ids=[c["name"] for c in sc.SM_CASES])
def test_softmax_rows_against_float64(cuda, c):
    """Exactly the planted rows are NaN, every other row is inside the bound, the pad columns n..ld-1 are exactly 0.0 in every row
    (they went in as NaN), the floats behind rows * ld and the input's bias are untouched."""
    buf, bias, planted = sc.sm_input(c)
    ref, bound = sc.sm_reference(buf, bias, c)
    d, bd = buf.cuda(), _dev(bias)
    _ops().softmax_rows(d, c["rows"], c["ld"], c["n"], c["scale"], bd, c["ld_bias"], max(1, c["bias_rows"]))
    after = d.cpu()
    body = after[:c["rows"] * c["ld"]].view(c["rows"], c["ld"])[:, :c["n"]]
    rep = sc.rows_report(body, ref, bound, planted)
    _note(f"softmax {c['name']}", rep["ratio"])
    assert len(rep["nan_rows"]) == len(planted) and rep["nan_rows"] == planted and not rep["partial_nan"], rep
    assert rep["ratio"] <= 1.0, rep
    assert sc.sm_violations(after, c, ref, bound, planted) == set()
    if bias is not None:
        assert torch.equal(bd.cpu().nan_to_num(7.0), bias.nan_to_num(7.0))


@gpu
def test_softmax_rows_refusals(cuda):
    L = _L()
    x = torch.zeros((64,), device="cuda")
    b = torch.zeros((64,), device="cuda")
    assert L.ofx_softmax_rows(_p(x), 4, 8, 9, 1.0, None, 0, 1, _stream()) == sc.EINVAL            # ld < n
    assert L.ofx_softmax_rows(_p(x), 4, 8, 8, 1.0, _p(b), 7, 1, _stream()) == sc.EINVAL           # ld_bias < n
    assert L.ofx_softmax_rows(_p(x), 4, 8, 8, 1.0, _p(b), 8, 0, _stream()) == sc.EINVAL           # no bias rows
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. unfused attention

def _attention_raw(q, k, v, bias, scale, ws_bytes=None, ws_null=False):
    """ofx_attention_f32 called directly with a workspace of exactly `ws_bytes` (default: ofx_attention_workspace_bytes) and
    AT_GUARD sentinel bytes behind it.  Returns (status, out on the CPU or None)."""
    L = _L()
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    need = L.ofx_attention_workspace_bytes(BH, Nq, Nk, D)
    if D % 4 == 0:
        assert need == sc.at_workspace_bytes(BH, Nq, Nk, D)
    n = need if ws_bytes is None else ws_bytes
    ws = torch.full((need + sc.AT_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    qd, kd, vd, bd = q.cuda(), k.cuda(), v.cuda(), _dev(bias)
    obuf = _guarded(torch.full((q.numel(),), float("nan")))
    st = L.ofx_attention_f32(_p(qd), _p(kd), _p(vd), _p(bd), Nq * Nk if (bias is not None and bias.dim() == 3) else 0, _p(obuf), BH, Nq, Nk, D,
                             scale, None if ws_null else _p(ws), n, _stream())
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "written past the workspace"
    assert bool((obuf[q.numel():] == 12345.0).all()), "written past out"
    out = obuf[:q.numel()].view(BH, Nq, D).cpu()
    if st != 0:
        assert bool(torch.isnan(out).all()) and bool((ws == 0xA5).all()), "a refused call launched something"
        return st, None
    return st, out


@gpu
@pytest.mark.parametrize("c", sc.AT_CASES, ids=[c["name"] for c in sc.AT_CASES])
def test_unfused_attention_against_float64(cuda, c):
    """Only the planted rows are NaN (and all of them), every other row is inside the bound -- with a workspace of exactly
    ofx_attention_workspace_bytes, and again through ops.attention sliced to one batch-head at a time."""
    assert c["D"] not in sc.FLASH_D
    q, k, v, bias = sc.at_input(c)
    scale = sc.at_scale(c)
    ref, bound = sc.at_reference(q, k, v, bias, scale)
    planted = sc.at_planted(c)
    flat = lambda t: t.reshape(-1, c["D"])
    st, out = _attention_raw(q, k, v, bias, scale)
    assert st == 0
    sliced = _ops().attention(q.cuda(), k.cuda(), v.cuda(), _dev(bias), scale=c["scale"], max_workspace_bytes=1).cpu()
    for how, o in (("exact workspace", out), ("one batch-head at a time", sliced)):
        rep = sc.rows_report(flat(o), flat(ref), flat(bound), planted)
        _note(f"attention {c['name']} ({how})", rep["ratio"])
        assert len(rep["nan_rows"]) == len(planted) and rep["nan_rows"] == planted and not rep["partial_nan"], (how, rep)
        assert rep["ratio"] <= 1.0, (how, rep)


@gpu
def test_unfused_attention_refusals(cuda):
    q, k, v = torch.randn((2, 5, 48)), torch.randn((2, 7, 48)), torch.randn((2, 7, 48))
    need = sc.at_workspace_bytes(2, 5, 7, 48)
    assert _attention_raw(q, k, v, None, 0.1, ws_bytes=need - 1)[0] == sc.ENOMEM
    assert _attention_raw(q, k, v, None, 0.1, ws_null=True)[0] == sc.EALIGN
    assert _attention_raw(q[..., :6].contiguous(), k[..., :6].contiguous(), v[..., :6].contiguous(), None, 0.1)[0] == sc.EALIGN      # D % 4 != 0
    assert _attention_raw(q, k, v, None, 0.1)[0] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. CPU self-tests: what the tables cover, what the checker catches, where the yardstick stands

def test_tables_cover_every_layout_and_padding_residue():
    cs = sc.GN_CASES
    lays = [(sc.gn_layout(c["B"], c["HW"], c["C"], c["groups"]), c) for c in cs]
    assert {c["C"] for c in cs} >= {4, 32, 64, 128, 320, 512, 1024, 1280}
    assert {c["groups"] for c in cs} >= {1, 32, 5, 512} and {c["HW"] for c in cs} >= {1, 63, 256, 257, 1000, 4099}
    assert {c["B"] for c in cs} == {1, 3, 4, 5}
    assert all(c["B"] * c["HW"] * c["C"] < 8_000_000 for c in cs)
    assert any(c["groups"] == 5 and c["C"] == 60 and l["tpg"] == 51 for l, c in lays)
    assert any(c["groups"] == 512 and c["C"] == 1024 and l["fin_passes"] == 2 and l["tpg"] == 1 for l, c in lays)
    assert {c["C"] for l, c in lays if l["cpg"] == 1} >= {4, 32, 1024} and max(l["fin_passes"] for l, _ in lays) == 4
    assert any(l["ncg"] == [80] and l["rws"] == [3] and l["idle"] and l["trips"] == 2 for l, _ in lays)
    assert any(c["HW"] == 1000 and l["per"] == 4 and l["full"] == 250 and l["nonempty"] == 250 and l["slices"] == 256 for l, c in lays)
    # every thread-row count of one channel pass, a second pass, and both with single-pixel and with multi-pixel slices
    assert {l["rws"][0] for l, _ in lays} >= {256, 32, 16, 8, 3, 17, 2, 1}
    for trips in (False, True):
        assert any(l["ncg"] == [256, 64] and (l["trips"] > 1) == trips for l, _ in lays)
        assert any(l["rws"][0] == 256 and (l["trips"] > 1) == trips for l, _ in lays)
        assert any(l["slices"] == 64 and (l["trips"] > 1) == trips for l, _ in lays)
        assert any(l["slices"] == 256 and (l["trips"] > 1) == trips for l, _ in lays)
    assert any(l["slices"] == 64 and l["nonempty"] == 1 for l, _ in lays) and any(l["nonempty"] < l["slices"] and l["per"] > 1 for l, _ in lays)
    # the data kinds: every one on its own against the single-group layout, all five inside every mixed case (groups >= 5)
    assert {c["data"] for c in cs if c["groups"] == 1 and c["HW"] == 63} == set(sc.KINDS)
    assert all(c["groups"] >= 5 for c in cs if c["data"] == "mixed")
    assert all(c["data"] == "mixed" for c in cs if c["groups"] >= 5)
    assert {c["affine"] for c in cs} == {"both", "no_gamma", "no_beta", "none"}
    assert {c["silu"] for c in cs} == {False, True} and {c["alias"] for c in cs} == {False, True}
    assert all(l["apply_trips"] == 1 for l, _ in lays)
    g = sc.GN_LARGE
    assert sc.gn_layout(g["B"], g["HW"], g["C"], g["groups"])["apply_trips"] == 2
    # softmax
    sm = sc.SM_CASES
    assert {c["n"] for c in sm} == {1, 3, 255, 256, 257, 1000}
    assert {(c["n"], c["ldk"]) for c in sm} == {(n, k) for n in (1, 3, 255, 256, 257, 1000) for k in ("n", "up4", "n+37")}
    assert all(c["ld"] >= c["n"] for c in sm) and any(c["ld"] % 4 for c in sm)
    assert min(c["rows"] for c in sm) == 1 and max(c["rows"] for c in sm) >= 300
    for b in (None, "shared", "row"):
        assert {c["scale"] for c in sm if c["bias"] == b} == {1.0, sc.SM_SCALE}, b
    assert all(1 < c["bias_rows"] < c["rows"] for c in sm if c["bias"] == "shared")
    assert {c["rows"] % c["bias_rows"] == 0 for c in sm if c["bias"] == "shared"} == {False, True}     # attention's whole batch-heads, and not
    assert all(c["ld_bias"] > c["n"] for c in sm if c["bias"])
    assert sum(len(sc.planted_rows(c["rows"])) == 3 for c in sm) >= 12
    assert any(c["n"] < 256 and sc.planted_rows(c["rows"]) for c in sm)
    # attention
    at = sc.AT_CASES
    assert {c["D"] for c in at} == {4, 36, 48, 96, 512} and not {c["D"] for c in at} & set(sc.FLASH_D)
    assert {c["Nk"] for c in at} == {1, 7, 31, 32, 33, 77, 130} and {c["Nq"] for c in at} == {1, 65, 130} and {c["BH"] for c in at} == {1, 2, 5}
    assert {c["bias"] for c in at} == {None, "shared", "per"} and any(c["scale"] is not None for c in at) and any(c["mag"] == 6.0 for c in at)
    assert {c["D"] % 32 for c in at} >= {0, 4, 16} and {c["Nk"] % 4 for c in at} >= {0, 1, 2, 3} and any(c["Nk"] % 32 == 0 for c in at)
    planted = [(z, r, c) for c in at for z, r in c["planted"]]
    assert any(r == 0 for _, r, _ in planted) and any(r == c["Nq"] - 1 for _, r, c in planted)
    assert any(z == c["BH"] - 1 and r == c["Nq"] - 1 and c["bias"] == "per" for z, r, c in planted)
    assert sum(0 < r < c["Nq"] - 1 and c["Nk"] % 32 != 0 for _, r, c in planted) >= 3           # the K padding beside a NaN row
    assert all(len(set(sc.at_planted(c))) == len(sc.at_planted(c)) for c in at)


def test_the_groupnorm_checker_catches_each_simulated_bug_at_every_case():
    """A float64 GroupNorm from the kernel's own partial sums (the naive variance, clamped) passes at every case, its float32
    rounding and the SiLU of it included; each simulated bug is caught at every case at which it changes anything, and the table
    leaves no bug without such a case."""
    seen = {b: 0 for b in sc.GN_BUGS}
    for c in sc.GN_CASES:
        x, gamma, beta = sc.gn_input(c)
        lay = sc.gn_layout(c["B"], c["HW"], c["C"], c["groups"])
        ref = sc.gn_reference(x, gamma, beta, c["groups"])
        (S, Q), _ = sc.gn_partials(x, lay)
        scale, shift = sc.gn_finalize64(S, Q, c["HW"], gamma, beta, c["groups"])
        good = sc.gn_apply64(x, scale, shift)
        assert sc.gn_ratios(good, x, ref, False)[0] <= 1.0, c["name"]
        assert sc.gn_ratios(good.float(), x, ref, False)[0] <= 1.0, c["name"]
        if c["silu"]:
            y32 = good.float()
            assert sc.gn_ratios(y32 / (1.0 + torch.exp(-y32)), x, ref, True)[0] <= 1.0, c["name"]
        for bug in sc.GN_BUGS:
            if not sc.gn_bug_visible(bug, c, lay):
                continue
            seen[bug] += 1
            bad = sc.gn_bugged(bug, x, gamma, beta, c, lay)
            if c["silu"]:
                bad = bad * torch.sigmoid(bad)
            assert not sc.gn_ratios(bad, x, ref, c["silu"])[0] <= 1.0, (c["name"], bug)
    assert all(n >= 5 for n in seen.values()), seen


def test_the_row_checker_catches_each_simulated_softmax_bug_at_every_case():
    leaks = pads = mods = 0
    for c in sc.SM_CASES:
        buf, bias, planted = sc.sm_input(c)
        ref, bound = sc.sm_reference(buf, bias, c)
        rows, n, ld = c["rows"], c["n"], c["ld"]
        good = torch.cat([torch.zeros((rows, ld)).index_copy_(1, torch.arange(n), ref.float()).flatten(), buf[rows * ld:]])
        assert sc.sm_violations(good, c, ref, bound, planted) == set(), c["name"]
        body = lambda t: t[:rows * ld].view(rows, ld)
        if ld > n:                                   # a pad column left non-zero (the smallest denormal will do), also in a masked row
            for r in {0, rows - 1}:
                bad = good.clone()
                body(bad)[r, ld - 1] = 1e-45
                assert sc.sm_violations(bad, c, ref, bound, planted) == {"pad"}, c["name"]
            pads += 1
        bad = good.clone()
        bad[rows * ld + 1] = 0.0
        assert sc.sm_violations(bad, c, ref, bound, planted) == {"sentinel"}
        if c["bias"] == "shared" and n > 1:          # the bias row taken without the modulo (rows past the table read its last row; n = 1: always 1)
            wrong, _ = sc.sm_reference(buf, bias, c, bias_row=torch.arange(rows).clamp_max(c["bias_rows"] - 1))
            bad = good.clone()
            body(bad)[:, :n] = wrong.float()
            assert "bound" in sc.sm_violations(bad, c, ref, bound, planted), c["name"]
            mods += 1
        if planted:
            leaks += 1
            for r in planted:                        # a NaN row leaking into its neighbour
                bad = good.clone()
                nb = r + 1 if r + 1 < rows else r - 1
                if nb in planted:
                    continue
                body(bad)[nb, 0] = float("nan")
                assert sc.sm_violations(bad, c, ref, bound, planted) >= {"count", "which", "bound"}, c["name"]
                bad = good.clone()                   # a masked row that comes out as numbers: the count is wrong
                body(bad)[r, :n] = 0.0
                assert sc.sm_violations(bad, c, ref, bound, planted) >= {"count", "which"}, c["name"]
            bad = good.clone()                       # the NaN moved to another row: the count is right, the rows are not
            body(bad)[planted[0], :n] = 1.0 / n
            other = next(r for r in range(rows) if r not in planted)
            body(bad)[other, :n] = float("nan")
            assert sc.sm_violations(bad, c, ref, bound, planted) == {"which", "bound"}, c["name"]
    assert leaks >= 12 and pads >= 10 and mods >= 5


def test_the_row_checker_catches_a_nan_leak_and_a_wrong_count_at_every_attention_case():
    n = 0
    for c in sc.AT_CASES:
        q, k, v, bias = sc.at_input(c)
        ref, bound = sc.at_reference(q, k, v, bias, sc.at_scale(c))
        planted = sc.at_planted(c)
        flat = lambda t: t.reshape(-1, c["D"])
        R = c["BH"] * c["Nq"]
        assert [r for r in range(R) if bool(torch.isnan(flat(ref)[r]).all())] == planted, c["name"]
        assert not bool(torch.isnan(flat(ref)).any(1).logical_xor(torch.isnan(flat(ref)).all(1)).any())
        good = flat(ref).float()
        assert sc.rows_violations(good, flat(ref), flat(bound), planted) == set(), c["name"]
        # a q k^T that lost its last term: outside the bound
        if c["D"] > 4 and c["Nk"] > 1:               # (a single key has probability 1 whatever its score)
            short, _ = sc.at_reference(q[..., :-1], k[..., :-1], v, bias, sc.at_scale(c))
            assert "bound" in sc.rows_violations(flat(short).float(), flat(ref), flat(bound), planted), c["name"]
        for r in planted:
            n += 1
            nb = r + 1 if r + 1 < R else r - 1
            if nb < 0 or nb in planted:
                continue
            bad = good.clone()                       # NaN times a zero weight: the whole neighbouring row is poisoned
            bad[nb] = float("nan")
            assert sc.rows_violations(bad, flat(ref), flat(bound), planted) >= {"count", "which"}, c["name"]
            bad = good.clone()
            bad[r] = 0.0
            assert sc.rows_violations(bad, flat(ref), flat(bound), planted) >= {"count", "which"}, c["name"]
    assert n >= 20


def test_the_cpu_yardstick_is_where_the_header_says():
    """The measured term's yardstick: torch's float32 exp and division against float64 on the arguments the kernels see in these
    tables -- the shifted logits of the softmax and attention cases and the SiLU arguments of the GroupNorm cases."""
    worst_e = worst_d = 0.0
    for c in sc.SM_CASES:
        buf, bias, _ = sc.sm_input(c)
        x = buf[:c["rows"] * c["ld"]].view(c["rows"], c["ld"])[:, :c["n"]]
        v = x * c["scale"] + (0 if bias is None else bias[:, :c["n"]][torch.arange(c["rows"]) % c["bias_rows"]])
        t = v - v.max(1, keepdim=True).values
        worst_e = max(worst_e, sc.exp_yardstick(t))
        e = torch.exp(t)
        s = e.sum(1, keepdim=True)
        ok = torch.isfinite(s.flatten()) & (s.flatten() > 0)
        worst_d = max(worst_d, sc.div_yardstick(e[ok], s[ok].expand_as(e[ok])))
    for c in sc.AT_CASES:
        q, k, v, bias = sc.at_input(c)
        s = torch.einsum("zqd,zkd->zqk", q, k) * sc.at_scale(c) + (0 if bias is None else bias)
        worst_e = max(worst_e, sc.exp_yardstick(s - s.max(-1, keepdim=True).values))
    for c in sc.GN_CASES:
        if c["silu"] and c["B"] * c["HW"] * c["C"] < 1_000_000:
            x, gamma, beta = sc.gn_input(c)
            ref = sc.gn_reference(x, gamma, beta, c["groups"])
            y = sc.gn_apply64(x, ref["scale"], ref["shift"]).float()
            worst_e = max(worst_e, sc.exp_yardstick(-y))
            worst_d = max(worst_d, sc.div_yardstick(y, 1.0 + torch.exp(-y)))
    _note("yardstick exp", worst_e)
    _note("yardstick div", worst_d)
    assert 0.0 < worst_e <= sc.Y_EXP and 0.0 < worst_d <= sc.Y_DIV, (worst_e, worst_d)
