"""Float64 restatement, derived error bound and a torch emulation with switchable bugs for the fp16 form of the fused attention kernel
(csrc/attn_flash.hip, flash_attn_f16_kernel: ofx_attention_prec / ofx_attention_bnhd_prec with OFX_PREC_F16, `ops.attention(precision=
"fp16")`).  Not a conftest: imported by name, and importable without a device.  The case table, the inputs, the geometry, fa_compare,
the denominator chain and E_EXP2 come from flash_attn_check as they stand; U, FLOOR, E_DIV, _softmax_bound from sd_ops_check.

The kernel keeps the fp32 kernel's skeleton and BK (64 keys per tile at D = 40, 32 otherwise), so `flash_attn_check.fa_geometry` holds
for it unchanged and the table's 2 BK + 1 cases reuse both of its LDS buffers.

Reference.  The contract rounds q, k and v to fp16 once (nearest even), and that rounding is the mode, not an error of the kernel:
    ref = softmax(scale * q16 . k16 + bias) @ v16,   x16 = x.half().double(),   in float64.
u = 2^-24, u16 = 2^-11.  Natural units of the logit v_j = scale q16 . k16_j + bias_j, as in flash_attn_check.

The logit, as this kernel forms it (a_j = |scale| sum_d |q16_d k16_jd|, mx = the row maximum):
  score      a product of two fp16 numbers has 22 significant bits: exact in fp32.  What is left is the fp32 accumulation of the
             v_mfma_f32_32x32x16_f16 chain over DP = 16 ceil(D / 16) terms (D = 40 runs as 48; the pad terms are exact zeros but are
             counted): every term passes through at most DP roundings, in any order                                  DP u a_j
  scale      q is NOT scaled before it is rounded; scale_log2e = fl(scale * kLog2e) carries one rounding               u a_j
             (with 0.01 for the second order of (DP + 1) u up to DP = 160:  K_SCORE16(D) = DP + 1.01)
  fma        x_j = fma(S_j, scale_log2e, fl(bias_j * kLog2e)): the bias product is rounded once, the fma once,
             relative to its result (without a bias: fl(S_j * scale_log2e), the same single rounding)                  u |bias_j| + u |v_j|
  maximum    the subtractions of the running maximum telescope, as in flash_attn_check                                 u |v_j - mx|
  constant   the float kLog2e, common to scale_log2e and the bias product                                              E_L2E |v_j - mx|
      Delta_j = K_SCORE16(D) u a_j + u |bias_j| + u |v_j| + (u + E_L2E) |v_j - mx|
  -> |p~_j / p_j - 1| <= e^(Delta_j) S+ - 1 =: r_j (sd_ops_check._softmax_bound), far logits as in flash_attn_check (FAR).
Chains.  nb = ceil(Nk / 32) blocks; key j sits in block b_j, in P V MFMA s_j = (j % 32) / 16 of its block (a 32x32x16 MFMA sums 16
keys), and in accumulator register r_j = 4 ((j % 32) / 8) + j % 4 (the C layout is the fp32 kernel's).
  exponent   v_exp_f32 once per probability                                                                          E_EXP2 u
  rounding P  NEW.  The probability at the time it is used, e_j = exp2(x_j - m_use) <= 1, is rounded to fp16, nearest even: where
             it is a normal fp16 number (e_j >= 2^-14) the error is at most u16 e_j; where it is subnormal or rounds to zero it is
             at most half the subnormal spacing, 2^-25, absolute.  Every later alpha <= 1 only shrinks both.  The output is O / l
             with l >= 1 (the maximum's own exponential is 1), and l is summed from the UNROUNDED fp32 probabilities, so it carries
             none of this: in the output the normal part is at most u16 p_j (1 + r_j) |v_jd| per key and the rest 2^-25 |v_jd|:
                 u16 sum_j p_j (1 + r_j) |v16_jd| + 2^-25 sum_j |v16_jd|
             The product of the rounded probability and v16 is again exact in fp32.
  numerator  each P V MFMA adds 16 keys to the accumulator: a term passes through at most 16 roundings in its own MFMA and in every
             later one that holds a key < Nk (an MFMA whose keys are all past Nk adds exact zeros), and a multiplication by alpha
             with alpha's own exponential per later block:
                 c_num16(j) = 16 #{MFMAs at or after (b_j, s_j) with a key < Nk} + (nb - 1 - b_j) (1 + E_EXP2)
  denominator, final, floor   as in flash_attn_check (c_den(j), R_den, E_DIV, FLOOR): this kernel sums l the same way.
    |out_d - ref_d| <= sum_j p_j r_j |v_jd| + 1.001 u sum_j p_j (1 + r_j) (E_EXP2 + c_num16(j)) |v_jd|
                       + 1.001 u (E_EXP2 + R_den + E_DIV + 1) sum_j p_j (1 + r_j) |v_jd|
                       + 1.001 (u16 sum_j p_j (1 + r_j) |v_jd| + 2^-25 sum_j |v_jd|) + FLOOR (sum_j |v_jd| + nb),    v = v16.
Nothing in it is measured except E_EXP2 (flash_attn_check's yardstick, unchanged).  The P term dominates: u16 against some tens of u.

Simulated bugs (`fa16_emulate`, a torch emulation of the contract: operands through .half(), exact fp32 products, the fma formed in
float64 and rounded once, 32-key blocks with the kernel's rescale rule, P through .half() into the second product, l from the
unrounded P).  FA16_BUGS are the ways THIS kernel can go wrong plus the bugs of flash_attn_check.FA_BUGS that still apply (all but
"p_off_64u": 64 u is 1/128 of the u16 the contract itself allows on P).  Measured on the CPU (test_attn_f16_host.py prints them):
  the unmodified emulation is inside the bound at every case: worst ratio 0.753 (d64-nk3tiles-per-leadBK-grouped).  The fp32
  kernel's worst is 0.07: here the rounding of P is really made and its bound is tight -- u16 per key with no slack of D, met
  within 25 % where a row has one or two open keys.
  Every bug of FA16_CATCHABLE is caught at one case or more of every head size where it applies (pad_columns_nan: D = 40 only,
  the one head size with pad columns; it is caught by the NaN set at all 19 cases of D = 40).  Closest to escaping:
  bias_rounded_to_half (largest ratio per head size 3.2 .. 4.8, at 8 cases each) and q_scaled_before_rounding (8.4 .. 20, 9 to 11
  cases); every other one is outside by 1e3 and more or by its NaN set.
  UNCATCHABLE by a bound, listed and not asserted (FA16_UNCATCHABLE), with the largest ratio over the table:
    p_not_rounded      0.028.  P fed to the second product unrounded is CLOSER to float64 than the contract: the bound grants the P
                       term, so its absence cannot be seen.  fp16 MFMAs cannot take fp32 operands, so the kernel cannot do this
                       without ceasing to be the fp16 kernel; the exactness tests and the timing hold the rest.
    l_from_rounded_p   0.611 (the unmodified emulation has 0.753 at the same case).  O and l then carry the same rounding, which
                       partly cancels in O / l; what remains is at most u16 relative, which the bound grants.
  What no bound can hold is held by the exactness tests of test_gpu_flash_attn_f16.py (one-hot selection, scale 0): there
  v_natural_key_order, a transposed-read slip or a stale LDS buffer return another key's row, bit for bit.

Worst ratios measured on an MI355X (gfx950) over tests/test_gpu_flash_attn_f16.py, 2026-10-19 (the tests print every ratio, run
with -s to re-measure).  No kernel bug was found: all 95 cases pass through both entries, the exactness tests hold bit for bit.
    test_flash_attention_f16_against_float64                   0.7529  (d64-nk3tiles-per-leadBK-grouped)     margin 1.33
        per head size   0.6427 (d40-nk77-shared-lead32) / 0.7529 / 0.6977 (d80-nk3tiles-per-leadBK-grouped) /
                        0.6237 (d128-nk77-shared-lead32) / 0.5724 (d160-nk3tiles-per-leadBK-grouped)
    test_flash_attention_bnhd_f16_on_slices_of_one_qkv_buffer   the same figures: bit for bit the contiguous entry in every case
  The device sits where the emulation sits (0.7533 at the same case): the ratio is the rounding of P, made once and bounded
  tightly, not accumulated fp32 noise.  NaN appears exactly where the reference has it in every case.
"""
import functools

import torch
import torch.nn.functional as F

import flash_attn_check as fc
from flash_attn_check import E_EXP2, E_L2E, FA_CASES, FAR, LOG2E_F32, NINF, fa_bk, fa_chains, fa_compare, fa_input, fa_planted, fa_scale
from sd_ops_check import E_DIV, FLOOR, U, _cdiv, _softmax_bound

FLASH_D = fc.FLASH_D
U16 = 2.0 ** -11
P_SUB = 2.0 ** -25                               # half the spacing of the fp16 subnormals
K_SCORE16_EXTRA = 1.01
PREC_FP32, PREC_F16 = 0, 5                       # include/ofx.h


def fa16_dp(D):
    return _cdiv(D, 16) * 16


def half64(t):
    """fp32 -> fp16 (nearest even, overflow to inf, subnormals kept) -> float64."""
    return t.half().double()


def fa16_key_perm():
    """perm[pos] = the key (within a 32-key block) whose probability sits at fragment position pos = 16 s + 8 h + j of the P V
    MFMAs: 16 s + 8 (j >> 2) + 4 h + (j & 3)."""
    pos = torch.arange(32)
    s, h, j = pos // 16, (pos // 8) % 2, pos % 8
    return 16 * s + 8 * (j // 4) + 4 * h + (j % 4)


def fa16_chains(Nk):
    """c_num16(j) [Nk] float64 (header) and flash_attn_check's c_den(j)."""
    nb = _cdiv(Nk, 32)
    j = torch.arange(Nk)
    b, s = j // 32, (j % 32) // 16
    low = (torch.arange(nb).view(-1, 1) * 32 + 16 * torch.arange(2)).flatten()          # the lowest key of MFMA (b, s)
    live = (low < Nk).double()
    after = live.flip(0).cumsum(0).flip(0)
    later = (nb - 1 - b).double()
    c_num = 16.0 * after[b * 2 + s] + later * (1.0 + E_EXP2)
    _, c_den = fa_chains(Nk)
    return c_num, c_den


def fa16_reference(q, k, v, bias, scale):
    """float64 softmax(scale q16 k16^T + bias) v16 [BH, Nq, D] and its bound (header)."""
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    nb = _cdiv(Nk, 32)
    q16, k16, vd = half64(q), half64(k), half64(v)
    lg, a, b = fc.fa_logits64(q16, k16, bias, scale)
    fin = torch.isfinite(lg)
    mx = torch.where(fin, lg, torch.full_like(lg, -1e300)).max(-1, keepdim=True).values
    dist = torch.where(fin, (lg - mx).abs(), torch.zeros_like(lg))
    dv = (fa16_dp(D) + K_SCORE16_EXTRA) * U * a + U * torch.where(fin, lg.abs(), torch.zeros_like(lg))
    if b is not None:
        dv = dv + U * torch.where(torch.isfinite(b), b.abs(), torch.zeros_like(b))
    dv = dv + E_L2E * dist
    far = fin & (lg - mx < -FAR)
    assert bool((dv + U * dist)[far].le(0.5 * dist[far]).all()), "a far logit's perturbation reaches half its distance from the maximum"
    lg = torch.where(far, torch.full_like(lg, NINF), lg)
    p, r = _softmax_bound(lg, torch.where(far, torch.zeros_like(dv), dv), -(_cdiv(Nk, 256) + 9))
    c_num, c_den = fa16_chains(Nk)
    w = p * (1.0 + r)
    va = vd.abs()
    ref = torch.einsum("zqk,zkd->zqd", p, vd)
    r_den = (w * c_den).sum(-1, keepdim=True)
    wv = torch.einsum("zqk,zkd->zqd", w, va)
    bound = (torch.einsum("zqk,zkd->zqd", p * r, va)
             + 1.001 * U * torch.einsum("zqk,zkd->zqd", w * (E_EXP2 + c_num), va)
             + 1.001 * U * (E_EXP2 + r_den + E_DIV + 1.0) * wv
             + 1.001 * (U16 * wv + P_SUB * va.sum(1, keepdim=True))
             + FLOOR * (va.sum(1, keepdim=True) + nb))
    return ref, bound


@functools.lru_cache(maxsize=None)
def _case_data(name):
    c = next(c for c in FA_CASES if c["name"] == name)
    q, k, v, bias = fa_input(c)
    ref, bound = fa16_reference(q, k, v, bias, fa_scale(c))
    return q, k, v, bias, ref, bound


def fa16_case_data(c):
    """(q, k, v, bias, ref, bound) of a case of FA_CASES for the fp16 kernel, computed once and shared: leave them unchanged."""
    return _case_data(c["name"])


# ---------------------------------------------------------------------------------------------------------------------------------
# torch emulation of the contract, with switches for simulated bugs

FA16_OWN_BUGS = ("v_natural_key_order", "pad_columns_nan", "q_scaled_before_rounding", "bias_rounded_to_half", "kv_buffer_reused_early")
FA16_KEPT_BUGS = tuple(b for b in fc.FA_BUGS if b != "p_off_64u")
FA16_CATCHABLE = FA16_OWN_BUGS + FA16_KEPT_BUGS
FA16_UNCATCHABLE = ("p_not_rounded", "l_from_rounded_p")
FA16_BUGS = FA16_CATCHABLE + FA16_UNCATCHABLE


def fa16_applies(bug, D):
    return D == 40 if bug == "pad_columns_nan" else True


def fa16_emulate(q, k, v, bias, scale, bug=None):
    """The contract in torch: q, k, v through fp16, exact products with fp32 accumulation, x = fma(S, scale_log2e, bias kLog2e),
    32-key blocks, running maximum with m_use = 0 while every key so far is masked, alpha on l and O, l per wave half from the fp32
    probabilities, P through fp16 into O, 1 / l at the end."""
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    nb = _cdiv(Nk, 32)
    pad = nb * 32 - Nk
    l2e = torch.tensor(LOG2E_F32, dtype=torch.float32)
    c = torch.tensor(scale, dtype=torch.float32) * (1.0 if bug == "scale_without_log2e" else l2e)
    if bias is not None:
        bias = bias.expand(BH, Nq, Nk)
        if bug == "bias_head_stride_0":
            bias = bias[0:1].expand(BH, Nq, Nk)
        if bug == "bias_row_0":
            bias = bias[:, 0:1].expand(BH, Nq, Nk)
        bias = F.pad(bias, (0, pad))
    q16 = ((q * c) if bug == "q_scaled_before_rounding" else q).half().float()
    k16 = F.pad(k, (0, 0, 0, pad)).half().float()
    v16 = F.pad(v, (0, 0, 0, pad)).half().float()
    if bug == "kv_buffer_reused_early":
        # tile t + 1 (BK keys) is read where tile t belongs; the last tile has no successor and is itself
        bk = fa_bk(D)
        nt = _cdiv(Nk, bk)
        tot = nt * bk
        kk, vv = F.pad(k16, (0, 0, 0, tot - k16.shape[1])), F.pad(v16, (0, 0, 0, tot - v16.shape[1]))
        src = torch.arange(tot)
        src = torch.where(src // bk < nt - 1, src + bk, src)
        k16, v16 = kk[:, src][:, :nb * 32], vv[:, src][:, :nb * 32]
    s_all = torch.matmul(q16, k16.transpose(1, 2))
    if bug == "pad_columns_nan" and D == 40:
        s_all = s_all + float("nan")                                      # 0 * NaN of a pad column enters every score
    if bug == "q_scaled_before_rounding":
        x = s_all if bias is None else s_all + bias * l2e
    else:
        bl = None if bias is None else bias * l2e
        if bug == "bias_rounded_to_half" and bl is not None:
            bl = bl.half().float()
        x = s_all.double() * c.double()
        if bl is not None:
            x = x + bl.double()
        x = x.float()                                                     # one rounding: the fma
    live = torch.arange(nb * 32) < Nk
    half1 = (torch.arange(32) % 8) >= 4
    perm = fa16_key_perm()
    m_run = torch.full((BH, Nq), NINF)
    l0, l1 = torch.zeros((BH, Nq)), torch.zeros((BH, Nq))
    o = torch.zeros((BH, Nq, D))
    d_half0 = (torch.arange(D) % 8) < 4
    for t in range(nb):
        sl = slice(32 * t, 32 * t + 32)
        s = x[..., sl]
        if bug != "pad_keys_weighted":
            s = torch.where(live[sl], s, torch.full_like(s, NINF))
        mx = torch.where(torch.isnan(s), torch.full_like(s, NINF), s).max(-1).values
        m_new = torch.maximum(m_run, mx)
        m_use = m_new if bug == "m_use_minus_inf" else torch.where(m_new == NINF, torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m_run - m_use)
        p = torch.exp2(s - m_use.unsqueeze(-1))
        p16 = p if bug == "p_not_rounded" else p.half().float()
        pl = p16 if bug == "l_from_rounded_p" else p
        l0 = l0 * alpha + pl[..., ~half1].sum(-1)
        l1 = l1 * alpha + pl[..., half1].sum(-1)
        ao = alpha.unsqueeze(-1).expand(BH, Nq, D)
        if bug == "no_rescale" and t > 0:
            ao = torch.ones_like(ao)
        elif bug == "rescale_one_half":
            ao = torch.where(d_half0, ao, torch.ones_like(ao))
        pv = p16[..., perm] if bug == "v_natural_key_order" else p16
        o = o * ao + torch.matmul(pv, v16[:, sl])
        m_run = m_new
    l = l0 if bug == "second_half_l_dropped" else l0 + l1
    out = o * (1.0 / l).unsqueeze(-1)
    if bug == "masked_row_zero":
        out = torch.where((l == 0).unsqueeze(-1), torch.zeros_like(out), out)
    elif bug == "nan_row_leaks":
        flat = out.reshape(-1, D).clone()
        rows = torch.isnan(flat).all(1).nonzero().flatten().tolist()
        for r in rows:
            nb_row = r + 1 if r + 1 < flat.shape[0] else r - 1
            if nb_row >= 0 and nb_row not in rows:
                flat[nb_row] = float("nan")
        out = flat.view(BH, Nq, D)
    elif bug == "batch_heads_swapped" and BH % 8 == 0:
        out = torch.cat([out[1:2], out[0:1], out[2:]])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# exactness cases, which a bound cannot replace

def fa16_onehot_case(D):
    """Nq = Nk = 2 BK + 1, BH = 3: a per-batch-head bias that is 0 at key pi(q) and -inf elsewhere, pi a seeded permutation per
    batch-head.  p is exactly 1 at one key and 0 elsewhere, l = 1: the output equals v16[pi(q)] bit for bit."""
    g = torch.Generator().manual_seed(1600 + D)
    N, BH = 2 * fa_bk(D) + 1, 3
    q = torch.randn((BH, N, D), generator=g)
    k = torch.randn((BH, N, D), generator=g)
    v = torch.randn((BH, N, D), generator=g) * 1.5 + 0.25
    pi = torch.stack([torch.randperm(N, generator=g) for _ in range(BH)])
    bias = torch.full((BH, N, N), NINF)
    bias.scatter_(2, pi.unsqueeze(-1), 0.0)
    want = torch.gather(v.half().float(), 1, pi.unsqueeze(-1).expand(BH, N, D))
    return q, k, v, bias, want


def fa16_mean_case(D, Nk):
    """scale = 0, no bias, V integer-valued with |v| <= 8, Nk a power of two <= 32: every p is exactly 1, l = Nk, every partial sum
    an integer below 2^11: out == mean(v) bit for bit."""
    assert Nk & (Nk - 1) == 0 and Nk <= 32
    g = torch.Generator().manual_seed(1700 + D + Nk)
    BH, Nq = 3, 33
    q = torch.randn((BH, Nq, D), generator=g)
    k = torch.randn((BH, Nk, D), generator=g)
    v = torch.randint(-8, 9, (BH, Nk, D), generator=g).float()
    want = (v.sum(1, keepdim=True) / Nk).expand(BH, Nq, D).contiguous()
    return q, k, v, want
