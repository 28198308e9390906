"""Float64 restatement, derived error bound, case table and a float32 emulation with switchable bugs for the fused attention kernel
(csrc/attn_flash.hip: ofx_attention_f32 at head sizes 40 / 64 / 80 / 128 / 160 and ofx_attention_bnhd_f32).  Not a conftest:
imported by name, and importable without a device.  U, FLOOR, E_DIV, _worst, _gen and _softmax_bound come from sd_ops_check.

u = 2^-24.  Everything below is in NATURAL units of the logit v_j = scale q.k_j + bias_j; the kernel works in base 2 (x = v log2 e),
where an error d of the exponent is a relative error d ln 2 of exp2 -- the same number as the natural-unit error of v.

The logit, as the kernel forms it (a_j = |scale| sum_d |q_d k_jd|, mx = the row maximum):
  scale      scale_log2e = fl(scale * kLog2e): one rounding, then fl(q_d * scale_log2e): one more                     2 u a_j
  score      a D-term sum on the 32x32x2 fp32 matrix cores: every term passes through at most D roundings            D u a_j
             (with 0.01 for the second order of (D + 2) u up to D = 160:  K_SCORE(D) = D + 2.01)
  bias       fl(bias_j * kLog2e), and the addition to the score, rounded relative to its result                      u |bias_j| + u |v_j|
  maximum    exp2(x_j - m1) alpha_2 alpha_3 ..., alpha_i = exp2(m_(i-1) - m_i): the subtractions telescope,
             |x_j - m1| + (m1 - m2) + ... = |x_j - m_final|, each rounded relative to its own result                    u |v_j - mx|
  constant   the float kLog2e is 1.34e-8 above log2 e (relative).  It is the same float in scale_log2e and in the bias
             product, a common factor of the whole logit: differences of logits scale by it                           E_L2E |v_j - mx|
      Delta_j = K_SCORE(D) u a_j + u |bias_j| + u |v_j| + (u + E_L2E) |v_j - mx|
  A softmax whose logits move by at most Delta_j has |p~_j / p_j - 1| <= e^(Delta_j) S+ - 1 =: r_j (sd_ops_check._softmax_bound,
  called with extra_k = -K_SUM so that the unfused kernel's summation term drops out; this kernel's own chains follow).
  A logit more than FAR = 2000 below mx has p < e^-1000 before and after any perturbation smaller than half that distance
  (asserted): such keys (the -1000 fill beside an open key has p = e^-1000, the finite -FLT_MAX fill overflows to -inf in
  bias * kLog2e) count as masked and are covered by FLOOR.
Chains.  nb = ceil(Nk / 32) blocks; key j sits in block b_j and in MFMA r_j = 4 ((j % 32) / 8) + j % 4 of its block, together with
key j +- 4 of the other wave half (the same register 4i + j' of each half).
  exponent   v_exp_f32 once per probability                                                                          E_EXP2 u
  numerator  o += v p: the product, then two additions per MFMA from its own to the last MFMA holding a key < Nk:
                 c_num(j) = 1 + 2 #{MFMAs at or after (b_j, r_j) with a key < Nk} + (nb - 1 - b_j) (1 + E_EXP2)
             (an MFMA whose keys are all past Nk adds exact zeros: p = exp2(-inf) = 0, V rows are zero-filled.)  The last term is
             one multiplication by alpha and alpha's own v_exp_f32 per later block -- at most: alpha is exactly 1.0 for a query
             whose maximum did not move, whether or not the wave takes the rescale branch.
  denominator  16 in-lane additions (register e passes through 16 - e of them), l alpha + ps (a multiplication and an addition per
             block, alpha's exponential with it), the two half-wave sums added once:
                 c_den(j) = 18 - r_j + (nb - 1 - b_j) (2 + E_EXP2)
             all terms are positive, so the sum is off by at most R_den u = sum_j p_j (1 + r_j) c_den(j) u, relative.
  alpha multiplies l and O of a query alike, and the same float in both.  The bound does NOT rely on that: it is common to the keys
  of the earlier blocks only, not to the later ones, so it does not cancel in O / l; its exponential and its two roundings are
  counted in c_num and in c_den separately.
  final      1.0f / l (E_DIV u, as in sd_ops_check) and the multiplication by it (u), the exponentials inside l (E_EXP2 u)
  floor      FLOOR sum_j |v_jd| for exponentials below the normal range (l >= 1: the maximum's own exponential is 1), and
             FLOOR nb for an O element flushed by a rescale
    |out_d - ref_d| <= sum_j p_j r_j |v_jd| + 1.001 u sum_j p_j (1 + r_j) (E_EXP2 + c_num(j)) |v_jd|
                       + 1.001 u (E_EXP2 + R_den + E_DIV + 1) sum_j p_j (1 + r_j) |v_jd| + FLOOR (sum_j |v_jd| + nb)
A perturbation common to a probability in l and in O cancels and is no error; the simulated bug "p_off_64u" therefore perturbs
the probabilities that multiply V and not those summed into l.

Measured term (v_exp_f32).  Yardstick: torch's float32 exp2 on the CPU against float64 over the tables' own shifted arguments
(x_j - max, base 2), in u of the result -- `exp2_yardstick`; test_the_exp2_yardstick_is_where_the_header_says re-measures it.
    Y_EXP2 = 1.2 (measured 1.17, rounded up).  The kernel may use twice that: E_EXP2 = 2 Y_EXP2 = 2.4 (v_exp_f32 is specified to
    1 ulp, at most 2 u).  Never measured on the kernel.

Simulated bugs (`fa_emulate`, a float32 emulation of the online softmax in 32-key blocks with the kernel's rescale rule): the
unmodified emulation stays inside the bound at every case (worst ratio 0.073, d40-nk77-shared-fill1000); every bug of FA_BUGS is
caught at one case or more of every head size (test_the_checker_catches_each_simulated_bug_at_every_head_size, which prints the
counts).  Closest to escaping: "p_off_64u", caught only where the logits carry no rounding of their own (scale 0), at 9 cases in
all: ratio 2.25 at d*-nk1-scale0 (a bound of 28.5 u |v| against an error of 64 u |v|: a margin of 2.25, so a uniform error of 29 u
and more is caught, less is not); at unit data the D roundings of a score (K_SCORE u a_j, some hundreds of u) hide it, as they
hide any honest error of that size.  Every other bug is outside by a factor of 1e3 and more, or by its NaN set.

Worst ratios measured on an MI355X (gfx950) over tests/test_gpu_flash_attn.py, 2026-10-18 (the tests print every ratio, run with -s
to re-measure); margin = 1 / ratio.  No kernel bug was found: all 95 cases pass through both entries.
    test_flash_attention_against_float64            0.0737  (d40-nk77-shared-fill1000)                 margin 13.6
        per head size, the same case each time      0.0737 / 0.0715 / 0.0679 / 0.0566 / 0.0557 (d40 / d64 / d80 / d128 / d160)
    test_flash_attention_bnhd_against_float64       0.0737  (the same case; bit for bit the contiguous entry in every case)
    test_ops_attention_against_float64              0.0244  (d40-nk3tiles-per-leadBK-grouped)          margin 41
    test_gpu_transformer.py, the bnhd check at D = 40 with a shared bias, under min(this bound, the unfused one)   0.0283
  NaN appears exactly where the reference has it in every case.  The ratios are far below 1 because the bound is a worst case
  over D + Nk roundings of one sign; the -1000 fill comes closest because there two roundings of 1443 (1.2e-4 each) dominate and
  do not average out.  That the bound still bites is what the simulated bugs above show.
"""
import functools

import torch
import torch.nn.functional as F

import sd_ops_check as sc
from sd_ops_check import E_DIV, FLOOR, U, _cdiv, _gen, _softmax_bound, _worst

FLASH_D = sc.FLASH_D
Y_EXP2 = 1.2
E_EXP2 = 2.0 * Y_EXP2
E_L2E = 1.4e-8                                   # float(1.4426950408889634f) / log2(e) - 1 = 1.34e-8
K_SCORE_EXTRA = 2.01
FAR = 2000.0
LOG2E_F32 = 1.4426950408889634                   # kLog2e; rounded to float32 where it is used
FMAX = float(torch.finfo(torch.float32).max)
NINF = float("-inf")


def exp2_yardstick(t):
    """float32 base-2 arguments -> the worst error of torch's float32 exp2 against float64 in units of u exp2(t), over the
    arguments whose exponential is a normal number."""
    t = t.float().flatten()
    t = t[torch.isfinite(t) & (t > -126.0) & (t < 127.0)]
    ref = torch.exp2(t.double())
    return _worst((torch.exp2(t).double() - ref).abs(), U * ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel's geometry, restated

def fa_bk(D):
    return 64 if D == 40 else 32


def fa_block_map(BH, qtiles):
    """(batch-head, query tile) of every workgroup id, as flash_attn_kernel computes it."""
    out = []
    for bid in range(BH * qtiles):
        if BH % 8 == 0:
            xcd, slot = bid & 7, bid >> 3
            out.append(((slot // qtiles) * 8 + xcd, slot % qtiles))
        else:
            out.append((bid // qtiles, bid % qtiles))
    return out


def fa_geometry(c):
    """qtiles, the waves as (tile, wave, first query, live queries), 32-key blocks nb, BK, K/V tiles nt, the grouped flag."""
    BH, Nq, Nk, D = c["BH"], c["Nq"], c["Nk"], c["D"]
    qtiles = _cdiv(Nq, 128)
    waves = [(t, w, t * 128 + w * 32, max(0, min(32, Nq - (t * 128 + w * 32)))) for t in range(qtiles) for w in range(4)]
    bk = fa_bk(D)
    return dict(qtiles=qtiles, waves=waves, dead_waves=sum(1 for w in waves if w[3] == 0), nb=_cdiv(Nk, 32), BK=bk, nt=_cdiv(Nk, bk),
                grouped=BH % 8 == 0, blocks=fa_block_map(BH, qtiles))


def fa_chains(Nk):
    """c_num(j), c_den(j) [Nk] float64 (header)."""
    nb = _cdiv(Nk, 32)
    j = torch.arange(Nk)
    b, w = j // 32, j % 32
    r = 4 * (w // 8) + w % 4
    # the MFMAs in order (block, r'): the lowest key of MFMA r' is 32 b + 8 (r' / 4) + r' % 4 (wave half 0)
    rr = torch.arange(16)
    low = (torch.arange(nb).view(-1, 1) * 32 + 8 * (rr // 4) + rr % 4).flatten()
    live = (low < Nk).double()
    after = live.flip(0).cumsum(0).flip(0)                       # live MFMAs at or after position (b, r)
    later = (nb - 1 - b).double()
    c_num = 1.0 + 2.0 * after[b * 16 + r] + later * (1.0 + E_EXP2)
    c_den = 18.0 - r.double() + later * (2.0 + E_EXP2)
    return c_num, c_den


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table

def _fa(D, name, BH, Nq, Nk, bias=None, data="unit", scale=None, mask=None, planted=(), schedule=None, nonfinite=None):
    return dict(name=f"d{D}-{name}", D=D, BH=BH, Nq=Nq, Nk=Nk, bias=bias, data=data, scale=scale, mask=mask, planted=list(planted),
                schedule=schedule, nonfinite=nonfinite)


def _cases_of(D):
    bk = fa_bk(D)
    n3 = 2 * bk + 1                                               # nt = 3: both LDS buffers are used again
    big = round(60.0 / D ** 0.5, 3)                               # logits of +-80 and beyond: most exponentials underflow
    return [
        _fa(D, "nk1-scale0", 1, 1, 1, data="scale0", scale=0.0),
        _fa(D, "nk1-per-unit", 3, 33, 1, "per", planted=[(1, 3)]),
        _fa(D, "nk31-per-rand30", 3, 33, 31, "per", mask="rand30", planted=[(0, 0), (1, 31), (1, 32), (2, 32)]),
        _fa(D, "nk32-mag6", 8, 32, 32, data="mag6", scale=0.05),
        _fa(D, "nk33-negscale", 1, 33, 33, data="negscale", scale=-0.2),
        _fa(D, "nk33-shared-fmax", 3, 32, 33, "shared", mask="fmax"),
        _fa(D, "nk77-shared-lead32", 3, 129, 77, "shared", mask="lead32", planted=[(None, 0), (None, 31), (None, 32), (None, 127), (None, 128)]),
        _fa(D, "nk77-per-trail", 16, 33, 77, "per", mask="trail"),
        _fa(D, "nk77-shared-fill1000", 1, 128, 77, "shared", mask="fill1000"),
        _fa(D, "nkBK-scale0", 1, 32, bk, data="scale0", scale=0.0),
        _fa(D, "nkBK+1-big80", 3, 33, bk + 1, data="big80", scale=big),
        _fa(D, "nk3tiles-per-leadBK-grouped", 8, 257, n3, "per", mask="leadBK", planted=[(3, 127), (3, 128), (7, 256)]),
        _fa(D, "nk3tiles-ascending", 1, 33, n3, schedule="ascending"),
        _fa(D, "nk3tiles-descending", 1, 33, n3, schedule="descending"),
        _fa(D, "nk3tiles-one-lane-moves", 1, 33, n3, schedule="one_lane"),
        _fa(D, "nk33-nan-bias", 3, 33, 33, "per", nonfinite="nan_bias"),
        _fa(D, "nk33-nan-query", 3, 33, 33, nonfinite="nan_q"),
        _fa(D, "nk33-inf-bias", 3, 33, 33, "per", nonfinite="inf_bias"),
        _fa(D, "nk33-inf-v-at-masked-key", 3, 33, 33, "per", nonfinite="inf_v"),
    ]


# planted: (batch-head, row) pairs whose every key is masked; z = None: in every batch-head (a shared bias)
FA_CASES = [c for D in FLASH_D for c in _cases_of(D)]
FA_GUARD = 64
DATA_MAG = {"unit": 1.0, "mag6": 6.0, "big80": 1.0, "scale0": 1.0, "negscale": 1.0}
NF_AT = (1, 5, 7)                                                 # (batch-head, query, key) of a planted non-finite bias entry
NF_Q = (1, 31)                                                    # the NaN query row
NF_V = (1, 3)                                                     # (batch-head, key): masked for every query, V row = inf
ONE_LANE = 5                                                      # the query of schedule "one_lane" whose maximum is in the last block


def fa_scale(c):
    return float(c["D"]) ** -0.5 if c["scale"] is None else float(c["scale"])


def fa_planted(c):
    """Flat row indices z * Nq + row that are NaN in the reference: the planted rows and what the non-finite inputs make."""
    out = []
    for z, r in c["planted"]:
        out += [zz * c["Nq"] + r for zz in (range(c["BH"]) if z is None else [z])]
    nf = c["nonfinite"]
    if nf in ("nan_bias", "inf_bias"):
        out.append(NF_AT[0] * c["Nq"] + NF_AT[1])
    elif nf == "nan_q":
        out.append(NF_Q[0] * c["Nq"] + NF_Q[1])
    elif nf == "inf_v":
        out += [NF_V[0] * c["Nq"] + r for r in range(c["Nq"])]
    return sorted(set(out))


def fa_input(c):
    """q [BH, Nq, D], k, v [BH, Nk, D] float32 and the bias ([Nq, Nk], [BH, Nq, Nk] or None)."""
    g = _gen(c["name"])
    BH, Nq, Nk, D = c["BH"], c["Nq"], c["Nk"], c["D"]
    bk = fa_bk(D)
    mag = DATA_MAG[c["data"]]
    q = torch.randn((BH, Nq, D), generator=g) * mag
    k = torch.randn((BH, Nk, D), generator=g) * mag
    v = torch.randn((BH, Nk, D), generator=g) * 1.5 + 0.25
    if c["schedule"]:
        # every query is a positive multiple of q0, so all of them order the keys as q0 does; the keys are sorted by q0's score
        q0 = torch.randn((BH, 1, D), generator=g)
        f = 0.5 + (torch.arange(Nq) % 7).float().view(1, Nq, 1) / 6.0
        q = q0 * f
        order = torch.einsum("zd,zkd->zk", q0[:, 0].double(), k.double()).argsort(1, descending=c["schedule"] != "ascending")
        k = torch.gather(k, 1, order.unsqueeze(-1).expand(BH, Nk, D)).contiguous()
        if c["schedule"] == "one_lane":
            q[:, ONE_LANE] = -q[:, ONE_LANE]
    bias = None
    if c["bias"]:
        shape = (Nq, Nk) if c["bias"] == "shared" else (BH, Nq, Nk)
        bias = torch.randn(shape, generator=g) * 2.0
        holes = torch.rand(shape, generator=g) < 0.3
        mask = c["mask"]
        if mask == "rand30":
            holes[..., 0] = False
            bias[holes] = NINF
        elif mask == "fmax":
            holes[..., 0] = False
            bias[holes] = -FMAX
        elif mask in ("lead32", "leadBK"):
            n0 = 32 if mask == "lead32" else bk
            holes[..., n0] = False
            bias[holes] = NINF
            bias[..., :n0] = NINF
        elif mask == "trail":
            holes[..., 0] = False
            bias[holes] = NINF
            bias[..., 32:] = NINF
        elif mask == "fill1000":
            bias = torch.full(shape, -1000.0)
            bias[..., 0:40, 0:40] = 0.0
            bias[..., 64:100, 40:Nk] = 0.0
        for z, r in c["planted"]:
            if z is None:
                bias[..., r, :] = NINF
            else:
                bias[z, r] = NINF
    nf = c["nonfinite"]
    if nf == "nan_bias":
        bias[NF_AT] = float("nan")
    elif nf == "inf_bias":
        bias[NF_AT] = float("inf")
    elif nf == "nan_q":
        q[NF_Q] = float("nan")
    elif nf == "inf_v":
        bias[NF_V[0], :, NF_V[1]] = NINF
        v[NF_V] = float("inf")
    return q, k, v, bias


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference and bound

def fa_logits64(q, k, bias, scale):
    """The float64 logits [BH, Nq, Nk] and a_j = |scale| sum_d |q_d k_d|, with the float the ABI receives as the scale."""
    s = float(torch.tensor(scale, dtype=torch.float32).double())
    qd, kd = q.double(), k.double()
    v = torch.einsum("zqd,zkd->zqk", qd, kd) * s
    a = torch.einsum("zqd,zkd->zqk", qd.abs(), kd.abs()) * abs(s)
    b = None
    if bias is not None:
        b = bias.double().expand(q.shape[0], q.shape[1], k.shape[1])
        v = v + b
    return v, a, b


def fa_reference(q, k, v, bias, scale):
    """float64 softmax(q k^T scale + bias) v [BH, Nq, D] and its bound (header)."""
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    nb = _cdiv(Nk, 32)
    lg, a, b = fa_logits64(q, k, bias, scale)
    fin = torch.isfinite(lg)
    mx = torch.where(fin, lg, torch.full_like(lg, -1e300)).max(-1, keepdim=True).values
    dist = torch.where(fin, (lg - mx).abs(), torch.zeros_like(lg))
    dv = (D + K_SCORE_EXTRA) * U * a + U * torch.where(fin, lg.abs(), torch.zeros_like(lg))
    if b is not None:
        dv = dv + U * torch.where(torch.isfinite(b), b.abs(), torch.zeros_like(b))
    dv = dv + E_L2E * dist
    far = fin & (lg - mx < -FAR)
    assert bool((dv + U * dist)[far].le(0.5 * dist[far]).all()), "a far logit's perturbation reaches half its distance from the maximum"
    lg = torch.where(far, torch.full_like(lg, NINF), lg)
    p, r = _softmax_bound(lg, torch.where(far, torch.zeros_like(dv), dv), -(_cdiv(Nk, 256) + 9))
    c_num, c_den = fa_chains(Nk)
    w = p * (1.0 + r)
    vd = v.double()
    va = vd.abs()
    ref = torch.einsum("zqk,zkd->zqd", p, vd)
    r_den = (w * c_den).sum(-1, keepdim=True)
    bound = (torch.einsum("zqk,zkd->zqd", p * r, va)
             + 1.001 * U * torch.einsum("zqk,zkd->zqd", w * (E_EXP2 + c_num), va)
             + 1.001 * U * (E_EXP2 + r_den + E_DIV + 1.0) * torch.einsum("zqk,zkd->zqd", w, va)
             + FLOOR * (va.sum(1, keepdim=True) + nb))
    return ref, bound


def fa_compare(out, ref, bound):
    """out against (ref, bound), element by element, none left out: dict(ratio: worst |error| / bound over the elements whose
    reference is a number -- NaN or inf there counts as infinite; nan_missing / nan_extra: elements that are NaN in the reference
    and not in `out` / in `out` and not in the reference; ok: ratio <= 1 and both counts 0)."""
    out = out.reshape(ref.shape)
    rn, on = torch.isnan(ref), torch.isnan(out)
    ratio = _worst((out.double() - ref).abs()[~rn], bound[~rn])
    missing, extra = int((rn & ~on).sum()), int((on & ~rn).sum())
    return dict(ratio=ratio, nan_missing=missing, nan_extra=extra, ok=bool(ratio <= 1.0) and missing == 0 and extra == 0)


@functools.lru_cache(maxsize=None)
def _case_data(name):
    c = next(c for c in FA_CASES if c["name"] == name)
    q, k, v, bias = fa_input(c)
    ref, bound = fa_reference(q, k, v, bias, fa_scale(c))
    return q, k, v, bias, ref, bound


def fa_case_data(c):
    """(q, k, v, bias, ref, bound) of a case, computed once and shared by every test: leave them unchanged."""
    return _case_data(c["name"])


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernel's online softmax, with switches for simulated bugs

FA_BUGS = ("no_rescale", "rescale_one_half", "second_half_l_dropped", "pad_keys_weighted", "m_use_minus_inf", "bias_head_stride_0",
           "bias_row_0", "batch_heads_swapped", "scale_without_log2e", "masked_row_zero", "nan_row_leaks", "p_off_64u")


def fa_base2_logits32(q, k, bias, scale, log2e=True):
    """float32 base-2 logits [BH, Nq, Nk] as the kernel forms them: (q scale_log2e) k^T + bias kLog2e."""
    l2e = torch.tensor(LOG2E_F32, dtype=torch.float32)
    c = torch.tensor(scale, dtype=torch.float32) * (l2e if log2e else 1.0)
    s = torch.matmul(q * c, k.transpose(1, 2))
    if bias is not None:
        s = s + bias * l2e
    return s


def fa_emulate(q, k, v, bias, scale, bug=None):
    """The kernel's arithmetic in float32 torch: 32-key blocks, running maximum, m_use = 0 while every key so far is masked,
    alpha = exp2(m_run - m_use) on l and O, a running sum per wave half (key % 8 < 4 or not), 1 / l at the end."""
    BH, Nq, D = q.shape
    Nk = k.shape[1]
    nb = _cdiv(Nk, 32)
    pad = nb * 32 - Nk
    if bias is not None:
        bias = bias.expand(BH, Nq, Nk)
        if bug == "bias_head_stride_0":
            bias = bias[0:1].expand(BH, Nq, Nk)
        if bug == "bias_row_0":
            bias = bias[:, 0:1].expand(BH, Nq, Nk)
        bias = F.pad(bias, (0, pad))
    s_all = fa_base2_logits32(q, F.pad(k, (0, 0, 0, pad)), bias, scale, log2e=bug != "scale_without_log2e")
    vp = F.pad(v, (0, 0, 0, pad))
    live = torch.arange(nb * 32) < Nk
    half1 = (torch.arange(32) % 8) >= 4
    m_run = torch.full((BH, Nq), NINF)
    l0, l1 = torch.zeros((BH, Nq)), torch.zeros((BH, Nq))
    o = torch.zeros((BH, Nq, D))
    d_half0 = (torch.arange(D) % 8) < 4                                  # the output columns wave half 0 holds
    for t in range(nb):
        sl = slice(32 * t, 32 * t + 32)
        s = s_all[..., sl]
        if bug != "pad_keys_weighted":
            s = torch.where(live[sl], s, torch.full_like(s, NINF))
        mx = torch.where(torch.isnan(s), torch.full_like(s, NINF), s).max(-1).values      # fmaxf passes over a NaN
        m_new = torch.maximum(m_run, mx)
        m_use = m_new if bug == "m_use_minus_inf" else torch.where(m_new == NINF, torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m_run - m_use)
        p = torch.exp2(s - m_use.unsqueeze(-1))
        l0 = l0 * alpha + p[..., ~half1].sum(-1)
        l1 = l1 * alpha + p[..., half1].sum(-1)
        ao = alpha.unsqueeze(-1).expand(BH, Nq, D)
        if bug == "no_rescale" and t > 0:
            ao = torch.ones_like(ao)
        elif bug == "rescale_one_half":
            ao = torch.where(d_half0, ao, torch.ones_like(ao))
        pv = p * (1.0 + 64.0 * U) if bug == "p_off_64u" else p
        o = o * ao + torch.matmul(pv, vp[:, sl])
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
