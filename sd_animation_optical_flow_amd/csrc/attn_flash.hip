// Fused attention for the UNet's head sizes: out = softmax(q k^T * scale + bias) v without the
// score matrix ever leaving the CU -- the form `xformers.ops.memory_efficient_attention` has at
// ldm/modules/attention.py:314,426 (16384 tokens x 8 heads at 1024x1024: 8.6 GB of scores per image in the unfused form).
//
// Written for the 32x32x2 fp32 matrix-core instruction, transposed so that nothing has to move between lanes:
//
//   S^T = K Q^T     A operand = K tile rows from LDS (b128 reads: a lane takes 4 consecutive d of its key),
//                   B operand = the wave's 32 queries, pre-scaled by scale * log2(e), held in registers for the whole key loop.
//                   The accumulator of lane (c = lane % 32, h = lane / 32) holds S^T[key = 8i + 4h + j][query = c]:
//                   one query per lane column, so the row maximum / row sum of the softmax are IN-LANE reductions over 16
//                   registers plus one exchange with lane ^ 32.
//   O^T += V^T P^T  the k index of this product is the key; the instruction wants, from half h of the wave, the key pair
//                   member h -- and register 4i + j of half h already holds key 8i + 4h + j.  So MFMA number 4i + j takes P^T
//                   straight from the accumulator register it was computed in, with the V operand read as
//                   V[key = 8i + 4h + j][d = c]: no shuffle, no LDS round trip for P.
//
// Online softmax in base 2 (v_exp_f32): m = running maximum, l = running sum per lane half (the halves share m, their partial
// sums are added once at the end), O rescaled only when some query's maximum moved (wave-uniform branch; exact, the factor
// is 1.0 otherwise).  K / V tiles of 64 (32 for d > 40) keys are double-buffered in LDS behind register-staged global loads.
// Everything is fp32; summation order differs from the unfused path, results agree to rounding.
//
// flash_attn_f16_kernel is the opt-in OFX_PREC_F16 form of the same skeleton (ofx_attention_prec / ofx_attention_bnhd_prec): 128
// queries per workgroup, 4 waves of 32 queries, double-buffered K / V tiles behind register-staged global loads, the same raster,
// bias forms, base-2 online softmax, wave-uniform rescale and m_use rule.  Its arithmetic contract:
//   operands   q, k, v are fp32 in memory; each element is rounded to fp16 ONCE, round-to-nearest-even (the _Float16 vector
//              conversion, v_cvt_pk_f16_f32 -- not the truncating pkrtz form), as it is staged.  q is rounded UNSCALED.  Magnitudes
//              beyond 65504 become infinities (as under torch.autocast); subnormals are kept, the matrix core multiplies them.
//   S^T = K Q^T  on v_mfma_f32_32x32x16_f16, fp32 accumulate: A = 8 halves of a K row from LDS (one b128 read), B = the wave's
//              queries in registers.  D = 40 runs as 48: the 8 pad columns are zeros in the Q fragment and are written as zeros
//              into both LDS buffers once before the loop (no tile store touches them; stale LDS times zero could be NaN).
//   logit      x = fma(S, scale * log2e, bias * log2e) on the fp32 score: scale and the fp32 bias never pass through fp16.
//   softmax    maximum, v_exp_f32, the running sum l, the O accumulators, the rescale and the final 1 / l are fp32; l sums the
//              fp32 probabilities BEFORE they are rounded.
//   O^T += V^T P^T  P is rounded to fp16 (RNE) straight from the accumulator registers: registers 8s .. 8s+7 converted pairwise are
//              the B fragment of k-step s, whose element j in lane half h is key 16s + 8(j>>2) + 4h + (j&3) of the block.  V is
//              staged ROW-MAJOR as halves ([key][LDV], the same coalesced float4 -> 4 halves store as K) and the A fragment is two
//              ds_read_b64_tr_b16 per k-step and 32-row tile: the hardware transpose hands lane (c, h) V[16s + 8a + 4h + e][32tt + c]
//              in element e of read a -- exactly that permuted key order.  Chosen over a transposed image because staging stays
//              one b64 store per float4 (a transposed image needs four b16 stores) and K and V share one store pattern.  Banks
//              (a 32-lane half reads 4 key rows x 16 dwords): LDV / 2 dwords = 16 * odd puts the four rows on four disjoint 16-bank
//              runs, conflict-free; LDK = DP + 8 halves = 4 * odd dwords, conflict-free for b128 reads as in the fp32 kernel.
//              LDV >= 32 * DT, so tiles with d >= D read inside their own row (rows of O^T that are never stored).
//   Two workgroups per CU (__launch_bounds__(256, 2)): one wave's softmax runs under the other's MFMAs.
//
// The two kernels share the raster (flash_raster) and nothing else on purpose: the bias / ragged mask, the online-softmax step and
// the output epilogue stay written out in both.  Forceinline helpers for any of them change the compiled instruction stream, and the
// softmax step as a helper moves register allocation in 12 of the 20 instantiations (flash_attn_kernel<40, 64, false>: 160 -> 176
// registers, occupancy 3 -> 2).  The raster helper leaves all 20 instruction-identical.
//
// The templates themselves are in attn_flash_kernels.h: this file instantiates the 20 kernels on one K and one V tensor (SEG = 0),
// attn_flash_segs.hip the 20 strided ones that read K / V through a per-image segment table (ofx_attention_bnhd_segs; SEG = 1 float32
// rows, SEG = 2 float16 rows).  SEG is a template parameter and every use of it `if constexpr`, so the 20 of this file compile to
// the registers they had without it (profiles/r38_kv_history_rate.txt has the table).
#include "attn_flash_kernels.h"

bool ofx_attention_flash_ok(int D) {
#define X(d, bk) if (D == d) return true;
    OFX_FLASH_SIZES(X)
#undef X
    return false;
}

// the launch of head size D from the list, for one kernel family and one addressing
template <bool F16, bool STRIDED>
static int flash_launch_d(const FlashArgs& a, int D, hipStream_t s) {
    switch (D) {
#define X(d, bk)                                                            \
    case d:                                                                 \
        if constexpr (F16) return launch_flash_f16<d, bk, STRIDED>(a, s);   \
        else return launch_flash<d, bk, STRIDED>(a, s);
        OFX_FLASH_SIZES(X)
#undef X
    }
    return OFX_EINVAL;
}

static int flash_dispatch(FlashArgs& a, int D, float scale, bool strided, int precision, hipStream_t s) {
    if (const int rc = flash_derive(a, scale, precision)) return rc;
    if (precision == OFX_PREC_F16) {
        OfxProfScope prof(strided ? "attn_flash_bnhd_f16" : "attn_flash_f16", s);
        prof.flops(4.0 * a.BH * (double)a.Nq * a.Nk * D);
        return strided ? flash_launch_d<true, true>(a, D, s) : flash_launch_d<true, false>(a, D, s);
    }
    OfxProfScope prof(strided ? "attn_flash_bnhd" : "attn_flash", s);
    prof.flops(4.0 * a.BH * (double)a.Nq * a.Nk * D);
    return strided ? flash_launch_d<false, true>(a, D, s) : flash_launch_d<false, false>(a, D, s);
}

int ofx_attention_flash_launch(const float* q, const float* k, const float* v, const float* bias, long bias_bstride, float* out, int BH, int Nq,
                               int Nk, int D, float scale, int precision, hipStream_t s) {
    FlashArgs a{};
    a.q = q; a.k = k; a.v = v; a.bias = bias; a.out = out;
    a.bias_bs = bias_bstride;
    a.BH = BH; a.Nq = Nq; a.Nk = Nk;
    return flash_dispatch(a, D, scale, false, precision, s);
}

int ofx_attention_flash_bnhd_launch(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* bias,
                                    long bias_bstride, float* out, int ldo, int B, int H, int Nq, int Nk, int D, float scale, int precision, hipStream_t s) {
    FlashArgs a{};
    a.q = q; a.k = k; a.v = v; a.bias = bias; a.out = out;
    a.bias_bs = bias_bstride;
    a.BH = B * H; a.Nq = Nq; a.Nk = Nk;
    a.H = H; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    return flash_dispatch(a, D, scale, true, precision, s);
}
